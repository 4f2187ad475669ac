"""What the CPU tests of the gather features hold the host binding to: every plan option crosses into libuvrt_host.so as one
field of host.PlanOptions (uvrt_host_plan_options in host/host_capi.cpp), through the two plan entry points."""


def check_plan_option(host, name, ctype, default):
    """PlanOptions has `name` once, with that ctype and that default; uvrt_host_rt_plan and uvrt_host_rt_plan_group are each
    bound once and resolve in the library"""
    assert [f for f, _ in host.PlanOptions._fields_].count(name) == 1
    assert dict(host.PlanOptions._fields_)[name] is ctype
    assert getattr(host.PlanOptions(), name) == default
    for entry in ("uvrt_host_rt_plan", "uvrt_host_rt_plan_group"):
        assert [n for n, _, _ in host.SYMBOLS].count(entry) == 1 and hasattr(host.lib(), entry)
