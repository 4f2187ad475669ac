"""No GPU: the host-only parts of planning from the direct gather (include/uvrt.h "planning from the direct gather") -- the
new symbols in both libraries, the refusals that need no device, the CLI's refusals of --plan-gather and the binding's
gather_samples argument."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np

from conftest import GLB, GOLDEN
from plan_options_pin import check_plan_option

NEW = ("uvrt_plan_begin_expected", "uvrt_plan_capture_expected", "uvrt_plan_read_exposure_expected", "uvrt_write_expected")


def test_symbols_are_bound_and_resolve_in_both_libraries(pkg):
    names = [name for name, _, _ in pkg.capi.SYMBOLS]
    for n in NEW:
        assert names.count(n) == 1
        for path in (pkg.capi.LIB_PATH, pkg.capi.LIB_DEV_PATH):
            assert hasattr(C.CDLL(path), n), (path, n)
        for dev in (False, True):
            assert getattr(pkg.capi.lib(dev), n).restype is C.c_int
    for m in ("plan_begin_expected", "plan_capture_expected", "plan_read_exposure_expected", "write_expected"):
        assert hasattr(pkg.capi.Ctx, m)
    from uvrt_amd import host
    check_plan_option(host, "gather_samples", C.c_int, 0)


def test_a_null_context_is_refused_without_a_gpu(pkg):
    buf = np.zeros(4, dtype=np.float64)
    for dev in (False, True):
        L = pkg.capi.lib(dev)
        calls = (("uvrt_plan_begin_expected", lambda: L.uvrt_plan_begin_expected(None, 3)),
                 ("uvrt_plan_capture_expected", lambda: L.uvrt_plan_capture_expected(None, 0)),
                 ("uvrt_plan_read_exposure_expected", lambda: L.uvrt_plan_read_exposure_expected(None, 0, buf.ctypes.data, 0, 4)),
                 ("uvrt_write_expected", lambda: L.uvrt_write_expected(None, buf.ctypes.data, 0, 4)))
        for name, call in calls:
            assert call() == -1 and name.encode() in L.uvrt_last_error(), name          # UVRT_ERR_INVALID


def test_cli_refuses_plan_gather_with_gather_batch_gpus_and_holdout(pkg):
    cli = os.path.join(os.path.dirname(pkg.capi.LIB_PATH), "uvrt_cli")
    base = [cli, "--room", GLB, "--route-dir", GOLDEN, "--route", "lange_route"]
    for extra, word in ((["--gather", "4"], "--gather"), (["--batch", "2"], "--batch"), (["--gpus", "2"], "--gpus"),
                        (["--plan-holdout", "7"], "--plan-holdout"), (["--plan", "50", "--batch", "2"], "--batch"),
                        (["--plan-drive", "0.1", "--gpus", "2"], "--gpus")):
        for args in (["--plan-gather", "4"] + extra, extra + ["--plan-gather", "4"]):
            r = subprocess.run(base + args, capture_output=True, text=True, timeout=60)
            assert r.returncode == 2, (args, r.stdout, r.stderr)
            assert "--plan-gather" in r.stderr and word in r.stderr.replace("--plan-gather", ""), (args, r.stderr)
    for s in ("0", "-3", "4097"):
        r = subprocess.run(base + ["--plan-gather", s], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "--plan-gather" in r.stderr, (s, r.stderr)
    r = subprocess.run(base + ["--plan-gather"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2


def test_plan_durations_accepts_gather_samples(pkg):
    from uvrt_amd import host
    sig = inspect.signature(host.RayTracer.PlanDurations)
    assert sig.parameters["gather_samples"].default == 0
    # the two entry points take the options as one struct; the arguments from before the gather are its first fields
    by_name = {n: a for n, _, a in host.SYMBOLS}
    assert len(by_name["uvrt_host_rt_plan"]) == 4 and len(by_name["uvrt_host_rt_plan_group"]) == 5
    for name, ctype, default in (("min_dose", C.c_float, -1.0), ("min_photons", C.c_int, 16), ("margin", C.c_double, 1e-6),
                                 ("rel_gap", C.c_double, 1e-3), ("max_iterations", C.c_int, 200), ("mask", C.c_void_p, None),
                                 ("gather_samples", C.c_int, 0)):
        check_plan_option(host, name, ctype, default)


def test_plan_options_mirror_the_library_struct(pkg):
    """host.PlanOptions against uvrt_host_plan_options: every offset and the size as the C++ compiler laid them out, and the
    defaults of RayTracer::PlanOptions{} written over a struct that held something else"""
    from uvrt_amd import host
    names = [f for f, _ in host.PlanOptions._fields_]
    want = [getattr(host.PlanOptions, f).offset for f in names] + [C.sizeof(host.PlanOptions)]
    got = (C.c_int * 64)()
    n = host.lib().uvrt_host_plan_options_layout(got, 64)
    assert n == len(want) and list(got[:n]) == want
    o = host.PlanOptions()
    C.memset(C.byref(o), 0x5A, C.sizeof(o))
    host.lib().uvrt_host_plan_options_init(C.byref(o))
    defaults = dict(min_dose=-1.0, min_photons=16, margin=1e-6, rel_gap=1e-3, max_iterations=200, gather_max_extra=64,
                    reflect_samples=16)
    for f in names:
        assert getattr(o, f) == (None if f == "mask" else defaults.get(f, 0)), f
