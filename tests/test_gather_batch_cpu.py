"""No GPU: the host-only parts of the batched direct gather (include/uvrt.h "batched direct gather") -- the four
symbols in both libraries, in the header and in the bindings, the refusals that need no device, the CLI's --gather-batch and
the binding's gather_batch."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import GLB, GOLDEN, ROOT
from plan_options_pin import check_plan_option

NEW = ("uvrt_gather_direct_batch", "uvrt_gather_batch_select", "uvrt_gather_batch_info", "uvrt_read_gather_batch")


def test_symbols_are_bound_and_resolve_in_both_libraries(pkg):
    names = [name for name, _, _ in pkg.capi.SYMBOLS]
    header = open(os.path.join(ROOT, "include", "uvrt.h")).read()
    assert "enum { UVRT_GATHER_BATCH_MAX = 64 };" in header
    for n in NEW:
        assert names.count(n) == 1
        assert ("int %s(uvrt_ctx* ctx, " % n) in header
        for path in (pkg.capi.LIB_PATH, pkg.capi.LIB_DEV_PATH):
            assert hasattr(C.CDLL(path), n), (path, n)
        for dev in (False, True):
            assert getattr(pkg.capi.lib(dev), n).restype is C.c_int
    by_name = {n: a for n, _, a in pkg.capi.SYMBOLS}
    assert [len(by_name[n]) for n in NEW] == [5, 2, 2, 6]
    for m in ("gather_direct_batch", "gather_batch_select", "gather_batch_info", "read_gather_batch"):
        assert hasattr(pkg.capi.Ctx, m)
    assert header.index("adaptive gather: extra shadow rays") < header.index("batched direct gather: one shadow-ray pass") \
        < header.index("one diffuse bounce: a closest-hit query")


def test_null_arguments_are_refused_without_a_gpu(pkg):
    buf = np.full(16, 7.0, dtype=np.float64)
    info = np.full(4, 7, dtype=np.int32)
    prm = (pkg.capi.GatherParams * 2)()
    for dev in (False, True):
        L = pkg.capi.lib(dev)
        calls = (("uvrt_gather_direct_batch", lambda: L.uvrt_gather_direct_batch(None, C.cast(prm, C.c_void_p), 2, 0, 4)),
                 ("uvrt_gather_direct_batch", lambda: L.uvrt_gather_direct_batch(None, None, 2, 0, 4)),
                 ("uvrt_gather_batch_select", lambda: L.uvrt_gather_batch_select(None, 0)),
                 ("uvrt_gather_batch_info", lambda: L.uvrt_gather_batch_info(None, info.ctypes.data)),
                 ("uvrt_gather_batch_info", lambda: L.uvrt_gather_batch_info(None, None)),
                 ("uvrt_read_gather_batch", lambda: L.uvrt_read_gather_batch(None, 0, 0, buf.ctypes.data, 0, 4)),
                 ("uvrt_read_gather_batch", lambda: L.uvrt_read_gather_batch(None, 0, 0, None, 0, 4)))
        for name, call in calls:
            assert call() == -1 and name.encode() in L.uvrt_last_error(), name          # UVRT_ERR_INVALID
    assert np.all(buf == 7.0) and np.all(info == 7)


def test_cli_refuses_a_batch_it_cannot_run(pkg):
    cli = os.path.join(os.path.dirname(pkg.capi.LIB_PATH), "uvrt_cli")
    base = [cli, "--room", GLB, "--route-dir", GOLDEN, "--route", "lange_route"]
    for extra in (["--gather-batch", "3"],                                  # alone: neither --gather nor --plan-gather
                  ["--gather", "0", "--gather-batch", "3"],
                  ["--gather", "4", "--gather-batch", "65"],
                  ["--gather", "4", "--gather-batch", "-1"],
                  ["--gather", "4", "--gather-batch", "x"],
                  ["--gather", "4", "--gather-batch", "3x"],
                  ["--plan-gather", "4", "--gather-batch", "2.5"]):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2, (extra, r.stdout, r.stderr)
        assert "--gather-batch" in r.stderr, (extra, r.stderr)
    r = subprocess.run(base + ["--gather", "4", "--gather-batch"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2
    # the existing refusals stay, with the flag beside them
    for extra, word in ((["--gather", "4", "--gather-batch", "3", "--batch", "2"], "--batch"),
                        (["--gather", "4", "--gather-batch", "3", "--gpus", "2"], "--gpus"),
                        (["--plan-gather", "4", "--gather-batch", "3", "--batch", "2"], "--batch"),
                        (["--plan-gather", "4", "--gather-batch", "3", "--gather", "4"], "--gather")):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and word in r.stderr and "--gather-batch B" not in r.stderr, (extra, r.stderr)


def test_the_binding_carries_gather_batch(pkg):
    from uvrt_amd import host
    check_plan_option(host, "gather_batch", C.c_int, 0)
    check_plan_option(host, "reflect_bounces", C.c_int, 0)                          # the options from before stay
    assert "gatherBatch" in host._FIELDS and "gatherBatch" in host._INT_FIELDS
    rt = host.RayTracer(init=False)
    try:
        assert rt.gather_batch == 0 and rt.gatherBatch == 0                         # the default: launch by launch
        rt.gather_batch = 5
        assert rt.gather_batch == 5 and rt.gatherBatch == 5
        rt.gatherBatch = 64
        assert rt.gather_batch == 64
        for bad in (-1, 65, 2.5):
            with pytest.raises(ValueError, match="gather_batch"):
                rt.gather_batch = bad
            with pytest.raises(ValueError, match="gather_batch"):
                rt.gatherBatch = bad
            with pytest.raises(ValueError, match="gather_batch"):
                rt.PlanDurationsBatched(bad, gather_samples=4)
            with pytest.raises(ValueError, match="gather_batch"):
                rt.PlanDurationsRefined(0.5, gather_samples=4, gather_batch=bad)
        assert rt.gather_batch == 64
        with pytest.raises(ValueError, match="gather_batch needs gather_samples"):
            rt.PlanDurationsBatched(4)
        with pytest.raises(TypeError, match="unknown arguments"):
            rt.PlanDurationsBatched(4, gather_samples=4, gather_rel_error=0.5)
        with pytest.raises(ValueError, match="gather_confidence"):                  # an existing refusal stays
            rt.PlanDurationsReflect(0.1, 4, gather_samples=16, gather_confidence=2.0, gather_batch=4)
    finally:
        rt.close()


def test_a_route_file_gets_no_tag(pkg, tmp_path):
    from uvrt_amd import host
    rt = host.RayTracer(init=False)
    try:
        rt.set_route_dir(GOLDEN + os.sep)
        rt.LoadRoute("lange_route")
        rt.gatherSamples = 4
        rt.set_route_dir(str(tmp_path) + os.sep)
        rt.SaveRoute("plain")
        rt.gather_batch = 7
        rt.SaveRoute("batched")
        assert (tmp_path / "plain.xml").read_bytes() == (tmp_path / "batched.xml").read_bytes()
    finally:
        rt.close()
