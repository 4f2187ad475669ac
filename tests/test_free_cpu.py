"""CPU: the host-only parts of the free-ray / sweep interface (include/uvrt.h "free rays"): the SEED a sweep leaves
behind, the ABI bindings, and the route file's drive speed."""
import os

import numpy as np

from conftest import GOLDEN
from sweep_restate import seed_next_sweep


def test_seed_next_sweep_equals_the_restatement(pkg, orc):
    """uvrt_seed_next_sweep = work-item 0's RNG state after generate.cl:13-35 at `from` and one more draw"""
    rng = np.random.default_rng(5)
    cases = [((-0.255, -0.995, -3.31), 1.0, 0), ((0.0, 0.0, 0.0), 1.0, 0), ((1.5, -0.2, 2.25), 0.8, 0xFFFFFFFF),
             ((-3.0, 0.4, 7.5), 1.3, 123456789)]
    cases += [(tuple(rng.uniform(-5, 5, 3)), float(rng.uniform(0.5, 1.5)), int(rng.integers(0, 2 ** 32))) for _ in range(40)]
    for frm, length, prev in cases:
        got = pkg.capi.seed_next_sweep(frm, length, prev)
        assert got == seed_next_sweep(orc, frm, length, prev), (frm, length, prev)
        # one more draw than a stop at the same place: never the stop's SEED (xorshift has no fixed point but 0)
        stop = pkg.capi.seed_next(frm, length, prev)
        assert got != stop or stop == 0
    # the chain: a sweep's SEED feeds the next launch
    s = r = 0
    for frm, length, _ in cases[:6]:
        s = pkg.capi.seed_next_sweep(frm, length, s)
        r = seed_next_sweep(orc, frm, length, r)
        assert s == r
    assert s != 0


def test_new_symbols_are_bound(pkg):
    names = {n for n, _, _ in pkg.capi.SYMBOLS}
    assert {"uvrt_write_free_rays", "uvrt_generate_sweep", "uvrt_seed_next_sweep"} <= names
    L = pkg.capi.lib()
    for n in ("uvrt_write_free_rays", "uvrt_generate_sweep", "uvrt_seed_next_sweep"):
        assert getattr(L, n).argtypes is not None
    assert hasattr(pkg.capi.Ctx, "write_free_rays") and hasattr(pkg.capi.Ctx, "generate_sweep")
    from uvrt_amd import host
    assert "driveSpeed" in host._FIELDS
    assert "uvrt_host_rt_compute_segment" in {n for n, _, _ in host.SYMBOLS}
    assert hasattr(host.RayTracer, "ComputeSegmentDosageMap")


def test_route_file_keeps_the_drive_speed(pkg, tmp_path):
    """<rijsnelheid> is written only when the route drives; a route saved at 0 is byte for byte what the tag-less writer
    saved (tests/golden/lange_route.xml is a fixed point of that writer: loaded and saved, it came back unchanged)."""
    from uvrt_amd import host
    rt = host.RayTracer(init=False)
    rt.set_route_dir(GOLDEN + os.sep)
    rt.LoadRoute("lange_route")
    assert rt.driveSpeed == 0.0
    rt.set_route_dir(str(tmp_path) + os.sep)
    rt.SaveRoute("still")
    plain = (tmp_path / "still.xml").read_bytes()
    assert plain == open(os.path.join(GOLDEN, "lange_route.xml"), "rb").read()
    assert b"rijsnelheid" not in plain
    rt.driveSpeed = 0.125
    rt.SaveRoute("driving")
    driving = (tmp_path / "driving.xml").read_bytes()
    line = b"    <rijsnelheid>0.125</rijsnelheid>\n"
    assert driving.count(line) == 1 and driving.replace(line, b"") == plain
    assert driving.index(line) == driving.index(b"</minimale_bestralingssterkte>\n") + len(b"</minimale_bestralingssterkte>\n")
    rt2 = host.RayTracer(init=False)
    rt2.set_route_dir(str(tmp_path) + os.sep)
    rt2.LoadRoute("driving")
    assert np.float32(rt2.driveSpeed) == np.float32(0.125) and rt2.lamps() == rt.lamps()
    rt2.LoadRoute("still")                      # absent: back to 0
    assert rt2.driveSpeed == 0.0
    rt.close(); rt2.close()
