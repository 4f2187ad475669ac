"""No GPU: the host-only parts of the one-bounce gather (include/uvrt.h "one diffuse bounce") -- the symbols in both
libraries and in the bindings, the layout of uvrt_indirect_params against a C compiler's, the refusals that need no device,
route files with and without the tags, the CLI's and the binding's refusals -- and the estimator itself
(tests/gather_indirect_restate.py over the oracle): the closed cube, where it is exact, and the room.

Measured by test_the_room_gains_the_triangles_no_lamp_sees (position 0 of lange_route.xml, direct S = 16 seed 0 N = 2^21; S2 = 8,
seed 1, rho = 0.1): 0 self-hits, 36.0 % of the samples miss, 5 of 358 928 samples fall back to the disc's centre, the oracle's
stack reaches 14 entries, 13 825 of the 18 804 triangles without a direct estimate become positive."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gather_indirect_restate as gi
import gather_restate as gr
from conftest import GLB, GOLDEN, ROOT
from plan_options_pin import check_plan_option

NEW = ("uvrt_closest_hits", "uvrt_indirect_source_from_expected", "uvrt_read_indirect_source", "uvrt_write_indirect_source",
       "uvrt_gather_indirect", "uvrt_gather_indirect_rays")
f32 = np.float32


class HandScene:
    def __init__(self, orc, tris):
        self.tris = np.ascontiguousarray(tris, dtype=f32)
        self.T = self.tris.shape[0]
        self.nodes, self.triIdx = orc.build_bvh(self.tris)


def test_symbols_are_bound_and_resolve_in_both_libraries(pkg):
    names = [name for name, _, _ in pkg.capi.SYMBOLS]
    for n in NEW:
        assert names.count(n) == 1
        for path in (pkg.capi.LIB_PATH, pkg.capi.LIB_DEV_PATH):
            assert hasattr(C.CDLL(path), n), (path, n)
        for dev in (False, True):
            assert getattr(pkg.capi.lib(dev), n).restype is C.c_int
    by_name = {n: a for n, _, a in pkg.capi.SYMBOLS}
    assert len(by_name["uvrt_closest_hits"]) == 5 and by_name["uvrt_closest_hits"][2] is C.c_int64
    assert len(by_name["uvrt_gather_indirect"]) == 4 and len(by_name["uvrt_gather_indirect_rays"]) == 5
    for m in ("closest_hits", "indirect_source_from_expected", "read_indirect_source", "write_indirect_source", "gather_indirect",
              "gather_indirect_rays"):
        assert hasattr(pkg.capi.Ctx, m)
    from uvrt_amd import host
    check_plan_option(host, "reflectance", C.c_float, 0.0)
    check_plan_option(host, "reflect_samples", C.c_int, 16)
    assert hasattr(host.RayTracer, "PlanDurationsReflect")


def test_struct_layout_matches_the_c_compiler(pkg, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text("""#include <stddef.h>
#include <stdio.h>
#include "uvrt.h"
int main(void)
{
    printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(uvrt_indirect_params), offsetof(uvrt_indirect_params, reflectance),
           offsetof(uvrt_indirect_params, samples), offsetof(uvrt_indirect_params, seed), offsetof(uvrt_indirect_params, add),
           offsetof(uvrt_indirect_params, reserved));
    return 0;
}
""")
    exe = tmp_path / "layout"
    subprocess.run([os.environ.get("CC", "cc"), "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    line = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")[0]
    P = pkg.capi.IndirectParams
    assert [int(v) for v in line.split()] == [C.sizeof(P), P.reflectance.offset, P.samples.offset, P.seed.offset, P.add.offset,
                                              P.reserved.offset] == [24, 0, 4, 8, 12, 16]


def test_null_arguments_are_refused_without_a_gpu(pkg):
    buf = np.full(16, 7.0, dtype=np.float64)
    tri = np.full(4, 7, dtype=np.int32)
    dist = np.full(4, 7, dtype=np.float32)
    rays = np.zeros(4, dtype=pkg.capi.RAY_DT)
    prm = pkg.capi.IndirectParams(0.25, 4, 1, 0)
    for dev in (False, True):
        L = pkg.capi.lib(dev)
        calls = (("uvrt_closest_hits", lambda: L.uvrt_closest_hits(None, rays.ctypes.data, 4, dist.ctypes.data, tri.ctypes.data)),
                 ("uvrt_closest_hits", lambda: L.uvrt_closest_hits(None, None, 4, None, None)),
                 ("uvrt_indirect_source_from_expected", lambda: L.uvrt_indirect_source_from_expected(None)),
                 ("uvrt_read_indirect_source", lambda: L.uvrt_read_indirect_source(None, buf.ctypes.data, 0, 4)),
                 ("uvrt_write_indirect_source", lambda: L.uvrt_write_indirect_source(None, buf.ctypes.data, 0, 4)),
                 ("uvrt_gather_indirect", lambda: L.uvrt_gather_indirect(None, C.byref(prm), 0, 4)),
                 ("uvrt_gather_indirect", lambda: L.uvrt_gather_indirect(None, None, 0, 4)),
                 ("uvrt_gather_indirect_rays", lambda: L.uvrt_gather_indirect_rays(None, C.byref(prm), 0, 1, buf.ctypes.data)),
                 ("uvrt_gather_indirect_rays", lambda: L.uvrt_gather_indirect_rays(None, None, 0, 1, None)))
        for name, call in calls:
            assert call() == -1 and name.encode() in L.uvrt_last_error(), name          # UVRT_ERR_INVALID
    assert np.all(buf == 7.0) and np.all(tri == 7) and np.all(dist == 7)


def test_route_file_keeps_the_reflectance(pkg, tmp_path):
    """<reflectance> and <reflect_samples> are written only when reflectance > 0, after the gather tags; a route saved at 0 is
    byte for byte what the tag-less writer saved; absent tags load as 0 / 16."""
    from uvrt_amd import host
    golden = open(os.path.join(GOLDEN, "lange_route.xml"), "rb").read()
    rt = host.RayTracer(init=False)
    rt.set_route_dir(GOLDEN + os.sep)
    rt.LoadRoute("lange_route")
    assert rt.reflectance == 0.0 and rt.reflectSamples == 16
    rt.set_route_dir(str(tmp_path) + os.sep)
    rt.SaveRoute("photons")
    assert (tmp_path / "photons.xml").read_bytes() == golden
    rt.reflectSamples = 8                        # without a reflectance: no bounce, no tag
    rt.gatherSamples = 16
    rt.SaveRoute("direct")
    direct = (tmp_path / "direct.xml").read_bytes()
    assert b"reflect" not in direct
    rt.reflectance = 0.125
    rt.gatherSampling = 1
    rt.SaveRoute("bounce")
    bounce = (tmp_path / "bounce.xml").read_bytes()
    lines = b"    <reflectance>0.125</reflectance>\n    <reflect_samples>8</reflect_samples>\n"
    assert bounce.count(lines) == 1 and bounce.replace(lines, b"").replace(b"    <gather_sampling>1</gather_sampling>\n", b"") == direct
    assert bounce.index(b"<gather_sampling>") < bounce.index(lines) < bounce.index(b"<lamp_lengte>")
    rt2 = host.RayTracer(init=False)
    rt2.set_route_dir(str(tmp_path) + os.sep)
    rt2.LoadRoute("bounce")
    assert rt2.reflectance == 0.125 and rt2.reflectSamples == 8 and rt2.gatherSamples == 16 and rt2.lamps() == rt.lamps()
    rt2.SaveRoute("again")
    assert (tmp_path / "again.xml").read_bytes() == bounce
    rt2.LoadRoute("direct")                     # absent: back to 0 / 16
    assert rt2.reflectance == 0.0 and rt2.reflectSamples == 16 and rt2.gatherSamples == 16
    rt.close(); rt2.close()


def test_the_binding_refuses_a_bounce_it_cannot_run(pkg):
    from uvrt_amd import host
    rt = host.RayTracer(init=False)
    try:
        for rho, kw in ((0.1, {}), (0.1, dict(gather_samples=0))):
            with pytest.raises(ValueError, match="gather_samples"):
                rt.PlanDurationsReflect(rho, **kw)
        for rho in (-0.1, 1.5, float("nan")):
            with pytest.raises(ValueError, match="reflectance"):
                rt.PlanDurationsReflect(rho, gather_samples=16)
        with pytest.raises(ValueError, match="gather_confidence"):
            rt.PlanDurationsReflect(0.1, gather_samples=16, gather_confidence=2.0)
        for s2 in (0, 1, 3, 4098, -2):
            with pytest.raises(ValueError, match="reflect_samples"):
                rt.PlanDurationsReflect(0.1, s2, gather_samples=16)
        with pytest.raises(TypeError, match="unknown arguments"):
            rt.PlanDurationsReflect(0.1, gather_sample=16)
    finally:
        rt.close()


def test_cli_refuses_a_bounce_without_a_gather(pkg):
    cli = os.path.join(os.path.dirname(pkg.capi.LIB_PATH), "uvrt_cli")
    base = [cli, "--room", GLB, "--route-dir", GOLDEN, "--route", "lange_route"]
    for extra in (["--reflect", "0.1"], ["--plan", "50", "--reflect", "0.1"], ["--reflect", "0.1", "--gather", "0"],
                  ["--drive-speed", "0.1", "--reflect", "0.1,8"],
                  ["--plan-gather", "16", "--plan-confidence", "2", "--reflect", "0.1"],
                  ["--gather", "16", "--reflect", "-0.1"], ["--gather", "16", "--reflect", "1.5"], ["--gather", "16", "--reflect", "nan"],
                  ["--gather", "16", "--reflect", "tenth"], ["--gather", "16", "--reflect", "0.1x"], ["--gather", "16", "--reflect", "0.1,"],
                  ["--gather", "16", "--reflect", "0.1,3"], ["--gather", "16", "--reflect", "0.1,0"], ["--gather", "16", "--reflect", "0.1,4098"],
                  ["--plan-gather", "16", "--reflect", "0.1,8x"]):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2, (extra, r.stdout, r.stderr)
        assert "--reflect" in r.stderr, (extra, r.stderr)
    r = subprocess.run(base + ["--gather", "16", "--reflect"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2


# ---------------------------------------------------------------- the estimator
def test_the_rng_of_the_restatement_is_the_oracles(orc):
    gr.check_rng(orc, 256)


@pytest.mark.parametrize("S2", (2, 4, 64, 1024))
def test_the_closed_cube_returns_a_quarter_of_its_source_exactly(orc, S2):
    """Inside a closed cube whose every triangle carries the same irradiance (source = 0.5 nn x 1000) a quarter of it comes
    back at rho = 0.25, exactly: half of the samples leave the outer face and miss, every other one hits a lit triangle."""
    cube = HandScene(orc, gi.cube_tris())
    _, _, _, nn = gr.tri_normals(cube.tris)
    assert np.all(nn == 16.0)
    source = 0.5 * nn * 1000.0
    ind, rays, h, fell_back = gi.indirect(orc, cube, source, 0.25, S2, 7)
    t = np.repeat(np.arange(12), S2)
    assert not fell_back.any() and not (h == t).any()
    assert (h < 0).sum() * 2 == h.size
    assert np.all(rays["dist"] == gi.MISS)
    assert np.array_equal(ind, 0.25 * source)


def test_what_is_not_traced(orc):
    """a triangle without area -- a point, and one whose edges vanish in f32 -- shoots nothing: dir = (0, 1, 0), tmax = 0"""
    rows = gi.cube_tris()
    rows = np.concatenate([rows, np.zeros((2, 16), dtype=f32)])
    rows[12, 0:3] = rows[12, 4:7] = rows[12, 8:11] = (1.0, 1.0, 1.0)             # a point
    rows[13, 0:3], rows[13, 4:7], rows[13, 8:11] = (1, 1, 1), (1 + 1e-30, 1, 1), (1, 1, 1 + 1e-30)      # collapses in f32
    r, _ = gi.rays(orc, rows, 4, 3)
    for t in (12, 13):
        rt = r[4 * t:4 * t + 4]
        assert np.all(rt["dist"] == 0) and np.all(rt["diry"] == 1) and np.all(rt["dirx"] == 0) and np.all(rt["dirz"] == 0)
    assert np.all(r[:48]["dist"] == gi.MISS)
    scene = HandScene(orc, rows)
    ind, _, h, _ = gi.indirect(orc, scene, np.full(14, 5.0), 0.5, 4, 3)
    assert np.all(ind[12:] == 0.0) and np.all(h[48:] == -1)


@pytest.fixture(scope="module")
def room(orc, oscene, oroute):
    lamp = oroute["lamps"][0]
    lp = (f32(lamp[0]), f32(f32(oscene.floorHeight) + f32(oroute["lightHeight"])), f32(lamp[1]))
    direct, _, _ = gr.gather(orc, oscene, lp, lp, oroute["lightLength"], 16, 0, 1 << 21)
    st = {}
    ind, rays, h, fell_back = gi.indirect(orc, oscene, direct, 0.1, 8, 1, stats=st)
    return direct, ind, h, fell_back, st


def test_the_room_gains_the_triangles_no_lamp_sees(oscene, room):
    direct, ind, h, fell_back, st = room
    t = np.repeat(np.arange(oscene.T), 8)
    self_hits, miss, gained = int((h == t).sum()), float((h < 0).mean()), int(((direct == 0) & (ind > 0)).sum())
    print("self-hits %d, %.1f %% miss, %d of %d fall back, stack %d, %d of %d zero-direct triangles gained, indirect / direct %.3f"
          % (self_hits, 100 * miss, int(fell_back.sum()), h.size, st["max_stack"], gained, int((direct == 0).sum()),
             ind.sum() / direct.sum()))
    assert self_hits <= 0.001 * h.size
    assert fell_back.sum() <= 0.0001 * h.size
    assert gained >= 10000
    assert st["max_stack"] > 8, "the rays must leave the LDS stack rows (PS6 = 8)"
    assert np.all(ind >= 0) and np.all(np.isfinite(ind))
