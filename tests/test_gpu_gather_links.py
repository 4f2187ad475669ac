"""GPU: recorded hit links and the multi-bounce gather over them (uvrt_indirect_links_build, uvrt_read_indirect_links,
uvrt_gather_indirect_linked; csrc/uvrt_links.hip) against the restatement (tests/gather_links_restate.py) and, at one bounce,
against uvrt_gather_indirect on the same context: every link and every bit of `expected` on the closed cube, the edge scene and
the whole room, whatever the capacity and the cut into ranges; what the calls leave alone and what they forget; the links'
lifecycle; the refusals; RayTracer::reflectBounces through host.py, uvrt_cli --reflect-bounces and a plan."""
import os
import subprocess

import numpy as np
import pytest

import gather_edge_scene as ge
import gather_indirect_restate as gi
import gather_links_restate as gl
import gather_restate as gr
from conftest import GLB, GOLDEN, ROOT, ROUTE
from sweep_restate import segment_duration

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "small-project-uv-robot-ray-tracer_amd", "uvrt_cli")
N = 1 << 20
SEED = 7
RHO = 0.1
ROOM_S2 = 16


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def new_ctx(pkg, scene, cap, dev=False):
    c = pkg.capi.Ctx(0, dev=dev)
    c.set_scene(scene.tris, scene.nodes, scene.triIdx)
    c.resize_rays(cap)
    return c


@pytest.mark.parametrize("fl", (0, 1))
def test_the_closed_cube(pkg, orc, fl):
    """S2 = 2, 4 and 64: the links are the restatement's; one bounce is uvrt_gather_indirect's plane, every bit, for both `add`
    values; two and five bounces are the restatement's"""
    cube = ge.HandScene(orc, gi.cube_tris())
    source = 0.5 * gl.normals(cube.tris) * np.random.default_rng(5).uniform(1.0, 1000.0, 12)
    base = np.random.default_rng(1).uniform(0.0, 100.0, 12)
    c = new_ctx(pkg, cube, 12 * 64)
    c.set_flavour(fl)
    c.write_indirect_source(source)
    for s2 in (2, 4, 64):
        lk = gl.links(orc, cube, s2, 7, flavour=fl)
        c.indirect_links_build(s2, 7)
        assert c.indirect_links_info() == (s2, 7, fl)
        got = c.read_indirect_links()
        assert got.shape == (12, s2) and np.array_equal(got, lk), s2
        assert (lk < 0).sum() * 2 == lk.size
        for add in (0, 1):
            c.write_expected(base)
            c.gather_indirect(0.25, s2, 7, add=add)
            traced = c.read_expected()
            c.write_expected(base)
            c.gather_indirect_linked(0.25, 1, add=add)
            assert same(c.read_expected(), traced), (s2, add)
            assert same(traced, gl.linked(cube.tris, source, lk, 0.25, 1, base=base if add else None))
            for K in (2, 5):
                c.write_expected(base)
                c.gather_indirect_linked(0.25, K, add=add)
                assert same(c.read_expected(), gl.linked(cube.tris, source, lk, 0.25, K, base=base if add else None)), (s2, add, K)
        assert same(c.read_indirect_source(), source)
    c.sync()
    c.close()


def test_the_edge_scene(pkg, orc):
    """capacity 4 S2 + 1: the build runs many chunks of four triangles and a partial last one.  Triangles without area get 0
    and no link points at them; a range cut into two calls is one call."""
    scene = ge.edge_scene(orc)
    T, s2 = scene.T, 4
    source = np.random.default_rng(2).uniform(0.5, 50.0, T)
    base = np.random.default_rng(3).uniform(0.0, 10.0, T)
    lk = gl.links(orc, scene, s2, 11)
    assert T % 4 != 0 and (lk >= 0).sum() > 0.1 * lk.size
    assert not np.isin(lk, scene.no_area).any() and np.all(lk[scene.no_area] == -1)
    for dev in (False, True):
        c = new_ctx(pkg, scene, 4 * s2 + 1, dev=dev)
        c.write_indirect_source(source)
        c.indirect_links_build(s2, 11)
        got = c.read_indirect_links()
        assert np.array_equal(got, lk), "%d links differ" % int((got != lk).sum())
        first, count = scene.sub_range
        assert np.array_equal(c.read_indirect_links(first, count), lk[first:first + count])
        for K in (1, 4):
            want = gl.linked(scene.tris, source, lk, 0.5, K, base=base)
            c.write_expected(base)
            c.gather_indirect_linked(0.5, K, add=1)
            one = c.read_expected()
            assert same(one, want), "K = %d: %d entries differ" % (K, int((one != want).sum()))
            assert same(one[scene.no_area], base[scene.no_area]), "a triangle without area gets 0"
            c.write_expected(base)
            c.gather_indirect_linked(0.5, K, add=1, first_tri=first, tri_count=100)
            c.gather_indirect_linked(0.5, K, add=1, first_tri=first + 100, tri_count=count - 100)
            two = c.read_expected()
            assert same(two[first:first + count], want[first:first + count]) and same(two[:first], base[:first]), K
        c.write_expected(base)
        c.gather_indirect(0.5, s2, 11, add=1)
        assert same(c.read_expected(), gl.linked(scene.tris, source, lk, 0.5, 1, base=base)), "the traced bounce"
        c.sync()
        c.close()


@pytest.fixture(scope="module")
def place(orc, oscene, oroute):
    comp = orc.Computation(oscene, oroute["lamps"], N, oroute["lightHeight"], oroute["lightLength"], oroute["lightIntensity"])
    return comp.lamp_world_pos(oroute["lamps"][0])


@pytest.fixture(scope="module")
def room_links(orc, oscene):
    return gl.links(orc, oscene, ROOM_S2, SEED)


def test_the_room(pkg, oscene, oroute, place, room_links):
    """S2 = 16, the source a direct gather's plane at S = 16: every link is the restatement's; one bounce is
    uvrt_gather_indirect's plane, GPU against GPU, with the build in chunks of 1000 triangles and a ragged last one and in one
    chunk; three bounces are the restatement's"""
    T, length = oscene.T, oroute["lightLength"]
    print("%.3f of the room's links point at a triangle" % (room_links >= 0).mean())
    planes = []
    for cap in (1000 * ROOM_S2 + 3, T * ROOM_S2):
        c = new_ctx(pkg, oscene, T * ROOM_S2)
        c.gather_direct(place, place, length, 16, SEED, N)
        c.indirect_source_from_expected()
        direct = c.read_indirect_source()
        assert (direct > 0).sum() > 10000
        c.gather_indirect(RHO, ROOM_S2, SEED, add=1)
        traced = c.read_expected()
        c.resize_rays(cap)
        c.indirect_links_build(ROOM_S2, SEED)
        got = c.read_indirect_links()
        assert np.array_equal(got, room_links), "capacity %d: %d links differ" % (cap, int((got != room_links).sum()))
        c.write_expected(direct)
        c.gather_indirect_linked(RHO, 1, add=1)
        one = c.read_expected()
        assert same(one, traced), "capacity %d: %d entries differ from the traced bounce" % (cap, int((one != traced).sum()))
        c.gather_indirect_linked(RHO, 3)
        three = c.read_expected()
        want = gl.linked(oscene.tris, direct, room_links, RHO, 3)
        assert same(three, want), "K = 3: %d entries differ" % int((three != want).sum())
        assert ((direct == 0) & (three > 0)).sum() > 1000
        c.gather_indirect_linked(RHO, 3, add=0, first_tri=0, tri_count=777)
        c.gather_indirect_linked(RHO, 3, add=0, first_tri=777, tri_count=T - 777)
        assert same(c.read_expected(), want), "two ranges"
        planes.append(three)
        c.sync()
        c.close()
    assert same(planes[0], planes[1])


def test_one_bounce_is_the_traced_bounce_in_flavour_1_and_the_links_outlive_the_flavour(pkg, oscene, oroute, place):
    """links built in flavour 1 give flavour 1's traced bounce, also after uvrt_set_flavour(0) and in flavour 2, which traces
    no closest hits: the linked gather traces nothing; the info call keeps saying 1"""
    T, length = oscene.T, oroute["lightLength"]
    c = new_ctx(pkg, oscene, T * 4)
    c.set_flavour(1)
    c.gather_direct(place, place, length, 4, SEED, N)
    c.indirect_source_from_expected()
    c.gather_indirect(RHO, 4, SEED + 1)
    traced = c.read_expected()
    c.indirect_links_build(4, SEED + 1)
    lk = c.read_indirect_links()
    for fl in (1, 0, 2):
        c.set_flavour(fl)
        assert c.indirect_links_info() == (4, SEED + 1, 1)
        c.gather_indirect_linked(RHO, 1)
        assert same(c.read_expected(), traced), fl
        assert np.array_equal(c.read_indirect_links(), lk)
    with pytest.raises(pkg.capi.UvrtError, match="flavours 0 and 1"):
        c.indirect_links_build(4, SEED + 1)
    assert c.indirect_links_info() == (4, SEED + 1, 1) and np.array_equal(c.read_indirect_links(), lk)
    c.sync()
    c.close()


def test_what_the_calls_leave_and_what_they_forget(pkg, oscene, oroute, place):
    T, length = oscene.T, oroute["lightLength"]
    n = 1 << 14
    Err = pkg.capi.UvrtError
    c = new_ctx(pkg, oscene, T * 4)
    c.reset(True)
    c.seed = 0
    c.generate(place, length, 0, n)
    c.extend(n)
    counts, seed = c.read_counts(), c.seed
    assert counts.sum() > 0.9 * n
    c.set_gather_variance(1)
    c.gather_direct(place, place, length, 4, SEED, N)
    c.indirect_source_from_expected()
    source, var, expected = c.read_indirect_source(), c.read_variance(), c.read_expected()
    assert var.any() and source.any()
    c.indirect_links_build(4, SEED)
    assert c.seed == seed and np.array_equal(c.read_counts(), counts)
    assert same(c.read_indirect_source(), source) and same(c.read_variance(), var) and same(c.read_expected(), expected)
    with pytest.raises(Err, match="last generate"):               # the build drops the last generate
        c.extend(n)
    lk = c.read_indirect_links()
    extra, refined = c.gather_refine(0.5, 4, SEED + 100)          # ... and leaves the remembered gather
    assert refined > 0
    c.gather_direct(place, place, length, 4, SEED, N)
    c.gather_indirect_linked(RHO, 2, add=1)
    assert c.seed == seed and np.array_equal(c.read_counts(), counts)
    assert same(c.read_indirect_source(), source) and same(c.read_variance(), var) and np.array_equal(c.read_indirect_links(), lk)
    assert same(c.read_expected(), gl.linked(oscene.tris, source, lk, RHO, 2, base=expected))
    with pytest.raises(Err, match="no remembered gather"):
        c.gather_refine(0.5, 4, SEED + 100)
    # the linked gather leaves the last generate: generate -> linked gather -> extend counts what generate -> extend counts
    c.reset(True)
    c.seed = 0
    c.generate(place, length, 0, n)
    c.gather_indirect_linked(RHO, 2)
    c.extend(n)
    assert np.array_equal(c.read_counts(), counts) and c.seed == seed
    c.sync()
    c.close()


def test_lifecycle(pkg, orc):
    cube = ge.HandScene(orc, gi.cube_tris())
    Err = pkg.capi.UvrtError
    bare = pkg.capi.Ctx(0)
    assert bare.indirect_links_info() == (0, 0, 0)
    for call in (lambda: bare.indirect_links_build(4, 1), lambda: bare.gather_indirect_linked(RHO, 1, 0, 0, 0)):
        with pytest.raises(Err, match="no scene"):
            call()
    bare.close()
    c = new_ctx(pkg, cube, 12 * 8)
    assert c.indirect_links_info() == (0, 0, 0)
    with pytest.raises(Err, match="no links"):
        c.gather_indirect_linked(RHO, 1)
    c.indirect_links_build(4, 3)
    four = c.read_indirect_links()
    assert c.indirect_links_info() == (4, 3, 0) and np.array_equal(four, gl.links(orc, cube, 4, 3))
    c.indirect_links_build(8, 0x85EBCA6B)               # a second build replaces the first
    assert c.indirect_links_info() == (8, 0x85EBCA6B, 0)
    eight = c.read_indirect_links()
    assert eight.shape == (12, 8) and np.array_equal(eight, gl.links(orc, cube, 8, 0x85EBCA6B))
    for bad in (0, 1, 3, -2, 4098):
        with pytest.raises(Err, match="samples"):
            c.indirect_links_build(bad, 1)
    c.resize_rays(6)
    with pytest.raises(Err, match="capacity"):
        c.indirect_links_build(8, 1)
    c.resize_rays(12 * 8)
    prm = pkg.capi.LinksParams(4, 1)
    prm.reserved[1] = 1
    L = pkg.capi.lib()
    assert L.uvrt_indirect_links_build(c._h, pkg.capi.C.byref(prm)) == -1 and b"reserved" in L.uvrt_last_error()
    assert L.uvrt_indirect_links_build(c._h, None) == -1
    c.set_flavour(2)
    with pytest.raises(Err, match="flavours 0 and 1"):
        c.indirect_links_build(4, 1)
    c.set_flavour(0)
    assert c.indirect_links_info() == (8, 0x85EBCA6B, 0) and np.array_equal(c.read_indirect_links(), eight), "a refused build keeps the links"
    c.set_scene(cube.tris, cube.nodes, cube.triIdx)
    assert c.indirect_links_info() == (0, 0, 0), "uvrt_set_scene drops the links"
    with pytest.raises(Err, match="no links"):
        c.gather_indirect_linked(RHO, 1)
    with pytest.raises(Err, match="no links"):
        c.read_indirect_links()
    c.sync()
    c.close()


def test_refusals(pkg, orc):
    scene = ge.edge_scene(orc)
    T = scene.T
    Err = pkg.capi.UvrtError
    c = new_ctx(pkg, scene, T * 4)
    c.write_indirect_source(np.random.default_rng(2).uniform(0.5, 50.0, T))
    c.indirect_links_build(4, 11)
    c.gather_indirect_linked(0.5, 2)
    before = c.read_expected()
    assert before.any()
    lk = c.read_indirect_links()
    for first, count in ((0, T + 1), (-1, 10), (T, 1), (5, -1)):
        with pytest.raises(Err, match="outside"):
            c.gather_indirect_linked(0.5, 2, 0, first, count)
        with pytest.raises(Err, match="outside"):
            c.read_indirect_links(first, count)
    for bad in (0, -1, 17, 1 << 20):
        with pytest.raises(Err, match="bounces"):
            c.gather_indirect_linked(0.5, bad)
    for bad in (-0.1, 1.5, float("nan"), float("inf")):
        with pytest.raises(Err, match="reflectance"):
            c.gather_indirect_linked(bad, 2)
    for bad in (2, -1):
        with pytest.raises(Err, match="add"):
            c.gather_indirect_linked(0.5, 2, add=bad)
    L = pkg.capi.lib()
    for k in range(3):
        prm = pkg.capi.LinkedParams(0.5, 2, 0)
        prm.reserved[k] = 1
        assert L.uvrt_gather_indirect_linked(c._h, pkg.capi.C.byref(prm), 0, 16) == -1 and b"reserved" in L.uvrt_last_error()
    assert L.uvrt_gather_indirect_linked(c._h, None, 0, 1) == -1
    assert L.uvrt_read_indirect_links(c._h, None, 0, 1) == -1
    assert L.uvrt_indirect_links_info(c._h, None) == -1
    assert same(c.read_expected(), before) and np.array_equal(c.read_indirect_links(), lk), "a refused call changes nothing"
    c.gather_indirect_linked(0.5, 2, 0, T, 0)           # an empty range at the end is a range
    c.gather_indirect_linked(1.0, 16, 0, 0, 0)
    assert same(c.read_expected(), before)
    c.sync()
    c.close()


# ---------------------------------------------------------------- the host layer
LAMPS = 2
PHOTONS = 1 << 16
S = 4           # the direct gather's samples
S2 = 2          # the bounce's
SEED_XOR = 0x85EBCA6B


@pytest.fixture(scope="module")
def directs(orc, oscene, oroute):
    """the direct planes of one iteration over two positions driven at 0.1 m/s -- stop, stop, segment -- as RunLaunch gathers them
    with gatherSamples = 4: (plane, duration) each, the launch counter as the gather's seed"""
    lamps = oroute["lamps"][:LAMPS]
    comp = orc.Computation(oscene, lamps, PHOTONS, oroute["lightHeight"], oroute["lightLength"], oroute["lightIntensity"])
    ends = [(comp.lamp_world_pos(l), comp.lamp_world_pos(l), l[2]) for l in lamps]
    ends.append((comp.lamp_world_pos(lamps[0]), comp.lamp_world_pos(lamps[1]), segment_duration(lamps[0], lamps[1], 0.1)))
    return [(gr.gather(orc, oscene, frm, to, comp.lightLength, S, seed, comp.photonsPerLight)[0], duration)
            for seed, (frm, to, duration) in enumerate(ends)]


@pytest.fixture(scope="module")
def host_links(orc, oscene):
    return gl.links(orc, oscene, S2, gl.LINK_SEED)


def restated_route(orc, oscene, oroute, planes):
    """the maps after one iteration whose launches leave `planes` ((plane, duration): stop, stop, segment)"""
    lamps = oroute["lamps"][:LAMPS]
    comp = orc.Computation(oscene, lamps, PHOTONS, oroute["lightHeight"], oroute["lightLength"], oroute["lightIntensity"])
    comp.reset()
    for k, (plane, duration) in enumerate(planes):
        gr.accumulate_expected(comp.photonMap, comp.maxPhotonMap, plane, duration)
        if k < LAMPS:
            comp.photonMapSize += comp.photonsPerLight
    return comp


def run_raytracer(K):
    from uvrt_amd import host
    rt = host.RayTracer(GLB, ROUTE, device=0)
    rt.set_lamps(rt.lamps()[:LAMPS])
    rt.photonCount = PHOTONS
    rt.maxIterations = 1
    rt.driveSpeed = 0.1
    rt.gatherSamples = S
    rt.reflectance = RHO
    rt.reflectSamples = S2
    rt.reflectBounces = K
    rt.ResetDosageMap()
    rt.viewMode = host.VIEW_DOSAGE
    rt.ComputeDosageMap()
    rt.Shade()
    rt.Sync()
    got = (rt.read_dosage(), rt.ctx.read_photon_map(0), rt.ctx.read_photon_map(1), rt.ctx.seed, rt.photonMapSize,
           rt.ctx.indirect_links_info())
    rt.close()
    return got


def test_raytracer_and_cli_bounces(pkg, orc, oscene, oroute, directs, host_links, tmp_path):
    """reflectBounces = 1 and 3 on gatherSamples = 4, reflectance = 0.1, reflectSamples = 2 over two stops and the drive between
    them: the restated route; uvrt_cli --reflect-bounces 3 --dump gives host.py's dose; reflectBounces = 0 is the traced bounce"""
    doses = {}
    for K in (1, 3):
        comp = restated_route(orc, oscene, oroute, [(gl.linked(oscene.tris, d, host_links, RHO, K, base=d), t) for d, t in directs])
        got = run_raytracer(K)
        assert same(got[1], comp.photonMap) and same(got[2], comp.maxPhotonMap), K
        assert same(got[0], comp.dose()), K
        assert got[3] == 0 and got[4] == comp.photonMapSize and got[5] == (S2, gl.LINK_SEED, 0)
        doses[K] = got[0]
    assert not same(doses[1], doses[3])
    f = tmp_path / "dose.f32"
    cmd = [CLI, "--room", GLB, "--route-dir", GOLDEN, "--route", "lange_route", "--lamps", str(LAMPS), "--photons", str(PHOTONS),
           "--iterations", "1", "--gather", str(S), "--reflect", "%g,%d" % (RHO, S2), "--reflect-bounces", "3", "--drive-speed", "0.1",
           "--dump", str(f)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr + out.stdout
    assert np.array_equal(np.fromfile(f, dtype="<u4"), gr.bits(doses[3])), "uvrt_cli"
    # 0 bounces: the bounce traced per launch, as before
    comp = restated_route(orc, oscene, oroute, [(gi.indirect(orc, oscene, d, RHO, S2, seed ^ SEED_XOR, base=d)[0], t)
                                                for seed, (d, t) in enumerate(directs)])
    got = run_raytracer(0)
    assert same(got[0], comp.dose()) and same(got[1], comp.photonMap) and got[5] == (0, 0, 0)


def test_a_plan_captures_the_bounces(pkg, oscene, directs, host_links):
    """PlanOptions::reflectBounces = 2: every column of the plan's exposure matrix is the restated plane of its launch"""
    from uvrt_amd import host
    rt = host.RayTracer(GLB, ROUTE, device=0)
    try:
        rt.set_lamps(rt.lamps()[:LAMPS])
        rt.photonCount = PHOTONS
        rt.maxIterations = 1
        rt.driveSpeed = 0.1
        d, rep = rt.PlanDurationsReflect(RHO, S2, gather_samples=S, reflect_bounces=2)
        assert rep["positions"] == LAMPS + 1 and rt.reflectance == 0.0 and rt.reflectBounces == 0
        for p, (direct, _) in enumerate(directs):
            want = gl.linked(oscene.tris, direct, host_links, RHO, 2, base=direct)
            got = rt.ctx.plan_read_exposure_expected(p)
            assert same(got, want), "column %d: %d entries differ" % (p, int((got != want).sum()))
        rt.EndPlan()
    finally:
        rt.close()
    assert d.size == LAMPS and d.sum() > 0
