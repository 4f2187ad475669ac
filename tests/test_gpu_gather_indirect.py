"""GPU: the one-bounce gather (uvrt_gather_indirect, uvrt_gather_indirect_rays, the source plane; csrc/uvrt_indirect.hip) against
its restatement (tests/gather_indirect_restate.py): every bit of `expected` and every ray, on the closed cube (where the answer is
exact), the edge scene and the whole room in both flavours, whatever the capacity and the split into ranges; what the call leaves
alone and what it forgets; the maps and the dose after uvrt_accumulate_expected and uvrt_shade; the refusals;
RayTracer::reflectance through host.py, uvrt_cli --reflect and a plan with PlanOptions::reflectance."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import gather_edge_scene as ge
import gather_indirect_restate as gi
import gather_restate as gr
from conftest import GLB, GOLDEN, ROOT, ROUTE
from sweep_restate import segment_duration

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "small-project-uv-robot-ray-tracer_amd", "uvrt_cli")
S = 4           # the direct gather's samples
S2 = 2          # the bounce's
N = 1 << 20
SEED = 7
RHO = 0.1
SEED_XOR = 0x85EBCA6B


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def new_ctx(pkg, scene, cap, dev=False):
    c = pkg.capi.Ctx(0, dev=dev)
    c.set_scene(scene.tris, scene.nodes, scene.triIdx)
    c.resize_rays(cap)
    return c


def test_the_closed_cube(pkg, orc):
    """S2 = 2 and 64, both `add` values: rays and plane equal the restatement, and the plane is a quarter of the source exactly"""
    cube = ge.HandScene(orc, gi.cube_tris())
    _, _, _, nn = gr.tri_normals(cube.tris)
    source = 0.5 * nn * 1000.0
    base = np.random.default_rng(1).uniform(0.0, 100.0, 12)
    c = new_ctx(pkg, cube, 12 * 64)
    assert not c.read_indirect_source().any(), "made zeroed"
    c.write_indirect_source(source)
    ptr, nbytes = c.device_ptr(8)
    assert ptr != 0 and nbytes == 12 * 8
    for s2 in (2, 64):
        want, rays, _, _ = gi.indirect(orc, cube, source, 0.25, s2, 7)
        assert np.array_equal(want, 0.25 * source)
        assert same(c.gather_indirect_rays(0.25, s2, 7), rays), s2
        c.write_expected(base)
        c.gather_indirect(0.25, s2, 7, add=0)
        assert same(c.read_expected(), want), s2
        c.write_expected(base)
        c.gather_indirect(0.25, s2, 7, add=1)
        assert same(c.read_expected(), base + want), s2
        assert same(c.read_indirect_source(), source)
    c.gather_indirect(0.0, 2, 7)
    assert not c.read_expected().any(), "rho = 0"
    c.set_scene(cube.tris, cube.nodes, cube.triIdx)
    assert not c.read_indirect_source().any(), "uvrt_set_scene zeroes the plane"
    c.sync()
    c.close()


def test_the_edge_scene(pkg, orc):
    """triangles without area, tiny, huge and sliver ones, a random positive source plane, S2 = 4; a sub-range that starts and
    ends with a hand-made triangle, in chunks"""
    scene = ge.edge_scene(orc)
    T = scene.T
    source = np.random.default_rng(2).uniform(0.5, 50.0, T)
    base = np.random.default_rng(3).uniform(0.0, 10.0, T)
    want, rays, h, _ = gi.indirect(orc, scene, source, 0.5, 4, 11, base=base)
    t = np.repeat(np.arange(T), 4)
    assert np.all(rays["dist"][np.isin(t, scene.no_area)] == 0) and (rays["dist"] == gi.MISS).sum() > 0.9 * rays.size
    assert (h >= 0).sum() > 0.1 * h.size
    for dev in (False, True):
        c = new_ctx(pkg, scene, T * 4, dev=dev)
        c.write_indirect_source(source)
        got_rays = c.gather_indirect_rays(0.5, 4, 11)
        assert same(got_rays, rays), "%d rays differ" % int((got_rays != rays).sum())
        c.write_expected(base)
        c.gather_indirect(0.5, 4, 11, add=1)
        got = c.read_expected()
        assert same(got, want), "%d entries differ" % int((got != want).sum())
        first, count = scene.sub_range
        c.resize_rays(4 * 7 + 1)
        c.write_expected(base)
        c.gather_indirect(0.5, 4, 11, add=1, first_tri=first, tri_count=count)
        part = c.read_expected()
        assert same(part[first:first + count], want[first:first + count]) and same(part[:first], base[:first])
        assert same(c.gather_indirect_rays(0.5, 4, 11, first, count), rays[4 * first:4 * (first + count)])
        c.sync()
        c.close()


@pytest.fixture(scope="module")
def place(orc, oscene, oroute):
    comp = orc.Computation(oscene, oroute["lamps"], N, oroute["lightHeight"], oroute["lightLength"], oroute["lightIntensity"])
    return comp.lamp_world_pos(oroute["lamps"][0])


@pytest.fixture(scope="module")
def room(orc, oscene, oroute, place):
    """flavour -> (the direct plane at S = 4, its bounce at S2 = 2, the rays, the hit triangles)"""
    out = {}
    for fl in (0, 1):
        direct, _, _ = gr.gather(orc, oscene, place, place, oroute["lightLength"], S, SEED, N, flavour=fl)
        st = {}
        ind, rays, h, _ = gi.indirect(orc, oscene, direct, RHO, S2, SEED ^ 1, flavour=fl, stats=st)
        out[fl] = (direct, ind, rays, h, st)
    return out


def test_the_room_equals_the_restatement(pkg, oscene, oroute, place, room):
    """The source is a snapshot of a direct gather; every bit of the bounce and every ray, in both flavours; the same bits from a
    capacity that gives several chunks with a ragged last one, and from two triangle ranges."""
    T, length = oscene.T, oroute["lightLength"]
    for fl in (0, 1):
        direct, ind, rays, h, st = room[fl]
        print("flavour %d: %.3f of the rays hit, deepest stack %d, %d triangles gain an estimate" % (
            fl, (h >= 0).mean(), st["max_stack"], int(((direct == 0) & (ind > 0)).sum())))
        assert st["max_stack"] > 8 and ((direct == 0) & (ind > 0)).sum() > 1000
        c = new_ctx(pkg, oscene, T * S)
        c.set_flavour(fl)
        c.gather_direct(place, place, length, S, SEED, N)
        c.indirect_source_from_expected()
        assert same(c.read_indirect_source(), direct) and same(c.read_expected(), direct)
        c.gather_indirect(RHO, S2, SEED ^ 1)
        got = c.read_expected()
        assert same(got, ind), "flavour %d: %d entries differ" % (fl, int((got != ind).sum()))
        got_rays = c.gather_indirect_rays(RHO, S2, SEED ^ 1)
        assert same(got_rays, rays), "flavour %d: %d rays differ" % (fl, int((got_rays != rays).sum()))
        assert same(c.read_expected(), ind) and same(c.read_indirect_source(), direct), "the ray hook changes no plane"
        # several chunks, the last one ragged
        c.resize_rays(1000 * S2 + 3)
        c.write_expected(np.zeros(T))
        c.gather_indirect(RHO, S2, SEED ^ 1)
        assert same(c.read_expected(), ind), "capacity 1000 S2 + 3"
        assert same(c.gather_indirect_rays(RHO, S2, SEED ^ 1, 500, 3001), rays[S2 * 500:S2 * 3501])
        # two ranges, the second added onto the direct plane
        c.write_expected(direct)
        c.gather_indirect(RHO, S2, SEED ^ 1, add=0, first_tri=0, tri_count=777)
        c.gather_indirect(RHO, S2, SEED ^ 1, add=1, first_tri=777, tri_count=T - 777)
        two = c.read_expected()
        assert same(two[:777], ind[:777]) and same(two[777:], direct[777:] + ind[777:]), "two ranges"
        c.sync()
        c.close()


def test_one_lit_triangle_shows_a_form_factor(pkg, orc, oscene, room):
    """a source plane with a single lit triangle: every other triangle's bounce is its share of rays that reach it"""
    T = oscene.T
    _, _, rays, h, _ = room[0]
    lit = int(np.bincount(h[h >= 0]).argmax())
    source = np.zeros(T)
    source[lit] = 1e6
    want = gi.reduce(oscene.tris, source, h, 1.0, S2)
    assert (want > 0).sum() >= 2 and want[lit] == 0.0
    c = new_ctx(pkg, oscene, T * S2)
    c.write_indirect_source(source)
    c.gather_indirect(1.0, S2, SEED ^ 1)
    assert same(c.read_expected(), want)
    c.close()


def test_what_the_call_leaves_and_what_it_forgets(pkg, orc, oscene, oroute, place, room):
    """source, variance, SEED and tempPhotonMap are untouched; the remembered gather survives the snapshot and the reads and is
    forgotten by the bounce; the maps, the dose and the colours after uvrt_accumulate_expected + uvrt_shade."""
    T, length = oscene.T, oroute["lightLength"]
    direct, ind, _, _, _ = room[0]
    n = 1 << 14
    scaled = np.float32(np.float32(oroute["lightIntensity"]) * np.float32(0.1))
    c = new_ctx(pkg, oscene, T * S)
    c.reset(True)
    c.seed = 0
    c.generate(place, length, 0, n)
    c.extend(n)
    counts, seed = c.read_counts(), c.seed
    assert counts.sum() > 0.9 * n
    c.set_gather_variance(1)
    c.gather_direct(place, place, length, S, SEED, N)
    var = c.read_variance()
    assert var.any()
    c.indirect_source_from_expected()
    c.read_indirect_source()
    c.gather_indirect_rays(RHO, S2, SEED ^ 1, 0, 16)
    extra, refined = c.gather_refine(0.5, 4, SEED + 100)          # still remembered
    assert refined > 0
    c.gather_direct(place, place, length, S, SEED, N)
    c.indirect_source_from_expected()
    var = c.read_variance()
    c.gather_indirect(RHO, S2, SEED ^ 1, add=1)
    with pytest.raises(pkg.capi.UvrtError, match="no remembered gather"):
        c.gather_refine(0.5, 4, SEED + 100)
    with pytest.raises(pkg.capi.UvrtError, match="last generate"):
        c.extend(n)
    total = direct + ind
    assert same(c.read_expected(), total) and same(c.read_indirect_source(), direct) and same(c.read_variance(), var)
    assert np.array_equal(c.read_counts(), counts) and c.seed == seed
    pm, mx = np.zeros(T), np.zeros(T)
    c.accumulate(0.0)               # the photon launch's counts, with no time: the maps stay zero
    c.accumulate_expected(60.0)
    gr.accumulate_expected(pm, mx, total, 60.0)
    c.shade(0, N, scaled, oroute["minDosage"], 0)
    dose = orc.compute_dosage(pm, oscene.tris, N, scaled)
    assert same(c.read_photon_map(0), pm), "photonMap"
    assert same(c.read_dosage(), dose)
    assert same(c.read_color(), orc.dosage_to_color(dose, oroute["minDosage"], False))
    c.sync()
    c.close()


def test_refusals(pkg, oscene, room):
    T = oscene.T
    Err = pkg.capi.UvrtError
    bare = pkg.capi.Ctx(0)
    for call in (lambda: bare.gather_indirect(RHO, S2, 1, 0, 0, 0), lambda: bare.gather_indirect_rays(RHO, S2, 1, 0, 0),
                 bare.indirect_source_from_expected, lambda: bare.read_indirect_source(0, 0), lambda: bare.write_indirect_source(np.zeros(1))):
        with pytest.raises(Err, match="no scene"):
            call()
    bare.close()
    direct = room[0][0]
    c = new_ctx(pkg, oscene, 4096)
    c.write_indirect_source(direct)
    c.gather_indirect(RHO, S2, 1, 0, 0, 2048)
    before = c.read_expected()
    assert before[:2048].any()
    for first, count in ((0, T + 1), (-1, 10), (T, 1)):
        with pytest.raises(Err, match="outside"):
            c.gather_indirect(RHO, S2, 1, 0, first, count)
        with pytest.raises(Err, match="outside"):
            c.gather_indirect_rays(RHO, S2, 1, first, count)
    for bad in (0, 1, 3, -2, 4098, 4097):
        with pytest.raises(Err, match="samples"):
            c.gather_indirect(RHO, bad, 1)
    c.resize_rays(3)
    with pytest.raises(Err, match="capacity"):
        c.gather_indirect(RHO, 4, 1)
    c.resize_rays(4096)
    for bad in (-0.1, 1.5, float("nan"), float("inf")):
        with pytest.raises(Err, match="reflectance"):
            c.gather_indirect(bad, S2, 1)
    for bad in (2, -1):
        with pytest.raises(Err, match="add"):
            c.gather_indirect(RHO, S2, 1, add=bad)
    prm = pkg.capi.IndirectParams(RHO, S2, 1, 0)
    prm.reserved[1] = 1
    L = pkg.capi.lib()
    assert L.uvrt_gather_indirect(c._h, pkg.capi.C.byref(prm), 0, 16) == -1 and b"reserved" in L.uvrt_last_error()
    assert L.uvrt_gather_indirect(c._h, None, 0, 1) == -1
    c.set_flavour(2)
    with pytest.raises(Err, match="flavours 0 and 1"):
        c.gather_indirect(RHO, S2, 1)
    c.set_flavour(0)
    with pytest.raises(Err, match="outside"):
        c.read_indirect_source(T - 1, 2)
    with pytest.raises(Err, match="outside"):
        c.write_indirect_source(np.zeros(2), T - 1)
    with pytest.raises(Err, match="0..8"):
        c.device_ptr(9)
    assert same(c.read_expected(), before) and same(c.read_indirect_source(), direct), "a refused call changes nothing"
    c.sync()
    c.close()


# ---------------------------------------------------------------- the host layer
LAMPS = 2
PHOTONS = 1 << 16


@pytest.fixture(scope="module")
def launches(orc, oscene, oroute):
    """the launches of one iteration over two positions driven at 0.1 m/s -- stop, stop, segment -- as RunLaunch runs them with
    gatherSamples = 4, reflectance = 0.1, reflectSamples = 2: (plane, duration) each, the launch counter as the gather's seed"""
    lamps = oroute["lamps"][:LAMPS]
    comp = orc.Computation(oscene, lamps, PHOTONS, oroute["lightHeight"], oroute["lightLength"], oroute["lightIntensity"])
    ends = [(comp.lamp_world_pos(l), comp.lamp_world_pos(l), l[2]) for l in lamps]
    ends.append((comp.lamp_world_pos(lamps[0]), comp.lamp_world_pos(lamps[1]), segment_duration(lamps[0], lamps[1], 0.1)))
    out = []
    for seed, (frm, to, duration) in enumerate(ends):
        direct, _, _ = gr.gather(orc, oscene, frm, to, comp.lightLength, S, seed, comp.photonsPerLight)
        total, _, _, _ = gi.indirect(orc, oscene, direct, RHO, S2, seed ^ SEED_XOR, base=direct)
        assert (total > direct).sum() > 1000
        out.append((total, duration))
    return out


def restated_route(orc, oscene, oroute, launches, speed):
    lamps = oroute["lamps"][:LAMPS]
    comp = orc.Computation(oscene, lamps, PHOTONS, oroute["lightHeight"], oroute["lightLength"], oroute["lightIntensity"])
    comp.reset()
    for k, (plane, duration) in enumerate(launches[:LAMPS + (1 if speed > 0 else 0)]):
        gr.accumulate_expected(comp.photonMap, comp.maxPhotonMap, plane, duration)
        if k < LAMPS:
            comp.photonMapSize += comp.photonsPerLight
    return comp


def test_raytracer_and_cli_reflect(pkg, orc, oscene, oroute, launches, tmp_path):
    """reflectance = 0.1, reflectSamples = 2 on gatherSamples = 4 through host.py and through uvrt_cli --gather 4 --reflect 0.1,2
    --dump, for stops and with a drive speed; reflectance 0 is the gather alone."""
    from uvrt_amd import host
    for speed in (0.0, 0.1):
        comp = restated_route(orc, oscene, oroute, launches, speed)
        want = comp.dose()
        rt = host.RayTracer(GLB, ROUTE, device=0)
        rt.set_lamps(rt.lamps()[:LAMPS])
        rt.photonCount = PHOTONS
        rt.maxIterations = 1
        rt.driveSpeed = speed
        rt.gatherSamples = S
        rt.reflectance = RHO
        rt.reflectSamples = S2
        rt.ResetDosageMap()
        rt.viewMode = host.VIEW_DOSAGE
        rt.ComputeDosageMap()
        rt.Shade()
        rt.Sync()
        got = (rt.read_dosage(), rt.ctx.read_photon_map(0), rt.ctx.read_photon_map(1), rt.ctx.seed, rt.photonMapSize)
        rt.close()
        assert same(got[1], comp.photonMap) and same(got[2], comp.maxPhotonMap), speed
        assert same(got[0], want), speed
        assert got[3] == 0 and got[4] == comp.photonMapSize
        f = tmp_path / "dose.f32"
        cmd = [CLI, "--room", GLB, "--route-dir", GOLDEN, "--route", "lange_route", "--lamps", str(LAMPS), "--photons", str(PHOTONS),
               "--iterations", "1", "--gather", str(S), "--reflect", "%g,%d" % (RHO, S2), "--dump", str(f)]
        if speed > 0:
            cmd += ["--drive-speed", str(speed)]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr + out.stdout
        assert np.array_equal(np.fromfile(f, dtype="<u4"), gr.bits(want)), "uvrt_cli, speed %g" % speed


def test_a_plan_captures_the_bounce(pkg, oscene, launches, tmp_path):
    """PlanOptions::reflectance: every column of the plan's exposure matrix is the restated plane of its launch, bounce included;
    uvrt_cli --plan-gather 4 --reflect 0.1,2 --plan-drive 0.1 plans the same durations and saves the bounce with the route"""
    from uvrt_amd import host
    rt = host.RayTracer(GLB, ROUTE, device=0)
    try:
        rt.set_lamps(rt.lamps()[:LAMPS])
        rt.photonCount = PHOTONS
        rt.maxIterations = 1
        rt.driveSpeed = 0.1
        d, rep = rt.PlanDurationsReflect(RHO, S2, gather_samples=S)
        assert rep["positions"] == LAMPS + 1 and rt.reflectance == 0.0 and rt.gatherSamples == 0
        for p, (plane, _) in enumerate(launches):
            got = rt.ctx.plan_read_exposure_expected(p)
            assert same(got, plane), "column %d: %d entries differ" % (p, int((got != plane).sum()))
        rt.EndPlan()
    finally:
        rt.close()
    assert d.size == LAMPS and d.sum() > 0
    shutil.copy(os.path.join(GOLDEN, "lange_route.xml"), tmp_path / "lange_route.xml")
    out = subprocess.run([CLI, "--room", GLB, "--route-dir", str(tmp_path), "--route", "lange_route", "--lamps", str(LAMPS), "--photons",
                          str(PHOTONS), "--iterations", "1", "--plan-gather", str(S), "--reflect", "%g,%d" % (RHO, S2), "--plan-drive", "0.1",
                          "--save-route", "planned"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "plan: one diffuse bounce, reflectance 0.1, 2 samples per triangle and launch\n" in out.stdout
    saved = host.RayTracer(init=False)
    saved.set_route_dir(str(tmp_path) + os.sep)
    saved.LoadRoute("planned")
    cli_d = np.array([l[2] for l in saved.lamps()], dtype=np.float32)
    assert (saved.gatherSamples, saved.reflectSamples, np.float32(saved.reflectance)) == (S, S2, np.float32(RHO))
    saved.close()
    assert np.array_equal(gr.bits(cli_d), gr.bits(d))
