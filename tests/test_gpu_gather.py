"""GPU: the per-triangle direct gather (uvrt_gather_direct, uvrt_accumulate_expected; csrc/uvrt_occlude.hip) against its
restatement (tests/gather_restate.py): every bit of the expected plane over the whole room at a stop and on a segment, whatever
the capacity and the split into ranges; the maps and the dose after uvrt_accumulate_expected and uvrt_shade; photon launches
and gather launches in one map; the refusals; RayTracer::gatherSamples through host.py and through uvrt_cli."""
import os
import subprocess

import numpy as np
import pytest

import gather_restate as gr
from conftest import GLB, GOLDEN, ROOT, ROUTE
from sweep_restate import segment_duration

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "small-project-uv-robot-ray-tracer_amd", "uvrt_cli")
S = 4
N = 1 << 20
SEED = 7


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def new_ctx(pkg, oscene, cap, dev=False):
    c = pkg.capi.Ctx(0, dev=dev)
    c.set_scene(oscene.tris, oscene.nodes, oscene.triIdx)
    c.resize_rays(cap)
    return c


@pytest.fixture(scope="module")
def places(orc, oscene, oroute):
    comp = orc.Computation(oscene, oroute["lamps"], N, oroute["lightHeight"], oroute["lightLength"], oroute["lightIntensity"])
    return [comp.lamp_world_pos(l) for l in oroute["lamps"][:3]]


@pytest.fixture(scope="module")
def restated(orc, oscene, oroute, places):
    """(from, to, flavour) -> (expected, rays, occluded) of the whole room at S = 4"""
    out = {}
    for tag, frm, to, fl in (("stop", places[0], places[0], 0), ("segment", places[0], places[1], 0), ("stop fl1", places[0], places[0], 1)):
        out[tag] = (frm, to, fl) + gr.gather(orc, oscene, frm, to, oroute["lightLength"], S, SEED, N, flavour=fl)
    return out


def test_gather_equals_the_restatement(pkg, oscene, oroute, restated):
    """Every bit of `expected` and every occlusion byte, at a stop and on a segment; the same bits from a capacity that gives
    several chunks with a ragged last one, and from two triangle ranges."""
    T, length = oscene.T, oroute["lightLength"]
    for tag, (frm, to, fl, want, rays, occ) in restated.items():
        visible = 1.0 - occ.mean()
        print("%s: %.3f of the samples see the lamp, %d triangles with an estimate" % (tag, visible, int((want > 0).sum())))
        assert visible >= 0.2 and occ.mean() >= 0.2
        assert np.isfinite(want).all() and (want > 0).sum() > 0.3 * T
        c = new_ctx(pkg, oscene, T * S)
        c.set_flavour(fl)
        c.gather_direct(frm, to, length, S, SEED, N)
        got = c.read_expected()
        assert same(got, want), "%s: %d entries differ" % (tag, int((got != want).sum()))
        assert np.array_equal(c.occluded(rays), occ), tag
        ptr, nbytes = c.device_ptr(6)
        assert ptr != 0 and nbytes == T * 8
        # a range writes its entries only
        c.set_scene(oscene.tris, oscene.nodes, oscene.triIdx)
        assert not c.read_expected().any(), "uvrt_set_scene zeroes the plane"
        c.gather_direct(frm, to, length, S, SEED, N, 100, 150)
        part = c.read_expected()
        assert same(part[100:250], want[100:250]) and not part[:100].any() and not part[250:].any()
        c.close()
        # several chunks, the last one ragged
        c = new_ctx(pkg, oscene, 1000 * S + 3)
        c.set_flavour(fl)
        c.gather_direct(frm, to, length, S, SEED, N)
        assert same(c.read_expected(), want), tag + ", capacity 1000 S + 3"
        # two ranges (the second in chunks again)
        c.set_scene(oscene.tris, oscene.nodes, oscene.triIdx)
        c.gather_direct(frm, to, length, S, SEED, N, 0, 777)
        c.gather_direct(frm, to, length, S, SEED, N, 777, T - 777)
        assert same(c.read_expected(), want), tag + ", two ranges"
        c.sync()
        c.close()


def test_accumulate_expected_and_shade(pkg, orc, oscene, oroute, restated):
    """uvrt_accumulate_expected is accumulate.cl on the plane; uvrt_shade then works unchanged: maps and dose bit for bit."""
    T, length = oscene.T, oroute["lightLength"]
    scaled = np.float32(np.float32(oroute["lightIntensity"]) * np.float32(0.1))
    pm, mx = np.zeros(T), np.zeros(T)
    c = new_ctx(pkg, oscene, T * S)
    c.reset(True)
    for tag, step in (("stop", 60.0), ("segment", 7.25)):
        frm, to, _, want, _, _ = restated[tag]
        c.gather_direct(frm, to, length, S, SEED, N)
        c.accumulate_expected(step)
        gr.accumulate_expected(pm, mx, want, step)
        assert not c.read_expected().any(), "the plane is zeroed like tempPhotonMap"
        assert same(c.read_photon_map(0), pm) and same(c.read_photon_map(1), mx), tag
        c.shade(0, N, scaled, oroute["minDosage"], 0)
        dose = orc.compute_dosage(pm, oscene.tris, N, scaled)
        assert same(c.read_dosage(), dose), tag
        assert same(c.read_color(), orc.dosage_to_color(dose, oroute["minDosage"], False)), tag
    assert (dose > 0).sum() > 0.3 * T
    # a part of the triangles only
    frm, to, _, want, _, _ = restated["stop"]
    c.gather_direct(frm, to, length, S, SEED, N)
    c.accumulate_expected(2.0, 1000)
    gr.accumulate_expected(pm[:1000], mx[:1000], want[:1000], 2.0)
    rest = c.read_expected()
    assert same(c.read_photon_map(0), pm) and same(c.read_photon_map(1), mx)
    assert not rest[:1000].any() and same(rest[1000:], want[1000:])
    c.close()


def test_photon_launches_and_gather_launches_share_the_maps(pkg, orc, oscene, oroute, places, restated):
    """photons (generate -> extend -> accumulate, its accumulate deferred) then a gather launch, and the other way round: the
    maps see launch order; SEED and tempPhotonMap are not the gather's business."""
    T, length = oscene.T, oroute["lightLength"]
    n = 1 << 16
    scaled = np.float32(np.float32(oroute["lightIntensity"]) * np.float32(0.1))
    frm, to, _, want, _, _ = restated["segment"]
    rays, seed1 = orc.generate(0, n, places[2], length, 0)
    counts = np.zeros(T, dtype=np.int32)
    orc.extend(counts, oscene.tris, rays, oscene.nodes, oscene.triIdx)
    for order in ("photons first", "gather first", "gather between extend and accumulate"):
        pm, mx, tmp = np.zeros(T), np.zeros(T), counts.copy()
        c = new_ctx(pkg, oscene, T * S)
        c.reset(True)
        c.seed = 0
        if order == "gather first":
            c.gather_direct(frm, to, length, S, SEED, N)
            c.accumulate_expected(30.0)
            gr.accumulate_expected(pm, mx, want, 30.0)
            assert c.seed == 0
        c.generate(places[2], length, 0, n)
        c.extend(n)
        if order == "gather between extend and accumulate":
            c.gather_direct(frm, to, length, S, SEED, N)
            assert np.array_equal(c.read_counts(), counts) and c.seed == seed1
        c.accumulate(60.0)
        orc.accumulate(pm, mx, tmp, 60.0)
        if order == "photons first":
            c.gather_direct(frm, to, length, S, SEED, N)
        if order != "gather first":
            c.accumulate_expected(30.0)
            gr.accumulate_expected(pm, mx, want, 30.0)
        c.shade(0, n, scaled, oroute["minDosage"], 0)
        c.sync()
        assert c.seed == seed1, order
        assert same(c.read_photon_map(0), pm) and same(c.read_photon_map(1), mx), order
        assert same(c.read_dosage(), orc.compute_dosage(pm, oscene.tris, n, scaled)), order
        assert not c.read_counts().any(), order
        c.close()


def test_refusals(pkg, oscene, oroute, places, restated):
    T, length = oscene.T, oroute["lightLength"]
    lp = places[0]
    bare = pkg.capi.Ctx(0)
    with pytest.raises(pkg.capi.UvrtError, match="no scene"):
        bare.gather_direct(lp, lp, length, S, SEED, N, 0, 0)
    bare.close()
    c = new_ctx(pkg, oscene, 4096)
    c.gather_direct(lp, lp, length, S, SEED, N, 0, 2048)
    before = c.read_expected()
    assert before[:2048].any()
    Err = pkg.capi.UvrtError
    with pytest.raises(Err, match="outside"):
        c.gather_direct(lp, lp, length, S, SEED, N, 0, T + 1)
    with pytest.raises(Err, match="outside"):
        c.gather_direct(lp, lp, length, S, SEED, N, -1, 10)
    with pytest.raises(Err, match="outside"):
        c.gather_direct(lp, lp, length, S, SEED, N, T, 1)
    for bad in (0, -1, 4097):
        with pytest.raises(Err, match="samples"):
            c.gather_direct(lp, lp, length, bad, SEED, N)
    c.resize_rays(3)
    with pytest.raises(Err, match="capacity"):
        c.gather_direct(lp, lp, length, 4, SEED, N)
    c.resize_rays(4096)
    for bad in (0, -5):
        with pytest.raises(Err, match="photons_equiv"):
            c.gather_direct(lp, lp, length, S, SEED, bad)
    c.set_flavour(2)
    with pytest.raises(Err, match="flavours 0 and 1"):
        c.gather_direct(lp, lp, length, S, SEED, N)
    c.set_flavour(0)
    assert pkg.capi.lib().uvrt_gather_direct(c._h, None, 0, 1) == -1
    with pytest.raises(Err, match="tri_count"):
        c.accumulate_expected(1.0, T + 1)
    with pytest.raises(Err, match="outside"):
        c.read_expected(T - 1, 2)
    assert same(c.read_expected(), before), "a refused call changes nothing"
    # the last generate is dropped
    c.generate(lp, length, 0, 1024)
    c.gather_direct(lp, lp, length, S, SEED, N, 0, 16)
    with pytest.raises(Err, match="last generate"):
        c.extend(1024)
    with pytest.raises(Err, match="last generate"):
        c.read_rays(0, 1)
    c.generate(lp, length, 0, 1024)
    c.extend(1024)
    c.sync()
    c.close()


def restated_route(orc, oscene, oroute, lamps, photon_count, iterations, samples, speed):
    """RayTracer with gatherSamples > 0: per iteration every stop, then (driving) every segment, each a gather launch with the
    launch counter as its seed, followed by accumulate.cl on the plane"""
    comp = orc.Computation(oscene, lamps, photon_count, oroute["lightHeight"], oroute["lightLength"], oroute["lightIntensity"])
    comp.reset()
    launch = 0
    for _ in range(iterations):
        for lamp in lamps:
            lp = comp.lamp_world_pos(lamp)
            e, _, _ = gr.gather(orc, oscene, lp, lp, comp.lightLength, samples, launch, comp.photonsPerLight)
            gr.accumulate_expected(comp.photonMap, comp.maxPhotonMap, e, lamp[2])
            comp.photonMapSize += comp.photonsPerLight
            launch += 1
        if speed > 0:
            for a, b in zip(lamps[:-1], lamps[1:]):
                e, _, _ = gr.gather(orc, oscene, comp.lamp_world_pos(a), comp.lamp_world_pos(b), comp.lightLength, samples,
                                    launch, comp.photonsPerLight)
                gr.accumulate_expected(comp.photonMap, comp.maxPhotonMap, e, segment_duration(a, b, speed))
                launch += 1
    return comp


def test_raytracer_and_cli_gather(pkg, orc, oscene, oroute, tmp_path):
    """gatherSamples = 4 through host.py and through uvrt_cli --gather 4 --dump, for stops and with a drive speed; the capacity
    (photonCount = 98 304 rays) makes two chunks of every launch."""
    from uvrt_amd import host
    lamps = oroute["lamps"][:3]
    photons, iters = 3 << 15, 2
    for speed in (0.0, 0.1):
        comp = restated_route(orc, oscene, oroute, lamps, photons, iters, S, speed)
        want = comp.dose()
        assert (want > 0).sum() > 0.3 * oscene.T
        rt = host.RayTracer(GLB, ROUTE, device=0)
        rt.set_lamps(rt.lamps()[:3])
        rt.photonCount = photons
        rt.maxIterations = iters
        rt.driveSpeed = speed
        rt.gatherSamples = S
        rt.ResetDosageMap()
        rt.viewMode = host.VIEW_DOSAGE
        for _ in range(iters):
            rt.ComputeDosageMap()
            rt.Shade()
            rt.currIterations = rt.currIterations + 1
        rt.Sync()
        got = (rt.read_dosage(), rt.ctx.read_photon_map(0), rt.ctx.read_photon_map(1), rt.ctx.seed, rt.photonMapSize)
        rt.close()
        assert same(got[1], comp.photonMap) and same(got[2], comp.maxPhotonMap), speed
        assert same(got[0], want), speed
        assert got[3] == 0 and got[4] == comp.photonMapSize == iters * 3 * comp.photonsPerLight
        f = tmp_path / "dose.f32"
        cmd = [CLI, "--room", GLB, "--route-dir", GOLDEN, "--route", "lange_route", "--lamps", "3", "--photons", str(photons),
               "--iterations", str(iters), "--gather", str(S), "--dump", str(f)]
        if speed > 0:
            cmd += ["--drive-speed", str(speed)]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr + out.stdout
        assert np.array_equal(np.fromfile(f, dtype="<u4"), bits(want)), "uvrt_cli, speed %g" % speed
