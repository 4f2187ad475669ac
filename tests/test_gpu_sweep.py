"""GPU: a lamp that radiates while it moves.  uvrt_generate_sweep against its restatement from the oracle library's pieces
(tests/sweep_restate.py), the SEED chain, the degenerate segment against uvrt_generate, RayTracer::driveSpeed against a
Python sequence of oracle calls (per-launch and batched), route files and the command line."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GLB, GOLDEN, ROOT, ROUTE
from sweep_restate import segment_duration, sweep

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "small-project-uv-robot-ray-tracer_amd", "uvrt_cli")
RAY_FIELDS = ("dirx", "diry", "dirz", "origx", "origy", "origz")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_rays(got, want):
    return all(np.array_equal(bits(got[f]), bits(want[f])) for f in RAY_FIELDS)


@pytest.fixture(scope="module")
def host(pkg):
    from uvrt_amd import host
    return host


def lamp_pos(orc, oscene, oroute, k):
    comp = orc.Computation(oscene, oroute["lamps"], 1 << 16, oroute["lightHeight"], oroute["lightLength"], oroute["lightIntensity"])
    return comp.lamp_world_pos(oroute["lamps"][k])


def test_sweep_rays_and_seed_chain(pkg, orc, oscene, oroute):
    n = 1 << 16
    length = oroute["lightLength"]
    p = [lamp_pos(orc, oscene, oroute, k) for k in range(4)]
    tilt = (p[1][0], np.float32(p[1][1] + np.float32(0.37)), p[1][2])        # a segment that also climbs: orig.y moves too
    c = pkg.capi.Ctx(0)
    c.set_scene(oscene.tris, oscene.nodes, oscene.triIdx)
    c.resize_rays(n)
    c.set_record_hits(True)
    seed = 0
    for frm, to in ((p[0], tilt), (tilt, p[2]), (p[2], p[3])):                # three consecutive sweeps
        want, nxt = sweep(orc, 0, n, frm, to, length, seed)
        c.seed = seed
        c.generate_sweep(frm, to, length, 0, n)
        got = c.read_rays(0, n)
        assert same_rays(got, want)
        assert c.seed == nxt == pkg.capi.seed_next_sweep(frm, length, seed)
        assert max(np.unique(got["origx"]).size, np.unique(got["origz"]).size) > n // 2     # the origins do spread over the segment
        # split global-id ranges give the same rays and the same SEED
        for first, cnt in ((0, 1000), (1000, n - 1000), (n - 64, 64)):
            c.seed = seed
            c.generate_sweep(frm, to, length, first, cnt)
            assert same_rays(c.read_rays(0, cnt), want[first:first + cnt]) and c.seed == nxt
        seed = nxt
    # the chain without resetting the SEED in between: launch k reads what launch k - 1 left
    c.seed = 0
    s = 0
    for frm, to in ((p[0], tilt), (tilt, p[2]), (p[2], p[3])):
        c.generate_sweep(frm, to, length, 0, 256)
        want, s = sweep(orc, 0, 256, frm, to, length, s)
        assert same_rays(c.read_rays(0, 256), want) and c.seed == s
    c.close()


def test_degenerate_segment_equals_generate(pkg, orc, oscene, oroute):
    """from == to == lamp, SEED 0, first launch: the extra draw moves nothing (u * 0 = 0), so the rays are generate.cl's and
    the free-origin kernel must trace them exactly as the fixed-lamp kernel does.
    Work-item 0 reads SEED 0 in both calls: its ray and hit equal uvrt_generate + uvrt_extend's bit for bit.  Every other
    work-item reads SEED_k, and a sweep's SEED_k (work-item 0's state AFTER the draw of u) is by definition not
    uvrt_generate's, so their rays are generate.cl's under the sweep's SEED_k (orc.generate_fixed_seed) rather than
    uvrt_generate's own; the comparison of the two kernels is then made on identical rays: the sweep's, written back as
    rays of one lamp (they share orig.x / orig.z) and traced by the fixed-lamp kernel -- all hits and counts bit for bit."""
    n = 1 << 17
    lp = lamp_pos(orc, oscene, oroute, 0)
    length = oroute["lightLength"]

    def ctx():
        c = pkg.capi.Ctx(0)
        c.set_scene(oscene.tris, oscene.nodes, oscene.triIdx)
        c.resize_rays(n)
        c.set_record_hits(True)
        c.reset(False)
        return c

    c = ctx()
    c.generate(lp, length, 0, n)
    c.extend(n)
    c.sync()
    gen, gen_seed = c.read_rays(0, n), c.seed
    c.close()
    c = ctx()
    c.generate_sweep(lp, lp, length, 0, n)
    c.extend(n)
    c.sync()
    swp, swp_counts, swp_seed = c.read_rays(0, n), c.read_counts(), c.seed
    # the same rays through the fixed-lamp kernel
    rays = swp.copy()
    rays["dist"] = np.float32(1e30)
    rays["triID"] = 0
    c.reset(False)
    c.write_rays(rays)
    c.extend(n)
    c.sync()
    lamp, lamp_counts = c.read_rays(0, n), c.read_counts()
    c.close()
    assert swp_seed == pkg.capi.seed_next_sweep(lp, length, 0) != gen_seed
    assert same_rays(swp[:1], gen[:1]) and bits(swp["dist"])[0] == bits(gen["dist"])[0] and swp["triID"][0] == gen["triID"][0]
    fixed, _ = orc.generate_fixed_seed(0, n, lp, length, swp_seed)
    assert same_rays(swp[1:], fixed[1:])
    assert same_rays(swp, lamp) and np.array_equal(bits(swp["dist"]), bits(lamp["dist"])) and np.array_equal(swp["triID"], lamp["triID"])
    assert np.array_equal(swp_counts, lamp_counts) and swp_counts.sum() > 0.9 * n


def oracle_route_with_driving(orc, oscene, oroute, lamps, photon_count, iterations, speed):
    comp = orc.Computation(oscene, lamps, photon_count, oroute["lightHeight"], oroute["lightLength"], oroute["lightIntensity"])
    comp.reset()
    for _ in range(iterations):
        comp.iteration()                                     # the stops, as orc.Computation does them
        for a, b in zip(lamps[:-1], lamps[1:]):              # then every segment: sweep -> extend -> accumulate(len / speed)
            rays, comp.SEED = sweep(orc, 0, comp.photonsPerLight, comp.lamp_world_pos(a), comp.lamp_world_pos(b),
                                    comp.lightLength, comp.SEED)
            orc.extend(comp.temp, oscene.tris, rays, oscene.nodes, oscene.triIdx)
            orc.accumulate(comp.photonMap, comp.maxPhotonMap, comp.temp, segment_duration(a, b, speed))
    return comp


def test_route_with_driving(host, orc, oscene, oroute):
    lamps = oroute["lamps"][:3]
    photons, iters, speed = 3 << 16, 2, 0.1
    comp = oracle_route_with_driving(orc, oscene, oroute, lamps, photons, iters, speed)
    want = comp.dose()                                       # N = photonMapSize / lamps: the stops only
    assert comp.photonMapSize == iters * 3 * comp.photonsPerLight

    def tracer(drive):
        rt = host.RayTracer(GLB, ROUTE, device=0)
        rt.set_lamps(rt.lamps()[:3])
        rt.photonCount = photons
        rt.maxIterations = iters
        rt.driveSpeed = drive
        rt.ResetDosageMap()
        rt.viewMode = host.VIEW_DOSAGE
        return rt

    rt = tracer(speed)
    for _ in range(iters):
        rt.ComputeDosageMap()
        rt.Shade()
        rt.currIterations = rt.currIterations + 1
    rt.Sync()
    loop = (rt.read_dosage(), rt.ctx.read_photon_map(0), rt.ctx.read_photon_map(1), rt.ctx.read_color(), rt.ctx.seed)
    assert rt.photonMapSize == comp.photonMapSize
    rt.close()
    assert np.array_equal(bits(loop[0]), bits(want))
    assert np.array_equal(loop[1], comp.photonMap) and np.array_equal(loop[2], comp.maxPhotonMap)
    assert loop[4] == comp.SEED
    assert np.array_equal(bits(loop[3]), bits(orc.dosage_to_color(want, oroute["minDosage"], False)))

    rt = tracer(speed)
    rt.ComputeIterationsBatched(iters)
    rt.Sync()
    batched = (rt.read_dosage(), rt.ctx.read_photon_map(0), rt.ctx.read_photon_map(1), rt.ctx.read_color(), rt.ctx.seed)
    assert rt.currIterations == iters and rt.photonMapSize == comp.photonMapSize
    rt.close()
    for a, b in zip(batched[:4], loop[:4]):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert batched[4] == loop[4]

    # one segment through the Python binding = the first segment of an iteration
    rt = tracer(speed)
    first = orc.Computation(oscene, lamps, photons, oroute["lightHeight"], oroute["lightLength"], oroute["lightIntensity"])
    first.reset()
    rays, s1 = sweep(orc, 0, first.photonsPerLight, first.lamp_world_pos(lamps[0]), first.lamp_world_pos(lamps[1]), first.lightLength, 0)
    orc.extend(first.temp, oscene.tris, rays, oscene.nodes, oscene.triIdx)
    orc.accumulate(first.photonMap, first.maxPhotonMap, first.temp, segment_duration(lamps[0], lamps[1], speed))
    rt.ComputeSegmentDosageMap(lamps[0][:2], lamps[1][:2], rt.photonsPerLight, oscene.T)
    rt.Sync()
    assert np.array_equal(rt.ctx.read_photon_map(0), first.photonMap) and rt.ctx.seed == s1 and rt.photonMapSize == 0
    rt.close()

    # driveSpeed 0 is today's dose: an instance that never heard of the field
    plain = orc.Computation(oscene, lamps, photons, oroute["lightHeight"], oroute["lightLength"], oroute["lightIntensity"])
    plain.reset()
    for _ in range(iters):
        plain.iteration()
    doses = []
    for touch in (False, True):
        rt = host.RayTracer(GLB, ROUTE, device=0)
        rt.set_lamps(rt.lamps()[:3])
        rt.photonCount = photons
        rt.maxIterations = iters
        if touch:
            rt.driveSpeed = 0.0
        rt.ResetDosageMap()
        rt.viewMode = host.VIEW_DOSAGE
        for _ in range(iters):
            rt.ComputeDosageMap()
            rt.Shade()
            rt.currIterations = rt.currIterations + 1
        rt.Sync()
        doses.append((rt.read_dosage(), rt.ctx.seed))
        rt.close()
    assert np.array_equal(bits(doses[0][0]), bits(doses[1][0])) and doses[0][1] == doses[1][1] == plain.SEED
    assert np.array_equal(bits(doses[0][0]), bits(plain.dose()))
    assert not np.array_equal(bits(doses[0][0]), bits(want))               # and driving does add dose
    assert np.nansum(want.astype(np.float64)) > 1.02 * np.nansum(doses[0][0].astype(np.float64))   # (8.5 s and 6 s of driving beside three 60 s stops)


def test_route_file_and_cli(host, orc, oscene, oroute, tmp_path):
    # a route saved while driving loads back with the same speed; saved at 0 it is today's file
    rt = host.RayTracer(init=False)
    rt.set_route_dir(GOLDEN + os.sep)
    rt.LoadRoute("lange_route")
    rt.set_route_dir(str(tmp_path) + os.sep)
    rt.SaveRoute("still")
    assert (tmp_path / "still.xml").read_bytes() == open(ROUTE, "rb").read()
    rt.driveSpeed = 0.1
    rt.SaveRoute("driving")
    back = host.RayTracer(init=False)
    back.set_route_dir(str(tmp_path) + os.sep)
    back.LoadRoute("driving")
    assert np.float32(back.driveSpeed) == np.float32(0.1) and back.lamps() == rt.lamps()
    rt.close(); back.close()

    lamps = oroute["lamps"][:3]
    photons, iters, speed = 3 << 16, 2, 0.1
    want = oracle_route_with_driving(orc, oscene, oroute, lamps, photons, iters, speed).dose()
    base = [CLI, "--room", GLB, "--lamps", "3", "--photons", str(photons), "--iterations", str(iters)]
    golden = ["--route-dir", GOLDEN, "--route", "lange_route"]
    runs = {"option": golden + ["--drive-speed", "0.1"], "batched": golden + ["--drive-speed", "0.1", "--batch", "2"],
            "route file": ["--route-dir", str(tmp_path), "--route", "driving"]}
    for tag, extra in runs.items():
        f = tmp_path / "dose.f32"
        out = subprocess.run(base + extra + ["--dump", str(f)], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, tag + ": " + out.stderr + out.stdout
        assert np.array_equal(np.fromfile(f, dtype="<u4"), bits(want)), tag
    for extra, msg in ((["--plan"], "--plan"), (["--gpus", "2"], "--gpus")):
        out = subprocess.run(base + golden + ["--drive-speed", "0.1"] + extra, capture_output=True, text=True, timeout=300)
        assert out.returncode != 0 and "--drive-speed" in out.stderr and msg in out.stderr, out.stderr
