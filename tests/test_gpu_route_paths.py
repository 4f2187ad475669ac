"""GPU: the consumers of RayTracer::RouteLaunches on one route -- positions 0, 1, 1, 2 of lange_route (a zero-length
segment) driven at 0.05 m/s.  The per-launch loop, ComputeIterationsBatched, the explicit C-ABI sequence written out from
host.route_launches, the direct gather and PlanDurations must agree bit for bit."""
import numpy as np
import pytest

from conftest import GLB, ROUTE

pytestmark = pytest.mark.gpu

f32 = np.float32
PHOTONS, ITERATIONS, SPEED = 4 * 2048, 2, 0.05


@pytest.fixture(scope="module")
def host(pkg):
    from uvrt_amd import host
    return host


def tracer(host, view, gather=0):
    rt = host.RayTracer(GLB, ROUTE, device=0)
    lamps = rt.lamps()
    rt.set_lamps([lamps[k] for k in (0, 1, 1, 2)])
    rt.photonCount = PHOTONS
    rt.maxIterations = ITERATIONS
    rt.driveSpeed = SPEED
    rt.gatherSamples = gather
    rt.ctx.seed = 0
    rt.ResetDosageMap()
    rt.viewMode = view
    return rt


def state(ctx):
    ctx.sync()
    return {"dose": ctx.read_dosage(), "colour": ctx.read_color(), "sum map": ctx.read_photon_map(0),
            "max map": ctx.read_photon_map(1), "SEED": np.array([ctx.seed], dtype=np.uint32)}


def assert_same(got, want):
    for name in want:
        print("%s: %d of %d bytes differ" % (name, int((got[name].view(np.uint8) != want[name].view(np.uint8)).sum()), want[name].nbytes))
    for name in want:
        assert np.array_equal(got[name].view(np.uint8), want[name].view(np.uint8)), name


_loops = {}


def the_loop(host, view, gather=0):
    """(a): ResetDosageMap; 2 x {ComputeDosageMap; Shade; currIterations++} -- run once per (view mode, gather)"""
    if (view, gather) not in _loops:
        rt = tracer(host, view, gather)
        try:
            for _ in range(ITERATIONS):
                rt.ComputeDosageMap()
                rt.Shade()
                rt.currIterations = rt.currIterations + 1
            s = state(rt.ctx)
            assert s["dose"].any() and s["max map"].any()
            _loops[(view, gather)] = (s, rt.photonMapSize, rt.currIterations)
        finally:
            rt.close()
    return _loops[(view, gather)]


def shade_args(host, rt, view, photon_map_size, n_lamps):
    """RayTracer::Shade's arguments (raytracer.cpp:96-116)"""
    if view == host.VIEW_MAXPOWER:
        return (1, rt.photonsPerLight, f32(rt.lightIntensity) * f32(100), rt.minPower, 0)
    return (0, photon_map_size // n_lamps, f32(rt.lightIntensity) * f32(0.1), rt.minDosage, 0)


def explicit(pkg, host, view, gather=0):
    """the C-ABI calls of the same computation on a context of its own, record by record of host.route_launches"""
    rt = tracer(host, view)                 # the route's fields and the mesh; its own context stays idle
    c = pkg.capi.Ctx(0)
    try:
        lamps = rt.lamps()
        launches = host.route_launches(lamps, f32(rt.mesh.floorHeight) + f32(rt.lightHeight), SPEED)
        assert len(launches) == 7 and launches["duration"][5].tobytes() == f32(0.0).tobytes()
        ppl, length = rt.photonsPerLight, rt.lightLength
        assert ppl == 2048
        c.set_scene(rt.mesh.tris(), rt.mesh.nodes(), rt.mesh.triIdx())
        c.resize_rays(PHOTONS)
        c.reset(True)
        c.seed = 0
        size = gathers = 0
        for _ in range(ITERATIONS):
            for l in launches:
                sweep = l["kind"] == pkg.capi.LAUNCH_SWEEP
                if gather:
                    c.gather_direct(l["from"], l["to"] if sweep else l["from"], length, gather, gathers, ppl)
                    gathers += 1
                    c.accumulate_expected(l["duration"])
                else:
                    if sweep:
                        c.generate_sweep(l["from"], l["to"], length, 0, ppl)
                    else:
                        c.generate(l["from"], length, 0, ppl)
                    c.extend(ppl)
                    c.accumulate(l["duration"])
                size += 0 if sweep else ppl
            c.shade(*shade_args(host, rt, view, size, len(lamps)))
        return state(c), size
    finally:
        c.close()
        rt.close()


VIEWS = pytest.mark.parametrize("view", [0, 1], ids=["dosage", "maxpower"])


@VIEWS
def test_the_loop_equals_the_batched_computation(host, view):
    want, want_size, want_iterations = the_loop(host, view)
    rt = tracer(host, view)
    try:
        rt.ComputeIterationsBatched(ITERATIONS)
        assert_same(state(rt.ctx), want)
        assert rt.photonMapSize == want_size == ITERATIONS * 4 * 2048
        assert rt.currIterations == want_iterations == ITERATIONS
    finally:
        rt.close()


@VIEWS
def test_the_loop_equals_the_explicit_sequence(pkg, host, view):
    want, want_size, _ = the_loop(host, view)
    got, size = explicit(pkg, host, view)
    assert_same(got, want)
    assert size == want_size


@VIEWS
def test_the_gather_loop_equals_the_explicit_sequence(pkg, host, view):
    want, want_size, _ = the_loop(host, view, gather=2)
    got, size = explicit(pkg, host, view, gather=2)
    assert_same(got, want)
    assert size == want_size and want["SEED"][0] == 0       # the gather draws nothing from SEED


def test_plans_carry_the_durations_of_the_list(host):
    rt = tracer(host, host.VIEW_DOSAGE)
    try:
        launches = host.route_launches(rt.lamps(), f32(rt.mesh.floorHeight) + f32(rt.lightHeight), SPEED)
        want = launches["duration"][4:]
        _, rep = rt.PlanDurations()
        assert rep["segment_durations"].tobytes() == want.tobytes() and rep["fixed_columns"] == 3
        rt.EndPlan()
        rt.ctx.seed = 0
        rt.ResetDosageMap()
        _, rep = rt.PlanDurations(gather_samples=2)
        assert rep["segment_durations"].tobytes() == want.tobytes()
        assert rt.gatherSamples == 0
        rt.EndPlan()
    finally:
        rt.close()
