"""GPU: the batched direct gather (include/uvrt.h "batched direct gather", csrc/uvrt_gather_batch.hip).  Every
plane of a batch against the restatement (tests/gather_restate.py and its stratified / variance companions) and against
uvrt_gather_direct, bit for bit, whatever the capacity and the cut into ranges; uvrt_gather_batch_select against the single
call, with the refine behind it; what the batch call leaves alone; its lifecycle and refusals; and the host layer's
gather_batch, whose dose, plan and dump are the bytes of the launch-by-launch path."""
import os
import subprocess

import numpy as np
import pytest

import gather_edge_scene as ge
import gather_restate as gr
import gather_stratified_restate as gs
import gather_variance_restate as gv
from conftest import GLB, GOLDEN, ROOT, ROUTE

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "small-project-uv-robot-ray-tracer_amd", "uvrt_cli")
N = 1 << 20
S = 4
MODES = (("independent", gv.INDEPENDENT), ("stratified", gv.STRATIFIED))
SUB = (37, 200)             # a range inside the edge scene, hand-made triangles in its middle


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def launch(frm, to, length, seed, photons_equiv=N, samples=S):
    return dict(frm=frm, to=to, light_length=length, samples=samples, seed=seed, photons_equiv=photons_equiv)


# a stop, the sweep, a stop with another light_length (0: the underflow samples), another photons_equiv, a repeated seed
EDGE_LAUNCHES = (launch(ge.LAMP, ge.LAMP, 1.0, 3), launch(ge.LAMP, ge.SEGMENT_TO, 1.0, 4), launch(ge.LAMP, ge.LAMP, 0.0, 5),
                 launch(ge.LAMP, ge.LAMP, 1.0, 6, 12345), launch(ge.LAMP, ge.SEGMENT_TO, 1.0, 3))


def new_ctx(pkg, scene, cap, mode=0, variance=1, flavour=0):
    c = pkg.capi.Ctx(0)
    c.set_scene(scene.tris, scene.nodes, scene.triIdx)
    c.resize_rays(cap)
    c.set_gather_sampling(mode)
    c.set_gather_variance(variance)
    c.set_flavour(flavour)
    return c


def single(c, l, first=0, count=None):
    c.gather_direct(l["frm"], l["to"], l["light_length"], l["samples"], l["seed"], l["photons_equiv"], first, count)


@pytest.fixture(scope="module")
def edge(orc):
    gr.check_rng(orc, 256)
    return ge.edge_scene(orc)


@pytest.fixture(scope="module")
def edge_restated(orc, edge):
    """(mode, flavour) -> [(expected, variance) of launch k over the whole edge scene], computed once"""
    out = {}
    for _, mode in MODES:
        for fl in (0, 1):
            planes = []
            for l in EDGE_LAUNCHES:
                rays, w = gs.samples(orc, edge.tris, l["frm"], l["to"], l["light_length"], S, l["seed"], 0, None, mode)
                occ = gr.occluded(orc, edge, rays, fl)
                e, v = gv.reduce_var(edge.tris, w, occ, S, l["photons_equiv"], mode)
                assert same(e, gr.reduce(edge.tris, w, occ, S, l["photons_equiv"]))
                e.setflags(write=False)
                v.setflags(write=False)
                planes.append((e, v))
            out[(mode, fl)] = planes
    return out


def check_planes(c, want, var, first, count, what):
    """every plane of the context's batch: the restated bits inside [first, first + count), +0.0 outside"""
    T = want[0][0].size
    for k, (we, wv) in enumerate(want):
        for which, w in ((0, we), (1, wv))[:2 if var else 1]:
            got = c.read_gather_batch(k, which)
            assert same(got[first:first + count], w[first:first + count]), "%s: plane %d of launch %d, %d entries differ" % (
                what, which, k, int((got[first:first + count] != w[first:first + count]).sum()))
            assert not got[:first].view(np.uint64).any() and not got[first + count:].view(np.uint64).any(), (what, k, which)
            assert got.size == T


# ---------------------------------------------------------------- the planes
@pytest.mark.parametrize("fl", (0, 1))
@pytest.mark.parametrize("name,mode", MODES)
def test_edge_scene_planes_equal_the_restatement_and_the_single_calls(pkg, edge, edge_restated, name, mode, fl):
    """T = 310, S = 4, five launches.  Capacity S: one pair per chunk; 7 S + 1: seven pairs per chunk, so chunks straddle the
    launch boundaries (310 is no multiple of 7) and the last one is ragged; 5 T S: one chunk."""
    T = edge.T
    assert T % 7 != 0 and T == 310
    want = edge_restated[(mode, fl)]
    assert not same(want[0][0], want[4][0]) and not same(want[0][0], want[3][0])
    for var in (1, 0):
        ref = new_ctx(pkg, edge, T * S, mode, var, fl)
        for cap in (S, 7 * S + 1, 5 * T * S):
            what = "%s, flavour %d, variance %d, capacity %d" % (name, fl, var, cap)
            c = new_ctx(pkg, edge, cap, mode, var, fl)
            c.gather_direct_batch(EDGE_LAUNCHES)
            assert c.gather_batch_info() == (5, S, 0, T)
            check_planes(c, want, var, 0, T, what)
            if not var:
                with pytest.raises(pkg.capi.UvrtError, match="error -1.*no variance plane"):
                    c.read_gather_batch(0, 1)
            # GPU against GPU: uvrt_gather_direct on a second context
            for k, l in enumerate(EDGE_LAUNCHES):
                single(ref, l)
                assert same(c.read_gather_batch(k), ref.read_expected()), (what, k)
                if var:
                    assert same(c.read_gather_batch(k, 1), ref.read_variance()), (what, k)
            # a range: 0 outside it; and the range cut into two batch calls
            c.gather_direct_batch(EDGE_LAUNCHES, SUB[0], SUB[1])
            assert c.gather_batch_info() == (5, S, SUB[0], SUB[1])
            check_planes(c, want, var, SUB[0], SUB[1], what + ", a range")
            c.gather_direct_batch(EDGE_LAUNCHES, SUB[0], 63)
            check_planes(c, want, var, SUB[0], 63, what + ", the range's first part")
            c.gather_direct_batch(EDGE_LAUNCHES, SUB[0] + 63, SUB[1] - 63)
            check_planes(c, want, var, SUB[0] + 63, SUB[1] - 63, what + ", the range's second part")
            c.gather_direct_batch(EDGE_LAUNCHES, 5, 0)                       # a valid empty batch
            assert c.gather_batch_info() == (5, S, 5, 0)
            check_planes(c, want, var, 5, 0, what + ", empty")
            c.close()
        ref.close()


@pytest.fixture(scope="module")
def places(orc, oscene, oroute):
    comp = orc.Computation(oscene, oroute["lamps"], N, oroute["lightHeight"], oroute["lightLength"], oroute["lightIntensity"])
    return [comp.lamp_world_pos(l) for l in oroute["lamps"][:3]]


def test_room_planes_equal_the_single_calls(pkg, orc, oscene, oroute, places):
    """T = 44 866, S = 4: stop 0, the segment 0 -> 1, stop 2, at a capacity of 1000 pairs and 3 rays per chunk and at one
    that holds the batch; GPU against GPU on the same context, and the segment's plane against the restatement"""
    T, length = oscene.T, oroute["lightLength"]
    launches = (launch(places[0], places[0], length, 0), launch(places[0], places[1], length, 1), launch(places[2], places[2], length, 2))
    restated = gr.gather(orc, oscene, places[0], places[1], length, S, 1, N)[0]
    for cap in (1000 * S + 3, 3 * T * S):
        c = new_ctx(pkg, oscene, cap, 0, 1)
        c.gather_direct_batch(launches)
        planes = [(c.read_gather_batch(k), c.read_gather_batch(k, 1)) for k in range(3)]
        assert same(planes[1][0], restated), "capacity %d: %d entries differ from the restatement" % (cap, int((planes[1][0] != restated).sum()))
        for k, l in enumerate(launches):
            single(c, l)
            assert same(planes[k][0], c.read_expected()), (cap, k)
            assert same(planes[k][1], c.read_variance()), (cap, k)
            assert (planes[k][0] > 0).sum() > 0.3 * T and (planes[k][1] > 0).sum() > 0.2 * T
        assert same(c.read_gather_batch(2), planes[2][0])                    # the single calls left the batch alone
        c.close()


# ---------------------------------------------------------------- select
@pytest.mark.parametrize("name,mode", MODES)
def test_select_leaves_what_the_single_call_leaves(pkg, edge, name, mode):
    T = edge.T
    first, count = SUB
    sent_e, sent_v = np.full(T, 7.0), np.full(T, -3.0)
    c, ref = new_ctx(pkg, edge, 7 * S + 1, mode), new_ctx(pkg, edge, T * S, mode)
    c.gather_direct_batch(EDGE_LAUNCHES, first, count)
    for k in (2, 0, 2, 4, 1):                                               # any order, repeatedly
        l = EDGE_LAUNCHES[k]
        for x in (c, ref):
            x.write_expected(sent_e)
            x.write_variance(sent_v)
        c.gather_batch_select(k)
        single(ref, l, first, count)
        got_e, got_v = c.read_expected(), c.read_variance()
        assert same(got_e, ref.read_expected()) and same(got_v, ref.read_variance()), (name, k)
        assert same(got_e[:first], sent_e[:first]) and same(got_e[first + count:], sent_e[first + count:])
        assert same(got_v[:first], sent_v[:first]) and same(got_v[first + count:], sent_v[first + count:])
        assert same(got_e[first:first + count], c.read_gather_batch(k, 0, first, count))
        # the remembered gather is launch k's: the refine gives the planes, the n_t plane and the report of the single call's
        rseed = ~l["seed"] & 0xFFFFFFFF
        assert c.gather_refine(0.25, 8, rseed, 0.0, first + 3, count - 5) == ref.gather_refine(0.25, 8, rseed, 0.0, first + 3, count - 5)
        assert same(c.read_expected(), ref.read_expected()) and same(c.read_variance(), ref.read_variance()), (name, k)
        assert same(c.read_gather_extra(), ref.read_gather_extra()) and c.read_gather_extra().any()
        with pytest.raises(pkg.capi.UvrtError, match="error -1.*no remembered gather"):       # one refine per gather
            c.gather_refine(0.25, 8, rseed)
    # the batch survived the refines, which traced through lane 0's ray buffers
    ref.gather_direct_batch(EDGE_LAUNCHES, first, count)
    for k in range(5):
        assert same(c.read_gather_batch(k), ref.read_gather_batch(k)) and same(c.read_gather_batch(k, 1), ref.read_gather_batch(k, 1))
    c.close()
    ref.close()


def test_select_without_a_variance_plane_forgets_the_remembered_gather(pkg, edge):
    T = edge.T
    c = new_ctx(pkg, edge, T * S)
    single(c, EDGE_LAUNCHES[0])                                             # remembered
    c.set_gather_variance(0)
    c.gather_direct_batch(EDGE_LAUNCHES)
    c.set_gather_variance(1)                                                # the batch's recorded state counts, not the context's
    sent_v = np.full(T, -3.0)
    c.write_variance(sent_v)
    single(c, EDGE_LAUNCHES[0])                                             # remembered again ...
    v0 = c.read_variance()
    c.gather_batch_select(1)                                                # ... and forgotten: uvrt_gather_direct with the state off
    assert same(c.read_expected(), c.read_gather_batch(1)) and same(c.read_variance(), v0)
    with pytest.raises(pkg.capi.UvrtError, match="error -1.*no remembered gather"):
        c.gather_refine(0.25, 8, 99)
    c.close()


# ---------------------------------------------------------------- what the batch call leaves
def test_the_batch_call_leaves_the_rest_of_the_context(pkg, edge):
    T = edge.T
    c, ref = new_ctx(pkg, edge, 4096), new_ctx(pkg, edge, 4096)
    source = np.linspace(1.0, 2.0, T)
    for x in (c, ref):
        x.generate(ge.LAMP, 1.0, 0, 4096)
        x.extend(4096)
        x.write_indirect_source(source)
        single(x, EDGE_LAUNCHES[1])                                         # an older gather, remembered
    seed, counts, e0, v0 = c.seed, c.read_counts(), c.read_expected(), c.read_variance()
    assert counts.any() and seed != 0
    c.gather_direct_batch(EDGE_LAUNCHES[2:])
    assert c.seed == seed and same(c.read_counts(), counts) and same(c.read_expected(), e0) and same(c.read_variance(), v0)
    assert same(c.read_indirect_source(), source)
    rseed = 77
    assert c.gather_refine(0.25, 8, rseed) == ref.gather_refine(0.25, 8, rseed)     # the older gather is still the remembered one
    assert same(c.read_expected(), ref.read_expected()) and same(c.read_variance(), ref.read_variance())
    # like every shadow-ray call it drops "the last generate"
    c.generate(ge.LAMP, 1.0, 0, 4096)
    c.gather_direct_batch(EDGE_LAUNCHES[:2])
    with pytest.raises(pkg.capi.UvrtError, match="error -1"):
        c.extend(4096)
    c.close()
    ref.close()


# ---------------------------------------------------------------- lifecycle and refusals
def test_lifecycle_and_refusals(pkg, edge):
    T = edge.T
    L = pkg.capi.lib()
    c = new_ctx(pkg, edge, 64 * S)
    assert c.gather_batch_info() == (0, 0, 0, 0)                             # before any batch
    for call in (lambda: c.gather_batch_select(0), lambda: c.read_gather_batch(0)):
        with pytest.raises(pkg.capi.UvrtError, match="error -1.*no batch"):
            call()
    c.gather_direct_batch(EDGE_LAUNCHES[:3], 10, 100)
    c.set_scene(edge.tris, edge.nodes, edge.triIdx)                         # a new scene drops the batch
    assert c.gather_batch_info() == (0, 0, 0, 0)
    with pytest.raises(pkg.capi.UvrtError, match="error -1.*no batch"):
        c.gather_batch_select(0)
    c.gather_direct_batch(EDGE_LAUNCHES[:3], 10, 100)
    first = [c.read_gather_batch(k) for k in range(3)]
    c.gather_direct_batch(EDGE_LAUNCHES[3:], 20, 50)                        # a second batch replaces the first
    assert c.gather_batch_info() == (2, S, 20, 50)
    with pytest.raises(pkg.capi.UvrtError, match="error -1.*outside the batch"):
        c.read_gather_batch(2)
    assert not same(c.read_gather_batch(0), first[0])
    # every refusal: UVRT_ERR_INVALID, the batch and the context's planes as they were
    info, plane, plane_v = c.gather_batch_info(), c.read_gather_batch(1), c.read_gather_batch(1, 1)
    sent = np.full(T, 5.0)
    c.write_expected(sent)
    bad = lambda k, **kw: [dict(l, **kw) if i == k else l for i, l in enumerate(EDGE_LAUNCHES)]
    refusals = [("null", lambda: c._ck(L.uvrt_gather_direct_batch(c._h, None, 2, 0, T))),
                ("count 0", lambda: c.gather_direct_batch([])),
                ("count 65", lambda: c.gather_direct_batch([EDGE_LAUNCHES[0]] * 65)),
                ("differing samples", lambda: c.gather_direct_batch(bad(2, samples=8))),
                ("S = 0", lambda: c.gather_direct_batch(bad(0, samples=0))),
                ("S > capacity", lambda: c.gather_direct_batch([dict(l, samples=64 * S + 1) for l in EDGE_LAUNCHES])),
                ("photons_equiv 0 in launch 3", lambda: c.gather_direct_batch(bad(3, photons_equiv=0))),
                ("variance with S = 1", lambda: c.gather_direct_batch([dict(l, samples=1) for l in EDGE_LAUNCHES])),
                ("a range past T", lambda: c.gather_direct_batch(EDGE_LAUNCHES, T - 3, 4)),
                ("a negative range", lambda: c.gather_direct_batch(EDGE_LAUNCHES, -1, 4)),
                ("k = -1", lambda: c.gather_batch_select(-1)),
                ("k = count", lambda: c.gather_batch_select(2)),
                ("read k = count", lambda: c.read_gather_batch(2)),
                ("read which = 2", lambda: c.read_gather_batch(0, 2)),
                ("read past T", lambda: c.read_gather_batch(0, 0, T - 1, 2))]

    def refused(tag, call):
        with pytest.raises(pkg.capi.UvrtError, match="error -1"):
            call()
        assert c.gather_batch_info() == info, tag
        assert same(c.read_gather_batch(1), plane) and same(c.read_gather_batch(1, 1), plane_v), tag
        assert same(c.read_expected(), sent), tag

    for tag, call in refusals:
        refused(tag, call)
    c.set_flavour(2)
    refused("flavour 2", lambda: c.gather_direct_batch(EDGE_LAUNCHES))
    c.set_flavour(0)
    c.gather_direct_batch([EDGE_LAUNCHES[0]] * 64, 0, 3)                     # 64 launches are served
    assert c.gather_batch_info() == (64, S, 0, 3)
    assert same(c.read_gather_batch(63), c.read_gather_batch(0))
    c.close()


# ---------------------------------------------------------------- the host layer
PPL = 1 << 16


@pytest.fixture(scope="module")
def rt(pkg):
    from uvrt_amd import host
    r = host.RayTracer(GLB, ROUTE, device=0)
    r.set_lamps(r.lamps()[:3])
    r.photonCount = 3 * PPL
    r.maxIterations = 2
    r.viewMode = host.VIEW_DOSAGE
    yield r
    r.close()


def _run(rt, batch, speed=0.0, rel_error=0.0, reflectance=0.0, bounces=0):
    """the plain pipeline with gatherSamples = S from ResetDosageMap; (dose, colours, photonMap, maxPhotonMap) as bytes"""
    rt.gatherSamples, rt.driveSpeed, rt.gather_batch = S, speed, batch
    rt.set_gather_refine(rel_error, 8)
    rt.reflectance, rt.reflectSamples, rt.reflectBounces = reflectance, 4, bounces
    rt.ResetDosageMap()
    for _ in range(rt.maxIterations):
        rt.ComputeDosageMap()
        rt.Shade()
        rt.currIterations = rt.currIterations + 1
    rt.Sync()
    out = [np.ascontiguousarray(a).tobytes() for a in (rt.read_dosage(), rt.ctx.read_color(), rt.ctx.read_photon_map(0), rt.ctx.read_photon_map(1))]
    rt.gather_batch = 0
    rt.set_gather_refine(0.0, 64)
    rt.reflectance, rt.reflectBounces, rt.driveSpeed = 0.0, 0, 0.0
    return out


@pytest.mark.parametrize("tag,kw", [("three stops", {}), ("driving", dict(speed=0.5)), ("refined", dict(speed=0.5, rel_error=0.5)),
                                    ("a traced bounce", dict(reflectance=0.3)), ("linked bounces", dict(reflectance=0.3, bounces=2))])
def test_host_dose_bytes_do_not_depend_on_gather_batch(rt, tag, kw):
    """B = 2: groups of 2, 1 (stops) or 2, 2, 1 (driving); B = 5: one group; two iterations, so the seed counter runs on"""
    want = _run(rt, 0, **kw)
    assert np.frombuffer(want[0], dtype=np.float32).any()
    for B in (2, 5):
        assert _run(rt, B, **kw) == want, (tag, B)
    if tag == "driving":
        rt.gatherSamples, rt.driveSpeed, rt.gather_batch = S, 0.5, 2           # ComputeSegments alone walks in groups too
        segs = []
        for B in (0, 2):
            rt.gather_batch = B
            rt.ResetDosageMap()
            rt.ComputeSegments()
            rt.Shade()
            rt.Sync()
            segs.append(rt.ctx.read_photon_map(0).tobytes())
        rt.gather_batch, rt.driveSpeed = 0, 0.0
        assert segs[0] == segs[1] and np.frombuffer(segs[0], dtype=np.float64).any()


@pytest.mark.parametrize("confidence", (0.0, 2.0))
def test_plan_durations_do_not_depend_on_gather_batch(rt, confidence):
    rt.gatherSamples, rt.driveSpeed = 0, 0.5
    lamps = rt.lamps()

    def plan(B):
        rt.set_lamps(lamps)                     # (a plan writes its durations into the positions)
        d, rep = rt.PlanDurationsBatched(B, gather_samples=S, gather_confidence=confidence)
        cols = [rt.ctx.plan_read_exposure_expected(p).tobytes() for p in range(5)]
        if confidence:
            cols += [rt.ctx.plan_read_exposure_variance(p).tobytes() for p in range(5)]
        rt.EndPlan()
        rep = {k: (v.tobytes() if isinstance(v, np.ndarray) else v) for k, v in rep.items()}
        return d.tobytes(), rep, cols

    try:
        want = plan(0)
        got = plan(4)
        assert got[0] == want[0] and got[1] == want[1] and got[2] == want[2]
        assert np.frombuffer(want[2][0], dtype=np.float64).any() and np.frombuffer(want[0], dtype=np.float32).any()
    finally:
        rt.driveSpeed = 0.0
        rt.set_lamps(lamps)


def test_cli_dump_is_the_dump_without_the_flag(pkg, tmp_path):
    base = [CLI, "--room", GLB, "--route-dir", GOLDEN, "--route", "lange_route", "--lamps", "4", "--photons", str(4 * PPL),
            "--iterations", "1", "--gather", str(S)]
    a, b = tmp_path / "plain.bin", tmp_path / "batched.bin"
    for extra, out in (([], a), (["--gather-batch", "3"], b)):
        r = subprocess.run(base + extra + ["--dump", str(out)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (extra, r.stdout, r.stderr)
    assert a.read_bytes() == b.read_bytes() and np.frombuffer(a.read_bytes(), dtype=np.float32).any()
