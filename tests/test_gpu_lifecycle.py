"""GPU: a context can be destroyed in every state it can be in (uvrt_ctx.h: the context, its lanes, its batch sets and the
plan own their buffers, streams and events; uvrt_destroy waits for every stream and deletes).  A context is brought to a
stage and closed; a fresh context with the same SEED then traces one launch, and its tempPhotonMap must equal, bit for bit,
that of a first context nothing came before.  The last stage keeps the loaded context and swaps its scene instead.
Test room (44 866 triangles), 16 384 photons per launch: the smallest launch that builds a hot-record renumbering."""
import numpy as np
import pytest

from scene_layout_restate import pair_order

pytestmark = pytest.mark.gpu

N = 16384
SEED = 12345
f32 = np.float32


@pytest.fixture(scope="module")
def lamps(orc, oscene, oroute):
    comp = orc.Computation(oscene, oroute["lamps"][:2], N, oroute["lightHeight"], oroute["lightLength"],
                           oroute["lightIntensity"])
    return [tuple(float(x) for x in comp.lamp_world_pos(l)) for l in oroute["lamps"][:2]]


def _launch(c, lamps, oroute):
    c.reset(True)
    c.seed = SEED
    c.generate(lamps[0], oroute["lightLength"], 0, N)
    c.extend(N)
    c.sync()
    return c.read_counts()


def _fresh_launch(pkg, oscene, oroute, lamps):
    c = pkg.capi.Ctx(0)
    try:
        c.set_scene(oscene.tris, oscene.nodes, oscene.triIdx)
        c.resize_rays(N)
        return _launch(c, lamps, oroute)
    finally:
        c.close()


@pytest.fixture(scope="module")
def first_counts(pkg, oscene, oroute, lamps):
    counts = _fresh_launch(pkg, oscene, oroute, lamps)
    assert counts.sum() > 0
    return counts


# ---- the steps, each on top of the ones before it
def _scene(c, pkg, oscene, oroute, lamps):
    c.set_scene(oscene.tris, oscene.nodes, oscene.triIdx)
    c.resize_rays(N)
    c.reset(True)


def _extended(c, pkg, oscene, oroute, lamps):
    c.generate(lamps[0], oroute["lightLength"], 0, N)
    c.extend(N)


def _deferred(c, pkg, oscene, oroute, lamps):
    c.accumulate(1.0)                                   # all triangles: deferred until the next call (PendingAcc)


def _timed(c, pkg, oscene, oroute, lamps):
    c.set_timing(True)
    for k in range(3):                                  # over both launch lanes; the last accumulate stays deferred
        c.generate(lamps[k % 2], oroute["lightLength"], 0, N)
        c.extend(N)
        c.accumulate(1.0)


def _batch(c, pkg, oscene, oroute, lamps):
    a, b = lamps
    up = (a[0], a[1] + 0.25, a[2])                      # a second stop on a's lamp column
    c.trace_batch_launches([pkg.capi.stop(a), pkg.capi.stop(up), pkg.capi.sweep(a, b)], oroute["lightLength"], 0, N)


def _captured(c, pkg, oscene, oroute, lamps):
    c.fold_batch()
    c.plan_begin(2)
    c.plan_capture_batch([0, 0, 1])


def _solved(c, pkg, oscene, oroute, lamps):
    s = f32(f32(oroute["lightIntensity"]) * f32(0.1))
    d, rep = c.plan_solve(100.0, s, N)
    assert rep["required"] > 0 and d.sum() > 0
    d, rep, brep = c.plan_solve_bounded(100.0, s, N, lower=[0.5, 1.0], fixed=[0, 1])
    assert brep["fixed_columns"] == 1 and d[1] == f32(1.0)
    c.plan_model_dose(d)


def _gathered(c, pkg, oscene, oroute, lamps):
    c.plan_begin_expected(1)
    c.gather_direct(lamps[0], lamps[1], oroute["lightLength"], 4, 7, N, 0, 256)
    c.plan_capture_expected(0)


STEPS = [_scene, _extended, _deferred, _timed, _batch, _captured, _solved, _gathered]
STAGES = ["created"] + [f.__name__[1:] for f in STEPS]


@pytest.mark.parametrize("stage", range(len(STAGES)), ids=STAGES)
def test_destroy_at_stage(pkg, oscene, oroute, lamps, first_counts, stage):
    c = pkg.capi.Ctx(0)
    try:
        for step in STEPS[:stage]:
            step(c, pkg, oscene, oroute, lamps)
    finally:
        c.close()
    assert np.array_equal(_fresh_launch(pkg, oscene, oroute, lamps), first_counts)


def test_scene_swap_with_everything_live(pkg, orc, oscene, oroute, lamps, first_counts):
    """every step on one context, then CalibratePower's detour: a 2-triangle scene and the room again"""
    tris = np.zeros((2, 16), dtype=np.float32)
    h, d, w = f32(-0.5), f32(1.0), f32(0.1)
    tris[0, 0:3] = (w, h + w, d); tris[0, 4:7] = (-w, h + w, d); tris[0, 8:11] = (w, h - w, d)
    tris[1, 0:3] = (-w, h - w, d); tris[1, 4:7] = (-w, h + w, d); tris[1, 8:11] = (w, h - w, d)
    nodes = np.zeros(1, dtype=orc.NODE_DT)
    nodes[0]["leftFirst"], nodes[0]["triCount"] = 0, 2
    c = pkg.capi.Ctx(0)
    try:
        for step in STEPS:
            step(c, pkg, oscene, oroute, lamps)
        c.set_scene(tris, nodes, np.array([0, 1], dtype=np.uint32))
        c.set_scene(oscene.tris, oscene.nodes, oscene.triIdx)
        assert np.array_equal(_launch(c, lamps, oroute), first_counts)
    finally:
        c.close()


# ---- a scene swap that keeps T: no buffer is reallocated for the size's sake, so whatever uvrt_set_scene forgets to void
# ---- shows as the earlier scene's geometry
SWAP_T, SWAP_N = 300, 4096
SWAP_LAMP, SWAP_TO = (0.1, 0.2, -0.1), (0.4, 0.2, 0.3)


def _soup_scene(orc, seed):
    rng = np.random.default_rng(seed)
    tris = np.zeros((SWAP_T, 16), dtype=np.float32)
    centre = rng.uniform(-2.0, 2.0, size=(SWAP_T, 1, 3))
    tris[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]] = (centre + rng.normal(scale=0.3, size=(SWAP_T, 3, 3))).reshape(SWAP_T, 9).astype(np.float32)
    nodes, idx = orc.build_bvh(tris)
    return tris, nodes, idx


def _free_rays(orc, seed, tmax):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(SWAP_N, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    o = rng.uniform(-2.0, 2.0, size=(SWAP_N, 3)).astype(np.float32)
    r = np.zeros(SWAP_N, dtype=orc.RAY_DT)
    r["dirx"], r["diry"], r["dirz"] = d[:, 0], d[:, 1], d[:, 2]
    r["origx"], r["origy"], r["origz"] = o[:, 0], o[:, 1], o[:, 2]
    r["dist"] = np.float32(tmax)
    return r


def _observe(c, free, shadow):
    """what a caller sees of the scene: hits and counts of a lamp, a free-ray and a wide launch, shadow answers, a small gather"""
    out = {}

    def launched(what):
        c.extend(SWAP_N)
        c.sync()
        rays = c.read_rays(0, SWAP_N)
        out[what] = (c.read_counts(), rays["dist"].view(np.uint32), rays["triID"])

    c.set_record_hits(True)
    c.resize_rays(SWAP_N)
    for what, wide in (("lamp", False), ("wide", True)):
        c.set_wide_bvh(wide)
        c.reset(True)
        c.seed = SEED
        c.generate(SWAP_LAMP, 1.0, 0, SWAP_N)
        launched(what)
    c.set_wide_bvh(False)
    c.reset(True)
    c.write_free_rays(free)
    launched("free")
    out["shadow"] = (c.occluded(shadow),)
    c.set_gather_variance(1)
    c.gather_direct(SWAP_LAMP, SWAP_TO, 1.0, 4, 7, SWAP_N, 10, 64)
    out["gather"] = (c.read_expected().view(np.uint64), c.read_variance().view(np.uint64))
    c.set_record_hits(False)
    return out


def test_scene_swap_that_keeps_the_triangle_count(pkg, orc):
    """every per-scene cache warm on one 300-triangle soup, then another soup of 300 triangles: the context behaves as a
    fresh one with the second soup does, and what was remembered of the first is refused"""
    a, b = _soup_scene(orc, 1), _soup_scene(orc, 2)
    pairs_a, pairs_b = pair_order(a[1]).size, pair_order(b[1]).size
    assert pairs_a > 128 and pairs_b > 128                  # the scenes get automatic hot renumberings
    free, shadow = _free_rays(orc, 3, 1e30), _free_rays(orc, 4, 1.5)
    c = pkg.capi.Ctx(0)
    try:
        c.set_scene(*b)
        want = _observe(c, free, shadow)
    finally:
        c.close()
    assert want["lamp"][0].sum() > 0 and want["free"][0].sum() > 0 and 0 < want["shadow"][0].sum() < SWAP_N
    assert (want["gather"][0] != 0).any() and (want["gather"][1] != 0).any()
    c = pkg.capi.Ctx(0)
    try:
        c.set_scene(*a)
        c.resize_rays(16384)
        c.reset(True)
        c.write_free_rays(free)                             # a free-ray extend: the free records
        c.extend(SWAP_N)
        c.occluded(shadow)
        c.set_gather_variance(1)                            # the gather's triangles, both planes, the memo, n_t
        c.gather_direct(SWAP_LAMP, SWAP_TO, 1.0, 4, 7, SWAP_N)
        assert c.gather_refine(0.01, 16, 5)[0] > 0
        c.gather_direct(SWAP_LAMP, SWAP_TO, 1.0, 4, 7, SWAP_N)      # remembered again: a refine would be accepted
        c.set_wide_bvh(True)                                # the lanes' 4-wide records
        c.generate(SWAP_LAMP, 1.0, 0, SWAP_N)
        c.extend(SWAP_N)
        c.set_wide_bvh(False)
        c.set_record_perm(np.arange(pairs_a, dtype=np.uint32)[::-1].copy())     # a caller's renumbering ...
        c.generate(SWAP_LAMP, 1.0, 0, SWAP_N)
        c.extend(SWAP_N)
        c.set_record_perm(None)
        c.generate(SWAP_LAMP, 1.0, 0, 16384)                # ... and an automatic one
        c.extend(16384)
        assert not np.array_equal(c.read_record_perm(pairs_a), np.arange(pairs_a, dtype=np.uint32))
        c.set_record_perm(np.arange(pairs_a, dtype=np.uint32)[::-1].copy())
        c.trace_batch([SWAP_LAMP] * 4 + [SWAP_TO], 1.0, 0, SWAP_N)      # a traced batch that is not replayed ...
        c.fold_batch()
        c.plan_begin(2)                                     # ... and an active plan that has captured it
        c.plan_capture_batch([0, 0, 0, 0, 1])
        assert c.plan_read_exposure(0).sum() > 0
        c.sync()

        c.set_scene(*b)
        with pytest.raises(pkg.capi.UvrtError, match="no remembered gather"):
            c.gather_refine(0.01, 16, 5)
        perm = c.read_record_perm(pairs_b)
        assert np.array_equal(perm, np.arange(pairs_b, dtype=np.uint32))
        ops = np.zeros(5, dtype=pkg.capi.REPLAY_OP_DT)
        ops["duration"] = 1.0
        with pytest.raises(pkg.capi.UvrtError, match="no traced batch"):
            c.replay_batch(ops)
        with pytest.raises(pkg.capi.UvrtError, match="no plan"):
            c.plan_read_exposure(0)
        got = _observe(c, free, shadow)
        for what in want:
            for k, (g, w) in enumerate(zip(got[what], want[what])):
                assert np.array_equal(g, w), (what, k)
        c.sync()
    finally:
        c.close()
