"""GPU: tri_count < T in uvrt_accumulate, uvrt_compute_dosage, uvrt_dosage_to_color, uvrt_shade and uvrt_replay_batch.

The reference's kernels run over tri_count work-items: accumulate.cl adds and zeroes tempPhotonMap below tri_count and leaves
it alone from there on, shade.cl writes dose and colour below it.  The per-launch calls are held to the oracle's accumulate /
computeDosage / dosageToColor over the slices, with everything from tri_count on bit-unchanged.

uvrt_replay_batch(ops, tri_count) replays triangles [0, tri_count) exactly as a full replay would (include/uvrt.h): the
counters of a plane keep their stride of T whatever the bound, in the replicas of a launch plane, in a folded plane and in a
class plane.  Below tri_count maps, dose and colour equal the per-launch model, from tri_count on they are unchanged, the planes
are left entirely clear (uvrt_batch_residue), and a full batch afterwards equals a fresh context's."""
import numpy as np
import pytest

import batch_sequences as bs
from test_gpu_dedupe_classes import small_scenes

pytestmark = pytest.mark.gpu

SEED0 = 0x1234
FIRST, N = 1200000, 4096


def new_ctx(capi, scene, n):
    c = capi.Ctx(0)
    c.set_scene(scene.tris, scene.nodes, scene.triIdx)
    c.resize_rays(n)
    c.reset(True)
    c.seed = SEED0
    return c


def state(c):
    return {"sum": c.read_photon_map(0), "max": c.read_photon_map(1), "dose": c.read_dosage(), "colour": c.read_color()}


def check(c, model, what):
    got = state(c)
    for name, want in (("sum", model.sum), ("max", model.max), ("dose", model.dose), ("colour", model.colour)):
        bad = np.flatnonzero((np.ascontiguousarray(got[name]).view(np.uint8).reshape(len(want), -1) !=
                              np.ascontiguousarray(want).view(np.uint8).reshape(len(want), -1)).any(axis=1))
        assert bad.size == 0, "%s: %s differs on %d triangles, the first %d" % (what, name, bad.size, bad[0])


# ---- the per-launch calls ----

@pytest.mark.parametrize("tc", [1, 1000, -1])
def test_per_launch_calls_over_a_part_of_the_triangles(pkg, orc, oscene, oroute, tc):
    capi = pkg.capi
    T = oscene.T
    tc = T - 1 if tc < 0 else tc
    pool, length = bs.lamp_pool(orc, oscene, oroute), oroute["lightLength"]
    model = bs.Model(orc, oscene)
    c = new_ctx(capi, oscene, N)
    try:
        def launch(lamp):
            c.generate(lamp, length, FIRST, N)
            c.extend(N)
            counts = c.read_counts()
            assert counts.sum() > 0.5 * N and (counts[tc:].any() or tc == T - 1), "the launch says nothing from tri_count on"
            return counts
        # a full launch first: maps, dose and colour hold something everywhere a photon lands
        counts = launch(pool["A"])
        c.accumulate(30.0)
        c.shade(0, N, 44.0197, 100.0, 0)
        model.launch(counts, (30.0, 1, 0, N, 44.0197, 100.0, 0))
        check(c, model, "after the full launch")
        # accumulate over [0, tc): tempPhotonMap zero below tc and kept from tc on
        counts = launch(pool["B"])
        c.accumulate(12.5, tc)
        model.launch(counts, (12.5, 0, 0, 0, 0.0, 0.0, 0), tc)
        check(c, model, "accumulate(tri_count = %d)" % tc)
        left = c.read_counts()
        assert not left[:tc].any() and np.array_equal(left[tc:], counts[tc:]), "tempPhotonMap after a partial accumulate"
        # computeDosage, then dosageToColor, each over [0, tc), with arguments that change every value below tc
        c.compute_dosage(1, 2 * N, 61.5, tc)
        model.dose[:tc] = orc.compute_dosage(model.max[:tc], oscene.tris, 2 * N, 61.5)
        check(c, model, "compute_dosage(tri_count = %d)" % tc)
        c.dosage_to_color(35.0, 1, tc)
        model.colour[:tc] = orc.dosage_to_color(model.dose[:tc].copy(), 35.0, 1)
        check(c, model, "dosage_to_color(tri_count = %d)" % tc)
        # Shade (both in one kernel) over [0, tc)
        c.shade(0, 3 * N, 17.25, 80.0, 0, tc)
        model.launch(np.zeros(T, dtype=np.int32), (0.0, 1, 0, 3 * N, 17.25, 80.0, 0), tc)
        check(c, model, "shade(tri_count = %d)" % tc)
        # the rest of tempPhotonMap goes with a full accumulate, and a partial Shade directly behind it: the fused kernel
        rest = left.copy()
        c.accumulate(5.0)
        c.shade(1, 4 * N, 23.0, 120.0, 1, tc)
        model.launch(rest, (5.0, 0, 0, 0, 0.0, 0.0, 0))
        model.launch(np.zeros(T, dtype=np.int32), (0.0, 1, 1, 4 * N, 23.0, 120.0, 1), tc)
        check(c, model, "a full accumulate with shade(tri_count = %d) behind it" % tc)
        assert not c.read_counts().any()
        # ... and with a launch's deposits in it
        counts = launch(pool["A"])
        c.accumulate(8.5)
        c.shade(0, 5 * N, 31.0, 90.0, 0, tc)
        model.launch(counts, (8.5, 0, 0, 0, 0.0, 0.0, 0))
        model.launch(np.zeros(T, dtype=np.int32), (0.0, 1, 0, 5 * N, 31.0, 90.0, 0), tc)
        check(c, model, "a launch, a full accumulate and shade(tri_count = %d)" % tc)
        assert not c.read_counts().any()
    finally:
        c.close()


# ---- uvrt_replay_batch ----

def room_shape(capi, orc, oscene, oroute):
    pool = bs.lamp_pool(orc, oscene, oroute)
    stop, sweep = capi.stop(pool["A"]), capi.sweep
    launches = [stop] * 3 + [sweep(pool["A"], pool["B"])] + [stop] * 5 + [sweep(pool["B"], pool["A2"])]
    return oscene, launches, oroute["lightLength"], FIRST, N


def three_triangle_shape(capi, orc, oroute):
    """tests/test_gpu_dedupe_classes.py test_small_scenes: every deposit of a plane lands on three counters"""
    scene = small_scenes(orc)["three triangles"]
    return scene, [capi.stop((0.0, -1.0, 0.0))] * 8, oroute["lightLength"], 2000000, 16384


def make_ops(capi, count, n, salt):
    ops = np.zeros(count, dtype=capi.REPLAY_OP_DT)
    for k in range(count):
        ops[k] = (5.0 + 7.0 * ((k + salt) % 5), 1 if k in (count // 2, count - 1) else 0, (k + salt) & 1, n * (k + 1 + salt),
                  44.0197 + salt, 100.0 - 10.0 * salt, (k + salt) & 1)
    return ops


_shapes = {}


def shape(pkg, orc, oscene, oroute, which):
    """(scene, launches, length, first, n, the per-launch counts of two batches in a row from SEED0, SEED after each): once"""
    if which not in _shapes:
        capi = pkg.capi
        scene, launches, length, first, n = room_shape(capi, orc, oscene, oroute) if which == "room" else three_triangle_shape(capi, orc, oroute)
        ref = new_ctx(capi, scene, n)
        try:
            counts, seeds = [], []
            for batch in range(2):
                for launch in launches:
                    if launch[2] == capi.LAUNCH_SWEEP:
                        ref.generate_sweep(launch[0], launch[1], length, first, n)
                    else:
                        ref.generate(launch[0], length, first, n)
                    ref.extend(n)
                    counts.append(ref.read_counts())
                    ref.accumulate(0.0)
                seeds.append(ref.seed)
        finally:
            ref.close()
        k = len(launches)
        assert all(cn.sum() > 0 for cn in counts), "a launch hits nothing"
        # launch 0 (a stop, from SEED0) against the oracle: the model does not rest on the GPU alone
        rays, _ = orc.generate(first, n, launches[0][0], length, SEED0)
        want = np.zeros(scene.T, dtype=np.int32)
        orc.extend(want, scene.tris, rays, scene.nodes, scene.triIdx)
        assert np.array_equal(counts[0], want), "launch 0 of the per-launch path differs from the oracle"
        _shapes[which] = (scene, launches, length, first, n, [counts[:k], counts[k:]], seeds)
    return _shapes[which]


CASES = [("room", 1000), ("room", -1), ("three triangles", 2), ("three triangles", 0)]      # (0: nothing is replayed, all is cleared)


@pytest.mark.parametrize("folded", [False, True], ids=["planes", "folded"])
@pytest.mark.parametrize("dedupe", [True, False], ids=["dedupe", "no-dedupe"])
@pytest.mark.parametrize("classes", [32, 0], ids=["classes", "no-classes"])
@pytest.mark.parametrize("which,tc", CASES)
def test_replay_over_a_part_of_the_triangles(pkg, orc, oscene, oroute, which, tc, classes, dedupe, folded):
    capi = pkg.capi
    scene, launches, length, first, n, counts, seeds = shape(pkg, orc, oscene, oroute, which)
    T = scene.T
    tc = T - 1 if tc < 0 else tc
    assert all(cn[tc:].any() for cn in counts[1]) or (which == "room" and tc == T - 1), "the batch says nothing from tri_count on"
    count = len(launches)
    ops = [make_ops(capi, count, n, 0), make_ops(capi, count, n, 1)]
    model = bs.Model(orc, scene)
    c = new_ctx(capi, scene, n)
    try:
        c.set_dedupe(dedupe)
        c.set_dedupe_classes(classes)
        # a full batch: maps, dose and colour hold something everywhere
        c.trace_batch_launches(launches, length, first, n)
        stops = sum(1 for l in launches if l[2] == capi.LAUNCH_STOP)
        assert (c.batch_traced_rays() < stops * n) == dedupe
        c.replay_batch(ops[0])
        model.replay(counts[0], ops[0])
        check(c, model, "the full batch")
        full = model.copy()
        assert c.seed == seeds[0]
        # the next batch, replayed over [0, tc)
        c.trace_batch_launches(launches, length, first, n)
        if dedupe:
            assert (c.batch_deposits() < 8 * n) == (classes > 0), "classes %d: %d deposits" % (classes, c.batch_deposits())
        if folded:
            c.fold_batch()
        c.replay_batch(ops[1], tc)
        model.replay(counts[1], ops[1], tc)
        check(c, model, "replay_batch(tri_count = %d)" % tc)
        assert c.seed == seeds[1]
        assert c.batch_residue() == 0, "counters left in the planes after a partial replay"
        # a full batch on the same context equals a fresh context's
        c.reset(True)
        c.seed = SEED0
        c.trace_batch_launches(launches, length, first, n)
        got = [c.read_batch_counts(k) for k in range(count)]
        for k in range(count):
            assert np.array_equal(got[k], counts[0][k]), "plane %d of the batch after the partial replay" % k
        c.replay_batch(ops[0])
        check(c, full, "the full batch after the partial replay")
        assert c.batch_residue() == 0
    finally:
        c.close()
