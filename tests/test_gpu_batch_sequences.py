"""GPU: sequences of batches of changing shape on ONE long-lived context (tests/batch_sequences.py).

Nothing clears a context's two buffer sets between batches; every batch's fold or replay has to read back and zero what the
batch wrote -- launch planes at the batch's own R, class planes behind them at an offset that follows its count, the folded
totals.  Each of six seeds runs eleven batches whose count, range, dedupe and class setting, flavour, seed mode, sweeps, helper
priority and way of consumption change from one batch of a set to the next.  After every step, bit for bit:

  * the planes that were read, both f64 maps, dose, colour and SEED equal the model's: a second context traces the same
    launches one by one (generate / generate_sweep -> extend -> read_counts), and the oracle's accumulate / computeDosage /
    dosageToColor turn those counts into maps, dose and colour on the CPU, in logical launch order;
  * one launch per step is traced by the CPU oracle as well (flavours 0 and 1), so the model does not rest on the GPU alone;
  * uvrt_batch_traced_rays is the stops' rays with dedupe off and the host plan's owners with it on (never more), and the
    groups' traced rays <= uvrt_batch_deposits <= the groups' occurrences;
  * uvrt_batch_residue is 0 after every replay.

Two seeds run the context under test as a pair over the two halves of the range, summed by uvrt_reduce_batch_group."""
import numpy as np
import pytest

import batch_sequences as bs
from sweep_restate import sweep as restated_sweep

pytestmark = pytest.mark.gpu

LAUNCH_SHADE = (4096, 44.0197, 100.0, 0)      # the Shade behind the per-launch launch of mode "launch"; the map is the step's


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def bits64(a):
    return np.ascontiguousarray(a).view(np.uint64)


def new_ctx(capi, scene):
    c = capi.Ctx(0)
    c.set_scene(scene.tris, scene.nodes, scene.triIdx)
    c.resize_rays(max(bs.NS))
    c.reset(True)
    c.seed = bs.SEED0
    return c


def one_launch(capi, c, launch, length, first, n):
    if launch[2] == capi.LAUNCH_SWEEP:
        c.generate_sweep(launch[0], launch[1], length, first, n)
    else:
        c.generate(launch[0], length, first, n)
    c.extend(n)


def oracle_counts(orc, scene, step, launch, length, seed):
    """the oracle's tempPhotonMap of one logical launch that starts at SEED `seed`"""
    first, n = step["first"], step["n"]
    orc.set_flavour(step["flavour"])
    try:
        if launch[2] == 1:
            rays, _ = restated_sweep(orc, first, n, launch[0], launch[1], length, seed)
        elif step["seed_mode"] == 0:
            rays, _ = orc.generate(first, n, launch[0], length, seed)
        else:
            rays, _ = orc.generate_fixed_seed(first, n, launch[0], length, seed, saturate=True)
        temp = np.zeros(scene.T, dtype=np.int32)
        orc.extend(temp, scene.tris, rays, scene.nodes, scene.triIdx)
        return temp
    finally:
        orc.set_flavour(0)


def check_state(c, model, what):
    assert np.array_equal(bits64(c.read_photon_map(0)), bits64(model.sum)), what + ": the sum map"
    assert np.array_equal(bits64(c.read_photon_map(1)), bits64(model.max)), what + ": the max map"
    assert np.array_equal(bits(c.read_dosage()), bits(model.dose)), what + ": the dose"
    assert np.array_equal(bits(c.read_color()), bits(model.colour)), what + ": the colour"


@pytest.mark.parametrize("seed", bs.SEEDS)
def test_sequence(pkg, orc, oscene, oroute, seed):
    capi = pkg.capi
    pool, length = bs.lamp_pool(orc, oscene, oroute), oroute["lightLength"]
    pair = seed in bs.PAIR_SEEDS
    under_test = [new_ctx(capi, oscene) for _ in range(2 if pair else 1)]
    ref = new_ctx(capi, oscene)
    model = bs.Model(orc, oscene)
    hits = 0
    try:
        for i, step in enumerate(bs.sequence(seed)):
            what = "seed %d step %d (%d launches, n %d from %d, dedupe %d, classes %d, flavour %d, seed mode %d, %s)" % (
                seed, i, len(step["launches"]), step["n"], step["first"], step["dedupe"], step["classes"], step["flavour"],
                step["seed_mode"], step["mode"])
            first, n, count = step["first"], step["n"], len(step["launches"])
            launches = bs.launches_of(capi, step, pool)
            chain = bs.seed_chain(capi, step, pool, length, ref.seed)
            # the model: the per-launch path on a context of its own, the oracle for one launch of the step
            ref.set_flavour(step["flavour"])
            ref.set_seed_mode(step["seed_mode"])
            counts = []
            for launch in launches:
                one_launch(capi, ref, launch, length, first, n)
                counts.append(ref.read_counts())
                ref.accumulate(0.0)             # (takes the deposits out of tempPhotonMap)
            assert ref.seed == chain[-1], what
            hits += sum(int(cn.sum()) for cn in counts)
            if step["flavour"] in (0, 1):
                k = step["oracle"]
                assert np.array_equal(counts[k], oracle_counts(orc, oscene, step, launches[k], length, chain[k])), \
                    what + ": launch %d of the per-launch path differs from the oracle" % k
            # the batch
            halves = [(first, n)] if not pair else [(first, n // 2), (first + n // 2, n - n // 2)]
            for c, (lo, m) in zip(under_test, halves):
                c.set_dedupe(step["dedupe"])
                c.set_dedupe_classes(step["classes"])
                c.set_flavour(step["flavour"])
                c.set_seed_mode(step["seed_mode"])
                c.set_helper_priority(step["prio"])
                c.trace_batch_launches(launches, length, lo, m)
                assert c.seed == chain[-1], what
                traced, deposits = c.batch_traced_rays(), c.batch_deposits()
                want_traced, occurrences = bs.owners(capi, step, pool, chain, lo, m)
                stops = sum(1 for l in step["launches"] if l[0] == "stop")
                print("%s: traced %d of %d, deposits %d" % (what, traced, stops * m, deposits))
                if not step["dedupe"]:
                    assert traced == stops * m and deposits == 0, what
                assert traced == want_traced <= stops * m, what
                in_groups = traced - (stops * m - occurrences)
                assert in_groups <= deposits <= occurrences, what + ": %d <= %d <= %d" % (in_groups, deposits, occurrences)
            if pair:
                capi.reduce_batch_group(under_test)
            for c in under_test:
                if step["mode"] == "read":
                    for k in range(count):
                        assert np.array_equal(c.read_batch_counts(k), counts[k]), what + ": plane %d" % k
                elif step["mode"] == "fold":
                    c.fold_batch()
                c.replay_batch(step["ops"])
            model.replay(counts, step["ops"])
            if step["mode"] == "launch":        # one per-launch launch on the same context before the next batch
                stop = capi.stop(pool["B"])
                one_launch(capi, ref, stop, length, first, n)
                extra = ref.read_counts()
                ref.accumulate(0.0)
                op = (step["launch_dt"], 1, step["launch_which"]) + LAUNCH_SHADE
                for c in under_test:
                    one_launch(capi, c, stop, length, first, n)
                    c.accumulate(op[0])
                    c.shade(op[2], op[3], op[4], op[5], op[6])
                    assert c.seed == ref.seed, what
                model.launch(extra, op)
            for c in under_test:
                check_state(c, model, what)
                assert c.seed == ref.seed, what
                assert c.batch_residue() == 0, what + ": counters left in the planes after the replay"
        assert hits > 0 and model.dose.any()
    finally:
        for c in under_test + [ref]:
            c.close()


def test_residue_is_refused_while_a_batch_is_traced(pkg, orc, oscene, oroute):
    capi = pkg.capi
    pool, length = bs.lamp_pool(orc, oscene, oroute), oroute["lightLength"]
    c = new_ctx(capi, oscene)
    try:
        assert c.batch_residue() == 0           # no batch yet: nothing allocated
        c.trace_batch([pool["A"]] * 8, length, 1200000, 4096)
        with pytest.raises(capi.UvrtError, match=r"uvrt error -1.*not been replayed"):
            c.batch_residue()
        c.replay_batch(np.zeros(8, dtype=capi.REPLAY_OP_DT))
        assert c.batch_residue() == 0
    finally:
        c.close()
