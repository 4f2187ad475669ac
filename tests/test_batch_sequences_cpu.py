"""CPU: the six batch sequences of tests/batch_sequences.py hold what they are for.

tests/test_gpu_batch_sequences.py can only find stale counters where a later batch of the same buffer set lays other planes over
them, so this file asks the host hooks (uvrt_seed_next*, uvrt_dedupe_plan, uvrt_dedupe_classes) what every generated step
really is -- its groups, whether it gets class planes -- and demands the transitions per sequence.  A seed that lacks one is a
reason to mend the generator, never to drop the seed."""
import numpy as np
import pytest

import batch_sequences as bs


@pytest.fixture(scope="module")
def pool(orc, oscene, oroute):
    return bs.lamp_pool(orc, oscene, oroute), oroute["lightLength"]


@pytest.fixture(scope="module")
def described(pkg, pool):
    """seed -> per step (step, SEED chain, groups, does it get class planes)"""
    lamps, length = pool
    out = {}
    for seed in bs.SEEDS:
        chain_seed, rows = bs.SEED0, []
        for step in bs.sequence(seed):
            chain = bs.seed_chain(pkg.capi, step, lamps, length, chain_seed)
            chain_seed = chain[-1]
            rows.append((step, chain, bs.groups_of(step, lamps), bs.is_classed(pkg.capi, step, lamps, chain)))
        out[seed] = rows
    return out


def same_set(rows):
    """the steps of each buffer set, in order (a batch goes into the set the previous one did not use)"""
    return [rows[0::2], rows[1::2]]


def test_the_generator_is_a_function_of_the_seed():
    for seed in bs.SEEDS:
        assert bs.sequence(seed) == bs.sequence(seed)
    assert len({repr(bs.sequence(seed)) for seed in bs.SEEDS}) == len(bs.SEEDS)


@pytest.mark.parametrize("seed", bs.SEEDS)
def test_every_step_is_one_the_abi_takes(seed):
    steps = bs.sequence(seed)
    assert len(steps) == bs.STEPS
    for i, step in enumerate(steps):
        count = len(step["launches"])
        sweeps = sum(1 for l in step["launches"] if l[0] == "sweep")
        assert count in bs.COUNTS and step["n"] in bs.NS and step["first"] in bs.FIRSTS and step["classes"] in bs.CLASSES, i
        assert step["mode"] in bs.MODES and 0 <= step["prio"] <= 3 and step["seed_mode"] in (0, 1), i
        assert step["flavour"] in ((0, 1, 2) if seed == bs.FLAVOUR2_SEED else (0, 1)), i
        assert 0 <= sweeps <= 3 and sweeps < count, i
        if sweeps:
            assert step["flavour"] in (0, 1) and step["seed_mode"] == 0, "step %d: a sweep the ABI refuses" % i
        assert len(step["ops"]) == count and step["ops"][-1][1] == 1, i
        assert step["launches"][step["oracle"]][0] == "stop" or step["flavour"] == 0, i
        if seed in bs.PAIR_SEEDS:
            assert step["n"] >= 2, "step %d: a half of the range would be empty" % i
    last = steps[-1]
    assert len(last["launches"]) == 64 and last["n"] == 1000 and all(l[0] == "stop" for l in last["launches"])
    if seed == bs.FLAVOUR2_SEED:
        assert any(s["flavour"] == 2 for s in steps)


def test_the_sequences_use_every_value_between_them():
    steps = [s for seed in bs.SEEDS for s in bs.sequence(seed)]
    assert {len(s["launches"]) for s in steps} == set(bs.COUNTS)
    assert {s["n"] for s in steps} == set(bs.NS) and {s["first"] for s in steps} == set(bs.FIRSTS)
    assert {s["classes"] for s in steps} == set(bs.CLASSES) and {s["mode"] for s in steps} == set(bs.MODES)
    assert {s["prio"] for s in steps} == {0, 1, 2, 3} and {s["seed_mode"] for s in steps} == {0, 1}
    assert {s["dedupe"] for s in steps} == {True, False}
    sizes = {len(g) for seed in bs.SEEDS for s in bs.sequence(seed) for g in bs.groups_of(s, {"A": (0, 0, 0), "B": (1, 0, 1), "A2": (0, 1, 0)})}
    assert min(sizes) == 2 and max(sizes) >= 20, sizes


@pytest.mark.parametrize("seed", bs.SEEDS)
def test_each_set_sees_three_shapes_in_a_row(described, seed):
    for which, rows in enumerate(same_set(described[seed])):
        pairs = [(len(step["launches"]), step["classes"]) for step, _, _, _ in rows]
        assert any(len(set(pairs[i:i + 3])) == 3 for i in range(len(pairs) - 2)), "set %d: %r" % (which, pairs)


@pytest.mark.parametrize("seed", bs.SEEDS)
def test_class_planes_come_and_go_on_one_set(described, seed):
    rows = described[seed]
    classed = [c for _, _, _, c in rows]
    assert sum(classed) >= 2, classed
    found = False
    for of_set in same_set(rows):
        cl = [c for _, _, _, c in of_set]
        on_off = any(a and not b for a, b in zip(cl, cl[1:]))
        off_on = any(b and not a for a, b in zip(cl, cl[1:]))
        found = found or (on_off and off_on)
    assert found, classed


@pytest.mark.parametrize("seed", bs.SEEDS)
def test_long_columns_sweeps_over_class_planes_and_dedupe_off_after_on(described, seed, pool):
    rows = described[seed]
    lamps = pool[0]
    long_column = False
    for step, _, groups, _ in rows:
        cols = {}
        for l in step["launches"]:
            if l[0] == "stop":
                cols.setdefault((lamps[l[1]][0], lamps[l[1]][2]), []).append(l[1])
        long_column = long_column or any(len(v) > bs.DEDUPE_MAX and step["dedupe"] and len(set(v)) == 1 for v in cols.values())
    assert long_column, "no column of more than 31 launches that gets split"
    sweep_after_classes = False
    for of_set in same_set(rows):
        for (_, _, _, c0), (step, _, _, _) in zip(of_set, of_set[1:]):
            sweep_after_classes = sweep_after_classes or (c0 and any(l[0] == "sweep" for l in step["launches"]))
    assert sweep_after_classes, "no sweep step directly after a classed step of its set"
    dedupe = [step["dedupe"] for step, _, _, _ in rows]
    assert any(a and not b for a, b in zip(dedupe, dedupe[1:])), dedupe


def test_which_ranges_hold_multi_bit_masks(pkg, pool):
    """What the hook finds for 8 launches of A from SEED 0x1234 over every (first_gid, n) of the generator: a mask of several
    bits needs two launches that draw one hash input inside the range, and their gids lie apart by the launches' SEED shift --
    n = 1 can hold none (that would take two launches with one sum), n = 63 holds a handful at 2 000 000 only.  Both stay as
    the edge sizes they are (one ray; less than a wave); every range of 1000 and more holds hundreds, and the classed steps of
    every sequence are drawn from those (test_class_planes_come_and_go_on_one_set holds them to the hook)."""
    capi = pkg.capi
    lamps, length = pool
    prev, nxt, seed = [], [], bs.SEED0
    for _ in range(8):
        prev.append(seed)
        seed = capi.seed_next(lamps["A"], length, seed, 0)
        nxt.append(seed)
    for first in bs.FIRSTS:
        for n in bs.NS:
            m = capi.dedupe_plan(lamps["A"], prev, nxt, 0, first, n)
            multi = int(((m & (m - np.uint32(1)) & np.uint32(0x7fffffff)) != 0).sum())
            print("first_gid %8d n %6d: %6d of %6d occurrences hold several launches" % (first, n, multi, 8 * n))
            if n >= 1000:
                assert multi >= 100 and len(capi.dedupe_classes(lamps["A"], prev, nxt, 0, first, n, 32)[0]) > 0, (first, n)
            if n == 1:
                assert multi == 0
