"""GPU: the knobs that move a batch's planes, run with dedupe groups and mask classes in the batch.

A buffer set holds the launch planes at a stride of R x T counters -- R chosen per call from n and capped by UVRT_REPLICAS --
and behind them the class planes, of which the first cls_repl = min(UVRT_DEDUPE_CLASS_REPLICAS, R) replicas take deposits and
which UVRT_DEDUPE_CLASS_MB deals to the groups; UVRT_BATCH_LANES and UVRT_BATCH_CHUNK_MB decide which lane's scratch a chunk of
a group uses.  The variables are read once in uvrt_create.  Two shapes -- 8 launches of lamp A, and A B A B ... of 10 -- run
twice each on one context, so both sets see both shapes and the second shape's planes lie over the first one's class planes.
Demanded against a default context with dedupe off: planes, both maps, dose, colour and SEED bit-identical,
uvrt_batch_residue() == 0 after every replay, and uvrt_batch_deposits equal to the host hook's figure."""
import numpy as np
import pytest

from test_gpu_dedupe import env, oracle_counts  # noqa: F401 (env: a fixture)
from test_gpu_dedupe_classes import expected_deposits, groups_of, make_ops, results

pytestmark = pytest.mark.gpu

FIRST, N = 1200000, 4096
KNOBS = ("UVRT_REPLICAS", "UVRT_DEDUPE_CLASS_REPLICAS", "UVRT_DEDUPE_CLASS_MB", "UVRT_BATCH_LANES", "UVRT_BATCH_CHUNK_MB")


def shapes(env):
    a, b = env["lamps"]
    return [[a] * 8, [a, b] * 5]


def new_ctx(env, dedupe=True):
    c = env["capi"].Ctx(0)
    s = env["scene"]
    c.set_scene(s.tris, s.nodes, s.triIdx)
    c.set_dedupe(dedupe)
    c.reset(True)
    return c


def run_batch(env, c, lamps, first, n, read):
    """reset, one batch from SEED 0, replayed (after reading every plane, or straight from the planes)"""
    c.reset(True)
    c.seed = 0
    c.trace_batch(lamps, env["length"], first, n)
    out = {"traced": c.batch_traced_rays(), "deposits": c.batch_deposits()}
    if read:
        out["counts"] = [c.read_batch_counts(k) for k in range(len(lamps))]
    c.replay_batch(make_ops(env["capi"], len(lamps), n))
    out["seed"] = c.seed
    out.update(results(c))
    return out


_reference = {}


def reference(env, monkeypatch, n):
    """per shape the batch on a default context (no knob in the environment) with dedupe off: made once per n"""
    if n not in _reference:
        for name in KNOBS:
            monkeypatch.delenv(name, raising=False)
        c = new_ctx(env, dedupe=False)
        try:
            _reference[n] = [run_batch(env, c, lamps, FIRST, n, True) for lamps in shapes(env)]
        finally:
            c.close()
        for ref, lamps in zip(_reference[n], shapes(env)):
            assert ref["traced"] == len(lamps) * n and ref["deposits"] == 0
            assert sum(int(cn.sum()) for cn in ref["counts"]) > 0.5 * len(lamps) * n
    return _reference[n]


def run_knob(env, monkeypatch, n, settings):
    """-> per shape the deposits of its two runs' first: both shapes twice on one context created under `settings`, each
    held to the reference"""
    ref = reference(env, monkeypatch, n)
    for name, value in settings.items():
        monkeypatch.setenv(name, str(value))
    c = new_ctx(env)
    deposits = []
    try:
        for which, lamps in enumerate(shapes(env)):
            for again in range(2):          # (the first run is read plane by plane, the second replayed from the planes)
                got = run_batch(env, c, lamps, FIRST, n, again == 0)
                what = "%r shape %d run %d" % (settings, which, again)
                if again == 0:
                    for k in range(len(lamps)):
                        assert np.array_equal(got["counts"][k], ref[which]["counts"][k]), what + ": plane %d" % k
                    deposits.append(got["deposits"])
                for name in ("sum", "max", "dose", "colour"):
                    assert np.array_equal(got[name], ref[which][name]), what + ": " + name
                assert got["seed"] == ref[which]["seed"], what
                assert got["traced"] < len(lamps) * n, what + ": nothing was deduped"
                assert got["deposits"] == deposits[which], what
                assert c.batch_residue() == 0, what + ": counters left in the planes"
    finally:
        c.close()
    return deposits


def hook_deposits(env, n):
    return [expected_deposits(env, lamps, FIRST, n, None, 0, 0) for lamps in shapes(env)]


@pytest.mark.parametrize("replicas", [1, 2, 3])
def test_replicas(env, monkeypatch, replicas):
    """R = min(UVRT_REPLICAS, 8) and cls_repl = min(4, R): strides of 1, 2 and 3 x T, and at 3 a quad of lanes that does not
    divide the replicas"""
    assert run_knob(env, monkeypatch, N, {"UVRT_REPLICAS": replicas}) == hook_deposits(env, N)


@pytest.mark.parametrize("replicas", [1, 3, 16])
def test_class_replicas(env, monkeypatch, replicas):
    """16 is clamped to the batch's R = 8: every replica of a class plane takes deposits"""
    assert run_knob(env, monkeypatch, N, {"UVRT_DEDUPE_CLASS_REPLICAS": replicas}) == hook_deposits(env, N)


def class_cap(env, mb, R=8):
    """class planes a buffer set holds: min(64, MB x 2^20 / (R x T x 4)) (UVRT_DEDUPE_CLASS_MB)"""
    return min(64, (mb << 20) // (R * env["scene"].T * 4))


def test_class_budget_of_no_plane(env, monkeypatch):
    """1 MB is less than one plane of 8 x 44 866 counters: classes are on and get nothing, every ray deposits per launch"""
    assert env["scene"].T == 44866 and class_cap(env, 1) == 0
    got = run_knob(env, monkeypatch, N, {"UVRT_DEDUPE_CLASS_MB": 1})
    assert got == [sum(len(p) for _, p, _ in groups_of(env, lamps, 0, 0)) * N for lamps in shapes(env)]
    assert got == [expected_deposits(env, lamps, FIRST, N, 0, 0, 0) for lamps in shapes(env)]


def test_class_budget_of_two_planes(env, monkeypatch):
    """3 MB: two class planes.  The single group gets its two most frequent classes; A B A B deals the two to its groups by
    sampled frequency, a to A's and 2 - a to B's."""
    capi = env["capi"]
    assert class_cap(env, 3) == 2
    got = run_knob(env, monkeypatch, N, {"UVRT_DEDUPE_CLASS_MB": 3})
    one, two = shapes(env)
    (lamp, prev, nxt), = groups_of(env, one, 0, 0)
    assert got[0] == capi.dedupe_classes(lamp, prev, nxt, 0, FIRST, N, 2)[1]
    assert got[0] < capi.dedupe_classes(lamp, prev, nxt, 0, FIRST, N, 0)[1], "two classes save nothing: the case shows nothing"
    (la, pa, na), (lb, pb, nb) = groups_of(env, two, 0, 0)
    ok = [capi.dedupe_classes(la, pa, na, 0, FIRST, N, a)[1] + capi.dedupe_classes(lb, pb, nb, 0, FIRST, N, 2 - a)[1] for a in range(3)]
    assert got[1] in ok, "A B A B: %d deposits, acceptable with (0, 2), (1, 1), (2, 0) classes for (A, B): %r" % (got[1], ok)


@pytest.mark.parametrize("lanes", [1, 3])
def test_batch_lanes(env, monkeypatch, lanes):
    """1 MB chunks cut the range of 20 000 into three chunks for the group of 8 (tests/test_gpu_dedupe_mark.py) and into two for
    the groups of 5: on one lane they share one scratch and one set of owner counters back to back, on three each chunk of a
    group has its own"""
    n = 20000
    assert run_knob(env, monkeypatch, n, {"UVRT_BATCH_LANES": lanes, "UVRT_BATCH_CHUNK_MB": 1}) == hook_deposits(env, n)


def test_twelve_replicas_and_eight_share_the_sets(env, monkeypatch):
    """R = 12 from n = 786 432 on (12 x 131 072 <= 2 n), with cls_repl = 4; R = 8 below.  3 launches of lamp A: big, small,
    big, small on one context -- the batches alternate between the sets, so big meets big and small meets small -- and then
    small and big once more, which puts each over the other's planes.  Every batch equals a fresh context's."""
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    big, small = 786432, N
    lamps = [env["lamps"][0]] * 3
    fresh = {}
    for n in (big, small):
        c = new_ctx(env)
        try:
            fresh[n] = run_batch(env, c, lamps, FIRST, n, True)
            assert c.batch_residue() == 0
        finally:
            c.close()
        # launch 1 of each against the oracle, at its place in the SEED chain
        seed1 = env["capi"].seed_next(lamps[0], env["length"], 0, 0)
        want = oracle_counts(env, lamps[:1], FIRST, n, seed=seed1)[0]
        assert np.array_equal(fresh[n]["counts"][1], want) and want.sum() > 0.5 * n, n
        assert fresh[n]["deposits"] == expected_deposits(env, lamps, FIRST, n, None, 0, 0)
    assert fresh[big]["traced"] < 3 * big, "nothing was deduped"
    assert fresh[big]["deposits"] < 3 * big, "no class saves a deposit: the class planes are idle"
    c = new_ctx(env)
    try:
        for i, n in enumerate((big, small, big, small, small, big)):
            got = run_batch(env, c, lamps, FIRST, n, i < 2)
            what = "batch %d (n = %d)" % (i, n)
            if i < 2:
                for k in range(3):
                    assert np.array_equal(got["counts"][k], fresh[n]["counts"][k]), what + ": plane %d" % k
            for name in ("sum", "max", "dose", "colour", "seed", "traced", "deposits"):
                assert np.array_equal(got[name], fresh[n][name]), what + ": " + name
            assert c.batch_residue() == 0, what + ": counters left in the planes"
    finally:
        c.close()
