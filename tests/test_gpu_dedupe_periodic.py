"""GPU: the period table of a dedupe group on the device (include/uvrt.h uvrt_set_dedupe_periodic; csrc/uvrt_dedupe.h "period
table"; csrc/uvrt_kernels.hip k_dedupe_mark, k_dedupe_write).

With the table on, the mark pass walks only the key intervals between the group's interiors, counts the interiors' owners
from the table in closed form, and the write pass takes an interior occurrence's deposit word from the table instead of the
mark pass's scratch.  Nothing a batch computes may change by a bit.

* The generate chain alone (uvrt_dedupe_generate_device): 8 launches of the headline's lamp and SEED chain, 32 768 gids from
  gid 300 000 (a constant pattern), 970 000 (the strata around 2^24) and 1 500 000 (period 4), and 4 096 gids from gid 0 (no
  interior: the general path alone).  Compacted rays, deposit words, the ray count and the deposit count with the table on
  equal those with it off, without classes and with the default's; without classes the words are the owners' masks of
  uvrt_dedupe_plan in (launch, gid) order, and with them the deposit count is uvrt_dedupe_classes'.  The CPU form of the
  rule (tests/test_dedupe_periodic_cpu.py) says how many of the occurrences the table takes: more than half in the three
  long cases, none in the short one, so that the cases show what they are meant to.
* One whole batch and its replay, 8 x 32 768 from gid 1 500 000: traced rays, deposits, every launch's plane, both maps,
  dose and colours on and off, in flavours 0 and 1 and seed modes 0 and 1."""
import numpy as np
import pytest

import dedupe_tiled_cases as cases
from test_dedupe_cpu import seed_chain
from test_gpu_dedupe import bits, bits64, env  # noqa: F401 (env: a fixture)
from test_gpu_dedupe_classes import make_ops, results

pytestmark = pytest.mark.gpu

K = 8
CHAIN_CASES = [(300000, 32768), (970000, 32768), (1500000, 32768), (0, 4096)]


@pytest.fixture(scope="module")
def lamp0(orc, oscene, oroute):
    return cases.lamp0_of(orc, oscene, oroute)


_plans = {}


def plan(capi, lamp, length, first, n):
    """(SEEDs before, SEEDs after, uvrt_dedupe_plan's masks, occurrences the table takes), once per case"""
    if (first, n) not in _plans:
        prev, nxt = seed_chain(capi, lamp, length, K, 0, 0)
        masks = capi.dedupe_plan(lamp, prev, nxt, 0, first, n)
        masks.setflags(write=False)
        _plans[(first, n)] = (prev, nxt, masks, capi.dedupe_plan_periodic(lamp, prev, nxt, 0, first, n)[2])
    return _plans[(first, n)]


def generate(capi, lamp, length, prev, nxt, first, n, classes, periodic):
    c = capi.Ctx(0)
    try:
        c.set_dedupe_classes(classes)
        c.set_dedupe_periodic(periodic)
        assert c.get_dedupe_periodic() == periodic
        return c.dedupe_generate_device(lamp, length, prev, nxt, 0, first, n)
    finally:
        c.close()


@pytest.mark.parametrize("first,n", CHAIN_CASES)
def test_generate_chain_alone(pkg, lamp0, first, n):
    capi = pkg.capi
    lamp, length = lamp0
    prev, nxt, masks, from_table = plan(capi, lamp, length, first, n)
    if n > 4096:          # (the short case is gid 0's: the general path at the start of the range, whatever else it holds)
        assert from_table > K * n // 2, "the case does not show what it is meant to"
    owners = masks[masks != 0]          # (launch, gid) order
    for classes in (0, capi.dedupe_classes_default()):
        rays_off, words_off, dep_off = generate(capi, lamp, length, prev, nxt, first, n, classes, False)
        rays_on, words_on, dep_on = generate(capi, lamp, length, prev, nxt, first, n, classes, True)
        assert len(words_on) == len(words_off) == owners.size, "the ray count"
        assert np.array_equal(words_on, words_off), "a deposit word differs"
        assert np.array_equal(bits(rays_on), bits(rays_off)), "a ray differs"
        assert dep_on == dep_off == capi.dedupe_classes(lamp, prev, nxt, 0, first, n, classes)[1]
        if classes == 0:
            assert np.array_equal(words_off, owners), "table off: the words are not the plan's masks"
            assert np.array_equal(words_on, owners), "table on: the words are not the plan's masks"


def run_batch(env, lamp, first, n, periodic, flavour, mode):
    capi, s = env["capi"], env["scene"]
    c = capi.Ctx(0)
    try:
        c.set_scene(s.tris, s.nodes, s.triIdx)
        c.set_flavour(flavour)
        c.set_seed_mode(mode)
        c.set_dedupe_periodic(periodic)
        c.reset(True)
        c.seed = 0
        c.trace_batch([lamp] * K, env["length"], first, n)
        out = {"counts": [c.read_batch_counts(k) for k in range(K)], "traced": c.batch_traced_rays(), "deposits": c.batch_deposits()}
        c.replay_batch(make_ops(capi, K, n))
        out["residue"] = c.batch_residue()
        out.update(results(c))
        return out
    finally:
        c.close()


@pytest.mark.parametrize("flavour,mode", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_whole_batch_on_and_off(env, lamp0, flavour, mode):  # noqa: F811
    lamp, _ = lamp0
    first, n = 1500000, 32768
    off = run_batch(env, lamp, first, n, False, flavour, mode)
    on = run_batch(env, lamp, first, n, True, flavour, mode)
    assert on["traced"] == off["traced"] < K * n and on["deposits"] == off["deposits"] and on["residue"] == off["residue"] == 0
    for k in range(K):
        assert np.array_equal(on["counts"][k], off["counts"][k]), "launch %d: a plane differs" % k
    assert sum(int(p.sum()) for p in off["counts"]) > 0.5 * K * n
    for what in ("sum", "max", "dose", "colour"):
        assert np.array_equal(on[what], off[what]), what
