"""CPU: which photons of a lamp column are the same photon (csrc/uvrt_dedupe.h, reached through the host-only hooks
uvrt_seed_input / uvrt_dedupe_plan of the C ABI library) against brute force.

The brute force restates generate.cl:13 in numpy -- the f32 sum 17 gid + 1 + 13 lx + 7 ly + 11 lz + (SEED >> 15), float -> uint
through int64 -- for every (launch, gid) of the group, puts all hash inputs through np.unique and applies the rule to the
counts: an input some launch holds twice and more is traced by each occurrence alone; otherwise the first launch that holds it
owns it with the mask of all launches that do.  Compared: the set of owners, every mask, and the sum over the masks' bits per
launch (every occurrence deposited exactly once)."""
import numpy as np
import pytest

from conftest import ROUTE


def np_seed_input(gids, lamp, seed_prev, seed_next, mode):
    f = np.float32
    gids = np.asarray(gids, dtype=np.int64)
    seed = np.where((gids == 0) | (mode == 1), np.uint32(seed_prev), np.uint32(seed_next)).astype(np.uint32)
    acc = ((gids * 17 + 1) & 0xFFFFFFFF).astype(np.uint32).view(np.int32).astype(f)      # int threadID arithmetic
    acc = acc + f(lamp[0]) * f(13.0)
    acc = acc + f(lamp[1]) * f(7.0)
    acc = acc + f(lamp[2]) * f(11.0)
    acc = acc + (seed >> np.uint32(15)).astype(f)
    assert acc.dtype == np.float32
    s = acc.astype(np.int64)
    if mode == 1:
        s = np.where(acc < 0, 0, s)
    return (s & 0xFFFFFFFF).astype(np.uint32)


def seed_chain(capi, lamp, length, count, seed0, mode):
    prev, nxt, s = [], [], seed0
    for _ in range(count):
        prev.append(s)
        s = capi.seed_next(lamp, length, s, mode)
        nxt.append(s)
    return prev, nxt


def brute_masks(h):
    """h: uint32[K][n] hash inputs -> expected masks uint32[K][n]"""
    K, n = h.shape
    uniq, inv = np.unique(h.reshape(-1), return_inverse=True)
    inv = inv.reshape(K, n)
    ones = np.zeros(uniq.size, dtype=np.uint32)
    many = np.zeros(uniq.size, dtype=bool)
    for j in range(K):
        cnt = np.bincount(inv[j], minlength=uniq.size)
        ones |= (cnt == 1).astype(np.uint32) << np.uint32(j)
        many |= cnt >= 2
    first = ones & (~ones + np.uint32(1))          # lowest set bit: the owner's launch
    out = np.empty((K, n), dtype=np.uint32)
    for k in range(K):
        bit = np.uint32(1 << k)
        u = inv[k]
        out[k] = np.where(many[u], bit, np.where(first[u] == bit, ones[u], np.uint32(0)))
    return out, uniq.size


def check_group(capi, lamp, length, K, seed0, mode, first_gid, n, chain=None):
    prev, nxt = chain if chain is not None else seed_chain(capi, lamp, length, K, seed0, mode)
    gids = first_gid + np.arange(n, dtype=np.int64)
    h = np.stack([np_seed_input(gids, lamp, prev[k], nxt[k], mode) for k in range(K)])
    # the seed function itself, at the ends and at gid 0's neighbours
    for k in (0, K - 1):
        for i in (0, 1, n // 2, n - 1):
            assert capi.seed_input(first_gid + i, lamp, prev[k], nxt[k], mode) == int(h[k, i])
    want, distinct = brute_masks(h)
    got = capi.dedupe_plan(lamp, prev, nxt, mode, first_gid, n)
    assert np.array_equal(got != 0, want != 0), "the set of owners differs"
    assert np.array_equal(got, want), "a mask differs"
    per_launch = [int(((got >> np.uint32(j)) & 1).sum()) for j in range(K)]
    assert per_launch == [n] * K, "an occurrence is deposited twice or not at all"
    return got, want, distinct


@pytest.fixture(scope="module")
def lamp0(orc, oscene, oroute):
    comp = orc.Computation(oscene, oroute["lamps"], 1 << 16, oroute["lightHeight"], oroute["lightLength"], oroute["lightIntensity"])
    return tuple(float(x) for x in comp.lamp_world_pos(oroute["lamps"][0])), oroute["lightLength"]


def test_headline_shape_has_8418915_owners(pkg, lamp0):
    """lamp 0, 8 x 2 073 600 from SEED 0: 16 588 800 photons, 8 418 915 distinct; the chain ends at the census's SEED"""
    lamp, length = lamp0
    prev, nxt = seed_chain(pkg.capi, lamp, length, 8, 0, 0)
    assert nxt[-1] == 0xbf71c277
    got, want, distinct = check_group(pkg.capi, lamp, length, 8, 0, 0, 0, 2073600)
    assert int((got != 0).sum()) == distinct == 8418915


@pytest.mark.parametrize("first_gid", [0, 1200000, 2000000])
def test_small_ranges(pkg, lamp0, first_gid):
    """8 x 4 096: a range that starts at gid 0 (work-item 0 reads the other SEED) and two that do not"""
    lamp, length = lamp0
    got, _, distinct = check_group(pkg.capi, lamp, length, 8, 0, 0, first_gid, 4096)
    assert int((got != 0).sum()) == distinct < 8 * 4096


def test_sums_past_2_28_are_not_injective(pkg, lamp0):
    """from gid 16 000 000 the sums pass 2^28 (ulp 32 > 17): a launch holds an input twice, and those are traced alone"""
    lamp, length = lamp0
    got, want, distinct = check_group(pkg.capi, lamp, length, 8, 0, 0, 16000000, 8192)
    solo = sum(int((got[k] == (1 << k)).sum()) for k in range(8))
    assert distinct < int((got != 0).sum()) and solo > 0


def stepped_chain(K, seed0, step):
    """a SEED chain of our own: launch j reads seed0 + j * step before and seed0 + (j + 1) * step after"""
    seeds = [(seed0 + j * step) & 0xFFFFFFFF for j in range(K + 1)]
    return seeds[:-1], seeds[1:]


def tie_chain(K, grid, seed0):
    """SEEDs whose SEED >> 15 is half a grid step above a multiple of `grid` in every launch: the last add of the sum is a tie"""
    seeds = []
    v = seed0 >> 15
    for j in range(K + 1):
        v = (v + 1000 * j + grid) // grid * grid + grid // 2
        seeds.append((v << 15) & 0xFFFFFFFF)
    return seeds[:-1], seeds[1:]


@pytest.mark.parametrize("first_gid", [9000000, 10000000, 15000000])
@pytest.mark.parametrize("case", ["ordinary", "lx8", "ties", "zero_lamp_ties"])
def test_sums_in_2_27_to_2_28_hold_keys_twice(pkg, case, first_gid):
    """ulp 16 against a step of 17: an add that ties rounds two neighbouring gids to one key -- SEED >> 15 = 8 mod 16, or a lamp
    with lx = 8 -- so a launch holds keys twice although no ulp has reached 17; those occurrences are traced alone"""
    n, K = 4000, 6
    lamp = {"ordinary": (-1.5, 1.25, 2.0), "lx8": (8.0, 0.0, 0.0), "ties": (-1.5, 1.25, 2.0), "zero_lamp_ties": (0.0, 0.0, 0.0)}[case]
    chain = tie_chain(K, 16, 0x02468ace) if "ties" in case else stepped_chain(K, 0x02468ace, 0x3c6ef372)
    got, want, distinct = check_group(pkg.capi, lamp, 1.0, K, 0, 0, first_gid, n, chain=chain)
    if case != "ordinary":
        assert sum(int((got[k] == (1 << k)).sum()) for k in range(K)) > 0 and distinct < K * n


@pytest.mark.parametrize("first_gid,grid", [(1100000, 2), (2500000, 4), (5000000, 8), (7800000, 8)])
@pytest.mark.parametrize("case", ["ordinary", "half_grid_lamp", "ties"])
def test_ties_below_2_27(pkg, case, first_gid, grid):
    """the same adversaries one, two and three binades further down (the headline's and the route's sums live there)"""
    n, K = 4000, 6
    lamp = (grid / 2.0, 0.0, 0.0) if case == "half_grid_lamp" else (-1.5, 1.25, 2.0)
    chain = tie_chain(K, grid, 0x02468ace) if case == "ties" else stepped_chain(K, 0x02468ace, 0x3c6ef372)
    check_group(pkg.capi, lamp, 1.0, K, 0, 0, first_gid, n, chain=chain)


def test_seed_mode_1_with_negative_sums(pkg, lamp0):
    """seed mode 1, a lamp whose first sums are negative: they all convert to 0, one input many times over"""
    length = lamp0[1]
    lamp = (-2000.0, 1.25, -1500.0)          # 13 lx + 11 lz = -42 500: the first ~2 500 gids are negative
    for first_gid in (0, 2000):
        got, want, _ = check_group(pkg.capi, lamp, length, 5, 0x1234, 1, first_gid, 6000)
        h0 = np_seed_input(first_gid + np.arange(6000), lamp, 0x1234, 0, 1)
        assert (h0 == 0).sum() > 100 and np.array_equal(got[0][h0 == 0], np.full((h0 == 0).sum(), 1, dtype=np.uint32))


def test_two_halves_as_shards(pkg, lamp0):
    """the halves of a range, each deduped within itself: every occurrence of each half deposited once"""
    lamp, length = lamp0
    whole, _, _ = check_group(pkg.capi, lamp, length, 8, 0, 0, 1000000, 8192)
    lo, _, _ = check_group(pkg.capi, lamp, length, 8, 0, 0, 1000000, 4096)
    hi, _, _ = check_group(pkg.capi, lamp, length, 8, 0, 0, 1004096, 4096)
    # a shard sees fewer duplicates than the whole range does
    assert int((lo != 0).sum()) + int((hi != 0).sum()) >= int((whole != 0).sum())


def test_groups_that_are_refused(pkg, lamp0):
    lamp, length = lamp0
    prev, nxt = seed_chain(pkg.capi, lamp, length, 2, 0, 0)
    with pytest.raises(pkg.capi.UvrtError):
        pkg.capi.dedupe_plan(lamp, prev, nxt, 0, 126322567 - 10, 64)          # 17 gid + 1 leaves int32
    with pytest.raises(pkg.capi.UvrtError):
        pkg.capi.dedupe_plan((float("nan"), 0.0, 0.0), prev, nxt, 0, 0, 64)
