"""CPU: the period table of a dedupe group (csrc/uvrt_dedupe.h "period table"; include/uvrt.h uvrt_dedupe_plan_periodic)
against the per-occurrence definition (uvrt_dedupe_plan, which tests/test_dedupe_cpu.py holds to brute force).

uvrt_dedupe_plan_periodic runs what a batch and its kernels run with the table on: the host builds the interiors and their
tables, the key intervals between them go through the tile functions of the mark pass, an interior occurrence's mask is read
from the table by its gid's residue, and the owners per launch and block of 2 048 gids come from the table in closed form.
Masks and owner counts must be uvrt_dedupe_plan's element for element on every group of tests/dedupe_tiled_cases.py and
tests/dedupe_strip_cases.py -- first gid 0, the ties, seed mode 1's runs of key 0, keys across 2^24 and 2^25, 31 / 17 / 16 / 2
launches -- and on four groups of the headline's lamp and SEED chain where the table carries real weight.  There the share of
occurrences taken from the table is held from below, so that a build which quietly sends everything down the general path
cannot pass: the interiors lose a margin of a few dozen gids at each of a stratum's ends and whatever the caps leave out (12
interiors, the longest; the headline's nine long ones hold 0.97 of it), which puts the headline group above 0.9 and a range
of 32 768 gids inside one or two strata above 0.5."""
import numpy as np
import pytest

import dedupe_strip_cases as strips
import dedupe_tiled_cases as cases
from test_dedupe_cpu import seed_chain
from test_gpu_dedupe_mark import block_owners

# the four groups of the table path: (first gid, n, least share of occurrences from the table)
WEIGHT = {"constant": (300000, 32768, 0.5), "period4": (1500000, 32768, 0.5), "cluster_2_24": (970000, 32768, 0.0),
          "headline": (0, 2073600, 0.9)}


@pytest.fixture(scope="module")
def lamp0(orc, oscene, oroute):
    return cases.lamp0_of(orc, oscene, oroute)


@pytest.fixture(scope="module")
def groups(pkg, lamp0):
    out = {g.name: g for g in cases.groups(pkg.capi, *lamp0)}
    out.update({g.name: g for g in strips.groups(pkg.capi, *lamp0)})
    return out


def expected(capi, g):
    return strips.plan(capi, g) if g.name in strips.NAMES else cases.plan(capi, g)


def check(capi, g, ref, first, n):
    masks, owners, from_table = capi.dedupe_plan_periodic(*g.args(), chunk_first=first, chunk_n=n)
    want = ref[:, first - g.first:first - g.first + n]
    assert np.array_equal(masks, want), "a mask differs"
    assert np.array_equal(owners, block_owners(want, capi.DEDUPE_BLOCK_GIDS)), "the owners of a block differ"
    return from_table


@pytest.mark.parametrize("name", cases.NAMES + strips.NAMES)
def test_case_lists(pkg, groups, name):
    capi, g = pkg.capi, groups[name]
    ref = expected(capi, g)
    for chunking in strips.CHUNKINGS:
        for first, n in strips.chunks(g, chunking):
            check(capi, g, ref, first, n)


@pytest.mark.parametrize("name", list(WEIGHT))
def test_table_path_carries_weight(pkg, lamp0, name):
    capi = pkg.capi
    first, n, share = WEIGHT[name]
    lamp, length = lamp0
    prev, nxt = seed_chain(capi, lamp, length, 8, 0, 0)
    g = cases.Group(name, lamp, prev, nxt, 0, first, n)
    ref = capi.dedupe_plan(*g.args())
    from_table = check(capi, g, ref, first, n)
    print("%s: %d of %d occurrences from the table (%.4f)" % (name, from_table, 8 * n, from_table / (8.0 * n)))
    assert from_table >= share * 8 * n
    if n <= 32768:          # a chunk that starts and ends inside a block, and two that meet
        check(capi, g, ref, first + 700, 3001)
        cut = n // 2 + 37
        assert check(capi, g, ref, first, cut) + check(capi, g, ref, first + cut, n - cut) == from_table
