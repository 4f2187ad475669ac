"""CPU: the tile form of the dedupe rule (csrc/uvrt_dedupe.h "one pass per key tile", reached through the host-only hook
uvrt_dedupe_plan_tiled) against the per-occurrence form (uvrt_dedupe_plan, which tests/test_dedupe_cpu.py holds to brute force).

The tile form inserts every launch's gid run of a key interval into a table and reads each occurrence's mask from its key's
entry; the device's k_dedupe_mark runs the same functions.  It must give uvrt_dedupe_plan's masks element for element,
whatever the tile width and whichever chunk of the range is asked for."""
import numpy as np
import pytest

import dedupe_tiled_cases as cases

WIDTHS = [64, 1000, None]          # None: the device's tile, capi.DEDUPE_TILE_KEYS


@pytest.fixture(scope="module")
def groups(pkg, orc, oscene, oroute):
    lamp0, length = cases.lamp0_of(orc, oscene, oroute)
    return {g.name: g for g in cases.groups(pkg.capi, lamp0, length)}


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("chunking", cases.CHUNKINGS)
@pytest.mark.parametrize("name", cases.NAMES)
def test_tiled_masks_equal_the_plan(pkg, groups, name, chunking, width):
    capi, g = pkg.capi, groups[name]
    width = capi.DEDUPE_TILE_KEYS if width is None else width
    want = cases.plan(capi, g)
    parts = []
    for first, n in g.chunks()[chunking]:
        got = capi.dedupe_plan_tiled(*g.args(), tile_keys=width, chunk_first=first, chunk_n=n)
        ref = want[:, first - g.first:first - g.first + n]
        assert got.shape == ref.shape
        assert np.array_equal(got, ref), "a mask differs"
        # the owners per launch of the chunk are its non-zero masks
        assert [int(x) for x in (got != 0).sum(axis=1)] == [int(x) for x in (ref != 0).sum(axis=1)]
        parts.append(got)
    if chunking == "meet":          # two chunks that meet: concatenated, the unchunked plan
        assert np.array_equal(np.concatenate(parts, axis=1), want)


def test_the_cases_hold_what_they_are_for(pkg, groups):
    """duplicates in every group; keys held twice where the sums tie or pass 2^28; a run of key 0 in seed mode 1"""
    capi = pkg.capi
    for g in groups.values():
        m = cases.plan(capi, g)
        solo = sum(int((m[k] == (1 << k)).sum()) for k in range(g.K))
        assert int((m != 0).sum()) < g.K * g.n or solo == g.K * g.n, g.name          # (ties in every launch: all traced alone)
        if g.name.startswith(("ties_first", "lx8", "mode1")) or g.name == "k8_first16000000":
            assert solo > 0, g.name
    for name, least in (("mode1_neg_first0", 2000), ("mode1_neg_long_first0", 4096), ("mode1_neg_long_first2000", 2048)):
        g = groups[name]
        zeros = sum(capi.seed_input(g.first + i, g.lamp, g.prev[0], g.nxt[0], 1) == 0 for i in range(0, g.n, 16)) * 16
        assert zeros > least, (name, zeros)


def test_arguments_that_are_refused(pkg, groups):
    capi, g = pkg.capi, groups["k2"]
    with pytest.raises(capi.UvrtError):
        capi.dedupe_plan_tiled(*g.args(), tile_keys=0)
    with pytest.raises(capi.UvrtError):
        capi.dedupe_plan_tiled(*g.args(), chunk_first=g.first + 10, chunk_n=g.n)          # ends past the range
    with pytest.raises(capi.UvrtError):
        capi.dedupe_plan_tiled(*g.args(), chunk_first=g.first - 1, chunk_n=10)
