"""CPU: the mark pass over strips of narrow tiles (csrc/uvrt_dedupe.h "strips of narrow tiles"), through the host-only hook
uvrt_dedupe_plan_tiled, against the per-occurrence definition (uvrt_dedupe_plan, which tests/test_dedupe_cpu.py holds to
brute force).

What the strips add to the tile rule, and what can break it: a tile's run bounds are carried from the tile before (only a
strip's first tile searches), a run ends where its keys leave the tile (dedupe_in_tile), and an occurrence sets the "held
twice" flag from the keys of its two neighbouring gids (dedupe_run_twice) instead of reading the table back.  The device's
k_dedupe_mark runs these functions with the width DEDUPE_MARK_KEYS; here they run at that width, at widths around it and at
one key per tile's worth of strips, for every group of tests/dedupe_tiled_cases.py and tests/dedupe_strip_cases.py."""
import numpy as np
import pytest

import dedupe_strip_cases as strips
import dedupe_tiled_cases as cases

WIDTHS = [None, 17, 959]          # None: the device's, capi.DEDUPE_MARK_KEYS; a gid's worth of keys; an odd width just below it


@pytest.fixture(scope="module")
def groups(pkg, orc, oscene, oroute):
    lamp0, length = cases.lamp0_of(orc, oscene, oroute)
    out = {g.name: g for g in cases.groups(pkg.capi, lamp0, length)}
    out.update({g.name: g for g in strips.groups(pkg.capi, lamp0, length)})
    return out


def expected(capi, g):
    return strips.plan(capi, g) if g.name in strips.NAMES else cases.plan(capi, g)


def test_the_constants_agree_with_the_header(pkg):
    capi = pkg.capi
    assert capi.DEDUPE_MARK_KEYS == 960 and capi.DEDUPE_MARK_KEYS % 64 == 0 and capi.DEDUPE_STRIP_TILES == 4
    assert capi.DEDUPE_MARK_KEYS * 4 <= 5 * 1024          # a wave's table within its share of the LDS beside a traversal grid


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("chunking", strips.CHUNKINGS)
@pytest.mark.parametrize("name", list(cases.NAMES) + strips.NAMES)
def test_strip_masks_equal_the_plan(pkg, groups, name, chunking, width):
    capi, g = pkg.capi, groups[name]
    width = capi.DEDUPE_MARK_KEYS if width is None else width
    want = expected(capi, g)
    parts = []
    for first, n in strips.chunks(g, chunking):
        got = capi.dedupe_plan_tiled(*g.args(), tile_keys=width, chunk_first=first, chunk_n=n)
        ref = want[:, first - g.first:first - g.first + n]
        assert got.shape == ref.shape
        assert np.array_equal(got, ref), "a mask differs"
        parts.append(got)
    if chunking == "meet":
        assert np.array_equal(np.concatenate(parts, axis=1), want)


@pytest.mark.parametrize("strip", [1, 3, 8, 1024])
@pytest.mark.parametrize("name", ["k8_first0", "ties_first9000000", "mode1_neg_long_first2000", "straddle_2_25", "k31"])
def test_masks_do_not_depend_on_the_strip_length(pkg, groups, name, strip):
    """the device's strips are DEDUPE_STRIP_TILES tiles and longer (its launcher's choice, or the developer's): every tile a
    search of its own, odd strips, the longest default, and one strip for the whole chunk"""
    capi, g = pkg.capi, groups[name]
    want = expected(capi, g)
    for chunking in ("whole", "odd"):
        for first, n in strips.chunks(g, chunking):
            got = capi.dedupe_plan_tiled(*g.args(), tile_keys=capi.DEDUPE_MARK_KEYS, chunk_first=first, chunk_n=n, strip_tiles=strip)
            assert np.array_equal(got, want[:, first - g.first:first - g.first + n]), "a mask differs"
    with pytest.raises(capi.UvrtError):
        capi.dedupe_plan_tiled(*g.args(), tile_keys=capi.DEDUPE_MARK_KEYS, strip_tiles=0)


def test_the_cases_hold_what_they_are_for(pkg, groups):
    capi = pkg.capi
    # the ulp changes inside the range of every launch
    for name, power in strips.STRADDLES.items():
        g = groups[name]
        for k in range(g.K):
            lo, hi = strips.keys_of(capi, g, k, [g.first, g.first + g.n - 1])
            assert lo < power < hi, (name, k)
    # ties: keys held twice, occurrences traced alone
    for first in (9000000, 10000000, 15000000):
        g = groups["ties4096_first%d" % first]
        m = strips.plan(capi, g)
        assert sum(int((m[k] == (1 << k)).sum()) for k in range(g.K)) > 0
    # equal SEED pairs: the second launch owns nothing, the first everything
    m = strips.plan(capi, groups["k2_equal_seeds"])
    assert not m[1].any() and (m[0] == 3).all()
    assert strips.plan(capi, groups["k31"]).shape[0] == 31
