"""The dedupe groups that tests/test_dedupe_strips_cpu.py and tests/test_gpu_dedupe_generate.py add to those of
tests/dedupe_tiled_cases.py for the mark pass over strips of narrow tiles (csrc/uvrt_dedupe.h "strips of narrow tiles"): a
group of 31 launches, the ties of [2^27, 2^28) over 4 096 gids, ranges whose keys straddle 2^24 and 2^25 (the ulp changes
inside a strip), and two launches with EQUAL SEED pairs (every occurrence of the second one is absorbed: a launch without an
owner).  The expected masks are uvrt_dedupe_plan's, computed once per group and shared (read only)."""
import numpy as np

import dedupe_tiled_cases as cases
from test_dedupe_cpu import seed_chain, tie_chain

NAMES = ["k31"] + ["ties4096_first%d" % f for f in (9000000, 10000000, 15000000)] + ["straddle_2_24", "straddle_2_25", "k2_equal_seeds"]
# the chunks a group is looked at through: tests/dedupe_tiled_cases.py's, and one that starts and ends inside a tile and inside
# a block of 2 048 gids, neither a multiple of 256 nor of 64 long
CHUNKINGS = cases.CHUNKINGS + ["odd"]
STRADDLES = {"straddle_2_24": 1 << 24, "straddle_2_25": 1 << 25}


def chunks(g, chunking):
    if chunking == "odd":
        return [(g.first + 700, 3001)]
    return g.chunks()[chunking]


def groups(capi, lamp0, length):
    out = []

    def chained(name, K, first, n):
        prev, nxt = seed_chain(capi, lamp0, length, K, 0, 0)
        out.append(cases.Group(name, lamp0, prev, nxt, 0, first, n))

    chained("k31", 31, 1200000, 4096)
    for first in (9000000, 10000000, 15000000):
        prev, nxt = tie_chain(6, 16, cases.TIE_SEED)
        out.append(cases.Group("ties4096_first%d" % first, cases.ORDINARY_LAMP, prev, nxt, 0, first, 4096))
    # key ~ 17 gid + offset, offset below 2^17 + the lamp's terms: 10 000 gids from 7 700 gids before (2^b / 17) on hold the
    # power of two in every launch (test_dedupe_strips_cpu.py asserts it)
    chained("straddle_2_24", 8, (1 << 24) // 17 - 8500, 10000)
    chained("straddle_2_25", 8, (1 << 25) // 17 - 8500, 10000)
    prev, nxt = seed_chain(capi, lamp0, length, 1, 0, 0)
    out.append(cases.Group("k2_equal_seeds", lamp0, prev * 2, nxt * 2, 0, 1200000, 4096))
    assert [g.name for g in out] == NAMES
    return out


_plans = {}


def plan(capi, g):
    if g.name not in _plans:
        m = capi.dedupe_plan(*g.args())
        m.setflags(write=False)
        _plans[g.name] = m
    return _plans[g.name]


def keys_of(capi, g, k, gids):
    """the keys of launch k at `gids`: the hash inputs as int32 (work-item 0's sum may be negative)"""
    h = np.array([capi.seed_input(int(x), g.lamp, g.prev[k], g.nxt[k], g.mode) for x in gids], dtype=np.uint32)
    return h.view(np.int32).astype(np.int64)
