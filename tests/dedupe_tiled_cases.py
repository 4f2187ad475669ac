"""The dedupe groups that tests/test_dedupe_tiled_cpu.py and tests/test_gpu_dedupe_mark.py put through the tile rule
(csrc/uvrt_dedupe.h, "one pass per key tile"): the small shapes where it can go wrong.  The expected masks are
uvrt_dedupe_plan's, which tests/test_dedupe_cpu.py holds to brute force; they are computed once per group and shared."""
import numpy as np

from test_dedupe_cpu import seed_chain, stepped_chain, tie_chain

TIE_SEED = 0x02468ace
ORDINARY_LAMP = (-1.5, 1.25, 2.0)


class Group:
    def __init__(self, name, lamp, prev, nxt, mode, first, n):
        self.name, self.lamp, self.prev, self.nxt, self.mode, self.first, self.n = name, lamp, list(prev), list(nxt), mode, first, n
        self.K = len(self.prev)

    def args(self):
        return self.lamp, self.prev, self.nxt, self.mode, self.first, self.n

    def chunks(self):
        """(first, n) of the chunks a group is looked at through: all of it, a strict inner part, two parts that meet"""
        cut = self.n // 2 + 37
        return {"whole": [(self.first, self.n)],
                "inner": [(self.first + 1000, 2000)],
                "meet": [(self.first, cut), (self.first + cut, self.n - cut)]}


def groups(capi, lamp0, length):
    """lamp0: the route's first lamp (the headline's), length: its rod"""
    out = []

    def chained(name, lamp, K, seed0, mode, first, n):
        prev, nxt = seed_chain(capi, lamp, length, K, seed0, mode)
        out.append(Group(name, lamp, prev, nxt, mode, first, n))
        return nxt[-1]

    # first gid 0 puts work-item 0 (the other SEED) in a tile of its own key; 16 M: sums past 2^28, keys held twice
    for first in (0, 1200000, 2000000, 16000000):
        chained("k8_first%d" % first, lamp0, 8, 0, 0, first, 4096)
    # the ties of test_dedupe_cpu.py: ulp 16 against a step of 17 in [2^27, 2^28) ...
    for first in (9000000, 10000000, 15000000):
        prev, nxt = tie_chain(6, 16, TIE_SEED)
        out.append(Group("ties_first%d" % first, ORDINARY_LAMP, prev, nxt, 0, first, 4000))
    prev, nxt = stepped_chain(6, TIE_SEED, 0x3c6ef372)
    out.append(Group("lx8", (8.0, 0.0, 0.0), prev, nxt, 0, 9000000, 4000))
    # ... and three binades down, where every second integer is a key
    prev, nxt = tie_chain(6, 2, TIE_SEED)
    out.append(Group("ties_grid2", ORDINARY_LAMP, prev, nxt, 0, 1100000, 4000))
    # seed mode 1, negative first sums: a run of clamped key 0 inside the range (about 2 500 gids, and one of about 5 000 that
    # spans three owner-count blocks)
    for name, lamp in (("neg", (-2000.0, 1.25, -1500.0)), ("neg_long", (-4000.0, 1.25, -3000.0))):
        for first in (0, 2000):
            chained("mode1_%s_first%d" % (name, first), lamp, 5, 0x1234, 1, first, 6000)
    # a column of 33 launches is split 17 + 16: the many flag sits beside 17 launch bits
    after17 = chained("k17", lamp0, 17, 0, 0, 1200000, 4096)
    chained("k16", lamp0, 16, after17, 0, 1200000, 4096)
    chained("k2", lamp0, 2, 0, 0, 1200000, 4096)
    chained("n4099", lamp0, 8, 0, 0, 1200000, 4099)
    assert [g.name for g in out] == NAMES
    return out


# (the names of groups(), for parametrize)
NAMES = (["k8_first%d" % f for f in (0, 1200000, 2000000, 16000000)] + ["ties_first%d" % f for f in (9000000, 10000000, 15000000)] +
         ["lx8", "ties_grid2"] + ["mode1_%s_first%d" % (nm, f) for nm in ("neg", "neg_long") for f in (0, 2000)] +
         ["k17", "k16", "k2", "n4099"])
CHUNKINGS = ["whole", "inner", "meet"]

_plans = {}


def plan(capi, g):
    """uvrt_dedupe_plan's masks of the whole group (read only)"""
    if g.name not in _plans:
        m = capi.dedupe_plan(*g.args())
        m.setflags(write=False)
        _plans[g.name] = m
    return _plans[g.name]


def lamp0_of(orc, oscene, oroute):
    comp = orc.Computation(oscene, oroute["lamps"], 1 << 16, oroute["lightHeight"], oroute["lightLength"], oroute["lightIntensity"])
    return tuple(float(x) for x in comp.lamp_world_pos(oroute["lamps"][0])), oroute["lightLength"]
