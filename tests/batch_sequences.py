"""Seeded sequences of batches for ONE long-lived context, and the model they are held to.

A context's two buffer sets are never cleared between batches: whatever a batch deposited, its fold or replay read back and
zeroed.  A breach shows in a LATER batch that lays planes of another shape over the stale counters, so the sequences here
change everything that moves the planes from one uvrt_trace_batch to the next on the same set: the launch count, the range
(R and the plane stride follow n), dedupe and the class setting (class planes sit behind the launch planes, at an offset that
follows the count), the flavour, the seed mode, sweeps, and how the batch is consumed.

sequence(seed) is pure Python: a list of steps, each a dict

    launches   symbolic, in logical order: ("stop", "A") / ("sweep", "A", "B") over the pool A, B, A2 (lamp_pool)
    first, n   the global-id range
    dedupe, classes, flavour, seed_mode, prio      set before the step
    mode       "read" (every launch's plane, then replay), "planes" (replay straight from the planes), "fold" (uvrt_fold_batch,
               then replay), "launch" (replay, then one per-launch generate / extend / accumulate / Shade on the same context)
    ops        uvrt_replay_op tuples, a Shade behind the last launch at least
    oracle     the logical launch the CPU oracle traces as well (flavours 0 and 1)

Steps alternate between the two sets, so steps i and i + 2 share one.  tests/test_batch_sequences_cpu.py asserts with the
host hooks that every sequence holds what it is for; tests/test_gpu_batch_sequences.py runs them.  This module imports
without a GPU."""
import random

import numpy as np

COUNTS = (1, 2, 3, 5, 8, 17, 33, 64)
NS = (1, 63, 1000, 4096, 20001)
FIRSTS = (0, 3, 1200000, 2000000)
CLASSES = (0, 1, 4, 32)
MODES = ("read", "planes", "fold", "launch")
SEEDS = (1, 2, 3, 4, 5, 6)
PAIR_SEEDS = (5, 6)           # run as two contexts over the halves of the range: no n = 1 (a half would be empty)
FLAVOUR2_SEED = 3             # the one sequence with stop-only steps in flavour 2
STEPS = 11
DEDUPE_MAX = 31               # launches of one dedupe group at most (csrc/uvrt_dedupe.h)
SEED0 = 0x1234

f32 = np.float32


def lamp_pool(orc, oscene, oroute):
    """A and B: lamps 0 and 5 of the route as tests/test_gpu_dedupe.py places them; A2: A raised by 0.37 -- A's column (x, z)
    and records, but a column whose lamps differ in y forms no dedupe group"""
    comp = orc.Computation(oscene, oroute["lamps"], 1 << 16, oroute["lightHeight"], oroute["lightLength"], oroute["lightIntensity"])
    a, b = (tuple(float(x) for x in comp.lamp_world_pos(oroute["lamps"][k])) for k in (0, 5))
    return {"A": a, "B": b, "A2": (a[0], float(f32(f32(a[1]) + f32(0.37))), a[2])}


def _stops(rng, count, kind):
    """`count` stops: "A" one column of A; "AB" A and B in turn (two groups); "mixed" a random order of A and B in runs;
    "A2" a column of A with one A2 in it (no group) beside a B column"""
    if kind == "A":
        return ["A"] * count
    if kind == "AB":
        return [("A", "B")[k & 1] for k in range(count)]
    if kind == "A2":
        out = [("A", "A", "B")[k % 3] for k in range(count)]
        out[rng.randrange(count)] = "A2"
        return out
    out = []
    while len(out) < count:
        out += [rng.choice(("A", "A", "B"))] * rng.choice((1, 2, 3, 7))
    return out[:count]


def _step(rng, count, kind, first, n, dedupe, classes, flavour=0, seed_mode=0, sweeps=0, mode=None):
    sweeps = min(sweeps, count - 1)
    names = _stops(rng, count - sweeps, kind)
    launches = [("stop", nm) for nm in names]
    for _ in range(sweeps):           # sweeps between the pool's points, anywhere in the logical order
        frm, to = rng.sample(("A", "B", "A2"), 2)
        launches.insert(rng.randrange(len(launches) + 1), ("sweep", frm, to))
    shade_at = {count - 1: rng.randrange(2)}
    if count > 2:
        shade_at[rng.randrange(count - 1)] = rng.randrange(2)
    ops = []
    for k in range(count):
        ops.append((float(f32(rng.choice((0.0, 5.0, 8.5, 30.0, 60.0)))), 1 if k in shade_at else 0, shade_at.get(k, 0),
                    n * (k + 1), 44.0197, 100.0, k & 1))
    stops = [k for k, l in enumerate(launches) if l[0] == "stop"]
    return {"launches": launches, "first": first, "n": n, "dedupe": dedupe, "classes": classes, "flavour": flavour,
            "seed_mode": seed_mode, "prio": rng.randrange(4), "mode": mode or rng.choice(MODES), "ops": ops,
            "oracle": rng.choice(stops if flavour != 0 else list(range(count))),
            "launch_dt": float(f32(rng.choice((0.0, 12.5, 40.0)))), "launch_which": rng.randrange(2)}


def sequence(seed):
    """The steps of sequence `seed` (one of SEEDS).  The skeleton is fixed -- what every sequence is for, see the module's
    text and tests/test_batch_sequences_cpu.py -- and the seed draws the rest.

    set 1 (steps 0, 2, ...): 64 launches of A with classes (a column of more than 31, and the set's largest allocation, so no
    later batch of the set gets fresh, zeroed memory) -> classes off -> classes on again -> sweeps, directly over the class
    planes -> drawn -> 64 stops at n = 1000, whose launch planes cover every address a smaller batch's class planes had.
    set 0 (steps 1, 3, ...): classes on -> dedupe off (after step 2 with it on) -> classes on -> drawn -> drawn."""
    rng = random.Random(0x5eed0000 + seed)
    ns = [v for v in NS if v != 1] if seed in PAIR_SEEDS else list(NS)
    big_n = (1000, 4096, 20001)            # ranges whose groups hold multi-bit masks (the CPU test asks the hook)
    far = (1200000, 2000000)

    def drawn(i):
        flavour = rng.choice((0, 0, 1))
        seed_mode = rng.randrange(2)
        if seed == FLAVOUR2_SEED and i == 7:
            flavour, seed_mode = 2, rng.randrange(2)
        sweeps_ok = flavour in (0, 1) and seed_mode == 0
        count = rng.choice(COUNTS[:-1])
        n = rng.choice(ns)
        if count >= 33 and n > 4096:
            n = 4096
        sweeps = min(rng.randrange(4), count - 1) if sweeps_ok else 0
        return _step(rng, count, rng.choice(("A", "AB", "mixed", "A2")), rng.choice(FIRSTS), n, rng.random() < 0.7,
                     rng.choice(CLASSES), flavour, seed_mode, sweeps)

    c2, c3 = rng.choice((2, 3, 5, 17)), rng.choice((2, 3, 5))
    steps = [
        _step(rng, 64, "A", rng.choice(far), 1000, True, 32),
        _step(rng, rng.choice((8, 17)), "A", rng.choice(far), rng.choice(big_n), True, rng.choice((1, 4)),
              flavour=rng.randrange(2), seed_mode=rng.randrange(2)),
        _step(rng, c2, rng.choice(("A", "AB", "mixed")), rng.choice(FIRSTS), rng.choice(ns), True, 0),
        _step(rng, c3, rng.choice(("A", "mixed", "A2")), rng.choice(FIRSTS), rng.choice(ns), False, rng.choice((0, 1, 4)),
              seed_mode=rng.randrange(2)),
        _step(rng, 8, "A", rng.choice(far), 4096, True, 4, flavour=rng.randrange(2)),
        _step(rng, rng.choice((8, 17)), "AB", 1200000, rng.choice((4096, 20001)), True, 32),
        _step(rng, rng.choice((3, 5, 8)), rng.choice(("A", "AB", "mixed")), rng.choice(FIRSTS), rng.choice(ns), rng.random() < 0.5,
              rng.choice(CLASSES), flavour=rng.randrange(2), sweeps=rng.choice((1, 2, 3))),
        drawn(7), drawn(8), drawn(9),
        _step(rng, 64, rng.choice(("AB", "mixed", "A2")), rng.choice(FIRSTS), 1000, True, 0),
    ]
    assert len(steps) == STEPS
    return steps


# ---- what a step means: its launches, its SEED chain, its dedupe groups ----

def launches_of(capi, step, pool):
    return [capi.stop(pool[l[1]]) if l[0] == "stop" else capi.sweep(pool[l[1]], pool[l[2]]) for l in step["launches"]]


def seed_chain(capi, step, pool, length, seed):
    """SEED before every launch of the step, and after the last"""
    chain = [seed]
    for l in step["launches"]:
        if l[0] == "sweep":
            seed = capi.seed_next_sweep(pool[l[1]], length, seed)
        else:
            seed = capi.seed_next(pool[l[1]], length, seed, step["seed_mode"])
        chain.append(seed)
    return chain


def groups_of(step, pool):
    """The dedupe groups uvrt_trace_batch makes of the step, as lists of logical launches: the stops of a lamp column (x, z) whose
    lamps agree in y too, two at least, a column of more than 31 split evenly; none with dedupe off"""
    if not step["dedupe"]:
        return []
    cols = {}
    for k, l in enumerate(step["launches"]):
        if l[0] == "stop":
            p = pool[l[1]]
            cols.setdefault((p[0], p[2]), []).append(k)
    out = []
    for ks in cols.values():
        if len(ks) < 2 or len({pool[step["launches"][k][1]][1] for k in ks}) != 1:
            continue
        pieces = (len(ks) + DEDUPE_MAX - 1) // DEDUPE_MAX
        k0 = 0
        for i in range(pieces):           # sizes that differ by one at most, the larger pieces first (64: 22 + 21 + 21)
            kc = len(ks) // pieces + (i < len(ks) % pieces)
            if kc >= 2:
                out.append(ks[k0:k0 + kc])
            k0 += kc
    return out


def group_args(step, pool, chain, group, first=None, n=None):
    """the arguments of capi.dedupe_plan / capi.dedupe_classes for one group (over a sub-range, if given)"""
    lamp = pool[step["launches"][group[0]][1]]
    return (lamp, [chain[k] for k in group], [chain[k + 1] for k in group], step["seed_mode"],
            step["first"] if first is None else first, step["n"] if n is None else n)


def class_lists(capi, step, pool, chain, first=None, n=None):
    """per group the class list the hook gives it at the step's setting (empty: classes off, dedupe off, 31 launches)"""
    if step["classes"] == 0:
        return [np.zeros(0, dtype=np.uint32) for _ in groups_of(step, pool)]
    return [capi.dedupe_classes(*group_args(step, pool, chain, g, first, n), step["classes"])[0] for g in groups_of(step, pool)]


def is_classed(capi, step, pool, chain):
    """does the batch lay class planes behind its launch planes?"""
    return any(len(cl) > 0 for cl in class_lists(capi, step, pool, chain))


def owners(capi, step, pool, chain, first=None, n=None):
    """rays uvrt_batch_traced_rays reports for the step's stops over the range: the owners of every group, and every ray of a
    stop outside the groups"""
    n = step["n"] if n is None else n
    groups = groups_of(step, pool)
    grouped = sum(len(g) for g in groups)
    stops = sum(1 for l in step["launches"] if l[0] == "stop")
    total = (stops - grouped) * n
    for g in groups:
        total += int((capi.dedupe_plan(*group_args(step, pool, chain, g, first, n)) != 0).sum())
    return total, grouped * n


# ---- the model: per-launch counts, everything else on the CPU ----

class Model:
    """f64 maps, dose and colour after every step, computed by the oracle's accumulate / computeDosage / dosageToColor from
    per-launch counts in logical launch order"""

    def __init__(self, orc, scene):
        self.orc, self.scene = orc, scene
        self.sum = np.zeros(scene.T, dtype=np.float64)
        self.max = np.zeros(scene.T, dtype=np.float64)
        self.dose = np.zeros(scene.T, dtype=np.float32)
        self.colour = np.zeros((scene.T, 9), dtype=np.float32)

    def launch(self, counts, op, tri_count=None):
        """accumulate.cl, then shade.cl where the op has a Shade, over triangles [0, tri_count): the rest stays as it is"""
        tc = self.scene.T if tri_count is None else tri_count
        duration, shade, which, ppl, power, min_value, threshold = op
        self.orc.accumulate(self.sum[:tc], self.max[:tc], counts[:tc].copy(), duration)      # (accumulate.cl zeroes its counts)
        if shade:
            self.dose[:tc] = self.orc.compute_dosage((self.max if which else self.sum)[:tc], self.scene.tris, ppl, power)
            self.colour[:tc] = self.orc.dosage_to_color(self.dose[:tc].copy(), min_value, threshold)

    def replay(self, counts, ops, tri_count=None):
        for cn, op in zip(counts, ops):
            self.launch(cn, op, tri_count)

    def copy(self):
        m = Model(self.orc, self.scene)
        m.sum, m.max, m.dose, m.colour = self.sum.copy(), self.max.copy(), self.dose.copy(), self.colour.copy()
        return m
