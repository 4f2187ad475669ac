"""Hand-made scenes for the gather and refine kernels (csrc/uvrt_occlude.hip k_gather_*, csrc/uvrt_refine.hip), shared by
tests/test_gpu_refine_gather_edges.py and tests/test_gather_refine_cpu.py.  The scanned room has no triangle without area and no
sample on the lamp; these scenes have both, and ranges long enough for every path of the refine's prefix sum.  Everything is
generated from seeds: bench.soup_triangles for the filling, orc.build_bvh for the tree.

The edge scene: EDGE_SOUP soup triangles with hand-made ones in the middle (from EDGE_MID on) and at the very end, the lamp's
foot at the origin, the rod along +y.  HAND names the hand-made triangles; edge_scene().hand maps a name to its index."""
import numpy as np

f32 = np.float32

LAMP = (0.0, 0.0, 0.0)              # the lamp's foot; the rod is x = z = 0, y in [0, light_length]
SEGMENT_TO = (0.75, 0.125, -0.5)    # where the one segment ends
EDGE_SOUP = 300
EDGE_SOUP_SEED = 24
EDGE_MID = 170                      # index of the first hand-made triangle

# name -> (v0, v1, v2).  "No area" below means cross(e1, e2) == 0 exactly in f64 (nn == 0).
_MID = (
    ("point", ((0.5, 0.5, 0.5),) * 3),                                                  # no area
    # edges of 1e-25 at the lamp's foot: nn = 1e-50 in f64, but with light_length = 0 every d is about 1e-25, d*d underflows
    # in f32 and r = 0 while R = |D| is finite in f64
    ("tiny at the foot", ((0.0, 0.0, 0.0), (1e-25, 0.0, 0.0), (0.0, 0.0, 1e-25))),
    ("collinear", ((1.0, 0.25, 1.0), (1.5, 0.25, 1.5), (2.0, 0.25, 2.0))),              # no area
    # x = 3e19 with edges of 1e19: d.x * d.x is 9e38 > FLT_MAX, r = inf while R is finite
    ("far and huge", ((3e19, 0.0, 0.0), (3e19, 1e19, 0.0), (3e19, 0.0, 1e19))),
    ("sliver", ((-1.0, 0.5, 1.0), (1.0, 0.5, 1.0), (0.0, 0.500001, 1.0))),              # 2 m long, 1e-6 high
    ("plane through the rod", ((0.5, 0.25, 0.0), (1.5, 0.25, 0.0), (0.5, 1.25, 0.0))),  # z = 0: n.D = 0 for every sample at a stop
)
_END = (
    ("pierced by the rod", ((-0.25, 0.5, -0.25), (0.5, 0.5, -0.25), (0.0, 0.5, 0.5))),   # y = 0.5 around x = z = 0
    ("repeated vertex", ((-1.0, 1.0, 2.0), (-1.0, 1.0, 2.0), (-0.5, 1.0, 2.5))),        # no area
    ("point at the foot", ((0.0, 0.0, 0.0),) * 3),                                      # no area, and d = 0 at light_length = 0
    ("point, last", ((-1.5, -1.25, 5.0),) * 3),                                         # no area; the last triangle of the scene
)
HAND = tuple(name for name, _ in _MID + _END)
NO_AREA = ("point", "collinear", "repeated vertex", "point at the foot", "point, last")


class HandScene:
    """what the restatements take of a scene: tris (64-byte Tri records), nodes, triIdx, T"""

    def __init__(self, orc, tris):
        self.tris = np.ascontiguousarray(tris, dtype=f32)
        self.T = self.tris.shape[0]
        self.nodes, self.triIdx = orc.build_bvh(self.tris)      # (fills the centroids of self.tris)
        self.tris.setflags(write=False)
        self.nodes.setflags(write=False)
        self.triIdx.setflags(write=False)


def _rows(hand):
    rows = np.zeros((len(hand), 16), dtype=f32)
    for k, (_, (v0, v1, v2)) in enumerate(hand):
        rows[k, 0:3], rows[k, 4:7], rows[k, 8:11] = v0, v1, v2
    return rows


def soup(T, seed):
    import bench
    return bench.soup_triangles(T, seed=seed)


def edge_scene(orc, soup_count=EDGE_SOUP, seed=EDGE_SOUP_SEED, mid=EDGE_MID):
    """soup[0, mid) + the hand-made middle ones + soup[mid, soup_count) + the hand-made end ones"""
    s = soup(soup_count, seed)
    scene = HandScene(orc, np.concatenate([s[:mid], _rows(_MID), s[mid:], _rows(_END)]))
    scene.hand = {name: mid + k for k, (name, _) in enumerate(_MID)}
    scene.hand.update({name: scene.T - len(_END) + k for k, (name, _) in enumerate(_END)})
    scene.no_area = np.array(sorted(scene.hand[n] for n in NO_AREA))
    scene.sub_range = (mid, scene.T - mid)          # starts and ends with a hand-made triangle
    return scene


ROW_X0, ROW_TAU = 4.0, 0.25        # r = rel_error * X0 = 1 exactly, so want = ceil(S0 * (V0 - 1))
ROW_WANTS = tuple(sorted({0, 1, 2, 3, 4} | {(1 << k) + d for k in range(1, 13) for d in (-1, 0, 1)})) + (1e300,)


def count_rule_rows(S0, max_extra):
    """Rows (X0, V0, want) for the count rule at rel_error = ROW_TAU: `want` is the value the rule's ceil() gives, None where the
    row does not pin it.  Every integer of ROW_WANTS and max_extra - 1, max_extra, max_extra + 1 twice: from just below
    (S0 * (V0 - 1) lies in (want - 1, want) whatever the rounding of the division by S0) and from V0 = 1 + want / S0 itself, which
    is exact where S0 is a power of two.  Then the values that are no number a gather leaves: zeros of both signs, subnormals,
    inf, NaN, negatives, r * r under- and overflowing, and X0 one ulp either side of ROW_X0 for min_expected = ROW_X0."""
    inf, nan, tiny = np.inf, np.nan, 5e-324
    rows = []
    for w in sorted(set(ROW_WANTS) | {max_extra - 1, max_extra, max_extra + 1}):
        rows.append((ROW_X0, 1.0 + (w - 0.5) / S0, w if w < 1e300 else None))
        rows.append((ROW_X0, 1.0 + w / S0, w if S0 & (S0 - 1) == 0 and w < 1e300 else None))
    rows += [(x, 1.0, None) for x in (0.0, -0.0, tiny, 1e-200, inf, nan, -4.0, 1e200)]      # 1e-200: r * r = 0, want = inf
    rows += [(ROW_X0, v, None) for v in (0.0, -0.0, tiny, -1.0, inf, nan)]
    rows += [(1e200, inf, None), (inf, inf, None), (tiny, tiny, None)]      # inf / inf twice: want is NaN; tiny / 0: inf
    rows += [(x, 100.0, None) for x in (np.nextafter(ROW_X0, 0.0), ROW_X0, np.nextafter(ROW_X0, inf))]
    X = np.array([r[0] for r in rows], dtype=np.float64)
    V = np.array([r[1] for r in rows], dtype=np.float64)
    return X, V, [r[2] for r in rows]


def restated_want(X0, V0, S0, rel_error=ROW_TAU):
    """`want` of the count rule (include/uvrt.h) in f64, one rounding per operator"""
    with np.errstate(all="ignore"):
        r = np.float64(rel_error) * np.asarray(X0, dtype=np.float64)
        return np.ceil(np.float64(S0) * (np.asarray(V0, dtype=np.float64) / (r * r) - 1.0))


def crafted_planes(scene, S0, max_extra):
    """(expected, variance) f64[T] of the edge scene: count_rule_rows over and over, and on the triangles without area a row
    that wants max_extra samples anywhere else"""
    X, V, _ = count_rule_rows(S0, max_extra)
    assert X.size <= scene.sub_range[1] - len(NO_AREA), "every row on a triangle with area of the sub-range"
    at = np.setdiff1d(np.arange(scene.T), scene.no_area)
    at = np.concatenate([at[at >= scene.sub_range[0]], at[at < scene.sub_range[0]]])       # the sub-range first: it holds every row
    E, W = np.empty(scene.T), np.empty(scene.T)
    E[at], W[at] = np.resize(X, at.size), np.resize(V, at.size)
    E[scene.no_area], W[scene.no_area] = ROW_X0, 1e6
    return E, W


BOUNDARY_T = 4200      # more than four blocks of the scan (1024 positions each)
CARRY_T = 263200        # more than 256 blocks: the second tile of k_refine_scan_sums, which takes the first one's carry


def soup_scene(orc, T, seed=2):
    return HandScene(orc, soup(T, seed))


def random_planes(T, seed, share=1.0 / 3.0, S0=4, rel_error=0.25, max_extra=64):
    """(expected, variance) f64[T] for the count rule at (S0, rel_error): about `share` of the rows want samples, log-uniformly
    from 1 to twice max_extra; the others have variance 0 or an estimate that is certain enough"""
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.5, 2.0, T)
    want = np.exp(rng.uniform(0.0, np.log(2.0 * max_extra), T))
    r = rel_error * X
    V = (want / S0 + 1.0) * (r * r)
    kind = rng.uniform(0.0, 1.0, T)
    V = np.where(kind < share, V, np.where(kind < 0.5 + 0.5 * share, 0.0, 0.5 * (r * r)))
    return X, V
