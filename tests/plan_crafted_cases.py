"""Hand-made scenes and exposure matrices for the duration planner (tests/test_plan_crafted_cpu.py without a GPU,
tests/test_gpu_plan_crafted.py with one).

Scenes: right triangles on a grid in the plane y = 0, legs 2^a and 2^b, so every f32 area is the power of two 2^(a+b-1); a
few triangles have no area (three equal points; three collinear points).  The exact setting s = 1, N = 2, m = 1, margin = 0
gives a triangle of area 0.5 the row scale r_t = 1, and every r_t is a power of two: the products below are exact.

A case is a dict: name, area_log2 (per triangle: the exponent of its area, None = no area), E (integer counts, P x T), X (the
expected plan's f64 matrix when it is not (double)E), prm (the solve's parameters), mask, solves (a list of (tag, lower,
fixed)), and for the closed forms `exact` per solve tag (f64[P], the optimum per column, NaN where it is not unique)."""
import numpy as np

EXACT = dict(s=1.0, N=2, m=1.0, margin=0.0)
REL_GAP = 1e-3
CELL, PER_ROW = 8.0, 32       # the grid: cell k at x = 8 (k mod 32), z = 8 (k div 32)


def make_tris(area_log2):
    """T x 16 float32 triangles (v0, v1, v2 at 0:3, 4:7, 8:11).  Triangle k stands at its grid cell with legs 2^ceil((e+1)/2)
    along x and 2^floor((e+1)/2) along z for area 2^e; without an area it is a point (even k) or three collinear points."""
    T = len(area_log2)
    tris = np.zeros((T, 16), dtype=np.float32)
    for k, e in enumerate(area_log2):
        x, z = CELL * (k % PER_ROW), CELL * (k // PER_ROW)
        tris[k, 0:3] = tris[k, 4:7] = tris[k, 8:11] = (x, 0.0, z)
        if e is None:
            if k % 2:
                tris[k, 4] += 1.0
                tris[k, 8] += 2.0
            continue
        la = (e + 2) // 2
        lb = e + 1 - la
        tris[k, 4] += 2.0 ** la
        tris[k, 10] += 2.0 ** lb
    return tris


def scene(orc, case):
    """(tris, nodes, triIdx) with the oracle's BVH builder; tris is the array to hand to set_scene and to take the areas from"""
    tris = make_tris(case["area_log2"])
    nodes, idx = orc.build_bvh(tris)
    return tris, nodes, idx


def _case(name, area_log2, E, prm, solves, mask=None, X=None, exact=None, counts_only=False):
    E = np.asarray(E, dtype=np.uint64)
    assert E.max() < 2 ** 32 and E.shape[1] == len(area_log2)
    return dict(name=name, area_log2=list(area_log2), E=E, X=X, prm=dict(prm), mask=mask, solves=solves, exact=exact or {},
                counts_only=counts_only)


# ---------------------------------------------------------------- A: the precedence table
A_LOWER = np.array([0.0, 0.0, 2.0 ** -3, 2.0 ** -1], dtype=np.float32)
A_FIXED = np.array([0, 0, 1, 1], dtype=np.uint8)
A_T = 513


def _table_rows():
    """(masked, E row, area exponent or None, what the row is) for every consistent combination.  With lower = (0, 0, 1/8, 1/2)
    every pattern's base = sum E lower is a power of two (or 0), so the area decides base * r against 1 exactly: r = 1 / (2 area)."""
    patterns = [  # (E row, row sum against min_photons = 8, free-column sum, base)
        ((0, 0, 0, 0), 0, 0, 0.0),
        ((0, 0, 4, 3), 7, 0, 2.0), ((3, 0, 4, 0), 7, 3, 0.5), ((7, 0, 0, 0), 7, 7, 0.0),
        ((0, 0, 8, 0), 8, 0, 1.0), ((4, 0, 4, 0), 8, 4, 0.5), ((8, 0, 0, 0), 8, 8, 0.0),
    ]
    rows = []
    for masked in (0, 1):
        for row, tot, fre, base in patterns:
            rows.append((masked, row, None, "no area, sum %d, free %d" % (tot, fre)))
            if base == 0.0:
                rows.append((masked, row, -1, "sum %d, free %d, base 0" % (tot, fre)))
                continue
            lb = int(np.log2(base))
            for what, e in (("< 1", lb), ("== 1", lb - 1), ("> 1", lb - 2)):      # area = base, base / 2, base / 4
                rows.append((masked, row, e, "sum %d, free %d, base r %s" % (tot, fre, what)))
    return rows


def case_A():
    table = _table_rows()
    # rho's clamp: base r = 1 - 2^-30 (rho = 2^-30 < 1e-9: clamped up) and 1 - 2^-29 (rho = 2^-29 > 1e-9: kept);
    # base = (2^30 - k) / 8, r = 2^-27 = 1 / (2 area) with area 2^26; one photon in free column 0 keeps the row active
    extra = [(0, (1, 0, 2 ** 30 - 1, 0), 26, "rho clamped"), (0, (1, 0, 2 ** 30 - 2, 0), 26, "rho not clamped"),
             (0, (7, 0, 0, 0), -1, "one ulp below min_photons (expected plan)")]
    rows = table + extra
    rng = np.random.default_rng(11)
    order = []
    while len(order) < A_T - 1:                  # whole shuffled copies of the table: each block of 256 holds every row kind
        order += [int(i) for i in rng.permutation(len(rows))]
    order = order[:A_T - 1] + [len(table)]       # triangle 512, alone in the third block: an active row
    E = np.array([rows[i][1] for i in order], dtype=np.uint64).T.copy()
    mask = np.array([0 if rows[i][0] else 1 for i in order], dtype=np.uint8)
    area_log2 = [rows[i][2] for i in order]
    X = E.astype(np.float64)
    ulp = len(rows) - 1
    for t, i in enumerate(order):
        if i == ulp:
            X[0, t] = np.nextafter(8.0, 0.0)     # sum 8 - 2^-50 < min_photons: unresolved, as the 7 of the counts plan
    c = _case("A", area_log2, E, dict(EXACT, min_photons=8), [("plain", None, None), ("bounded", A_LOWER, A_FIXED)],
              mask=mask, X=X)
    c["kinds"] = [rows[i][3] for i in order]
    return c


# ---------------------------------------------------------------- B: row sums beyond 2^32 (counts only)
def case_B2():
    E = np.array([[2 ** 31, 5, 0], [2 ** 31, 0, 7]], dtype=np.uint64)
    return _case("B2", [-1, -1, -1], E, dict(EXACT, min_photons=1), [("plain", None, None)], counts_only=True)


def case_B256():
    """row 0: 2^32 - 1 in every column (sum 2^40 - 256); row 1: 2^24 in every column (sum 2^32: 0 in uint32); row 2 below"""
    E = np.zeros((256, 3), dtype=np.uint64)
    E[:, 0] = 2 ** 32 - 1
    E[:, 1] = 2 ** 24
    E[:, 2] = 2 ** 22                             # sum 2^30 < min_photons: unresolved
    return _case("B256", [-1, -1, -1], E, dict(EXACT, min_photons=2 ** 31 - 1), [("plain", None, None)], counts_only=True)


# ---------------------------------------------------------------- C: sizes
C_SIZES = [(1, 1), (2, 255), (3, 256), (17, 257), (255, 513), (256, 513)]
C_PRM = dict(s=45.0, N=65536, m=100.0, margin=1e-6, min_photons=16)


def case_C(P, T):
    rng = np.random.default_rng(5)
    E = rng.integers(1, 5000, (P, T)).astype(np.uint64) * (rng.uniform(0, 1, (P, T)) >= 0.6)
    area_log2 = [int(e) for e in rng.integers(-6, 3, T)]
    for t in range(3, T, 50):                    # a few triangles without area
        area_log2[t] = None
    lower = np.where(np.arange(P) % 3 == 0, 8.0, 0.0).astype(np.float32)
    fixed = (np.arange(P) % 5 == 0).astype(np.uint8) if P > 1 else np.zeros(1, dtype=np.uint8)
    return _case("C%dx%d" % (P, T), area_log2, E, C_PRM, [("plain", None, None), ("bounded", lower, fixed)])


# ---------------------------------------------------------------- D: closed forms; E: beyond the old pivot floor
D_PRM = dict(EXACT, min_photons=1)


def case_D_range():
    return _case("D-range", [-1, -1], [[2 ** 31, 0], [0, 1]], D_PRM, [("plain", None, None)],
                 exact={"plain": np.array([2.0 ** -31, 1.0])})


def case_D_tie():
    return _case("D-tie", [-1, -1], [[2 ** 31, 0], [2 ** 31, 0], [0, 1]], D_PRM, [("plain", None, None)],
                 exact={"plain": np.array([2.0 ** -31, 0.0, 1.0])})


def case_D_ones():
    """every row the same columns: r_t = 2^-(t mod 5), so the plan needs sum d >= 16 and no column is told apart"""
    T = 300
    return _case("D-ones", [t % 5 - 1 for t in range(T)], np.ones((256, T), dtype=np.uint64), D_PRM, [("plain", None, None)],
                 exact={"plain": np.full(256, np.nan)})


def case_D_diag():
    return _case("D-diag", [-1] * 256, np.diag(np.arange(1, 257)).astype(np.uint64), D_PRM, [("plain", None, None)],
                 exact={"plain": 1.0 / np.arange(1, 257)})


def case_E_diag(e):
    """diagonal (2^32 - 1, 1) with areas 2^e and 0.5: r_0 = 2^-(e+1), so the scaled entries are (2^32 - 1) 2^-(e+1) and 1"""
    return _case("E-diag%d" % e, [e, -1], [[2 ** 32 - 1, 0], [0, 1]], D_PRM, [("plain", None, None)],
                 exact={"plain": np.array([1.0 / ((2.0 ** 32 - 1) * 2.0 ** -(e + 1)), 1.0])})


def case_E_rho():
    """column 0 fixed at 2^-30 with 2^30 - 1 on row A: base = 1 - 2^-30, rho clamped to 1e-9, the row scale 1e9;
    the free column 1 holds 2^20 there, the free column 2 holds 1 on row B"""
    lower = np.array([2.0 ** -30, 0, 0], dtype=np.float32)
    fixed = np.array([1, 0, 0], dtype=np.uint8)
    return _case("E-rho", [-1, -1], [[2 ** 30 - 1, 0], [2 ** 20, 0], [0, 1]], D_PRM, [("bounded", lower, fixed)],
                 exact={"bounded": np.array([2.0 ** -30, 1e-9 / 2.0 ** 20, 1.0])})


OVERFLOW_LAMP = (64.0, 1.0, 64.0)


def overflow_scene():
    """triangle 0 (area 2^26: legs 16384 and 8192 from the origin) lies under the lamp at OVERFLOW_LAMP; P = 1"""
    T = 5
    return _case("overflow", [26, -1, -1, None, -3], np.zeros((1, T), dtype=np.uint64), D_PRM, [("plain", None, None)],
                 counts_only=True)


def matrix(case, expected):
    """the matrix a plan of the given kind holds: uint64 counts (values below 2^32) or f64"""
    if not expected:
        return case["E"]
    return case["X"] if case["X"] is not None else case["E"].astype(np.float64)


def scaled_lp(case, tag, pr):
    """the LP the simplex sees for solve `tag`: (A[rows][free columns] = E r_t (/ rho_t), the free columns), from the restatement"""
    _, lower, fixed = [s for s in case["solves"] if s[0] == tag][0]
    tris = make_tris(case["area_log2"])
    c = pr.classify(case["E"], pr.areas(tris), mask=case["mask"], lower=lower, fixed=fixed, **case["prm"])
    cols = np.flatnonzero(~c["fixed"])
    A = case["E"][np.ix_(cols, c["rows"])].astype(np.float64).T * c["rd"][:, None]
    return np.ascontiguousarray(A), cols, c


def closed_cases():
    return [case_D_range(), case_D_tie(), case_D_ones(), case_D_diag(), case_E_diag(-11), case_E_diag(-21), case_E_rho()]


def duration_bound(exact, round_trip_up):
    """the largest f32 a closed-form column may come back as: round_trip_up(smallest f32 >= exact (1 + 4e-9)); 4e-9 is twice
    the LP's right-hand-side perturbation (uvrt_plan_lp.h: delta < 2e-9), the rest one rounding to f32 and the "%.8g" trip"""
    from plan_restate import f32_at_least
    return round_trip_up(f32_at_least(exact * (1.0 + 4e-9)))
