"""The duration planner's arithmetic (csrc/uvrt_plan.hip) restated in numpy f64, operation for operation, so that a test can
ask for equal bits: the f32 areas of k_prepare_scene, the row scale, the row sums and classes of k_plan_classify, the report's
counts and its areas in the kernel's order of summation, min_dose_ratio as k_plan_rowcheck / k_plan_xcheck form it, and
k_plan_model_dose.  Nothing here solves anything: the durations are an input."""
import numpy as np

f32 = np.float32
RHO_MIN = 1e-9          # PLAN_RHO_MIN
BLOCK = 256             # threads per block of every planning kernel


def areas(tris):
    """k_prepare_scene's f32 triangle areas; `tris` as handed to set_scene (T x 16 float32, or anything that views as such)"""
    t = np.ascontiguousarray(tris).view(np.float32).reshape(-1, 16)
    v0, v1, v2 = t[:, 0:3], t[:, 4:7], t[:, 8:11]
    a, b = v0 - v1, v0 - v2
    cx = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]
    cy = a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2]
    cz = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
    return np.sqrt(cx * cx + cy * cy + cz * cz) / np.float32(2.0)


def row_scale(area, s, N, m, margin):
    """(den_t as f64 of the f32 product area_t * f32(N), m' = m (1 + margin), r_t = (double)s / ((double)den_t * m'))"""
    den = (np.asarray(area, dtype=np.float32) * f32(N)).astype(np.float64)
    mprime = float(f32(m)) * (1.0 + float(margin))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = float(f32(s)) / (den * mprime)
    return den, mprime, r


def row_sums(E, rows=None):
    """the sum over the columns `rows` (all by default) of every triangle: exact uint64 for integer counts, f64 in ascending
    p from 0.0 for expected values"""
    E = np.asarray(E)
    sel = range(E.shape[0]) if rows is None else rows
    if E.dtype.kind in "ui":
        tot = np.zeros(E.shape[1], dtype=np.uint64)
        for p in sel:
            tot = tot + E[p].astype(np.uint64)
        return tot
    tot = np.zeros(E.shape[1], dtype=np.float64)
    for p in sel:
        tot = tot + E[p]
    return tot


def weighted(E, w):
    """sum_p (double)E[p][t] * w_p in ascending p from 0.0, one rounding per operator (the row kernels' inner loop)"""
    acc = np.zeros(np.asarray(E).shape[1], dtype=np.float64)
    for p in range(len(w)):
        acc = acc + np.asarray(E[p]).astype(np.float64) * float(w[p])
    return acc


def is_bounded(lower, fixed):
    """what makes uvrt_plan_solve_bounded take the bounded kernels: a non-zero lower bound or a fixed column"""
    lo = np.zeros(0) if lower is None else np.asarray(lower, dtype=np.float32)
    fx = np.zeros(0) if fixed is None else np.asarray(fixed)
    return bool(np.any(lo != 0)) or bool(np.any(fx != 0))


def classify(E, area, s, N, m, margin, min_photons, mask=None, lower=None, fixed=None):
    """k_plan_classify and k_plan_compact: a dict with cls (uint8[T], the header's order of testing: 3, 1, 2, then 4, 5, 0 for
    a bounded solve), den, mprime, r, base (sum_p E lower_p, before r), rho, and rows / rd of the compacted LP rows"""
    E = np.asarray(E)
    P, T = E.shape
    area = np.asarray(area, dtype=np.float32)
    bounded = is_bounded(lower, fixed)
    low = np.zeros(P, dtype=np.float32) if lower is None else np.asarray(lower, dtype=np.float32)
    fix = np.zeros(P, dtype=bool) if fixed is None else np.asarray(fixed) != 0
    den, mprime, r = row_scale(area, s, N, m, margin)
    tot = row_sums(E)
    fre = row_sums(E, [p for p in range(P) if not fix[p]])
    base = weighted(E, low.astype(np.float64))
    min_ph = max(1, int(min_photons))
    below = tot < (np.uint64(min_ph) if tot.dtype.kind == "u" else float(min_ph))
    with np.errstate(invalid="ignore", over="ignore"):
        b = base * r
    cls = np.full(T, 255, dtype=np.uint8)
    rho = np.full(T, np.nan)
    all_met = not (float(f32(m)) > 0.0)
    for t in range(T):
        if mask is not None and not mask[t]:
            k = 3
        elif tot[t] == 0 or not (area[t] > 0):
            k = 1
        elif below[t]:
            k = 2
        elif not bounded:
            k = 0
        elif all_met:
            k = 4
        elif b[t] >= 1.0:
            k = 4
        elif fre[t] == 0:
            k = 5
        else:
            k = 0
            rho[t] = max(1.0 - b[t], RHO_MIN)
        cls[t] = k
    rows = np.flatnonzero(cls == 0)
    rd = r[rows] / rho[rows] if bounded else r[rows]
    return dict(cls=cls, bounded=bounded, den=den, mprime=mprime, m=float(f32(m)), r=r, base=base, rho=rho, rows=rows, rd=rd,
                lower=low, fixed=fix, area=area, s=float(f32(s)), Nf=f32(N))


def tree_sum(v):
    """the 256-wide tree of the kernels: s[i] += s[i + o] for o = 128 ... 1"""
    s = np.zeros(BLOCK, dtype=np.float64)
    s[:len(v)] = v
    o = BLOCK // 2
    while o > 0:
        s[:o] = s[:o] + s[o:2 * o]
        o //= 2
    return float(s[0])


def report(c):
    """the class counts and areas of uvrt_plan_report / uvrt_plan_bounds_report from classify()'s dict: per block the tree sum
    of (double)area over the rows of the class, then the blocks in ascending order from 0.0"""
    cls, a64 = c["cls"], c["area"].astype(np.float64)
    T = cls.size
    NC = 6 if c["bounded"] else 4
    cnt, ar = [0] * 6, [0.0] * 6
    for first in range(0, T, BLOCK):
        k, a = cls[first:first + BLOCK], a64[first:first + BLOCK]
        for q in range(NC):
            cnt[q] += int((k == q).sum())
            ar[q] = ar[q] + tree_sum(np.where(k == q, a, 0.0))
    out = dict(required=cnt[0] + cnt[4], unreachable=cnt[1], unresolved=cnt[2], masked_out=cnt[3],
               area_required=ar[0] + ar[4] if c["bounded"] else ar[0], area_unreachable=ar[1], area_unresolved=ar[2],
               area_masked_out=ar[3])
    bout = dict(met_by_lower=cnt[4], short_rows=cnt[5], area_met_by_lower=ar[4], area_short=ar[5])
    return out, bout


def min_dose_ratio(E, c, out):
    """min_dose_ratio of the report for the f32 durations `out` the solve returned.
    unbounded: min_i((sum_q (double)E[q][t_i] (double)out_q) rd_i) (m'/m) over the LP's rows (k_plan_rowcheck);
    bounded: min over classes 0 and 4 of (sum_q E[q][t] out_q) ((double)s / ((double)den_t m')), times m'/m (k_plan_xcheck).
    +inf for an empty set or m <= 0."""
    x = np.asarray(out, dtype=np.float32).astype(np.float64)
    m, mprime = c["m"], c["mprime"]
    if not (m > 0.0):
        return float("inf")
    if not c["bounded"]:
        if c["rows"].size == 0:
            return float("inf")
        ad = weighted(np.asarray(E)[:, c["rows"]], x) * c["rd"]
        return float(ad.min()) * (mprime / m)
    req = np.flatnonzero((c["cls"] == 0) | (c["cls"] == 4))
    if req.size == 0:
        return float("inf")
    acc = weighted(np.asarray(E)[:, req], x)
    return float((acc * (c["s"] / (c["den"][req] * mprime))).min()) * (mprime / m)


def model_dose(E, area, s, N, durations, first=0, count=None):
    """k_plan_model_dose: (float)((double)s * acc / (double)den_t) over [first, first + count), acc in ascending p; a row
    without area divides by 0: NaN where acc is 0, inf elsewhere"""
    E = np.asarray(E)
    count = E.shape[1] - first if count is None else count
    d = np.asarray(durations, dtype=np.float32).astype(np.float64)
    sub = E[:, first:first + count]
    den = (np.asarray(area, dtype=np.float32)[first:first + count] * f32(N)).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return ((float(f32(s)) * weighted(sub, d)) / den).astype(np.float32)


def seq_sum(v):
    """the f64 sum of f32 values in ascending index from 0.0 (the report's total_duration and lower_total)"""
    acc = 0.0
    for x in np.asarray(v, dtype=np.float32):
        acc = acc + float(x)
    return acc


def f32_at_least(x):
    """the smallest f32 >= x (f64)"""
    f = np.float32(x)
    if float(f) < x:
        f = np.nextafter(f, np.float32(np.inf))
    return f
