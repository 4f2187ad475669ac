"""A restatement of the adaptive gather (include/uvrt.h "adaptive gather") in numpy f64, one rounding per
operator: the count rule that turns (expected, variance) into a triangle's number of extra samples, the merge of the extra
estimate into both planes, and the whole of uvrt_gather_refine.  The samples are gather_stratified_restate.samples', the
occlusion query gather_restate.occluded, and x, q and v gather_variance_restate's: a triangle's extra samples are a gather of
n_t samples with the refine's seed.  Shared by tests/test_gather_refine_cpu.py, tests/test_gpu_gather_refine.py and
tests/tools/gather_refine_quality.py."""
import numpy as np

from gather_restate import f32, occluded, tri_normals
import gather_stratified_restate as gs
import gather_variance_restate as gv

INDEPENDENT, STRATIFIED = gs.INDEPENDENT, gs.STRATIFIED


def count_rule(X0, V0, nn, S0, rel_error, min_expected, max_extra):
    """n_t int32[count] of the count rule: 0, or a power of two in [2, max_extra]"""
    X0, V0, nn = (np.asarray(a, dtype=np.float64) for a in (X0, V0, nn))
    assert max_extra >= 2 and max_extra & (max_extra - 1) == 0
    with np.errstate(all="ignore"):
        r = np.float64(rel_error) * X0
        want = np.ceil(np.float64(S0) * (V0 / (r * r) - 1.0))
        eligible = ~(nn == 0.0) & (X0 > 0.0) & (V0 > 0.0) & ~(X0 < np.float64(min_expected))
        some = eligible & (want >= 1.0)                              # a NaN compares false
        capped = some & (want >= np.float64(max_extra))
        w = np.where(some & ~capped, np.maximum(want, 2.0), 2.0)     # 2 <= w < max_extra
    n = np.full(w.shape, 2, dtype=np.int64)
    p = 4
    while p <= max_extra:                                            # the smallest power of two >= w
        n = np.where(w > p // 2, p, n)
        p *= 2
    return np.where(capped, max_extra, np.where(some, n, 0)).astype(np.int32)


def merge(X0, V0, X1, V1, S0, n):
    """(expected, variance) after n extra samples with estimate X1 and variance V1 joined the first S0"""
    a, b = np.float64(S0), np.asarray(n, dtype=np.float64)
    with np.errstate(all="ignore"):
        tot = a + b
        e = (a * X0 + b * X1) / tot
        v = ((a * a) * V0 + (b * b) * V1) / (tot * tot)
    return e, v


def refine(orc, scene, frm, to, length, S0, mode, photons_equiv, expected, variance, rel_error, max_extra, seed, min_expected=0.0,
           flavour=0, first=0, count=None):
    """uvrt_gather_refine on the planes `expected` and `variance` (f64[T], not modified) over triangles [first, first + count):
    (expected', variance', n f64/int32[T] with 0 outside the range).  frm, to, length, S0, mode and photons_equiv are the
    remembered gather's."""
    T = scene.tris.shape[0]
    count = T - first if count is None else count
    _, _, _, nn = tri_normals(np.ascontiguousarray(scene.tris[first:first + count], dtype=f32))
    e, v = np.array(expected, dtype=np.float64), np.array(variance, dtype=np.float64)
    n_range = count_rule(e[first:first + count], v[first:first + count], nn, S0, rel_error, min_expected, max_extra)
    n = np.zeros(T, dtype=np.int32)
    n[first:first + count] = n_range
    groups = []
    for k in sorted(set(n_range.tolist()) - {0}):
        idx = np.nonzero(n_range == k)[0]
        lo, hi = int(idx[0]), int(idx[-1]) + 1                       # the samples of the triangles in between are dropped
        rays, w = gs.samples(orc, scene.tris, frm, to, length, k, seed, first + lo, hi - lo, mode)
        sel = ((idx - lo)[:, None] * k + np.arange(k)[None, :]).ravel()
        groups.append((k, idx, rays[sel], w[sel]))
    if groups:
        occ = occluded(orc, scene, np.concatenate([g[2] for g in groups]), flavour)
        at = 0
        for k, idx, rays, w in groups:
            t = first + idx
            X1, V1 = gv.reduce_var(np.ascontiguousarray(scene.tris[t]), w, occ[at:at + rays.size], k, photons_equiv, mode)
            at += rays.size
            e[t], v[t] = merge(e[t], v[t], X1, V1, S0, k)
    return e, v, n


def gather_and_refine(orc, scene, frm, to, length, S0, seed, photons_equiv, mode, rel_error, max_extra, refine_seed=None,
                      min_expected=0.0, flavour=0, first=0, count=None):
    """uvrt_gather_direct with the variance on, then uvrt_gather_refine over the same range (refine_seed None: ~seed, the host
    layer's choice): (expected, variance, n) of the range, and the first pass's (expected, variance)"""
    T = scene.tris.shape[0]
    count = T - first if count is None else count
    e0, v0, _ = gv.gather(orc, scene, frm, to, length, S0, seed, photons_equiv, mode, flavour, first, count)
    E, V = np.zeros(T), np.zeros(T)
    E[first:first + count], V[first:first + count] = e0, v0
    rs = (~int(seed)) & 0xFFFFFFFF if refine_seed is None else refine_seed
    e, v, n = refine(orc, scene, frm, to, length, S0, mode, photons_equiv, E, V, rel_error, max_extra, rs, min_expected, flavour,
                     first, count)
    return e[first:first + count], v[first:first + count], n[first:first + count], e0, v0
