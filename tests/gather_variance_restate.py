"""A restatement of the gather's variance plane (include/uvrt.h uvrt_set_gather_variance) and of
uvrt_plan_lower_confidence in numpy f64, one rounding per operator, explicit ordered loops over the samples as
gather_restate.reduce has them.  The samples, the occlusion query and the normals are the existing restatements'
(tests/gather_restate.py, tests/gather_stratified_restate.py); only the second pass over x_s = occluded ? 0 : w_s is new.
Shared by tests/test_gather_variance_cpu.py, tests/test_gpu_gather_variance.py and tests/tools/gather_confidence.py."""
import numpy as np

from gather_restate import f32, occluded, tri_normals
import gather_stratified_restate as gs

INDEPENDENT, STRATIFIED = gs.INDEPENDENT, gs.STRATIFIED


def visible_weights(w, occ, S):
    """x[count][S]: x_s = occluded ? 0 : w_s"""
    return np.where(np.asarray(occ).reshape(-1, S) != 0, 0.0, np.asarray(w, dtype=np.float64).reshape(-1, S))


def mean_and_q(x, mode):
    """(sum in sample order, m = sum / S, q of the mode) of x[count][S], S >= 2"""
    count, S = x.shape
    assert S >= 2
    total = np.zeros(count, dtype=np.float64)
    for s in range(S):
        total = total + x[:, s]
    with np.errstate(all="ignore"):
        m = total / np.float64(S)
        q = np.zeros(count, dtype=np.float64)
        if mode == INDEPENDENT:
            for s in range(S):
                d = x[:, s] - m
                q = q + d * d
        else:
            for s in range(1, S):
                d = x[:, s] - x[:, s - 1]
                q = q + d * d
    return total, m, q


def v_of_q(q, S, mode):
    """v = q / SS (independent) or q / (2 SS) (stratified), SS = (double)S * (double)(S - 1)"""
    SS = np.float64(S) * np.float64(S - 1)
    with np.errstate(all="ignore"):
        return q / SS if mode == INDEPENDENT else q / (2.0 * SS)


def sample_variance_v(x):
    """the sample variance of the mean of x[count][S], whatever the sampling mode: what the stratified mode does NOT use"""
    _, _, q = mean_and_q(x, INDEPENDENT)
    return v_of_q(q, x.shape[1], INDEPENDENT)


def reduce_var(tris, w, occ, S, photons_equiv, mode, first=0, count=None):
    """(expected, variance) f64[count] of triangles [first, first + count): k_gather_reduce_var<mode>"""
    T = tris.shape[0]
    count = T - first if count is None else count
    _, _, _, nn = tri_normals(np.ascontiguousarray(tris[first:first + count], dtype=f32))
    x = visible_weights(w, occ, S)
    _, m, q = mean_and_q(x, mode)
    with np.errstate(all="ignore"):
        c = np.float64(photons_equiv) * (0.5 * nn)
        e = c * m
        var = (c * c) * v_of_q(q, S, mode)
    return np.where(nn == 0.0, 0.0, e), np.where(nn == 0.0, 0.0, var)


def gather(orc, scene, frm, to, length, S, seed, photons_equiv, mode, flavour=0, first=0, count=None):
    """(expected, variance, x[count][S]) of uvrt_gather_direct under uvrt_set_gather_sampling(mode) with the variance on"""
    rays, w = gs.samples(orc, scene.tris, frm, to, length, S, seed, first, count, mode)
    occ = occluded(orc, scene, rays, flavour)
    e, v = reduce_var(scene.tris, w, occ, S, photons_equiv, mode, first, count)
    return e, v, visible_weights(w, occ, S)


def lower_confidence(X, V, z):
    """uvrt_plan_lower_confidence: lo = X - z * sqrt(V); X = lo > 0 ? lo : 0 (z = 0: X as it is)"""
    X = np.asarray(X, dtype=np.float64)
    if z == 0.0:
        return X.copy()
    with np.errstate(all="ignore"):
        lo = X - np.float64(z) * np.sqrt(np.asarray(V, dtype=np.float64))
    return np.where(lo > 0.0, lo, 0.0)


def cover_and_tightness(expected, variance, counts, z, min_photons=400):
    """over the triangles with >= min_photons photons: (the share whose count is >= max(0, expected - z sqrt(variance)),
    the median of that bound over the count, the share of bounds that are 0)"""
    sel = counts >= min_photons
    lo = lower_confidence(expected[sel], variance[sel], z)
    c = counts[sel].astype(np.float64)
    return float((c >= lo).mean()), float(np.median(lo / c)), float((lo == 0.0).mean())
