"""A restatement of the stratified gather sampling (include/uvrt.h uvrt_set_gather_sampling) in numpy f32 /
uint32, one rounding per operator.  The RNG, the normals, the occlusion query and the reduction are tests/gather_restate.py's;
only the two lamp coordinates of a sample are formed differently, so `samples` below is gather_restate.samples with u_h and
u_m replaced (mode 0 hands over to gather_restate.samples itself).  Shared by tests/test_gather_stratified_cpu.py,
tests/test_gpu_gather_stratified.py and tests/tools/gather_quality.py."""
import numpy as np

from gather_restate import (FOUR_PI, TMAX_FACTOR, f32, u32, occluded, random_float, reduce, tri_normals, wang_hash)
import gather_restate as gr

INDEPENDENT, STRATIFIED = 0, 1
GOLDEN = u32(0x9E3779B9)
TWO_M24 = f32(2.0 ** -24)


def u_m_sequence(t, s, seed):
    """u_m of (triangle t, sample s): the golden-ratio Weyl sequence in uint32, rotated by a hash of (t, seed); f32, exact"""
    t = np.asarray(t, dtype=u32)
    s = np.asarray(s, dtype=u32)
    h_t = wang_hash(t ^ wang_hash(u32(seed) ^ GOLDEN))
    with np.errstate(over="ignore"):
        k = s * GOLDEN + h_t
    return (k >> u32(8)).astype(f32) * TWO_M24


def u_h_strata(s, xi_h, S):
    """u_h of sample s from its first draw: fl(fl((float)s + xi_h) / (float)S)"""
    u = (np.asarray(s).astype(f32) + xi_h) / f32(S)
    assert u.dtype == f32
    return u


def lamp_coordinates(first, count, S, seed):
    """(u_h, u_m, a, b before the fold) f32[count * S] of triangles [first, first + count) in stratified mode"""
    t = np.repeat(np.arange(first, first + count, dtype=np.uint64), S)
    s = np.tile(np.arange(S, dtype=np.uint64), count)
    j = ((t * np.uint64(S) + s) & np.uint64(0xFFFFFFFF)).astype(u32)
    rng = wang_hash(j ^ wang_hash(u32(seed)))
    xi_h, rng = random_float(rng)
    _, rng = random_float(rng)                       # xi_m: drawn and discarded
    a, rng = random_float(rng)
    b, rng = random_float(rng)
    return u_h_strata(s, xi_h, S), u_m_sequence(t.astype(u32), s.astype(u32), seed), a, b


def samples(orc, tris, frm, to, length, S, seed, first=0, count=None, mode=STRATIFIED):
    """The samples of triangles [first, first + count): (rays RAY_DT[count * S] with dist = tmax, w f64[count * S])"""
    if mode == INDEPENDENT:
        return gr.samples(orc, tris, frm, to, length, S, seed, first, count)
    T = tris.shape[0]
    count = T - first if count is None else count
    tris = np.ascontiguousarray(tris[first:first + count], dtype=f32)
    e1, e2, n, nn = tri_normals(tris)
    u_h, u_m, a, b = lamp_coordinates(first, count, S, seed)
    flip = (a + b) > f32(1.0)
    a = np.where(flip, f32(1.0) - a, a).astype(f32)
    b = np.where(flip, f32(1.0) - b, b).astype(f32)
    k = np.repeat(np.arange(count), S)
    v0 = tris[k, 0:3]
    p = (v0 + a[:, None] * e1[k]) + b[:, None] * e2[k]
    assert p.dtype == f32
    fr = [f32(v) for v in frm]
    sg = [f32(f32(x) - f32(v)) for x, v in zip(to, frm)]
    ox = fr[0] + u_m * sg[0]
    oy = (fr[1] + u_h * f32(length)) + u_m * sg[1]
    oz = fr[2] + u_m * sg[2]
    dx, dy, dz = p[:, 0] - ox, p[:, 1] - oy, p[:, 2] - oz
    with np.errstate(all="ignore"):
        r = np.sqrt((dx * dx + dy * dy) + dz * dz)
        assert r.dtype == f32
        traced = np.isfinite(r) & (r > 0)
        D = np.stack([dx, dy, dz], axis=1).astype(np.float64)
        R2 = (D[:, 0] * D[:, 0] + D[:, 1] * D[:, 1]) + D[:, 2] * D[:, 2]
        R = np.sqrt(R2)
        nk = n[k]
        ndotd = (nk[:, 0] * D[:, 0] + nk[:, 1] * D[:, 1]) + nk[:, 2] * D[:, 2]
        w = np.abs(ndotd) / ((nn[k] * (R2 * R)) * FOUR_PI)
        rays = np.zeros(count * S, dtype=orc.RAY_DT)
        rays["dirx"], rays["diry"], rays["dirz"] = dx / r, dy / r, dz / r
        rays["dist"] = r * TMAX_FACTOR
    rays["origx"], rays["origy"], rays["origz"] = ox, oy, oz
    for f, v in (("dirx", 0.0), ("diry", 1.0), ("dirz", 0.0), ("dist", 0.0)):
        rays[f][~traced] = f32(v)
    w[~traced] = 0.0
    return rays, w


def photon_counts(orc, scene, frm, to, length, N, u_seed=12345):
    """The truth an estimate is measured against: the per-triangle counts of N oracle photons of a lamp at `frm` (generate
    with SEED 0), on a sweep with every origin shifted along the segment by a uniform u of its own (numpy's PCG64, u_seed)"""
    rays, _ = orc.generate(0, N, frm, length, 0)
    if tuple(frm) != tuple(to):
        u = np.random.default_rng(u_seed).random(N, dtype=f32)
        rays["origx"] = rays["origx"] + u * f32(f32(to[0]) - f32(frm[0]))
        rays["origy"] = rays["origy"] + u * f32(f32(to[1]) - f32(frm[1]))
        rays["origz"] = rays["origz"] + u * f32(f32(to[2]) - f32(frm[2]))
    counts = np.zeros(scene.T, dtype=np.int32)
    orc.extend(counts, scene.tris, rays, scene.nodes, scene.triIdx)
    return counts


def quality(expected, counts, min_photons=400):
    """of expected / count over the triangles with >= min_photons photons: (5th, 50th, 95th percentile, rms of ratio - 1),
    and the number of zero-photon triangles with an estimate"""
    sel = counts >= min_photons
    ratio = expected[sel] / counts[sel]
    p5, p50, p95 = (float(v) for v in np.percentile(ratio, (5, 50, 95)))
    return p5, p50, p95, float(np.sqrt(np.mean((ratio - 1.0) ** 2))), int(((counts == 0) & (expected > 0)).sum())


def gather(orc, scene, frm, to, length, S, seed, photons_equiv, flavour=0, first=0, count=None, mode=STRATIFIED):
    """(expected f64[count], rays, occluded uint8) of uvrt_gather_direct under uvrt_set_gather_sampling(mode)"""
    rays, w = samples(orc, scene.tris, frm, to, length, S, seed, first, count, mode)
    occ = occluded(orc, scene, rays, flavour)
    return reduce(scene.tris, w, occ, S, photons_equiv, first, count), rays, occ
