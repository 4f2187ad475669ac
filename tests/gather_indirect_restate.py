"""A restatement of the closest-hit query and the one-bounce gather (include/uvrt.h "one diffuse bounce") in numpy f32 / f64,
one rounding per operator: the rays of uvrt_gather_indirect, the closest hit of each (orc.extend with `dist` preset to the
ray's tmax and `triID` read back), the look-up in the source plane and the reduction.  The RNG and the triangle normals are
gather_restate's.  Shared by tests/test_gather_indirect_cpu.py, tests/test_gpu_closest_hits.py and
tests/test_gpu_gather_indirect.py."""
import numpy as np

import gather_restate as gr

f32 = np.float32
u32 = np.uint32
MISS = f32(1e30)
ROUNDS = 8

CUBE_SIDE = 4.0
CUBE_QUADS = ((0, 1, 2, 3), (4, 5, 6, 7), (0, 1, 5, 4), (3, 2, 6, 7), (0, 3, 7, 4), (1, 2, 6, 5))


def cube_tris(side=CUBE_SIDE):
    """the closed cube: 12 Tri records, quads split as (a, b, c), (a, c, d)"""
    L = side
    c = [(0, 0, 0), (L, 0, 0), (L, L, 0), (0, L, 0), (0, 0, L), (L, 0, L), (L, L, L), (0, L, L)]
    rows = np.zeros((12, 16), dtype=f32)
    for q, (a, b, cc, d) in enumerate(CUBE_QUADS):
        for k, (i0, i1, i2) in enumerate(((a, b, cc), (a, cc, d))):
            rows[2 * q + k, 0:3], rows[2 * q + k, 4:7], rows[2 * q + k, 8:11] = c[i0], c[i1], c[i2]
    return rows


def rays(orc, tris, S, seed, first=0, count=None):
    """The rays of triangles [first, first + count): (RAY_DT[count * S] with dist = tmax, bool[count * S]: the sample fell back
    to the disc's centre after ROUNDS rejected rounds)"""
    T = tris.shape[0]
    count = T - first if count is None else count
    tr = np.ascontiguousarray(tris[first:first + count], dtype=f32)
    e1, e2, n, nn = gr.tri_normals(tr)
    t = np.repeat(np.arange(first, first + count, dtype=np.uint64), S)
    s = np.tile(np.arange(S, dtype=np.uint64), count)
    j = ((t * np.uint64(S) + s) & np.uint64(0xFFFFFFFF)).astype(u32)
    rng = gr.wang_hash(j ^ gr.wang_hash(u32(seed)))
    a, rng = gr.random_float(rng)
    b, rng = gr.random_float(rng)
    flip = (a + b) > f32(1.0)
    a = np.where(flip, f32(1.0) - a, a).astype(f32)
    b = np.where(flip, f32(1.0) - b, b).astype(f32)
    k = np.repeat(np.arange(count), S)
    with np.errstate(all="ignore"):
        p = (tr[k, 0:3] + a[:, None] * e1[k]) + b[:, None] * e2[k]
    assert p.dtype == f32
    x = np.zeros(count * S)
    y = np.zeros(count * S)
    done = np.zeros(count * S, dtype=bool)
    for _ in range(ROUNDS):
        xf, rng = gr.random_float(rng)      # (a sample that is done draws on, unused)
        yf, rng = gr.random_float(rng)
        xd = (xf * f32(2.0) - f32(1.0)).astype(np.float64)
        yd = (yf * f32(2.0) - f32(1.0)).astype(np.float64)
        take = ~done & ((xd * xd + yd * yd) <= 1.0)
        x[take], y[take] = xd[take], yd[take]
        done |= take
    with np.errstate(all="ignore"):
        z = np.sqrt(1.0 - (x * x + y * y))
        E = e1.astype(np.float64)
        l1 = np.sqrt((E[:, 0] * E[:, 0] + E[:, 1] * E[:, 1]) + E[:, 2] * E[:, 2])
        Tv = E / l1[:, None]
        Bv = np.stack([n[:, 1] * Tv[:, 2] - n[:, 2] * Tv[:, 1],
                       n[:, 2] * Tv[:, 0] - n[:, 0] * Tv[:, 2],
                       n[:, 0] * Tv[:, 1] - n[:, 1] * Tv[:, 0]], axis=1) / nn[:, None]
        zz = np.where((s & np.uint64(1)) != 0, -z, z) / nn[k]
        D = ((x[:, None] * Tv[k]) + (y[:, None] * Bv[k])) + (zz[:, None] * n[k])
        d = D.astype(f32)
    traced = (nn[k] != 0.0) & np.isfinite(d).all(axis=1) & (d != 0).any(axis=1)
    out = np.zeros(count * S, dtype=orc.RAY_DT)
    out["dirx"], out["diry"], out["dirz"] = np.where(traced, d[:, 0], f32(0)), np.where(traced, d[:, 1], f32(1)), np.where(traced, d[:, 2], f32(0))
    out["origx"], out["origy"], out["origz"] = p[:, 0], p[:, 1], p[:, 2]
    out["dist"] = np.where(traced, MISS, f32(0.0))
    return out, ~done


def closest(orc, scene, r, flavour=0, stats=None):
    """(dist f32[n], tri int32[n]) as extend.cl leaves them for rays whose dist is preset to r["dist"]; tri = -1 and dist = the
    preset (same bits) where nothing is accepted"""
    o = np.ascontiguousarray(r).copy()
    o["triID"] = 0
    temp = np.zeros(scene.T, dtype=np.int32)
    orc.set_flavour(flavour)
    try:
        st = orc.extend(temp, scene.tris, o, scene.nodes, scene.triIdx)
    finally:
        orc.set_flavour(0)
    if stats is not None:
        stats.update(st)
    hit = gr.bits(o["dist"]) != gr.bits(r["dist"])
    return o["dist"].copy(), np.where(hit, o["triID"].astype(np.int64), -1).astype(np.int32)


def reduce(tris, source, h, rho, S, first=0, count=None, base=None):
    """ind[first, first + count) from the hit triangles h (int[count * S], -1: a miss); with `base` (add = 1) base + ind"""
    T = tris.shape[0]
    count = T - first if count is None else count
    _, _, _, nn_all = gr.tri_normals(np.ascontiguousarray(tris, dtype=f32))
    nn = nn_all[first:first + count]
    h = np.asarray(h, dtype=np.int64).reshape(count, S)
    t = np.arange(first, first + count, dtype=np.int64)[:, None]
    hc = np.clip(h, 0, T - 1)
    with np.errstate(all="ignore"):
        dens = np.asarray(source, dtype=np.float64)[hc] / (0.5 * nn_all[hc])
        val = np.where((h >= 0) & (h != t) & (nn_all[hc] > 0), dens, 0.0)
        tot = np.zeros(count, dtype=np.float64)
        for s in range(S):
            tot = tot + val[:, s]
        ind = (np.float64(f32(rho)) * (0.5 * nn)) * ((2.0 * tot) / np.float64(S))
        ind = np.where(nn == 0.0, 0.0, ind)
        return ind if base is None else np.asarray(base, dtype=np.float64) + ind


def indirect(orc, scene, source, rho, S, seed, flavour=0, first=0, count=None, base=None, stats=None):
    """(expected f64[count] of uvrt_gather_indirect, rays, hit triangles int32, fallback flags)"""
    r, fell_back = rays(orc, scene.tris, S, seed, first, count)
    _, h = closest(orc, scene, r, flavour, stats)
    return reduce(scene.tris, source, h, rho, S, first, count, base), r, h, fell_back
