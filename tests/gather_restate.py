"""A restatement of the direct gather (include/uvrt.h "shadow rays and the direct gather") in numpy f32 / f64, one rounding
per operator: the samples of uvrt_gather_direct, their weights, the reduction, uvrt_accumulate_expected.  The RNG is
cl/tools.cl:2-4 written over numpy uint32 arrays and checked against the oracle library's orc_wang_hash / orc_random_float
(check_rng); the occlusion query is orc.extend with every ray's `dist` preset to its tmax.  Shared by
tests/test_gather_cpu.py, tests/test_gpu_shadow_rays.py and tests/test_gpu_gather.py."""
import ctypes as C

import numpy as np

f32 = np.float32
u32 = np.uint32
TMAX_FACTOR = f32(0.9990234375)            # 1 - 2^-10
FOUR_PI = 12.566370614359172


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def wang_hash(s):
    s = np.asarray(s, dtype=u32)
    with np.errstate(over="ignore"):
        s = (s ^ u32(61)) ^ (s >> u32(16))
        s = s * u32(9)
        s = s ^ (s >> u32(4))
        s = s * u32(0x27d4eb2d)
        s = s ^ (s >> u32(15))
    return s


def random_float(s):
    """(the float, the new state) of RandomFloat over an array of states"""
    s = s ^ (s << u32(13))
    s = s ^ (s >> u32(17))
    s = s ^ (s << u32(5))
    return s.astype(f32) * f32(2.3283064365387e-10), s


def check_rng(orc, n=4096):
    """the numpy RNG above against the oracle library's, on n states"""
    L = orc.lib()
    L.orc_random_float.restype = C.c_float
    L.orc_random_float.argtypes = [C.POINTER(C.c_uint32)]
    j = (np.arange(n, dtype=np.uint64) * np.uint64(2654435761) % np.uint64(1 << 32)).astype(u32)
    h = wang_hash(j)
    fl, st = random_float(h)
    for k in range(n):
        hk = L.orc_wang_hash(int(j[k]))
        assert hk == int(h[k])
        s = C.c_uint32(hk)
        v = L.orc_random_float(C.byref(s))
        assert f32(v).view(u32) == fl[k].view(u32) and s.value == int(st[k])


def tri_normals(tris):
    """(e1, e2 in f32, n = cross(e1, e2) in f64, nn = |n|) of the 64-byte Tri records"""
    v0, v1, v2 = tris[:, 0:3], tris[:, 4:7], tris[:, 8:11]
    e1 = (v1 - v0).astype(f32)
    e2 = (v2 - v0).astype(f32)
    a, b = e1.astype(np.float64), e2.astype(np.float64)
    n = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1],
                  a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                  a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)
    nn = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
    return e1, e2, n, nn


def samples(orc, tris, frm, to, length, S, seed, first=0, count=None):
    """The samples of triangles [first, first + count): (rays RAY_DT[count * S] with dist = tmax, w f64[count * S])"""
    T = tris.shape[0]
    count = T - first if count is None else count
    tris = np.ascontiguousarray(tris[first:first + count], dtype=f32)
    e1, e2, n, nn = tri_normals(tris)
    t = np.repeat(np.arange(first, first + count, dtype=np.uint64), S)
    s = np.tile(np.arange(S, dtype=np.uint64), count)
    j = ((t * np.uint64(S) + s) & np.uint64(0xFFFFFFFF)).astype(u32)
    rng = wang_hash(j ^ wang_hash(u32(seed)))
    u_h, rng = random_float(rng)
    u_m, rng = random_float(rng)
    a, rng = random_float(rng)
    b, rng = random_float(rng)
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


def occluded(orc, scene, rays, flavour=0, stats=None):
    """uint8[n]: orc.extend with dist preset to the ray's tmax accepted some triangle"""
    o = np.ascontiguousarray(rays).copy()
    o["triID"] = 0
    temp = np.zeros(scene.T, dtype=np.int32)
    orc.set_flavour(flavour)
    try:
        st = orc.extend(temp, scene.tris, o, scene.nodes, scene.triIdx)
    finally:
        orc.set_flavour(0)
    if stats is not None:
        stats.update(st)
    return (bits(o["dist"]) != bits(rays["dist"])).astype(np.uint8)


def reduce(tris, w, occ, S, photons_equiv, first=0, count=None):
    """expected[first, first + count) from the samples' weights and occlusion bytes"""
    T = tris.shape[0]
    count = T - first if count is None else count
    _, _, _, nn = tri_normals(np.ascontiguousarray(tris[first:first + count], dtype=f32))
    w = w.reshape(count, S)
    occ = occ.reshape(count, S)
    total = np.zeros(count, dtype=np.float64)
    for s in range(S):
        total = total + np.where(occ[:, s] != 0, 0.0, w[:, s])
    with np.errstate(all="ignore"):
        e = (np.float64(photons_equiv) * (0.5 * nn)) * (total / np.float64(S))
    return np.where(nn == 0.0, 0.0, e)


def gather(orc, scene, frm, to, length, S, seed, photons_equiv, flavour=0, first=0, count=None):
    """(expected f64[count], rays, occluded uint8) of uvrt_gather_direct"""
    rays, w = samples(orc, scene.tris, frm, to, length, S, seed, first, count)
    occ = occluded(orc, scene, rays, flavour)
    return reduce(scene.tris, w, occ, S, photons_equiv, first, count), rays, occ


def accumulate_expected(photon_map, max_map, expected, time_step):
    """uvrt_accumulate_expected on numpy f64 maps, in place; returns the zeroed plane"""
    photon_map[:] = photon_map + expected * np.float64(f32(time_step))
    max_map[:] = np.where(max_map < expected, expected, max_map)
    return np.zeros_like(expected)
