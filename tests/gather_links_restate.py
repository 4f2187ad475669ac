"""A restatement of the recorded hit links and the multi-bounce gather over them (include/uvrt.h "recorded hit links") in numpy
f64, one rounding per operator.  The rays and their closest hits are gather_indirect_restate's; the links add the filter of
the one-bounce gather's y_s, and `linked` is the ABI's rule with explicit loops over the samples and the bounces, in order.
Shared by tests/test_gather_links_cpu.py, tests/test_gpu_gather_links.py and tests/tools/gather_links_quality.py."""
import numpy as np

import gather_indirect_restate as gi
import gather_restate as gr

f32 = np.float32
LINK_SEED = 0x85EBCA6B          # the host layer's fixed seed (raytracer.h reflectBounces)


def normals(tris):
    """nn_t = |cross(e1, e2)| in f64 for every triangle"""
    return gr.tri_normals(np.ascontiguousarray(tris, dtype=f32))[3]


def links(orc, scene, S2, seed, flavour=0, first=0, count=None):
    """int32 [count, S2]: link[t][s] = h_s when the ray hits, h_s != t and nn_h > 0, else -1"""
    T = scene.T
    count = T - first if count is None else count
    r, _ = gi.rays(orc, scene.tris, S2, seed, first, count)
    _, h = gi.closest(orc, scene, r, flavour)
    h = h.astype(np.int64).reshape(count, S2)
    nn = normals(scene.tris)
    t = np.arange(first, first + count, dtype=np.int64)[:, None]
    keep = (h >= 0) & (h != t) & (nn[np.clip(h, 0, T - 1)] > 0)
    return np.where(keep, h, -1).astype(np.int32)


def irradiance(nn, plane):
    """e[h] = nn_h > 0 ? plane[h] / (0.5 * nn_h) : 0.0"""
    with np.errstate(all="ignore"):
        return np.where(nn > 0, np.asarray(plane, dtype=np.float64) / (0.5 * nn), 0.0)


def bounce(nn_rows, e, link_rows, rho):
    """g[t] for the triangles whose normals and links are given, from the irradiance e of ALL triangles"""
    link_rows = np.asarray(link_rows, dtype=np.int64)
    S2 = link_rows.shape[1]
    lc = np.clip(link_rows, 0, e.size - 1)
    with np.errstate(all="ignore"):
        tot = np.zeros(link_rows.shape[0], dtype=np.float64)
        for s in range(S2):
            tot = tot + np.where(link_rows[:, s] >= 0, e[lc[:, s]], 0.0)
        g = (np.float64(f32(rho)) * (0.5 * nn_rows)) * ((2.0 * tot) / np.float64(S2))
        return np.where(nn_rows == 0.0, 0.0, g)


def bounces(tris, source, links, rho, K):
    """[g_1, .., g_K], each f64[T], from the links of ALL T triangles"""
    nn = normals(tris)
    links = np.asarray(links).reshape(nn.size, -1)
    out = []
    e = irradiance(nn, source)
    for _ in range(K):
        out.append(bounce(nn, e, links, rho))
        e = irradiance(nn, out[-1])
    return out


def linked(tris, source, links, rho, K, first=0, count=None, base=None):
    """expected[first, first + count) of uvrt_gather_indirect_linked; with `base` (add = 1, f64[count]) base + total.
    `links`: those of all T triangles, or for K = 1 those of the range alone"""
    nn = normals(tris)
    T = nn.size
    count = T - first if count is None else count
    links = np.asarray(links)
    if K == 1 and links.shape[0] == count:
        total = bounce(nn[first:first + count], irradiance(nn, source), links, rho)
    else:
        g = bounces(tris, source, links, rho, K)
        total = g[0]
        for b in range(1, K):
            total = total + g[b]
        total = total[first:first + count]
    return total if base is None else np.asarray(base, dtype=np.float64) + total
