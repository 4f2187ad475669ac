"""A restatement of the face-resolved gather and bounces (include/uvrt.h "face-resolved gather and bounces") in numpy f32 / f64,
one rounding per operator: the face a direct sample arrives on (the sign of the n.D its weight takes the absolute value of),
the two face planes, the sided links and the rule of uvrt_gather_indirect_linked_sided with explicit loops over the samples,
the faces and the bounces, in order.  The samples, the occlusion query, the bounce's rays and their closest hits are
gather_restate's, gather_stratified_restate's, gather_indirect_restate's and gather_links_restate's.  Also the plates scene:
three parallel squares inside the closed cube, where the two-sided bounce lights what an opaque sheet shades.
Shared by tests/test_gather_faces_cpu.py, tests/test_gpu_gather_faces.py and tests/tools/gather_faces_quality.py."""
import numpy as np

import gather_indirect_restate as gi
import gather_links_restate as gl
import gather_restate as gr
import gather_stratified_restate as gs

f32 = np.float32
u32 = np.uint32


# ---------------------------------------------------------------- the direct gather's face planes
def sample_ndotd(tris, frm, to, length, S, seed, first=0, count=None, mode=gs.INDEPENDENT):
    """c_s = (n.x*D.x + n.y*D.y) + n.z*D.z, f64[count * S], of the samples gather_restate.samples (mode 0) or
    gather_stratified_restate.samples (mode 1) make: the same draws, the same point, the same origin"""
    T = tris.shape[0]
    count = T - first if count is None else count
    tr = np.ascontiguousarray(tris[first:first + count], dtype=f32)
    e1, e2, n, nn = gr.tri_normals(tr)
    if mode == gs.INDEPENDENT:
        t = np.repeat(np.arange(first, first + count, dtype=np.uint64), S)
        s = np.tile(np.arange(S, dtype=np.uint64), count)
        j = ((t * np.uint64(S) + s) & np.uint64(0xFFFFFFFF)).astype(u32)
        rng = gr.wang_hash(j ^ gr.wang_hash(u32(seed)))
        u_h, rng = gr.random_float(rng)
        u_m, rng = gr.random_float(rng)
        a, rng = gr.random_float(rng)
        b, rng = gr.random_float(rng)
    else:
        u_h, u_m, a, b = gs.lamp_coordinates(first, count, S, seed)
    flip = (a + b) > f32(1.0)
    a = np.where(flip, f32(1.0) - a, a).astype(f32)
    b = np.where(flip, f32(1.0) - b, b).astype(f32)
    k = np.repeat(np.arange(count), S)
    with np.errstate(all="ignore"):
        p = (tr[k, 0:3] + a[:, None] * e1[k]) + b[:, None] * e2[k]
        assert p.dtype == f32
        fr = [f32(v) for v in frm]
        sg = [f32(f32(x) - f32(v)) for x, v in zip(to, frm)]
        ox = fr[0] + u_m * sg[0]
        oy = (fr[1] + u_h * f32(length)) + u_m * sg[1]
        oz = fr[2] + u_m * sg[2]
        D = np.stack([p[:, 0] - ox, p[:, 1] - oy, p[:, 2] - oz], axis=1)
        assert D.dtype == f32
        D = D.astype(np.float64)
        nk = n[k]
        return (nk[:, 0] * D[:, 0] + nk[:, 1] * D[:, 1]) + nk[:, 2] * D[:, 2]


def sample_faces(ndotd):
    """f_s = c_s < 0 ? 0 : 1 (a NaN, which only a sample of weight 0 has, counts as face 1)"""
    with np.errstate(all="ignore"):
        return np.where(np.asarray(ndotd) < 0.0, 0, 1).astype(np.uint8)


def reduce_faces(tris, w, occ, face, S, photons_equiv, first=0, count=None):
    """faces[2][first, first + count): gather_restate.reduce over the samples of each face alone, in sample order from +0.0"""
    T = tris.shape[0]
    count = T - first if count is None else count
    nn = gr.tri_normals(np.ascontiguousarray(tris[first:first + count], dtype=f32))[3]
    w, occ, face = w.reshape(count, S), occ.reshape(count, S), face.reshape(count, S)
    out = np.zeros((2, count), dtype=np.float64)
    for f in (0, 1):
        total = np.zeros(count, dtype=np.float64)
        for s in range(S):
            # (a sample of the other face adds +0.0: every term is >= +0, so the bits are those of skipping it)
            total = total + np.where((face[:, s] == f) & (occ[:, s] == 0), w[:, s], 0.0)
        with np.errstate(all="ignore"):
            out[f] = np.where(nn == 0.0, 0.0, (np.float64(photons_equiv) * (0.5 * nn)) * (total / np.float64(S)))
    return out


def gather_faces(orc, scene, frm, to, length, S, seed, photons_equiv, flavour=0, first=0, count=None, mode=gs.INDEPENDENT):
    """(faces f64[2][count], expected f64[count]) of uvrt_gather_direct with uvrt_set_gather_faces(1)"""
    rays, w = gs.samples(orc, scene.tris, frm, to, length, S, seed, first, count, mode)
    occ = gr.occluded(orc, scene, rays, flavour)
    face = sample_faces(sample_ndotd(scene.tris, frm, to, length, S, seed, first, count, mode))
    return (reduce_faces(scene.tris, w, occ, face, S, photons_equiv, first, count),
            gr.reduce(scene.tris, w, occ, S, photons_equiv, first, count))


# ---------------------------------------------------------------- sided links
def sided_links(orc, scene, S2, seed, flavour=0, first=0, count=None):
    """int32 [count, S2]: link[t][s] = (h_s << 1) | a_s under the plain link's filter, else -1; a_s = 0 when the f32 direction
    of the sample meets the side n_h points to (n_h . dir < 0)"""
    T = scene.T
    count = T - first if count is None else count
    r, _ = gi.rays(orc, scene.tris, S2, seed, first, count)
    _, h = gi.closest(orc, scene, r, flavour)
    h = h.astype(np.int64)
    _, _, n, nn = gr.tri_normals(np.ascontiguousarray(scene.tris, dtype=f32))
    t = np.repeat(np.arange(first, first + count, dtype=np.int64), S2)
    hc = np.clip(h, 0, T - 1)
    keep = (h >= 0) & (h != t) & (nn[hc] > 0)
    d = np.stack([r["dirx"], r["diry"], r["dirz"]], axis=1).astype(np.float64)
    with np.errstate(all="ignore"):
        c = (n[hc, 0] * d[:, 0] + n[hc, 1] * d[:, 1]) + n[hc, 2] * d[:, 2]
    a = np.where(c < 0.0, 0, 1)
    return np.where(keep, (h << 1) | a, -1).astype(np.int32).reshape(count, S2)


# ---------------------------------------------------------------- the face-resolved linked gather
def irradiance(nn, faces):
    """e[f][h] = nn_h > 0 ? faces[f][h] / (0.5 * nn_h) : 0.0"""
    with np.errstate(all="ignore"):
        return np.where(nn > 0, np.asarray(faces, dtype=np.float64) / (0.5 * nn), 0.0)


def bounce(nn, e, links, rho):
    """g[2][T] from the irradiance e[2][T] and the sided links of all T triangles: sample s leaves face s & 1"""
    links = np.asarray(links, dtype=np.int64)
    T, S2 = links.shape
    g = np.zeros((2, T), dtype=np.float64)
    with np.errstate(all="ignore"):
        for f in (0, 1):
            tot = np.zeros(T, dtype=np.float64)
            for s in range(f, S2, 2):
                L = links[:, s]
                Lc = np.clip(L, 0, None)
                tot = tot + np.where(L >= 0, e[Lc & 1, Lc >> 1], 0.0)
            gf = (np.float64(f32(rho)) * (0.5 * nn)) * ((2.0 * tot) / np.float64(S2))
            g[f] = np.where(nn == 0.0, 0.0, gf)
    return g


def bounces(tris, faces, links, rho, K):
    """([g_1, .., g_K], [e_0, .., e_K]), each f64[2][T]"""
    nn = gl.normals(tris)
    links = np.asarray(links).reshape(nn.size, -1)
    e = [irradiance(nn, faces)]
    g = []
    for _ in range(K):
        g.append(bounce(nn, e[-1], links, rho))
        e.append(irradiance(nn, g[-1]))
    return g, e


def linked(tris, faces, links, rho, K, first=0, count=None, base=None):
    """expected[first, first + count) of uvrt_gather_indirect_linked_sided; with `base` (add = 1, f64[count]) base + total"""
    T = tris.shape[0]
    count = T - first if count is None else count
    g, _ = bounces(tris, faces, links, rho, K)
    total = g[0][0] + g[0][1]
    for b in range(1, K):
        total = total + (g[b][0] + g[b][1])
    total = total[first:first + count]
    return total if base is None else np.asarray(base, dtype=np.float64) + total


# ---------------------------------------------------------------- hand-made scenes
def inner_face(tris, centre):
    """int[T]: the face of each triangle that looks at `centre` (0: n points to it)"""
    tris = np.ascontiguousarray(tris, dtype=f32)
    n = gr.tri_normals(tris)[2]
    to = np.asarray(centre, dtype=np.float64)[None, :] - tris[:, 0:3].astype(np.float64)
    return np.where((n * to).sum(axis=1) > 0, 0, 1)


def cube_faces(source, side=gi.CUBE_SIDE):
    """the closed cube's face planes with `source` on the inner faces and 0 on the outer ones"""
    inner = inner_face(gi.cube_tris(side), (side / 2,) * 3)
    out = np.zeros((2, 12), dtype=np.float64)
    out[inner, np.arange(12)] = source
    return out


PLATE_LO, PLATE_HI = 1.0, 3.0              # the plates span [1, 3] x [1, 3] in x and z
PLATE_Y = {"C": 1.0, "A": 2.0, "B": 3.0}   # heights: C below, A in the middle, B above
PLATES = {"A": (12, 13), "B": (14, 15), "C": (16, 17)}     # triangle indices behind the cube's 12


def plates_tris():
    """the closed cube and, inside it, three parallel horizontal squares of two triangles each, wound so that n = +y: face 0 looks
    up, face 1 looks down"""
    rows = [gi.cube_tris()]
    lo, hi = PLATE_LO, PLATE_HI
    for name in ("A", "B", "C"):
        y = PLATE_Y[name]
        q = np.zeros((2, 16), dtype=f32)
        # (a, b, c), (a, c, d) with a = (lo, lo), b = (lo, hi), c = (hi, hi), d = (hi, lo) in (x, z): cross(e1, e2) = +y
        a, b, c, d = (lo, y, lo), (lo, y, hi), (hi, y, hi), (hi, y, lo)
        q[0, 0:3], q[0, 4:7], q[0, 8:11] = a, b, c
        q[1, 0:3], q[1, 4:7], q[1, 8:11] = a, c, d
        rows.append(q)
    return np.concatenate(rows)


def plates_faces(value=100.0):
    """face planes f64[2][18]: only A's face towards B (face 0, looking up) emits"""
    out = np.zeros((2, 18), dtype=np.float64)
    out[0, list(PLATES["A"])] = value
    return out
