"""A restatement of the mirror gather (include/uvrt.h "specular panels") in numpy f32 / f64, one rounding per
operator, with explicit loops over the panels k, the samples s and the faces f, in order.  The draws are gather_restate's
(mode 0) or gather_stratified_restate's (mode 1), the closest hit of leg A is gather_indirect_restate.closest, the occlusion
query of leg B gather_restate.occluded, the face of a sample gather_faces_restate.sample_faces.  Also the virtual-lamp scenes:
the closed cube with a mirror on the wall x = 4 and the same twelve records with that wall collapsed to a point outside.
Shared by tests/test_gather_mirror_cpu.py, tests/test_gpu_gather_mirror.py and tests/tools/gather_mirror_quality.py."""
import numpy as np

import gather_faces_restate as gf
import gather_indirect_restate as gi
import gather_restate as gr
import gather_stratified_restate as gs

f32 = np.float32
f64 = np.float64
u32 = np.uint32
MIRROR_MAX = 8
MISS = f32(1e30)
PULL = f32(2.0 ** -10)                      # leg B's origin moves this share of the leg off the mirror
TMAX_B = f32(1.0 - 2.0 ** -9)               # ... and its far end stops as far before the receiver


def panel(point, normal, rho):
    """a panel as the tests hand it around: (point, normal, reflectance), the values of a uvrt_mirror record"""
    return (tuple(float(f32(v)) for v in point), tuple(float(f32(v)) for v in normal), float(f32(rho)))


def plane(pn):
    """(q f64[3], mh f64[3], rho f64) as uvrt_set_mirrors forms them on the host"""
    q = np.array([f64(f32(v)) for v in pn[0]])
    m = np.array([f64(f32(v)) for v in pn[1]])
    length = np.sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2])
    return q, m / length, f64(f32(pn[2]))


def points(tris, frm, to, length, S, seed, first=0, count=None, mode=gs.INDEPENDENT):
    """(p f32[n, 3], o f32[n, 3], n f64[n, 3], nn f64[n]) of the samples of triangles [first, first + count), n = count * S: the
    four draws, the point on the triangle and the lamp point of uvrt_gather_direct, sample for sample"""
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
        fr = [f32(v) for v in frm]
        sg = [f32(f32(x) - f32(v)) for x, v in zip(to, frm)]
        o = np.stack([fr[0] + u_m * sg[0], (fr[1] + u_h * f32(length)) + u_m * sg[1], fr[2] + u_m * sg[2]], axis=1)
    assert p.dtype == f32 and o.dtype == f32
    return p, o, n[k], nn[k]


def weigh(p, src, n, nn):
    """uvrt_gather_direct's ray and weight from the source points `src` to p: (D f32[n, 3], r f32[n], c f64[n], w f64[n],
    traced bool[n]); w is 0 where the distance is degenerate"""
    with np.errstate(all="ignore"):
        D = p - src
        assert D.dtype == f32
        r = np.sqrt((D[:, 0] * D[:, 0] + D[:, 1] * D[:, 1]) + D[:, 2] * D[:, 2])
        assert r.dtype == f32
        traced = np.isfinite(r) & (r > 0)
        Dd = D.astype(f64)
        R2 = (Dd[:, 0] * Dd[:, 0] + Dd[:, 1] * Dd[:, 1]) + Dd[:, 2] * Dd[:, 2]
        R = np.sqrt(R2)
        c = (n[:, 0] * Dd[:, 0] + n[:, 1] * Dd[:, 1]) + n[:, 2] * Dd[:, 2]
        w = np.abs(c) / ((nn * (R2 * R)) * gr.FOUR_PI)
    return D, r, c, np.where(traced, w, 0.0), traced


def side(q, mh, x):
    """the signed distance of the f32 points x from the plane, f64"""
    xd = x.astype(f64)
    return ((xd[:, 0] - q[0]) * mh[0] + (xd[:, 1] - q[1]) * mh[1]) + (xd[:, 2] - q[2]) * mh[2]


def _rays(orc, origin, direction, tmax):
    r = np.zeros(origin.shape[0], dtype=orc.RAY_DT)
    r["origx"], r["origy"], r["origz"] = origin[:, 0], origin[:, 1], origin[:, 2]
    r["dirx"], r["diry"], r["dirz"] = direction[:, 0], direction[:, 1], direction[:, 2]
    r["dist"] = tmax
    return r


def leg_a(orc, pn, p, o, n, nn):
    """Leg A of every sample in panel `pn`: dict(rays RAY_DT[n] with dist = tmax, w f64[n] = rho * the image's weight, c f64[n],
    front bool[n]: d_o > 0 and d_p > 0, d_p f64[n], ra f32[n]: the length of leg A up to the plane)"""
    q, mh, rho = plane(pn)
    cnt = p.shape[0]
    with np.errstate(all="ignore"):
        d_o, d_p = side(q, mh, o), side(q, mh, p)
        front = (d_o > 0.0) & (d_p > 0.0)
        two = 2.0 * d_o
        image = (o.astype(f64) - two[:, None] * mh[None, :]).astype(f32)
        D, r, c, w, ok = weigh(p, image, n, nn)
        tau = d_o / (d_o + d_p)
        P = (image.astype(f64) + tau[:, None] * D.astype(f64)).astype(f32)
        A = P - o
        assert A.dtype == f32
        ra = np.sqrt((A[:, 0] * A[:, 0] + A[:, 1] * A[:, 1]) + A[:, 2] * A[:, 2])
        assert ra.dtype == f32
        traced = front & ok & np.isfinite(ra) & (ra > 0)
        direction = np.where(traced[:, None], A / ra[:, None], np.array([0, 1, 0], dtype=f32)[None, :]).astype(f32)
    rays = _rays(orc, o, direction, np.where(traced, MISS, f32(0.0)).astype(f32))
    assert cnt == rays.size
    return dict(rays=rays, w=np.where(traced, rho * w, 0.0), c=np.where(front, c, 0.0), front=front, traced=traced, d_p=d_p, ra=ra)


def leg_b(orc, a_rays, dist, h, p, panel_of_tri, k):
    """Leg B from leg A's rays, their closest hits (dist f32, h int32, -1: a miss) and the receiver points: (rays RAY_DT[n],
    lost bool[n], off bool[n]: leg A hit a triangle that is no member of panel k)"""
    T = panel_of_tri.size
    hc = np.clip(h, 0, T - 1)
    member = (h >= 0) & (h < T) & (panel_of_tri[hc] == k + 1)
    o = np.stack([a_rays["origx"], a_rays["origy"], a_rays["origz"]], axis=1)
    d = np.stack([a_rays["dirx"], a_rays["diry"], a_rays["dirz"]], axis=1)
    with np.errstate(all="ignore"):
        Ph = o + dist[:, None] * d
        B = p - Ph
        assert B.dtype == f32
        rb = np.sqrt((B[:, 0] * B[:, 0] + B[:, 1] * B[:, 1]) + B[:, 2] * B[:, 2])
        assert rb.dtype == f32
        kept = member & np.isfinite(rb) & (rb > 0)
        origin = np.where(kept[:, None], Ph + B * PULL, o).astype(f32)
        direction = np.where(kept[:, None], B / rb[:, None], np.array([0, 1, 0], dtype=f32)[None, :]).astype(f32)
        tmax = np.where(kept, rb * TMAX_B, f32(0.0)).astype(f32)
    return _rays(orc, origin, direction, tmax), ~kept, (h >= 0) & ~member


def gather(orc, scene, panels, panel_of_tri, frm, to, length, S, seed, photons_equiv, flavour=0, first=0, count=None,
           mode=gs.INDEPENDENT, base=None, faces_base=None, sided=False):
    """uvrt_gather_mirror over triangles [first, first + count).  Returns (expected f64[count], faces f64[2][count] or None,
    info): with `base` (add = 1) the plane starts from it; with `sided` the face planes start from `faces_base` (add = 1) or
    are written by panel 0.  info: per panel a dict of the samples' masks and planes (m: m_k, x: x_s f64[count, S])."""
    T = scene.T
    count = T - first if count is None else count
    panel_of_tri = np.ascontiguousarray(panel_of_tri, dtype=np.uint8)
    assert panel_of_tri.size == T and 1 <= len(panels) <= MIRROR_MAX and panel_of_tri.max(initial=0) <= len(panels)
    p, o, n, nn = points(scene.tris, frm, to, length, S, seed, first, count, mode)
    nn_t = nn.reshape(count, S)[:, 0]
    expected = None if base is None else np.asarray(base, dtype=f64).copy()
    faces = None
    if sided and faces_base is not None:
        faces = np.asarray(faces_base, dtype=f64).copy()
    info = []
    for k, pn in enumerate(panels):
        a = leg_a(orc, pn, p, o, n, nn)
        dist, h = gi.closest(orc, scene, a["rays"], flavour)
        b_rays, lost, off = leg_b(orc, a["rays"], dist, h, p, panel_of_tri, k)
        occ = gr.occluded(orc, scene, b_rays, flavour) != 0
        x = np.where(lost | occ, 0.0, a["w"]).reshape(count, S)
        face = gf.sample_faces(a["c"]).reshape(count, S)
        total = np.zeros(count, dtype=f64)
        for s in range(S):
            total = total + x[:, s]
        with np.errstate(all="ignore"):
            m = np.where(nn_t == 0.0, 0.0, (f64(photons_equiv) * (0.5 * nn_t)) * (total / f64(S)))
        expected = m if expected is None else expected + m
        if sided:
            mf = np.zeros((2, count), dtype=f64)
            for f in (0, 1):
                tot = np.zeros(count, dtype=f64)
                for s in range(S):
                    tot = tot + np.where(face[:, s] == f, x[:, s], 0.0)
                with np.errstate(all="ignore"):
                    mf[f] = np.where(nn_t == 0.0, 0.0, (f64(photons_equiv) * (0.5 * nn_t)) * (tot / f64(S)))
            faces = mf if faces is None else faces + mf
        info.append(dict(m=m, x=x, w=a["w"].reshape(count, S), front=a["front"].reshape(count, S), ra=a["ra"].reshape(count, S),
                         dist=dist.reshape(count, S),
                         traced=a["traced"].reshape(count, S), d_p=a["d_p"].reshape(count, S), h=h.reshape(count, S),
                         lost=lost.reshape(count, S), off=off.reshape(count, S), occluded=(occ & ~lost).reshape(count, S)))
    return expected, faces, info


# ---------------------------------------------------------------- the virtual lamp
LAMP_A = (1.0, 0.5, 2.0)                    # scene A: the lamp in the cube ...
LAMP_B = (7.0, 0.5, 2.0)                    # ... scene B: its image in the plane x = 4
MIRROR_TRIS = (10, 11)                      # the wall x = 4: the cube's last two records
OUTSIDE = (9.0, 9.0, 9.0)


def wall_panel(rho=1.0, normal=(-1.0, 0.0, 0.0)):
    return panel((gi.CUBE_SIDE, 0.0, 0.0), normal, rho)


def wall_members(T=12, tris=MIRROR_TRIS):
    pot = np.zeros(T, dtype=np.uint8)
    pot[list(tris)] = 1
    return pot


def cube_without_wall():
    """the cube's twelve records with the wall x = 4 collapsed to a point outside: the numbering, and with it every draw, stays"""
    rows = gi.cube_tris()
    assert np.all(rows[list(MIRROR_TRIS)][:, [0, 4, 8]] == f32(gi.CUBE_SIDE)), "records 10 and 11 are the wall x = 4"
    for t in MIRROR_TRIS:
        rows[t, 0:3] = rows[t, 4:7] = rows[t, 8:11] = OUTSIDE
    return rows


# ---------------------------------------------------------------- two panels on the edge scene (tests/gather_edge_scene.py)
def edge_panels(rho0=0.75, rho1=0.5):
    """a panel in the plane x = 1 that looks at the lamp's side, and a tilted one through z = -1: neither follows the soup's
    triangles, as a flat panel does not follow a scanned wall"""
    return [panel((1.0, 0.0, 0.0), (-1.0, 0.0, 0.0), rho0), panel((0.0, 0.0, -1.0), (0.0, 0.25, 1.0), rho1)]


def edge_members(scene):
    """panel_of_tri of edge_panels: the triangles beyond x = 0.8, then (taking over) those beyond z = -0.8"""
    cen = scene.tris[:, 12:15]
    members = np.zeros(scene.T, dtype=np.uint8)
    members[cen[:, 0] > f32(0.8)] = 1
    members[cen[:, 2] < f32(-0.8)] = 2
    return members


# ---------------------------------------------------------------- the rules file of RayTracer::mirrorMap
class RulesError(ValueError):
    pass


USAGE = "mirror takes X0 Y0 Z0 X1 Y1 Z1 RHO plane QX QY QZ MX MY MZ"


def parse_rules(text, name="rules"):
    """[(lo f32[3], hi f32[3], rho f32, q f32[3], m f32[3])], one per panel, in file order; RulesError names the file and the
    line"""
    rules = []
    for no, line in enumerate(text.splitlines(), 1):
        words = line.split("#", 1)[0].split()
        if not words:
            continue

        def bad(why):
            return RulesError("%s:%d: %s" % (name, no, why))
        if words[0] != "mirror":
            raise bad("unknown keyword '%s'" % words[0])
        if len(words) != 15 or words[8] != "plane":
            raise bad(USAGE)
        try:
            with np.errstate(over="ignore"):
                v = [f32(float(w)) for w in words[1:8]]
                q = np.array([f32(float(w)) for w in words[9:15]], dtype=f32)
        except ValueError:
            raise bad("not a number")
        if np.any(np.isnan(v)) or not np.all(np.isfinite(q)):                      # (a box may reach to infinity)
            raise bad("not a finite number")
        if not np.isfinite(v[6]) or not (f32(0.0) <= v[6] <= f32(1.0)):
            raise bad("RHO must be finite and in [0, 1]")
        if np.all(q[3:6] == 0):
            raise bad("the plane's normal is zero")
        lo, hi = np.array(v[0:3], dtype=f32), np.array(v[3:6], dtype=f32)
        if np.any(lo > hi):
            raise bad("a lower bound of the box lies above its upper bound")
        if len(rules) == MIRROR_MAX:
            raise bad("a ninth panel (at most %d)" % MIRROR_MAX)
        rules.append((lo, hi, v[6], q[0:3].copy(), q[3:6].copy()))
    return rules


def rules_panels(tris, text, name="rules"):
    """(panels: [panel(q, m, rho)], panel_of_tri uint8[T]) of a rules file: line k makes panel k, its members the triangles
    whose stored centroid (tris[:, 12:15]) lies in the closed box, compared in f32; a later line takes a triangle over"""
    tris = np.ascontiguousarray(tris, dtype=f32)
    cen = tris[:, 12:15]
    members = np.zeros(tris.shape[0], dtype=np.uint8)
    panels = []
    for k, (lo, hi, rho, q, m) in enumerate(parse_rules(text, name)):
        inside = np.all((cen >= lo[None, :]) & (cen <= hi[None, :]), axis=1)
        members[inside] = k + 1
        panels.append(panel(q, m, rho))
    return panels, members
