"""The scenes, cases and references of the radiometry tests, shared by tests/test_radiometry_cpu.py (the
restatements against the closed forms, and the power of every case) and tests/test_gpu_radiometry.py (the kernels against the
closed forms).  Geometry and expected values only: no kernel, no restatement and no RNG is used to form a reference.  The closed
cube and its wall panel are gather_indirect_restate.cube_tris and gather_mirror_restate.wall_panel, taken as geometry.

Every coordinate is rounded to f32 before the reference sees it, so the reference and the kernels speak of the same triangles
and the same lamp.  All scenes have at most 14 triangles."""
import functools
import json
import os

import numpy as np

import radiometry_reference as rr

f32 = np.float32
f64 = np.float64

N = 1 << 20                     # photons_equiv of every gather, and the photon count of the photon path
K = 8                           # calls per case, one seed each
S = 4096                        # samples per triangle and call (S2 for the bounces)
SEEDS = tuple(range(101, 101 + K))


def r32(v):
    return tuple(float(f32(x)) for x in v)


def rows_of(triangles):
    """64-byte Tri records from ((v0, v1, v2), ..)"""
    rows = np.zeros((len(triangles), 16), dtype=f32)
    for k, (v0, v1, v2) in enumerate(triangles):
        rows[k, 0:3], rows[k, 4:7], rows[k, 8:11] = v0, v1, v2
    return rows


def verts(rows):
    """f64 [T, 3, 3] of the records' f32 vertices"""
    rows = np.asarray(rows, dtype=f32)
    return np.stack([rows[:, 0:3], rows[:, 4:7], rows[:, 8:11]], axis=1).astype(f64)


def areas(rows):
    return np.array([rr.tri_normal(t)[1] for t in verts(rows)])


def quad(a, b, c, d, flip_second=True):
    """two triangles of the quad a b c d; with flip_second the second is wound the other way, so both windings occur"""
    return [(a, b, c), (a, d, c) if flip_second else (a, c, d)]


# ---------------------------------------------------------------- floor and plate
LAMP = r32((0.9, 1.6, 0.7))
# The rod stands lower than the point lamp: from its foot at y = 0.5 a 1.2 m rod and the point at its middle differ by 5 and more
# tolerances of the photon counts (from y = 1.6 by less than one), so the "rod at its midpoint" variant cannot pass
ROD_FOOT = r32((0.9, 0.5, 0.7))
SWEEP_TO = r32((1.4, 0.8, 0.7))             # the sweep stays in the plane z = LAMP.z, in which the edge-on triangle lies
ROD = float(f32(1.2))
PLATE = [r32(v) for v in ((0.8, 1.0, 0.8), (1.2, 1.0, 0.8), (1.2, 1.0, 1.2), (0.8, 1.0, 1.2))]
SHADOWED = tuple(r32(v) for v in ((0.9, 0.5, 1.0), (1.3, 0.5, 1.1), (1.0, 0.5, 1.5)))      # wholly in the plate's shadow
EDGE_ON = tuple(r32(v) for v in ((0.1, 0.2, 0.7), (0.5, 0.2, 0.7), (0.3, 0.6, 0.7)))       # in the plane z = LAMP.z


def floor_triangles():
    """a 2 x 2 floor at y = 0, four unit quads of two triangles; the quads' windings alternate"""
    out = []
    for i in range(2):
        for k in range(2):
            a, b, c, d = (i, 0, k), (i + 1, 0, k), (i + 1, 0, k + 1), (i, 0, k + 1)
            out += quad(a, b, c, d) if (i + k) % 2 == 0 else quad(a, d, c, b)
    return out


def floor_rows(plate):
    """floor (0..7) [+ plate (8, 9) + the shadowed triangle (10)] + the edge-on triangle (last)"""
    t = floor_triangles()
    if plate:
        t += quad(*PLATE) + [SHADOWED]
    return rows_of(t + [EDGE_ON])


CUBE_LAMP = r32((1.0, 0.5, 2.0))
CUBE_ROD = float(f32(2.4))                  # (a 1.2 m rod in this cube lies 2 tolerances from the point at its middle, this one 5)

DIRECT_CASES = {
    # name: (scene: "plate", "floor" or "cube", from, to, length)
    "point lamp, plate": ("plate", LAMP, LAMP, 0.0),
    "rod": ("floor", ROD_FOOT, ROD_FOOT, ROD),
    "sweep": ("floor", ROD_FOOT, SWEEP_TO, ROD),
    "rod in the closed cube": ("cube", CUBE_LAMP, CUBE_LAMP, CUBE_ROD),
}
# the order of the moments' tensor rule, where 12 (against 24) is not enough: the cube's walls are 4 m wide and 0.5 m from the lamp
MOMENTS_ORDER = {"rod in the closed cube": 32}


def direct_rows(name):
    kind = DIRECT_CASES[name][0]
    return cube_rows() if kind == "cube" else floor_rows(kind == "plate")


def direct_occluders(name):
    return (np.array(PLATE, dtype=f64),) if DIRECT_CASES[name][0] == "plate" else ()


def direct_dark(name):
    """how many triangles of the case have a reference of exactly 0"""
    return {"plate": 2, "floor": 1, "cube": 0}[DIRECT_CASES[name][0]]


def check_direct_scene(name):
    """what the references of a direct case rest on, asserted on the scene: a rod or a sweep meets no partly shadowed receiver (the
    lit triangles are coplanar, or the walls of a convex room, so none shades another, and the one that is neither has solid angle 0
    from everywhere on the lamp);
    the lamp stays on one side of every receiver; with the plate, three or more floor triangles are partly shadowed, one triangle
    lies wholly in the shadow and one is seen edge-on"""
    kind, frm, to, length = DIRECT_CASES[name]
    plate = kind == "plate"
    tris = verts(direct_rows(name))
    pts, _ = rr.lamp_points(frm, to, length, 8)
    T = tris.shape[0]
    assert T <= 32
    if kind == "cube":
        assert rr.on_convex_boundary(tris), "the cube's walls: none shades another"
        for t in tris:
            s = (pts - t[0]) @ rr.tri_normal(t)[0]
            assert np.all(s > 0.1) or np.all(s < -0.1), "the lamp stays inside"
        return
    assert np.all(rr.polygon_solid_angle(pts, tris[T - 1]) == 0.0), "the last triangle is edge-on from the whole lamp"
    for t in tris[:T - 1]:
        n, _ = rr.tri_normal(t)
        s = (pts - t[0]) @ n
        assert np.all(s > 0.1) or np.all(s < -0.1), "the lamp stays on one side of the receiver"
    if not plate:
        assert all(rr.coplanar(t, tris[0]) for t in tris[:T - 1]), "coplanar receivers: none shades another"
        return
    occ = direct_occluders(name)[0]
    lamp = np.array(frm)
    partly = 0
    for t in tris[:8]:
        reg = rr.visible_regions(lamp, t, (occ,))
        hidden = sum(rr.polygon_area(p) for s, p in reg if s < 0)
        partly += 0.02 < hidden / rr.tri_normal(t)[1] < 0.98
    assert partly >= 3, "several floor triangles are partly shadowed"
    assert rr.inside_cone(tris[10], lamp, occ, 0.01) and rr.visible_regions(lamp, tris[10], (occ,)) == []
    assert all(rr.visible_regions(lamp, t, (occ,))[0][0] > 0 and len(rr.visible_regions(lamp, t, (occ,))) == 1 for t in tris[8:10])


@functools.lru_cache(maxsize=None)
def direct_reference(name):
    """per triangle of a direct case, in photons of a launch of N: share (the share of the lamp's photons), mu = N share, sigma
    (of one sample), eps (quadrature), var and mu4 (of one sample), mom_err, and the wrong-physics values of mu"""
    _, frm, to, length = DIRECT_CASES[name]
    occ = direct_occluders(name)
    tris = verts(direct_rows(name))
    half = np.array([0.0, 0.5 * length, 0.0])
    order = MOMENTS_ORDER.get(name, 12)
    moves = tuple(frm) != tuple(to)
    out = dict(share=[], eps=[], var=[], mu4=[], mom_err=[], mom_mean=[], no_cosine=[], midpoint=[], still=[])
    for t in tris:
        p, e = rr.direct_mean(t, frm, to, length, occ)
        mo = rr.direct_moments(t, frm, to, length, occ, order)
        out["share"].append(p)
        out["eps"].append(N * e)
        out["var"].append(N * N * mo["var"])
        out["mu4"].append(N ** 4 * mo["mu4"])
        out["mom_err"].append(mo["err"])
        out["mom_mean"].append(N * mo["mean"])
        out["no_cosine"].append(N * rr.direct_moments(t, frm, to, length, occ, order, cosine=False)["mean"])
        out["midpoint"].append(N * rr.direct_mean(t, np.array(frm) + half, np.array(to) + half, 0.0, occ)[0])
        out["still"].append(N * rr.direct_mean(t, frm, frm, length, occ)[0] if moves else 0.0)
    ref = {k: np.array(v) for k, v in out.items()}
    ref["mu"] = N * ref["share"]
    ref["sigma"] = np.sqrt(ref["var"])
    ref["variants"] = {"no cosine": ref["no_cosine"], "2 pi for 4 pi": 2.0 * ref["mu"]}
    if length != 0:
        ref["variants"]["rod at its midpoint"] = ref["midpoint"]
    if moves:
        ref["variants"]["the lamp does not move"] = ref["still"]
    return ref


# ---------------------------------------------------------------- the closed cube (the photon path's total, the mirror)
def cube_rows():
    import gather_indirect_restate as gi
    return gi.cube_tris()


PANEL_RHO = 0.75


def wall_panel():
    import gather_mirror_restate as gm
    return gm.wall_panel(PANEL_RHO)


WALL = (10, 11)                             # the wall x = 4
MIRROR_CASES = {"whole wall": (10, 11), "half the wall": (10,)}


def wall_members(name):
    pot = np.zeros(12, dtype=np.uint8)
    pot[list(MIRROR_CASES[name])] = 1
    return pot


@functools.lru_cache(maxsize=None)
def cube_shares():
    """the share of a point lamp's photons at CUBE_LAMP on every triangle of the closed cube (they sum to 1)"""
    return np.array([rr.direct_mean(t, CUBE_LAMP, CUBE_LAMP, 0.0)[0] for t in verts(cube_rows())])


@functools.lru_cache(maxsize=None)
def mirror_reference(name):
    tris = verts(cube_rows())
    assert rr.on_convex_boundary(tris), "nothing in the cube stands in a leg's way"
    q, m, rho = wall_panel()
    windows = [tris[k] for k in MIRROR_CASES[name]]
    out = dict(mu=[], var=[], mom_err=[], mom_mean=[], no_cosine=[], mirror_point=[])
    for t in tris:
        mo = rr.mirror_moments(t, CUBE_LAMP, q, m, rho, windows)
        out["mu"].append(N * rr.mirror_mean(t, CUBE_LAMP, q, m, rho, windows))
        out["var"].append(N * N * mo["var"])
        out["mom_err"].append(mo["err"])
        out["mom_mean"].append(N * mo["mean"])
        out["no_cosine"].append(N * rr.mirror_moments(t, CUBE_LAMP, q, m, rho, windows, cosine=False)["mean"])
        out["mirror_point"].append(N * rr.mirror_moments(t, CUBE_LAMP, q, m, rho, windows, at_mirror_point=True)["mean"])
    ref = {k: np.array(v) for k, v in out.items()}
    ref["sigma"] = np.sqrt(ref["var"])
    ref["eps"] = np.zeros(12)
    ref["variants"] = {"no cosine": ref["no_cosine"], "2 pi for 4 pi": 2.0 * ref["mu"],
                       "the distance to the mirror point": ref["mirror_point"], "the panel's rho left out": ref["mu"] / rho}
    return ref


# ---------------------------------------------------------------- parallel squares and a corner
def squares_rows():
    """A: y = 0, B: y = 1 facing it, C: x = 0 along an edge of both; unit squares, each of two triangles wound both ways"""
    A = quad((0, 0, 0), (1, 0, 0), (1, 0, 1), (0, 0, 1))
    B = quad((0, 1, 0), (1, 1, 0), (1, 1, 1), (0, 1, 1))
    Cq = quad((0, 0, 0), (0, 1, 0), (0, 1, 1), (0, 0, 1))
    return rows_of(A + B + Cq)


SQUARES_CENTRE = (0.5, 0.5, 0.5)
BOUNCE_RHO = 0.625
# photons on each triangle, hand-written: the two facing squares bright, the corner dark.  Facing squares get less from a uniform
# hemisphere than from a cosine-weighted one and squares at a right angle more, so with the light on the facing pair the
# "uniform hemisphere" variant errs one way on every path and stands 4.8 tolerances off (a mix of both cancels down to 2)
SOURCE = np.array([400.0, 350.0, 450.0, 300.0, 40.0, 60.0])
OUTER = np.array([70.0, 900.0, 20.0, 400.0, 650.0, 30.0])            # ... and on the faces that look away from the others
RHO_INNER = np.array([0.875, 0.75, 1.0, 0.625, 0.25, 0.5], dtype=f32)
RHO_OUTER = np.array([0.375, 0.625, 0.0625, 1.0, 0.3125, 0.5], dtype=f32)


def inner_faces(rows, centre=SQUARES_CENTRE):
    """int[T]: the face of each triangle that looks at the centre (0: cross(e1, e2) points to it)"""
    tris = verts(rows)
    return np.array([0 if rr.tri_normal(t)[0] @ (np.array(centre) - t[0]) > 0 else 1 for t in tris])


def face_planes(inner, outer, rows=None):
    """f64[2][T] with `inner` on the faces that look at the others and `outer` on those that look away"""
    rows = squares_rows() if rows is None else rows
    face = inner_faces(rows)
    T = face.size
    out = np.zeros((2, T), dtype=np.asarray(inner).dtype)
    out[face, np.arange(T)] = inner
    out[1 - face, np.arange(T)] = outer
    return out


@functools.lru_cache(maxsize=None)
def squares_tables(uniform=False):
    tris = verts(squares_rows())
    assert rr.on_convex_boundary(tris), "no triangle of the squares stands between two others"
    assert set(inner_faces(squares_rows())) == {0, 1}, "both windings occur"
    return rr.form_factor_tables(tris, 64, uniform)


BOUNCE_CALLS = ("traced", "linked", "sided", "mapped")


def bounce_radiosity(call):
    """f64[2][T]: what each face sends back per unit area under the call's inputs.  The two-sided calls (traced, linked) take one
    source plane and one rho; the sided call the face planes and one rho; the mapped call the face planes and a rho per face"""
    A = areas(squares_rows())
    if call in ("traced", "linked"):
        return np.stack([BOUNCE_RHO * SOURCE / A] * 2)
    faces = face_planes(SOURCE, OUTER)
    if call == "sided":
        return BOUNCE_RHO * faces / A
    return face_planes(RHO_INNER, RHO_OUTER).astype(f64) * faces / A


@functools.lru_cache(maxsize=None)
def bounce_reference(call):
    tris = verts(squares_rows())
    r = bounce_radiosity(call)
    mu, sigma, eps = rr.bounce(tris, r, squares_tables())
    wrong, _, _ = rr.bounce(tris, r, squares_tables(True))
    return dict(mu=mu, sigma=sigma, eps=eps, variants={"uniform hemisphere": wrong})


# ---------------------------------------------------------------- K bounces over links: the squares and the uneven box
BOX = (1.0, 2.0, 3.0)
BOX_CENTRE = (0.5, 1.0, 1.5)
FAN = 0.25                                  # the fan's point (FAN, 0, 0) on the edge y = 0 of the wall z = 0
SERIES_K = 4
SERIES_SCENES = ("squares", "uneven box")
SERIES_CALLS = ("linked", "sided", "mapped")


def box_rows():
    """The cuboid [0, 1] x [0, 2] x [0, 3]: the 1 x 2 wall z = 0 as a fan of three triangles from (FAN, 0, 0) (0..2), the other
    five walls of two triangles each, wound both ways (3..12), and a triangle without area along the edge x = y = 0 (13).  The
    areas run from 0.25 to 3"""
    X, Y, Z = BOX
    p = (FAN, 0, 0)
    fan = [(p, (X, 0, 0), (X, Y, 0)), (p, (0, Y, 0), (X, Y, 0)), (p, (0, Y, 0), (0, 0, 0))]
    walls = (quad((0, 0, Z), (X, 0, Z), (X, Y, Z), (0, Y, Z)) + quad((0, 0, 0), (0, Y, 0), (0, Y, Z), (0, 0, Z))
             + quad((X, 0, 0), (X, Y, 0), (X, Y, Z), (X, 0, Z)) + quad((0, 0, 0), (X, 0, 0), (X, 0, Z), (0, 0, Z))
             + quad((0, Y, 0), (X, Y, 0), (X, Y, Z), (0, Y, Z)))
    return rows_of(fan + walls + [((0, 0, 0), (0, 0, 1.5), (0, 0, Z))])


BOX_FLAT = 13
# photons on the inward and the outward face of every triangle, and a reflectance for each: hand-written, unequal, the triangle
# without area included (what it holds must go nowhere).  The light sits on the small wall z = 0 and the floor y = 0, so that
# later bounces have to carry it to the large walls
BOX_SOURCE = np.array([900.0, 700.0, 500.0, 60.0, 40.0, 150.0, 90.0, 30.0, 120.0, 800.0, 600.0, 20.0, 50.0, 333.0])
BOX_OUTER = np.array([80.0, 950.0, 30.0, 410.0, 640.0, 25.0, 700.0, 55.0, 310.0, 15.0, 480.0, 860.0, 75.0, 222.0])
BOX_RHO_INNER = np.array([0.875, 0.25, 1.0, 0.625, 0.75, 0.5, 0.9375, 0.375, 0.8125, 0.3125, 1.0, 0.6875, 0.4375, 0.5], dtype=f32)
BOX_RHO_OUTER = np.array([0.375, 1.0, 0.0625, 0.5, 0.3125, 0.75, 0.125, 0.875, 0.25, 0.9375, 0.4375, 0.1875, 0.625, 0.75], dtype=f32)


def series_rows(scene):
    return squares_rows() if scene == "squares" else box_rows()


def series_inputs(scene):
    """(source, outer, rho_inner, rho_outer, centre) of a scene of the bounce series"""
    if scene == "squares":
        return SOURCE, OUTER, RHO_INNER, RHO_OUTER, SQUARES_CENTRE
    return BOX_SOURCE, BOX_OUTER, BOX_RHO_INNER, BOX_RHO_OUTER, BOX_CENTRE


def series_planes(scene, inner=None):
    """(faces f64[2][T], rho f32[2][T]) of the sided and the mapped call; `inner` replaces the inward source"""
    src, outer, ri, ro, centre = series_inputs(scene)
    rows = series_rows(scene)
    face = inner_faces(rows, centre)
    T = face.size

    def planes(a, b):
        out = np.zeros((2, T), dtype=np.asarray(a).dtype)
        out[face, np.arange(T)] = a
        out[1 - face, np.arange(T)] = b
        return out
    return planes(src if inner is None else inner, outer), planes(ri, ro)


@functools.lru_cache(maxsize=None)
def series_tables(scene, uniform=False):
    """form_factor_tables of the triangles with an area, laid into T x T: the one without is left out, nothing lands on it"""
    if scene == "squares":
        return squares_tables(uniform)
    tris = verts(box_rows())
    T = tris.shape[0]
    keep = np.nonzero(areas(box_rows()) > 0)[0]
    f, e, a = rr.form_factor_tables(tris[keep], 64, uniform)
    F, E, arrive = np.zeros((2, T, T)), np.zeros((2, T, T)), np.zeros((T, T), dtype=np.int64)
    F[:, keep[:, None], keep[None, :]] = f
    E[:, keep[:, None], keep[None, :]] = e
    arrive[keep[:, None], keep[None, :]] = a
    return F, E, arrive


def check_series_scene(scene):
    """what the model of the bounce series rests on, asserted on the scene"""
    rows = series_rows(scene)
    tris = verts(rows)
    A = areas(rows)
    F, E, arrive = series_tables(scene)
    inner = inner_faces(rows, series_inputs(scene)[4])
    assert rr.on_convex_boundary(tris), "no triangle shades another"
    assert set(inner[A > 0]) == {0, 1}, "both face 0 and face 1 look inwards somewhere"
    if scene == "squares":
        assert np.all(A > 0) and np.all(F.sum(axis=(0, 2)) < 0.9), "an open scene: many links miss"
        return
    T = A.size
    assert T <= 16 and A.max() / A[A > 0].min() >= 8.0, "unequal areas"
    assert (A == 0).sum() == 1 and A[BOX_FLAT] == 0, "exactly one triangle has nn == 0"
    assert np.all(F[:, BOX_FLAT] == 0) and np.all(F[:, :, BOX_FLAT] == 0)
    for t in np.nonzero(A > 0)[0]:
        assert abs(F[inner[t], t].sum() - 1.0) <= E[inner[t], t].sum(), "a closed box: an inward row sums to 1"
        assert F[1 - inner[t], t].sum() == 0.0, "an outward face sees nothing"
        assert np.all(arrive[t][F[inner[t], t] > 0] == inner[F[inner[t], t] > 0]), "light arrives on inward faces"
    src, outer, ri, ro, _ = series_inputs(scene)
    assert min(ri.min(), ro.min()) <= 0.25 and max(ri.max(), ro.max()) >= 1.0, "the mapped planes span [0.25, 1]"
    assert len(set(src)) == T and len(set(outer)) == T, "unequal sources"


def series_model(call, scene, tables=None, away=False):
    """rr.link_model of a call on a scene: one source on both faces and one rho for the plain call, the face planes and one rho for
    the sided call, the face planes and a rho per face for the mapped call.  away: light on the outward faces only"""
    rows = series_rows(scene)
    src = series_inputs(scene)[0]
    faces, rho = series_planes(scene, np.zeros(src.size) if away else None)
    if call == "linked":
        faces, rho = np.stack([src, src]), BOUNCE_RHO
    elif call == "sided":
        rho = BOUNCE_RHO
    else:
        rho = rho.astype(f64)
    return rr.link_model(series_tables(scene) if tables is None else tables, areas(rows), rho, faces)


def series_parts(g):
    """{"total": sum of g_1..g_K, "g1": g_1, ..} of g[K][R], folded to triangles"""
    g = rr.fold_faces(g)
    out = {"total": g.sum(axis=0)}
    out.update({"g%d" % (b + 1): g[b] for b in range(g.shape[0])})
    return out


@functools.lru_cache(maxsize=None)
def series_reference(call, scene, S2=S, away=False):
    """{part: dict(mu, series, sigma, eps, variants)} for part = "total" (K = 4) and "g1".."g4": mu the exact mean over link sets,
    series the mean-field value A Mbar^b e0, sigma that of one call, eps the form factors' quadrature error carried through
    (every entry of Mbar is >= 0, so the series is monotone in F: half the difference between F + E and F - E)"""
    Kb, Sp = SERIES_K, S2 // 2
    F, E, arrive = series_tables(scene)
    model = series_model(call, scene, away=away)
    P, rho, e0, A = model
    area = areas(series_rows(scene))
    exact = series_parts(rr.series_exact(P, rho, e0, A, Kb, Sp))
    mean_field = series_parts(rr.series(P, rho, e0, A, Kb))
    hi = series_parts(rr.series(*series_model(call, scene, (F + E, E, arrive), away), Kb))
    lo = series_parts(rr.series(*series_model(call, scene, (np.maximum(F - E, 0.0), E, arrive), away), Kb))
    wrong = {"uniform hemisphere": series_parts(rr.series(*series_model(call, scene, series_tables(scene, True), away), Kb))}
    names = ["no area", "rho once"] + (["receiver's rho"] if call == "mapped" else [])
    wrong.update({w: series_parts(rr.series_wrong(P, rho, e0, A, Kb, w)) for w in names})
    out = {}
    for part in exact:
        bounces = tuple(range(1, Kb + 1)) if part == "total" else (int(part[1:]),)
        variants = {w: v[part] for w, v in wrong.items() if not (w != "uniform hemisphere" and part == "g1")}
        if part == "total":
            variants["only the last bounce"] = mean_field["g%d" % Kb]
            variants["K times the first bounce"] = Kb * mean_field["g1"]
        out[part] = dict(mu=exact[part], series=mean_field[part], sigma=rr.series_sigma(P, rho, e0, area, Sp, bounces),
                         eps=0.5 * (hi[part] - lo[part]), variants=variants)
    return out


SERIES_VARIANTS = ("uniform hemisphere", "no area", "rho once", "receiver's rho", "only the last bounce", "K times the first bounce")


def series_bias(scene, S2):
    """the largest |exact mean / series - 1| over the lit triangles of the plain call's total of four bounces"""
    ref = series_reference("linked", scene, S2)["total"]
    lit = ref["series"] > 0
    return float(np.max(np.abs(ref["mu"][lit] / ref["series"][lit] - 1.0)))


# ---------------------------------------------------------------- the refine, conditional on its first pass
REFINE_CASE = "point lamp, plate"
REFINE_S0 = 16
REFINE_FIRST_SEED = 11
REFINE_SETTINGS = {
    # name: (rel_error, max_extra, refine seeds)
    "every triangle at the cap": (1e-5, 4096, tuple(range(301, 309))),
    "counts of their own": (0.1, 64, tuple(range(401, 465))),
}


def refine_reference(X0, V0, n, R):
    """(on, expected, variance): for a fixed first pass (X0, V0 of S0 samples) the merge is linear in the n extra samples, so over R
    refine seeds  E[expected'] = (a X0 + b mu) / (a + b)  and, with independent samples, E[variance'] = (a^2 V0 + b Var(x)) /
    (a + b)^2, a = S0, b = n_t; mu, sigma, Var(x) and mu4 are the direct gather's reference.  `on` are the triangles with n_t > 0;
    each is judged with its own b.  The variants: the two weights swapped, and the plain average of the two passes"""
    ref = direct_reference(REFINE_CASE)
    on = np.nonzero(np.asarray(n) > 0)[0]
    a, b = float(REFINE_S0), np.asarray(n, dtype=f64)[on]
    X0, V0 = np.asarray(X0, dtype=f64)[on], np.asarray(V0, dtype=f64)[on]
    mu, sigma, eps, var = ref["mu"][on], ref["sigma"][on], ref["eps"][on], ref["var"][on]
    w = b / (a + b)
    expected = dict(mu=(a * X0 + b * mu) / (a + b), tol=w * (6.0 * sigma / np.sqrt(R * b) + eps + 1e-5 * mu),
                    variants={"weights swapped": (b * X0 + a * mu) / (a + b), "plain average": 0.5 * (X0 + mu)})
    variance = dict(mu=(a * a * V0 + b * var) / (a + b) ** 2,
                    tol=w * w * rr.variance_tolerance(var, ref["mu4"][on], b, R, ref["mom_err"][on]))
    return on, expected, variance


def accept_refine(case, setting, X0, V0, e, v, n, independent):
    """the refine's rule over the R seeds' planes e, v [R][T] and counts n [R][T], and the conditions of the setting"""
    rel_error, max_extra, seeds = REFINE_SETTINGS[setting]
    R = len(seeds)
    e, v, n = np.asarray(e), np.asarray(v), np.asarray(n)
    assert e.shape[0] == R and np.all(n == n[0]), "the counts follow from the first pass alone"
    n = n[0]
    can = (X0 > 0) & (V0 > 0)
    assert np.all(n[~can] == 0) and can.sum() >= 8
    if max_extra == 4096:
        want = REFINE_S0 * (V0[can] / (rel_error * X0[can]) ** 2 - 1.0)
        assert np.all(want >= max_extra) and np.all(n[can] == max_extra), "every triangle that can be refined is at the cap"
    else:
        assert (n >= 16).sum() >= 3 and len(set(n[n > 0].tolist())) >= 2, "several counts, some of them large"
    off = n == 0
    assert np.all(e[:, off].view(np.int64) == X0[off].view(np.int64)) and np.all(v[:, off].view(np.int64) == V0[off].view(np.int64)), \
        "a triangle with n_t = 0 keeps every bit of both planes"
    on, expected, variance = refine_reference(X0, V0, n, R)
    accept("refine, %s, %s" % (setting, case), e.mean(axis=0)[on], expected, R, expected["tol"])
    if independent:
        accept("refine's variance, %s, %s" % (setting, case), v.mean(axis=0)[on], variance, R, variance["tol"])


# ---------------------------------------------------------------- acceptance, power and the margins file
MARGINS = {}


def ratio(err, tol):
    err, tol = np.asarray(err, dtype=f64), np.asarray(tol, dtype=f64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(tol > 0, err / tol, np.where(err == 0, 0.0, np.inf))


def power(ref, tol):
    """{variant: distance}: how far each wrong-physics value lies from the true one, in tolerances.  A case compares every triangle,
    so a wrong formula fails it as soon as one triangle is off: the distance of a variant is the largest over the triangles"""
    lit = tol > 0         # (a triangle whose reference is exactly 0 tells any other value apart: it is left out, the figure stays finite)
    return {name: float(np.max(np.abs(v - ref["mu"])[lit] / tol[lit])) for name, v in ref["variants"].items()}


def accept(case, mean, ref, samples, tol=None):
    """The acceptance rule, per triangle; prints every figure before it asserts and notes the margins"""
    tol = rr.tolerance(ref["sigma"], ref["eps"], ref["mu"], samples) if tol is None else tol
    err = np.abs(np.asarray(mean) - ref["mu"])
    worst = float(np.max(ratio(err, tol)))
    pw = power(ref, tol) if "variants" in ref else {}
    MARGINS[case] = dict(err_over_tol=worst, min_variant_distance=min(pw.values()) if pw else None, variants=pw)
    print("%s: |err| / tol = %.3f; variants %s" % (case, worst, {k: round(v, 1) for k, v in pw.items()}))
    print("   mean %s\n   ref  %s\n   tol  %s" % (np.asarray(mean), ref["mu"], tol))
    assert np.all(err <= tol), "%s: |err| / tol per triangle %s" % (case, ratio(err, tol))
    return worst


def series_power(ref):
    """{variant: distance}: the largest distance over the total and the single bounces of a case of the bounce series"""
    out = {}
    for part in ref.values():
        for name, d in power(part, rr.tolerance(part["sigma"], part["eps"], part["mu"], K)).items():
            out[name] = max(out.get(name, 0.0), d)
    return out


def accept_series(case, totals, ref):
    """The rule of the bounce series.  totals[seed][k - 1][t]: the call with k bounces on that seed's links.  The total of
    SERIES_K bounces and every single bounce g_b = total(b) - total(b - 1), as means over the K seeds, against the exact mean with
    6 sigma_call / sqrt(K) + eps_quad + 1e-5 mu; sigma_call is that of ONE call, so `samples` is K.  Every figure is printed first"""
    totals = np.asarray(totals, dtype=f64)
    assert totals.shape[:2] == (K, SERIES_K)
    got = {"total": totals[:, -1], "g1": totals[:, 0]}
    got.update({"g%d" % b: totals[:, b - 1] - totals[:, b - 2] for b in range(2, SERIES_K + 1)})
    worst, failed = 0.0, []
    for part, r in ref.items():
        tol = rr.tolerance(r["sigma"], r["eps"], r["mu"], K)
        mean = got[part].mean(axis=0)
        q = ratio(np.abs(mean - r["mu"]), tol)
        worst = max(worst, float(q.max()))
        print("%s, %s: |err| / tol = %.3f\n   mean %s\n   ref  %s\n   tol  %s" % (case, part, q.max(), mean, r["mu"], tol))
        if not np.all(q <= 1.0):
            failed.append((part, q))
    pw = series_power(ref)
    MARGINS[case] = dict(err_over_tol=worst, min_variant_distance=min(pw.values()), variants=pw)
    assert not failed, "%s: |err| / tol per triangle %s" % (case, failed)
    dark = ref["total"]["mu"] == 0
    assert np.all(totals[:, :, dark] == 0.0) and not np.signbit(totals[:, :, dark]).any(), "a reference of 0 demands +0.0 in every call"
    return worst


def accept_total(case, mean, ref, samples, total):
    """the closed room: what the lamp sends out arrives.  The triangles' samples are independent, so the sum of the means has the
    root of the summed squares of their sigmas; the quadrature and f32 terms add"""
    sigma = np.sqrt(np.sum(ref["sigma"] ** 2))
    tol = float(rr.tolerance(sigma, np.sum(ref["eps"]), total, samples))
    err = abs(float(np.sum(mean)) - total)
    assert abs(np.sum(ref["mu"]) / total - 1.0) < 1e-9, "the reference itself adds up"
    MARGINS[case]["total_err_over_tol"] = err / tol
    print("%s: the sum %.3f against %d, |err| / tol = %.3f" % (case, np.sum(mean), total, err / tol))
    assert err <= tol, case


def dump_margins(which):
    """writes the margins noted so far under the key `which` into the JSON file that UVRT_RADIOMETRY_MARGINS names, if it names one"""
    path = os.environ.get("UVRT_RADIOMETRY_MARGINS")
    if not path:
        return
    data = {}
    if os.path.exists(path):
        with open(path) as f:
            data = json.load(f)
    data[which] = {k: MARGINS[k] for k in sorted(MARGINS)}
    with open(path, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")
