"""The scenes, cases and references of the radiometry tests, shared by tests/test_radiometry_cpu.py (the
restatements against the closed forms, and the power of every case) and tests/test_gpu_radiometry.py (the kernels against the
closed forms).  Geometry and expected values only: no kernel, no restatement and no RNG is used to form a reference.  The closed
cube and its wall panel are gather_indirect_restate.cube_tris and gather_mirror_restate.wall_panel, taken as geometry.

Every coordinate is rounded to f32 before the reference sees it, so the reference and the kernels speak of the same triangles
and the same lamp.  All scenes have at most 12 triangles."""
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
    out = dict(share=[], eps=[], var=[], mu4=[], mom_err=[], mom_mean=[], no_cosine=[], midpoint=[])
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
    ref = {k: np.array(v) for k, v in out.items()}
    ref["mu"] = N * ref["share"]
    ref["sigma"] = np.sqrt(ref["var"])
    ref["variants"] = {"no cosine": ref["no_cosine"], "2 pi for 4 pi": 2.0 * ref["mu"]}
    if length != 0:
        ref["variants"]["rod at its midpoint"] = ref["midpoint"]
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
