"""CPU: the closed-form radiometry reference (tests/radiometry_reference.py) against itself, every restatement against it under
the acceptance rule of DESIGN.md 24, and the power of every case.  The restatements give the kernels' bits, so what passes here
passes in tests/test_gpu_radiometry.py; what this file adds over that one is that it needs no GPU and that it proves, from the
reference alone, that each case would notice each wrong formula it is meant to notice.

With UVRT_RADIOMETRY_MARGINS=FILE the margins of every case are written into FILE under "cpu"."""
import numpy as np
import pytest

import gather_edge_scene as ge
import gather_faces_restate as gf
import gather_indirect_restate as gi
import gather_links_restate as gl
import gather_mirror_restate as gm
import gather_refine_restate as grf
import gather_reflect_map_restate as grm
import gather_stratified_restate as gs
import gather_variance_restate as gv
import radiometry_reference as rr
import radiometry_scenes as rs

N, K, S, SEEDS = rs.N, rs.K, rs.S, rs.SEEDS
f32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def _margins():
    yield
    rs.dump_margins("cpu")


def hand_scene(orc, rows):
    return ge.HandScene(orc, np.array(rows, dtype=f32))


# ---------------------------------------------------------------- the reference against itself
def parallel_rectangles(X, Y):
    """the textbook form factor between two directly opposed X x Y rectangles at distance 1"""
    a, b = np.sqrt(1 + X * X), np.sqrt(1 + Y * Y)
    return 2.0 / (np.pi * X * Y) * (np.log(a * b / np.sqrt(1 + X * X + Y * Y)) + X * b * np.arctan(X / b) + Y * a * np.arctan(Y / a)
                                    - X * np.arctan(X) - Y * np.arctan(Y))


def perpendicular_squares():
    """the textbook form factor between two unit squares at a right angle along a shared edge (H = W = 1)"""
    return (np.pi / 2 - np.sqrt(2.0) * np.arctan(1 / np.sqrt(2.0)) + 0.25 * np.log((4.0 / 3.0) * 0.75 * 0.75)) / np.pi


def test_solid_angles():
    o = np.zeros(3)
    e = np.eye(3)
    assert abs(rr.solid_angle(o, e[0], e[1], e[2]) - np.pi / 2) < 1e-15, "an octant"
    assert abs(rr.polygon_solid_angle(o, np.array([(1, 1, 1), (-1, 1, 1), (-1, -1, 1), (1, -1, 1)], dtype=float)) - 4 * np.pi / 6) < 1e-14
    assert rr.solid_angle(np.array([5.0, 7.0, 0.25]), np.array([0, 0, 0.25]), np.array([1, 0, 0.25]), np.array([0, 1, 0.25])) == 0.0
    cube = rs.verts(rs.cube_rows())
    for lamp in (rs.CUBE_LAMP, (3.9, 3.9, 0.1), (2.0, 2.0, 2.0)):
        total = sum(rr.polygon_solid_angle(np.array(lamp), t) for t in cube)
        assert abs(total - 4 * np.pi) < 1e-12, lamp
    assert abs(rs.cube_shares().sum() - 1.0) < 1e-14
    many = rr.polygon_solid_angle(np.array([(0.0, 0, 0), (0.1, 0.2, -0.3)]), np.array([(1, 1, 1), (-1, 1, 1), (-1, -1, 1)], dtype=float))
    assert many.shape == (2,) and abs(many[0] - 4 * np.pi / 12) < 1e-14


def test_the_clipper():
    sq = np.array([(0, 0, 0), (1, 0, 0), (1, 0, 1), (0, 0, 1)], dtype=float)
    tri = np.array([(0, 0, 0), (2, 0, 0), (0, 0, 2)], dtype=float)
    assert abs(rr.polygon_area(rr.clip_convex(sq + (0.5, 0, 0.5), sq)) - 0.25) < 1e-15
    assert abs(rr.polygon_area(rr.clip_convex(tri, sq)) - 1.0) < 1e-15, "the square lies inside the triangle"
    assert abs(rr.polygon_area(rr.clip_convex(tri, sq + (0.5, 0, 0.5))) - 0.5) < 1e-15, "the hypotenuse halves the square"
    assert rr.clip_convex(tri, sq + (3, 0, 3)).shape[0] == 0
    assert abs(rr.polygon_area(rr.clip_halfspace(tri, np.array([1.0, 0, 0]), 1.0)) - 0.5) < 1e-15
    # the projecting planes against the projection itself, where the projection is bounded: the plate's shadow on the floor
    lamp, plate = np.array(rs.LAMP), np.array(rs.PLATE)
    shadow = rr.project_from(lamp, plate, np.zeros(3), rr.EY)
    assert abs(rr.polygon_area(shadow) - 0.16 * (1.6 / 0.6) ** 2) < 1e-6, "the shadow of a 0.4 x 0.4 plate, magnified by 1.6 / 0.6"
    floor = rs.verts(rs.floor_rows(True))[:8]
    total = 0.0
    for t in floor:
        by_planes, by_projection = rr.clip_to_cone(t, lamp, plate), rr.clip_convex(t, shadow)
        assert abs(rr.polygon_area(by_planes) - rr.polygon_area(by_projection)) < 1e-12
        total += rr.polygon_area(by_planes)
    z_lo, z_hi = shadow[:, 2].min(), shadow[:, 2].max()
    assert 0 < z_lo < 2.0 < z_hi and 0 < shadow[:, 0].min() and shadow[:, 0].max() < 2.0, "the floor's edge z = 2 cuts the shadow"
    assert abs(total - rr.polygon_area(shadow) * (2.0 - z_lo) / (z_hi - z_lo)) < 1e-12
    # a receiver in front of the occluder is not in its shadow
    above = np.array(rs.SHADOWED) + (0.0, 0.8, 0.0)
    assert rr.polygon_area(rr.clip_to_cone(above, lamp, plate)) == 0.0 and rr.polygon_area(rr.clip_to_cone(np.array(rs.SHADOWED), lamp, plate)) > 0
    assert rr.mirror_image((1.0, 0.5, 2.0), (4.0, 0, 0), (-2.0, 0, 0)).tolist() == [7.0, 0.5, 2.0]


def test_the_quadrature_rules():
    a, b, w = rr.triangle_nodes(6)
    assert abs(w.sum() - 1.0) < 1e-15 and abs(w @ (a * a * b * b) - 2.0 / 180.0) < 1e-16, "the mean of a^2 b^2 over the unit triangle"
    x, wx = rr.gauss01(5)
    assert abs(wx @ x ** 8 - 1.0 / 9.0) < 1e-15
    pts, wl = rr.lamp_points((0, 0, 0), (1, 0, 0), 2.0, 3)
    assert pts.shape == (9, 3) and abs(wl.sum() - 1) < 1e-15 and abs(wl @ pts[:, 0] - 0.5) < 1e-15 and abs(wl @ pts[:, 1] - 1.0) < 1e-15


def test_form_factors_against_the_tabulated_values():
    F, E, arrive = rs.squares_tables()
    # A = 0, 1; B = 2, 3; C = 4, 5; every triangle has area 1/2
    AB = 0.5 * sum(F[f][t][h] for f in (0, 1) for t in (0, 1) for h in (2, 3))
    AC = 0.5 * sum(F[f][t][h] for f in (0, 1) for t in (0, 1) for h in (4, 5))
    print("F(parallel) = %.9f, F(corner) = %.9f, largest quadrature error %.2e" % (AB, AC, E.max()))
    assert abs(AB - 0.199825) < 5e-7 + 4 * E.max() and abs(AC - 0.200044) < 5e-7 + 4 * E.max(), "the tabulated six digits"
    assert abs(AB / parallel_rectangles(1.0, 1.0) - 1) < 1e-6 and abs(AC / perpendicular_squares() - 1) < 1e-6
    # reciprocity (equal areas) and the faces that see nothing
    both = F[0] + F[1]
    assert np.abs(both - both.T).max() < 1e-6
    inner = rs.inner_faces(rs.squares_rows())
    assert all(F[1 - inner[t], t].max() == 0.0 for t in range(6)), "an outer face sees nothing"
    assert np.all(both[0, :2] == 0) and np.all(both[2, 2:4] == 0), "coplanar triangles do not see each other"
    see = both > 0
    assert see.sum() == 24 and np.all(arrive[see] == np.tile(inner, (6, 1))[see]), "every triangle sees the others' inner faces"


def test_point_form_factors():
    # an element under one corner of a parallel X x Y rectangle at distance 1
    X, Y = 0.7, 1.3
    rect = np.array([(0, 1, 0), (X, 1, 0), (X, 1, Y), (0, 1, Y)], dtype=float)
    a, b = np.sqrt(1 + X * X), np.sqrt(1 + Y * Y)
    want = (X / a * np.arctan(Y / a) + Y / b * np.arctan(X / b)) / (2 * np.pi)
    assert abs(rr.point_form_factor(np.zeros(3), rr.EY, rect) - want) < 1e-15
    # whatever way a point inside the closed cube faces, it sees form factor 1 in all: every wall is clipped at the horizon
    cube = rs.verts(rs.cube_rows())
    for n in ((0, 1, 0), (1, 2, -3), (-0.3, 0.1, 0.9)):
        n = np.array(n, dtype=float) / np.linalg.norm(n)
        assert abs(sum(rr.point_form_factor(np.array([1.0, 0.5, 2.5]), n, t) for t in cube) - 1.0) < 1e-13
    # the uniform-hemisphere variant sums to 1 as well, over one face of a triangle in the cube
    tri = np.array([(1.0, 1, 1), (2, 1.5, 1), (1, 2, 2.5)])
    for uniform in (False, True):
        total = sum(rr.form_factor(tri, 0, t, 8, uniform)[0] for t in cube)
        assert abs(total - 1.0) < 1e-9, uniform


def test_the_quadrature_errors_are_small():
    """below 1e-6 relative: the rod's and the sweep's Gauss-Legendre, the form factors' rule, and the tensor rule of the moments,
    whose mean has the exact solid angle to stand against"""
    for name in rs.DIRECT_CASES:
        rs.check_direct_scene(name)
        ref = rs.direct_reference(name)
        lit = ref["mu"] > 0
        assert np.all(ref["eps"][lit] / ref["mu"][lit] < 1e-6) and np.all(ref["mom_err"] < 1e-6), name
        assert np.all(np.abs(ref["mom_mean"] - ref["mu"])[lit] / ref["mu"][lit] < 1e-6), name
        assert np.all(ref["mu"][~lit] == 0) and np.all(ref["var"][~lit] == 0)
    plate = rs.direct_reference("point lamp, plate")
    assert plate["mu"][10] == 0.0 and plate["mu"][11] == 0.0 and np.all(plate["mu"][:10] > 0)
    for name in rs.MIRROR_CASES:
        ref = rs.mirror_reference(name)
        lit = ref["mu"] > 0
        assert np.all(ref["mom_err"] < 1e-6) and np.all(np.abs(ref["mom_mean"] - ref["mu"])[lit] / ref["mu"][lit] < 1e-6), name
        assert np.all(ref["mu"][list(rs.WALL)] == 0.0) and lit.sum() >= 5
    for call in rs.BOUNCE_CALLS:
        ref = rs.bounce_reference(call)
        assert np.all(ref["eps"] / ref["mu"] < 1e-6) and np.all(ref["mu"] > 0), call
    whole, half = rs.mirror_reference("whole wall"), rs.mirror_reference("half the wall")
    assert abs(whole["mu"].sum() / (rs.PANEL_RHO * N * rs.cube_shares()[list(rs.WALL)].sum()) - 1) < 1e-12, "what the wall receives, it sends back"
    assert np.all(half["mu"] <= whole["mu"] + 1e-9)


def test_every_case_has_the_power_to_tell_each_wrong_formula():
    """each wrong-physics value lies at least 3 tolerances from the true one, in every case it applies to"""
    samples = K * S
    refs = {"direct, " + n: rs.direct_reference(n) for n in rs.DIRECT_CASES}
    refs.update({"mirror, " + n: rs.mirror_reference(n) for n in rs.MIRROR_CASES})
    refs.update({"bounce, " + c: rs.bounce_reference(c) for c in rs.BOUNCE_CALLS})
    want = {"direct, point lamp, plate": 2, "direct, rod": 3, "direct, sweep": 4, "direct, rod in the closed cube": 3, "mirror, whole wall": 4,
            "mirror, half the wall": 4}
    for name, ref in refs.items():
        pw = rs.power(ref, rr.tolerance(ref["sigma"], ref["eps"], ref["mu"], samples))
        print(name, {k: round(v, 1) for k, v in pw.items()})
        assert len(pw) == want.get(name, 1) and min(pw.values()) >= 3.0, (name, pw)
    for name in ("point lamp, plate", "rod", "sweep"):
        ref = photon_reference(name)
        pw = rs.power(ref, ref["tol"])
        print("photons, " + name, {k: round(v, 1) for k, v in pw.items()})
        assert min(pw.values()) >= 3.0, (name, pw)


# ---------------------------------------------------------------- the direct gather's restatements
@pytest.mark.parametrize("fl", (0, 1))
@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("name", tuple(rs.DIRECT_CASES))
def test_the_restated_direct_gather(orc, name, mode, fl):
    _, frm, to, length = rs.DIRECT_CASES[name]
    scene = hand_scene(orc, rs.direct_rows(name))
    ref = rs.direct_reference(name)
    got = np.array([gs.gather(orc, scene, frm, to, length, S, seed, N, flavour=fl, mode=mode)[0] for seed in SEEDS])
    rs.accept("direct, %s, mode %d, flavour %d" % (name, mode, fl), got.mean(axis=0), ref, K * S)
    dark = ref["mu"] == 0
    assert dark.sum() == rs.direct_dark(name) and np.all(got[:, dark] == 0.0), "edge-on and wholly shadowed: exactly 0 in every call"
    if name == "rod in the closed cube":
        rs.accept_total("direct, %s, mode %d, flavour %d" % (name, mode, fl), got.mean(axis=0), ref, K * S, N)


@pytest.mark.parametrize("fl", (0, 1))
@pytest.mark.parametrize("name", tuple(rs.DIRECT_CASES))
def test_the_restated_variance_plane(orc, name, fl):
    _, frm, to, length = rs.DIRECT_CASES[name]
    scene = hand_scene(orc, rs.direct_rows(name))
    got = np.array([gv.gather(orc, scene, frm, to, length, S, seed, N, gv.INDEPENDENT, flavour=fl)[1] for seed in SEEDS])
    rs.accept("variance, %s, flavour %d" % (name, fl), got.mean(axis=0), *variance_reference(name))


def variance_reference(name):
    """(ref, samples, tol) for the mean over K calls of variance[t]: Var(x) / S, the tolerance from the fourth moment"""
    ref = rs.direct_reference(name)
    want = dict(mu=ref["var"] / S)
    return want, K * S, rr.variance_tolerance(ref["var"], ref["mu4"], S, K, ref["mom_err"])


# ---------------------------------------------------------------- the photon path's restatement: the oracle
def photon_reference(name):
    """counts of N photons: Binomial(N, share); the tolerance 6 sqrt(N p (1 - p)) plus the share's quadrature error"""
    ref = rs.direct_reference(name)
    p = ref["share"]
    return dict(mu=N * p, tol=rr.binomial_tolerance(N, p) + ref["eps"],
                variants={k: v for k, v in ref["variants"].items() if k != "no cosine"})


def oracle_counts(orc, scene, lamp, length):
    rays, _ = orc.generate(0, N, lamp, length, 0)
    counts = np.zeros(scene.T, dtype=np.int32)
    orc.extend(counts, scene.tris, rays, scene.nodes, scene.triIdx)
    return counts


@pytest.mark.parametrize("name", ("point lamp, plate", "rod"))
def test_the_oracles_photon_counts(orc, name):
    _, frm, _, length = rs.DIRECT_CASES[name]
    scene = hand_scene(orc, rs.direct_rows(name))
    ref = photon_reference(name)
    rs.accept("photons, " + name, oracle_counts(orc, scene, frm, length), ref, N, ref["tol"])


@pytest.mark.parametrize("length", (0.0, rs.ROD))
def test_the_oracles_photons_in_the_closed_cube(orc, length):
    scene = hand_scene(orc, rs.cube_rows())
    counts = oracle_counts(orc, scene, rs.CUBE_LAMP, length)
    assert counts.sum() == N, "no photon leaves a closed cube"
    if length == 0:
        p = rs.cube_shares()
        rs.accept("photons, cube", counts, dict(mu=N * p), N, rr.binomial_tolerance(N, p))


# ---------------------------------------------------------------- one bounce
def restated_bounce(orc, scene, call, seed, fl, faces=None):
    tris = scene.tris
    if call == "traced":
        return gi.indirect(orc, scene, rs.SOURCE, rs.BOUNCE_RHO, S, seed, flavour=fl)[0]
    if call == "linked":
        return gl.linked(tris, rs.SOURCE, gl.links(orc, scene, S, seed, flavour=fl), rs.BOUNCE_RHO, 1)
    faces = rs.face_planes(rs.SOURCE, rs.OUTER) if faces is None else faces
    links = gf.sided_links(orc, scene, S, seed, flavour=fl)
    if call == "sided":
        return gf.linked(tris, faces, links, rs.BOUNCE_RHO, 1)
    return grm.linked(tris, faces, links, rs.face_planes(rs.RHO_INNER, rs.RHO_OUTER), 1)


@pytest.mark.parametrize("fl", (0, 1))
@pytest.mark.parametrize("call", rs.BOUNCE_CALLS)
def test_the_restated_bounce(orc, call, fl):
    scene = hand_scene(orc, rs.squares_rows())
    got = np.array([restated_bounce(orc, scene, call, seed, fl) for seed in SEEDS])
    rs.accept("bounce, %s, flavour %d" % (call, fl), got.mean(axis=0), rs.bounce_reference(call), K * S)
    if call in ("sided", "mapped"):
        away = restated_bounce(orc, scene, call, SEEDS[0], fl, faces=rs.face_planes(np.zeros(6), rs.OUTER))
        assert np.all(away == 0.0), "light on faces turned away from every receiver reaches none"


# ---------------------------------------------------------------- the mirror
@pytest.mark.parametrize("fl", (0, 1))
@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("name", tuple(rs.MIRROR_CASES))
def test_the_restated_mirror_gather(orc, name, mode, fl):
    scene = hand_scene(orc, rs.cube_rows())
    ref = rs.mirror_reference(name)
    got = np.array([gm.gather(orc, scene, [rs.wall_panel()], rs.wall_members(name), rs.CUBE_LAMP, rs.CUBE_LAMP, 0.0, S, seed, N,
                              flavour=fl, mode=mode)[0] for seed in SEEDS])
    rs.accept("mirror, %s, mode %d, flavour %d" % (name, mode, fl), got.mean(axis=0), ref, K * S)
    assert np.all(got[:, list(rs.WALL)] == 0.0), "the wall itself"


# ---------------------------------------------------------------- K bounces over links: the model against itself
def random_model(rng):
    """6 rows (3 triangles x 2 faces), rows summing to 0.8, a zero diagonal; no geometry"""
    R = 6
    P = rng.random((R, R))
    np.fill_diagonal(P, 0.0)
    P /= P.sum(axis=1, keepdims=True) * 1.25
    return P, rng.uniform(0.3, 1.0, R), rng.uniform(10.0, 500.0, R), np.tile(rng.uniform(0.1, 1.5, R // 2), 2)


def drawn_series(rng, model, Sp, Kb, draws):
    """[draws][Kb][R]: A M^b e0 with every row of M one multinomial draw of S' samples"""
    P, rho, e0, A = model
    R = P.shape[0]
    pv = np.concatenate([P, 1.0 - P.sum(axis=1, keepdims=True)], axis=1)
    M = rng.multinomial(Sp, pv, size=(draws, R))[:, :, :R] / float(Sp) * rho[None, None, :]
    out, v = [], np.broadcast_to(e0, (draws, R))
    for _ in range(Kb):
        v = np.einsum("drc,dc->dr", M, v)
        out.append(A[None, :] * v)
    return np.stack(out, axis=1)


@pytest.mark.parametrize("Sp, draws", ((8, 20000), (2048, 4000)))
def test_the_link_model_against_drawn_multinomials(Sp, draws):
    """the exact mean and the first-order sigma_call of rr against the model drawn with numpy's generator: the drawn mean within 4
    standard errors of series_exact, the drawn sd within 0.9 .. 1.1 of series_sigma -- for the total of four bounces and for
    each bounce alone.  The mean-field series is NOT within the standard error at S' = 8: the bias is real"""
    rng = np.random.default_rng(2031)
    model = random_model(rng)
    P, rho, e0, A = model
    Kb = 4
    X = rr.fold_faces(drawn_series(rng, model, Sp, Kb, draws))
    exact = rr.fold_faces(rr.series_exact(P, rho, e0, A, Kb, Sp))
    mean_field = rr.fold_faces(rr.series(P, rho, e0, A, Kb))
    parts = [("total", X.sum(axis=1), exact.sum(axis=0), tuple(range(1, Kb + 1)))]
    parts += [("g%d" % b, X[:, b - 1], exact[b - 1], (b,)) for b in range(1, Kb + 1)]
    for name, x, want, bounces in parts:
        se = x.std(axis=0) / np.sqrt(draws)
        sd = x.std(axis=0) / rr.series_sigma(P, rho, e0, A[:3], Sp, bounces)
        print("S' = %d, %s: mean off by %s standard errors, sd / sigma_call %s" % (Sp, name, (x.mean(axis=0) - want) / se, sd))
        assert np.all(np.abs(x.mean(axis=0) - want) <= 4.0 * se), name
        assert np.all((0.9 <= sd) & (sd <= 1.1)), name
    assert np.allclose(exact[:2], mean_field[:2], rtol=1e-13, atol=0.0), "no path of one or two steps uses a row twice"
    bias = exact.sum(axis=0) / mean_field.sum(axis=0) - 1.0
    print("S' = %d: bias of the series over mu %s" % (Sp, bias))
    assert np.all(np.abs(bias) < (1e-2 if Sp == 8 else 1e-4)) and np.all(bias != 0.0)


def test_the_scenes_of_the_bounce_series():
    """the conditions of the model, asserted on both scenes; the references add up; what lies on outward faces never arrives"""
    for scene in rs.SERIES_SCENES:
        rs.check_series_scene(scene)
        for call in rs.SERIES_CALLS:
            ref = rs.series_reference(call, scene)
            A = rs.areas(rs.series_rows(scene))
            for part, r in ref.items():
                assert np.all(r["mu"][A > 0] > 0) and np.all(r["mu"][A == 0] == 0) and np.all(r["sigma"][A == 0] == 0), (scene, call, part)
                assert np.all(r["eps"][A > 0] / r["mu"][A > 0] < 2e-4), "the quadrature error is small beside 6 sigma"
                assert np.all(r["eps"] < 0.05 * rr.tolerance(r["sigma"], 0.0, 0.0, K) + (A == 0)), (scene, call, part)
            if call != "linked":
                away = rs.series_reference(call, scene, away=True)
                assert all(np.all(r["mu"] == 0) and np.all(r["sigma"] == 0) and np.all(r["eps"] == 0) for r in away.values())
    src, A = rs.BOX_SOURCE, rs.areas(rs.box_rows())
    for call in ("linked", "sided"):
        ref = rs.series_reference(call, "uneven box")
        for b in range(1, rs.SERIES_K + 1):
            r = ref["g%d" % b]
            want = rs.BOUNCE_RHO ** b * src[A > 0].sum()
            print("uneven box, %s, g%d: the sum %.6f against rho^b sum(source) = %.6f, eps %.2e" % (call, b, r["mu"].sum(), want, r["eps"].sum()))
            assert abs(r["mu"].sum() - want) <= r["eps"].sum(), "a closed box: every bounce keeps rho of what the last one held"


def test_the_bounce_series_can_tell_each_wrong_recursion():
    """every wrong formula that applies to a call lies at least 3 tolerances off on some triangle, in the total or in one of the
    single bounces, on each scene"""
    for scene in rs.SERIES_SCENES:
        for call in rs.SERIES_CALLS:
            pw = rs.series_power(rs.series_reference(call, scene))
            print(scene, call, {k: round(v, 1) for k, v in pw.items()})
            assert set(pw) == set(rs.SERIES_VARIANTS) - (set() if call == "mapped" else {"receiver's rho"})
            assert min(pw.values()) >= 3.0, (scene, call, pw)


def test_the_bias_of_the_series():
    """the exact mean over link sets against the mean-field series A Mbar^b e0, four bounces of the plain call: O(1 / S2), and at
    S2 = 4096 far inside the tolerance of the cases (DESIGN.md 24 has the table)"""
    for scene in rs.SERIES_SCENES:
        bias = [rs.series_bias(scene, s2) for s2 in (16, 64, 256, 4096)]
        print("%s: bias of four bounces at S2 = 16, 64, 256, 4096: %s" % (scene, ["%.2e" % b for b in bias]))
        rs.MARGINS["series bias, " + scene] = dict(zip(("S2=16", "S2=64", "S2=256", "S2=4096"), bias))
        # (at S' = 8 the terms in 1 / S'^2 of the paths of four steps still show: the first ratio may reach 5)
        assert 3.5 < bias[0] / bias[1] < 5.0 and 3.5 < bias[1] / bias[2] < 4.5 and 14 < bias[2] / bias[3] < 18, "it falls as 1 / S2"
        assert bias[0] < 1e-2 and bias[3] < 2e-5
        ref = rs.series_reference("linked", scene)["total"]
        assert np.all(np.abs(ref["mu"] - ref["series"]) <= 0.01 *rr.tolerance(ref["sigma"], ref["eps"], ref["mu"], K))


def restated_series(orc, scene, call, name, seed, fl, away=False):
    """(totals[4][T] of the call with 1..4 bounces on one set of links, the links' targets int[T][S]).  linked(.., k) adds
    g_1..g_k in order from g_1, so the prefix sums of one run of four bounces are its bits"""
    tris = scene.tris
    src = rs.series_inputs(name)[0]
    if call == "linked":
        links = gl.links(orc, scene, S, seed, flavour=fl)
        g = gl.bounces(tris, src, links, rs.BOUNCE_RHO, rs.SERIES_K)
        target = links
    else:
        faces, rho = rs.series_planes(name, np.zeros(src.size) if away else None)
        links = gf.sided_links(orc, scene, S, seed, flavour=fl)
        g = gf.bounces(tris, faces, links, rs.BOUNCE_RHO, rs.SERIES_K)[0] if call == "sided" else grm.bounces(tris, faces, links, rho, rs.SERIES_K)[0]
        g = [x[0] + x[1] for x in g]
        target = np.where(links >= 0, links >> 1, -1)
    totals = [g[0]]
    for b in range(1, rs.SERIES_K):
        totals.append(totals[-1] + g[b])
    if seed == SEEDS[0] and not away:
        k3 = (gl.linked(tris, src, links, rs.BOUNCE_RHO, 3) if call == "linked" else gf.linked(tris, faces, links, rs.BOUNCE_RHO, 3)
              if call == "sided" else grm.linked(tris, faces, links, rho, 3))
        assert np.array_equal(k3, totals[2]), "the prefix sums are the call's bits"
    return np.array(totals), target


@pytest.mark.parametrize("fl", (0, 1))
@pytest.mark.parametrize("name", rs.SERIES_SCENES)
@pytest.mark.parametrize("call", rs.SERIES_CALLS)
def test_the_restated_bounce_series(orc, call, name, fl):
    scene = hand_scene(orc, rs.series_rows(name))
    got = []
    for seed in SEEDS:
        totals, target = restated_series(orc, scene, call, name, seed, fl)
        got.append(totals)
        if name == "uneven box":
            assert not np.any(target == rs.BOX_FLAT) and np.all(target[rs.BOX_FLAT] == -1), "no link points at the triangle without area"
    rs.accept_series("series, %s, %s, flavour %d" % (call, name, fl), got, rs.series_reference(call, name))
    if call != "linked":
        away, _ = restated_series(orc, scene, call, name, SEEDS[0], fl, away=True)
        assert np.all(away == 0.0) and not np.signbit(away).any(), "light on faces turned away reaches no triangle, in any bounce"


# ---------------------------------------------------------------- the refine, conditional on its first pass
_REFINED = {}


def restated_refine(orc, setting, mode, fl):
    """(X0, V0, e[R][T], v[R][T], n[R][T]): the first pass once -- it is deterministic -- and one refine of it per seed"""
    key = (setting, mode, fl)
    if key not in _REFINED:
        _, frm, to, length = rs.DIRECT_CASES[rs.REFINE_CASE]
        rel_error, max_extra, seeds = rs.REFINE_SETTINGS[setting]
        scene = hand_scene(orc, rs.direct_rows(rs.REFINE_CASE))
        X0, V0, _ = gv.gather(orc, scene, frm, to, length, rs.REFINE_S0, rs.REFINE_FIRST_SEED, N, mode, fl)
        out = [grf.refine(orc, scene, frm, to, length, rs.REFINE_S0, mode, N, X0, V0, rel_error, max_extra, seed, flavour=fl)
               for seed in seeds]
        _REFINED[key] = (X0, V0) + tuple(np.array([o[k] for o in out]) for k in range(3))
    return _REFINED[key]


@pytest.mark.parametrize("fl", (0, 1))
@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("setting", tuple(rs.REFINE_SETTINGS))
def test_the_restated_refine(orc, setting, mode, fl):
    X0, V0, e, v, n = restated_refine(orc, setting, mode, fl)
    rs.accept_refine("mode %d, flavour %d" % (mode, fl), setting, X0, V0, e, v, n, mode == gv.INDEPENDENT)


@pytest.mark.parametrize("mode", (0, 1))
def test_the_refine_cases_can_tell_a_wrong_merge(orc, mode):
    """the two wrong merges lie 3 tolerances off on some triangle, in at least one of the two settings"""
    best = {}
    for setting, (_, _, seeds) in rs.REFINE_SETTINGS.items():
        X0, V0, _, _, n = restated_refine(orc, setting, mode, 0)
        _, expected, _ = rs.refine_reference(X0, V0, n[0], len(seeds))
        for name, d in rs.power(expected, expected["tol"]).items():
            best[name] = max(best.get(name, 0.0), d)
    print("refine, mode %d: %s" % (mode, best))
    assert set(best) == {"weights swapped", "plain average"} and min(best.values()) >= 3.0, best
