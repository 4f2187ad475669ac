"""The cases and references of the sensors' radiometry tests, shared by tests/test_radiometry_sensors_cpu.py (the
restatement against the closed forms, and the power of every case) and tests/test_gpu_radiometry_sensors.py (the kernels against
them).  A point receiver under a rod has a textbook closed form, so the sensors are anchored more tightly than any gather of a
triangle: no integral over the receiver is left.  Geometry and expected values only: no kernel, no restatement and no RNG forms
a reference.  The acceptance rule, its K, S and N, the scenes and the margins file are radiometry_scenes' (DESIGN.md 24).

A sensor is (position, normal or None): None is a spherical sensor.  All values are photons per square metre of a launch of N."""
import functools

import numpy as np

import radiometry_reference as rr
import radiometry_scenes as rs

f64 = np.float64
N, K, S, SEEDS = rs.N, rs.K, rs.S, rs.SEEDS
FOUR_PI = 4.0 * np.pi


def r32(v):
    return None if v is None else rs.r32(v)


def sensor_list(rows):
    return tuple((r32(p), r32(n)) for p, n in rows)


# ---------------------------------------------------------------- the direct part
def sample_value(p, n, o, cosine=True, two_sided=False):
    """x / N of one direct sample from the lamp points o (m, 3): cos theta / (4 pi R^2) on the side n points to, 1 / (4 pi R^2)
    for a spherical sensor (n None).  cosine=False: the planar sensor without its cosine; two_sided: |cos theta|"""
    D = np.asarray(p, dtype=f64)[None, :] - np.asarray(o, dtype=f64)
    R2 = np.sum(D * D, axis=1)
    if n is None:
        return 1.0 / (FOUR_PI * R2)
    n = np.asarray(n, dtype=f64)
    c = -(D @ n) / (np.linalg.norm(n) * np.sqrt(R2))
    c = np.abs(c) if two_sided else np.maximum(c, 0.0)
    if not cosine:
        c = (c > 0).astype(f64)
    return c / (FOUR_PI * R2)


def direct_moments(sensor, frm, to, length, order=64, **how):
    """(mean, variance of one sample, quadrature error) of x / N over the lamp: Gauss-Legendre of `order` per lamp coordinate,
    the error the difference to twice the order (0 for a point lamp)"""
    p, n = sensor

    def at(m):
        pts, w = rr.lamp_points(frm, to, length, m)
        x = sample_value(p, n, pts, **how)
        mean = float(w @ x)
        return mean, float(w @ (x * x)) - mean * mean
    if rr.is_point_lamp(frm, to, length):
        return at(1)[0], 0.0, 0.0
    (coarse, _), (fine, var) = at(order), at(2 * order)
    return fine, max(var, 0.0), abs(fine - coarse)


def rod_closed_form(sensor, foot, length):
    """x / N for a sensor at horizontal distance a from a vertical rod: the planar one facing the rod horizontally takes
    [h / sqrt(a^2 + h^2)] / (4 pi L a), the spherical one [arctan(h / a)] / (4 pi L a), h the height above the sensor, from the
    rod's foot to its top"""
    p, n = sensor
    p, foot = np.asarray(p, dtype=f64), np.asarray(foot, dtype=f64)
    d = np.array([p[0] - foot[0], 0.0, p[2] - foot[2]])
    a = float(np.linalg.norm(d))
    h0, h1 = foot[1] - p[1], foot[1] + length - p[1]
    if n is None:
        return (np.arctan(h1 / a) - np.arctan(h0 / a)) / (FOUR_PI * length * a)
    assert np.allclose(np.asarray(n, dtype=f64), -d / a, atol=1e-7), "the closed form is for a sensor that faces the rod"
    return (h1 / np.hypot(a, h1) - h0 / np.hypot(a, h0)) / (FOUR_PI * length * a)


def segment_blocked(a, b, tris, eps=1e-9):
    """the open segment a b meets one of the triangles [T, 3, 3] (Moeller-Trumbore in f64)"""
    a, b = np.asarray(a, dtype=f64), np.asarray(b, dtype=f64)
    d = b - a
    for t in np.asarray(tris, dtype=f64):
        e1, e2 = t[1] - t[0], t[2] - t[0]
        h = np.cross(d, e2)
        det = e1 @ h
        if abs(det) < 1e-14:
            continue
        s = a - t[0]
        u = (s @ h) / det
        q = np.cross(s, e1)
        v = (d @ q) / det
        tt = (e2 @ q) / det
        if u >= -eps and v >= -eps and u + v <= 1 + eps and eps < tt < 1 - eps:
            return True
    return False


# rod at a stop and on the sweep (radiometry_scenes "rod", "sweep": the 2 x 2 floor at y = 0 and the edge-on triangle)
ROD_SENSORS = sensor_list((
    ((2.4, 0.75, 0.7), (-1.0, 0.0, 0.0)),      # facing the rod at a = 1.5: the closed form
    ((2.4, 0.75, 0.7), None),                  # the same point, spherical: the closed form
    ((1.4, 0.25, 1.2), (0.0, 1.0, 0.0)),       # below the rod's foot, looking up
    ((1.15, 2.0, 0.7), (0.0, -1.0, 0.0)),      # above its top, looking down
    ((0.9, 2.5, 0.7), None),                   # on the rod's axis
    ((1.4, 0.9, 1.2), (0.0, 1.0, 0.0)),        # the rod stands on both sides of its plane: what tells one-sided from two-sided
))
CLOSED_FORM = (0, 1)
DIRECT_CASES = {"rod": ("floor", rs.ROD_FOOT, rs.ROD_FOOT, rs.ROD), "sweep": ("floor", rs.ROD_FOOT, rs.SWEEP_TO, rs.ROD)}


def direct_rows(name):
    return rs.floor_rows(DIRECT_CASES[name][0] == "plate")


@functools.lru_cache(maxsize=None)
def direct_reference(name, sensors=ROD_SENSORS):
    """dict(mu, sigma, eps, variants) per sensor of a direct case; a variant that does not apply to a sensor keeps its mu"""
    _, frm, to, length = DIRECT_CASES[name]
    tris = rs.verts(direct_rows(name))
    pts, _ = rr.lamp_points(frm, to, length, 4)
    half = np.array([0.0, 0.5 * length, 0.0])
    out = dict(mu=[], var=[], eps=[], no_cosine=[], midpoint=[], cosine_on_sphere=[], two_sided=[], still=[])
    for p, n in sensors:
        assert not any(segment_blocked(o, p, tris) for o in pts), "nothing of the scene stands between the lamp and a sensor"
        mean, var, eps = direct_moments((p, n), frm, to, length)
        out["mu"].append(N * mean)
        out["var"].append(N * N * var)
        out["eps"].append(N * eps)
        out["no_cosine"].append(N * direct_moments((p, n), frm, to, length, cosine=False)[0])
        out["two_sided"].append(N * direct_moments((p, n), frm, to, length, two_sided=True)[0])
        out["midpoint"].append(N * direct_moments((p, n), np.array(frm) + half, np.array(to) + half, 0.0)[0])
        out["cosine_on_sphere"].append(N * direct_moments((p, (0.0, 0.0, 1.0)), frm, to, length)[0] if n is None else N * mean)
        out["still"].append(N * direct_moments((p, n), frm, frm, length)[0])
    ref = {k: np.array(v) for k, v in out.items()}
    ref["sigma"] = np.sqrt(ref["var"])
    ref["variants"] = {"no cosine": ref["no_cosine"], "2 pi for 4 pi": 2.0 * ref["mu"], "rod at its midpoint": ref["midpoint"],
                       "a cosine on the spherical sensor": ref["cosine_on_sphere"], "two-sided planar": ref["two_sided"]}
    if tuple(frm) != tuple(to):
        ref["variants"]["the lamp does not move"] = ref["still"]
    return ref


# point lamp and plate (radiometry_scenes "point lamp, plate"): every sample has the same weight, only the f32 point error remains
PLATE_SENSORS = sensor_list((
    ((0.5, 0.1, 0.3), (0.0, 1.0, 0.0)),        # above the floor, in the light
    ((1.0, 0.5, 1.25), (0.0, 1.0, 0.0)),       # inside the plate's shadow: exactly 0
    ((0.5, 0.1, 0.3), (0.0, -1.0, 0.0)),       # lit, but facing away: exactly 0
    ((1.0, 0.5, 1.25), None),                  # inside the shadow, spherical: exactly 0
    ((0.5, 0.1, 0.3), None),                   # in the light, spherical
))


@functools.lru_cache(maxsize=None)
def plate_reference():
    lamp = np.array(rs.LAMP, dtype=f64)
    tris = rs.verts(rs.floor_rows(True))
    mu, wrong = [], []
    for p, n in PLATE_SENSORS:
        lit = not segment_blocked(lamp, p, tris)
        mu.append(N * float(sample_value(p, n, lamp[None, :])[0]) if lit else 0.0)
        wrong.append(N * float(sample_value(p, n, lamp[None, :], two_sided=True)[0]))     # two-sided and without the shadow
    mu = np.array(mu)
    assert [m > 0 for m in mu] == [True, False, False, False, True]
    return dict(mu=mu, sigma=np.zeros(mu.size), eps=np.zeros(mu.size),
                variants={"2 pi for 4 pi": 2.0 * mu}, no_shadow_two_sided=np.array(wrong))


# ---------------------------------------------------------------- the reflected part, on the squares of radiometry_scenes
BOUNCE_SENSORS = sensor_list((
    ((0.4, 0.3, 0.6), (0.0, 1.0, 0.0)),        # looks at B; C above its horizon
    ((0.7, 0.6, 0.3), (-1.0, 0.5, 0.25)),      # a normal off every axis: looks at C and B
    ((0.5, 0.5, 0.5), None),                   # the centre, spherical
    ((0.25, 0.7, 0.6), None),
))
BOUNCE_CALLS = ("source", "faces", "mapped")     # emitter 0 with one rho; emitter 1 with one rho; emitter 1 with the map


def bounce_inputs(call):
    """(source f64[T] or None, faces f64[2][T] or None, rho f32[2][T] or None) as the call reads them"""
    if call == "source":
        return rs.SOURCE, None, None
    faces = rs.face_planes(rs.SOURCE, rs.OUTER)
    return None, faces, (rs.face_planes(rs.RHO_INNER, rs.RHO_OUTER) if call == "mapped" else None)


def hemisphere_part(p, n, poly):
    part = rr.clip_halfspace(np.asarray(poly, dtype=f64), np.asarray(n, dtype=f64), float(np.asarray(n, dtype=f64) @ np.asarray(p, dtype=f64)))
    return part if part.shape[0] >= 3 and rr.polygon_area(part) > 0 else None


@functools.lru_cache(maxsize=None)
def bounce_reference(call):
    """dict(mu, sigma, eps, variants) per sensor: planar, sum_h F(p, n -> h) B_h with B_h the radiosity of the face of h that looks
    at the sensor; spherical, (1 / pi) sum_h Omega_h B_h.  One sample takes B_h (4 B_h) with probability F_h (Omega_h / 4 pi)"""
    rows = rs.squares_rows()
    tris = rs.verts(rows)
    A = rs.areas(rows)
    assert rr.on_convex_boundary(tris)
    inner = rs.inner_faces(rows)
    source, faces, rho = bounce_inputs(call)
    T = A.size
    if call == "source":
        B = rs.BOUNCE_RHO * source / A
        B_out = B
    else:
        r = rho.astype(f64) if rho is not None else np.full((2, T), rs.BOUNCE_RHO)
        rad = r * faces / A
        B, B_out = rad[inner, np.arange(T)], rad[1 - inner, np.arange(T)]
    out = dict(mu=[], var=[], outer=[], uniform=[], planar_as_sphere=[])
    for p, n in BOUNCE_SENSORS:
        pa = np.asarray(p, dtype=f64)
        assert np.all(pa > 0.05) and np.all(pa < 0.95), "inside the cube the squares bound: every ray arrives on an inward face"
        om = np.array([float(rr.polygon_solid_angle(pa, t)) for t in tris])
        if n is None:
            prob, val = om / FOUR_PI, 4.0 * B
            uniform = float(np.sum(om / FOUR_PI * 2.0 * B))          # "2 pi for 4 pi" of the fluence
            other = float(np.sum(prob * 4.0 * B_out))
            sphere = float(np.sum(prob * val))
        else:
            nh = np.asarray(n, dtype=f64) / np.linalg.norm(n)
            prob = np.array([rr.point_form_factor(pa, nh, t) for t in tris])
            val = B
            parts = [hemisphere_part(pa, nh, t) for t in tris]
            up = np.array([0.0 if q is None else float(rr.polygon_solid_angle(pa, q)) for q in parts])
            uniform = float(np.sum(up / (2.0 * np.pi) * B))          # a uniform hemisphere in place of the cosine
            other = float(np.sum(prob * B_out))
            sphere = float(np.sum(om / FOUR_PI * 4.0 * B))
        assert prob.sum() < 1.0
        mu = float(np.sum(prob * val))
        out["mu"].append(mu)
        out["var"].append(float(np.sum(prob * val * val)) - mu * mu)
        out["outer"].append(other)
        out["uniform"].append(uniform)
        out["planar_as_sphere"].append(sphere)
    ref = {k: np.array(v) for k, v in out.items()}
    ref["sigma"] = np.sqrt(np.maximum(ref["var"], 0.0))
    ref["eps"] = np.zeros(len(BOUNCE_SENSORS))
    ref["variants"] = {"uniform directions": ref["uniform"], "every sensor a sphere": ref["planar_as_sphere"]}
    if call != "source":
        ref["variants"]["the outer faces arrive"] = ref["outer"]
    if call == "mapped":
        ref["variants"]["one rho for the map"] = bounce_reference("faces")["mu"]
    return ref


# ---------------------------------------------------------------- in-situ calibration
CALIBRATION_SENSOR = ROD_SENSORS[0]
CALIBRATION_POWER = 2.5
CALIBRATION_SAMPLES = 4096          # RayTracer::sensorSamples of the calibrating launch


def calibration_reference():
    """the calibrated power 0.01 P / (closed form in photons per square metre and photon), with the direct case's sigma carried
    through the division to first order"""
    ref = direct_reference("rod")
    value = ref["mu"][0] / N
    mu = 0.01 * CALIBRATION_POWER / value
    return dict(mu=np.array([mu]), sigma=np.array([mu * ref["sigma"][0] / ref["mu"][0]]), eps=np.array([mu * ref["eps"][0] / ref["mu"][0]]),
                variants={"2 pi for 4 pi": np.array([0.5 * mu]), "rod at its midpoint": np.array([mu * ref["mu"][0] / ref["midpoint"][0]])})
