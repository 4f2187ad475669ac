"""Closed-form radiometry in numpy f64: what the gathers and the photon path are anchored to.

Nothing here comes from the package, from oracle/ or from a *_restate.py, and there is no RNG: every figure is a solid angle
(Van Oosterom-Strackee), a point-to-polygon form factor (Lambert's contour formula), a clipped polygon (Sutherland-Hodgman) or a
Gauss-Legendre quadrature of one of these, with an error estimate taken as the difference to the rule of twice the order.

The claims that are checked against it:
  direct   expected[t] / N  ->  the mean over the lamp (rod x sweep) of  visible solid angle of t / 4 pi
  photons  tempPhotonMap[t] ~   Binomial(N, that same share)
  bounce   expected[t]      ->  rho A_t sum_f sum_h F^f_{t->h} e_h        (f: the face of t a sample leaves, F: a form factor)
  mirror   expected[t] / N  ->  rho * (solid angle, from the lamp's mirror image, of the part of t seen through the panel) / 4 pi
  series   expected[t]      ->  E[A_t sum_{b <= K} (M^b e0)_t] over sets of links: M = rho n / S' with one multinomial n per leaving face
and the spread of one sample of each, which gives the tests their tolerances.

Conventions: a triangle is a (3, 3) array of vertices, a polygon a (k, 3) array of coplanar vertices in order, a lamp is
(rod_from, rod_to, length): the rod runs from its foot along +y for `length`, the foot moves from rod_from to rod_to.
Shared by tests/test_radiometry_cpu.py and tests/test_gpu_radiometry.py."""
import numpy as np

PI = np.pi
FOUR_PI = 4.0 * np.pi
EY = np.array([0.0, 1.0, 0.0])


def _dot(a, b):
    return np.sum(a * b, axis=-1)


def _norm(a):
    return np.sqrt(_dot(a, a))


# ---------------------------------------------------------------- solid angles
def solid_angle(o, a, b, c):
    """the signed solid angle of triangle (a, b, c) from o (Van Oosterom-Strackee); o may be an array of points (..., 3).
    A triangle seen edge-on gives exactly 0: the triple product is 0 and the denominator positive"""
    A, B, Cc = a - o, b - o, c - o
    la, lb, lc = _norm(A), _norm(B), _norm(Cc)
    num = _dot(A, np.cross(B, Cc))
    den = la * lb * lc + _dot(A, B) * lc + _dot(A, Cc) * lb + _dot(B, Cc) * la
    return 2.0 * np.arctan2(num, den)


def polygon_solid_angle(o, poly):
    """the solid angle (>= 0) of a planar convex polygon from o: the sum over its fan; o may be (..., 3)"""
    poly = np.asarray(poly, dtype=np.float64)
    o = np.asarray(o, dtype=np.float64)
    total = np.zeros(o.shape[:-1])
    for i in range(1, poly.shape[0] - 1):
        total = total + solid_angle(o, poly[0], poly[i], poly[i + 1])
    return np.abs(total)


# ---------------------------------------------------------------- clipping
def tri_normal(tri):
    """(unit normal of cross(e1, e2), area)"""
    n = np.cross(tri[1] - tri[0], tri[2] - tri[0])
    nn = _norm(n)
    return (n / nn if nn > 0 else n), 0.5 * nn


def polygon_area(poly):
    poly = np.asarray(poly, dtype=np.float64)
    if poly.shape[0] < 3:
        return 0.0
    s = np.zeros(3)
    for i in range(1, poly.shape[0] - 1):
        s = s + np.cross(poly[i] - poly[0], poly[i + 1] - poly[0])
    return 0.5 * float(_norm(s))


def clip_halfspace(poly, n, d):
    """Sutherland-Hodgman's one step: the part of the polygon with n.x >= d"""
    poly = np.asarray(poly, dtype=np.float64).reshape(-1, 3)
    m = poly.shape[0]
    if m == 0:
        return poly
    s = poly @ n - d
    out = []
    for i in range(m):
        j = (i + 1) % m
        if s[i] >= 0:
            out.append(poly[i])
        if (s[i] >= 0) != (s[j] >= 0):
            t = s[i] / (s[i] - s[j])
            out.append(poly[i] + t * (poly[j] - poly[i]))
    return np.array(out, dtype=np.float64).reshape(-1, 3)


def clip_convex(subject, clipper):
    """Sutherland-Hodgman: subject (any polygon in the clipper's plane) cut by every edge of the convex polygon `clipper`"""
    clipper = np.asarray(clipper, dtype=np.float64)
    k = clipper.shape[0]
    N = np.zeros(3)
    for i in range(1, k - 1):
        N = N + np.cross(clipper[i] - clipper[0], clipper[i + 1] - clipper[0])
    centre = clipper.mean(axis=0)
    out = np.asarray(subject, dtype=np.float64)
    for i in range(k):
        a, b = clipper[i], clipper[(i + 1) % k]
        inward = np.cross(N, b - a)
        if inward @ (centre - a) < 0:
            inward = -inward
        out = clip_halfspace(out, inward, inward @ a)
    return out


def project_from(apex, poly, plane_point, plane_normal):
    """the central projection of a polygon from `apex` onto a plane; every vertex must lie ahead of the apex"""
    poly = np.asarray(poly, dtype=np.float64)
    d = poly - apex
    t = ((plane_point - apex) @ plane_normal) / (d @ plane_normal)
    assert np.all(np.isfinite(t)) and np.all(t > 0), "a vertex does not project forward onto the plane"
    return apex + t[:, None] * d


def _cone_planes(apex, window):
    """the half-spaces n.x >= d whose intersection is what lies behind the convex polygon `window` as seen from apex: one plane
    through the apex per edge, and the window's own plane"""
    window = np.asarray(window, dtype=np.float64)
    centre = window.mean(axis=0)
    planes = []
    k = window.shape[0]
    for i in range(k):
        m = np.cross(window[i] - apex, window[(i + 1) % k] - apex)
        if m @ (centre - apex) < 0:
            m = -m
        planes.append((m, m @ apex))
    wn = np.cross(window[1] - window[0], window[2] - window[0])
    if wn @ (window[0] - apex) < 0:
        wn = -wn
    planes.append((wn, wn @ window[0]))
    return planes


def clip_to_cone(poly, apex, window):
    """The part of `poly` that lies behind the convex polygon `window` as seen from `apex`.  In poly's plane this is
    Sutherland-Hodgman against the window's central projection, done with the projecting planes themselves so that a window whose
    projection runs off to infinity (a wall that meets the receiver's plane) needs no special case"""
    out = np.asarray(poly, dtype=np.float64)
    for n, d in _cone_planes(np.asarray(apex, dtype=np.float64), window):
        out = clip_halfspace(out, n, d)
    return out


def inside_cone(points, apex, window, margin=1e-9):
    """every point lies strictly (by `margin`, in units of the plane's scaled distance) behind the window as seen from apex"""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    for n, d in _cone_planes(np.asarray(apex, dtype=np.float64), window):
        if np.any((points @ n - d) / _norm(n) <= margin):
            return False
    return True


def coplanar(tri, poly, tol=1e-12):
    n = np.cross(poly[1] - poly[0], poly[2] - poly[0])
    n = n / _norm(n)
    return bool(np.all(np.abs((np.asarray(tri) - poly[0]) @ n) < tol))


def visible_regions(o, tri, occluders):
    """[(sign, polygon)]: the triangle, minus what each occluder (a convex polygon, their shadows on the triangle disjoint) hides
    from the point o; [] when one occluder hides all of it"""
    regions = [(1.0, np.asarray(tri, dtype=np.float64))]
    for occ in occluders:
        occ = np.asarray(occ, dtype=np.float64)
        if coplanar(tri, occ):
            continue
        if inside_cone(tri, o, occ):
            return []
        part = clip_to_cone(tri, o, occ)
        if part.shape[0] >= 3 and polygon_area(part) > 0:
            regions.append((-1.0, part))
    return regions


def regions_solid_angle(o, regions):
    total = 0.0
    for sign, poly in regions:
        total = total + sign * polygon_solid_angle(o, poly)
    return total


# ---------------------------------------------------------------- quadrature
def gauss01(order):
    """Gauss-Legendre nodes and weights on [0, 1]"""
    x, w = np.polynomial.legendre.leggauss(int(order))
    return 0.5 * (x + 1.0), 0.5 * w


def lamp_points(rod_from, rod_to, length, order):
    """(points (L, 3), weights (L,) summing to 1) over the rod (u_h) and the sweep (u_m); a coordinate that does not move takes
    one node"""
    rod_from = np.asarray(rod_from, dtype=np.float64)
    seg = np.asarray(rod_to, dtype=np.float64) - rod_from
    xh, wh = gauss01(order) if length != 0 else (np.zeros(1), np.ones(1))
    xm, wm = gauss01(order) if np.any(seg != 0) else (np.zeros(1), np.ones(1))
    pts = rod_from[None, None, :] + xh[:, None, None] * float(length) * EY[None, None, :] + xm[None, :, None] * seg[None, None, :]
    return pts.reshape(-1, 3), (wh[:, None] * wm[None, :]).reshape(-1)


def is_point_lamp(rod_from, rod_to, length):
    return length == 0 and not np.any(np.asarray(rod_to, dtype=np.float64) != np.asarray(rod_from, dtype=np.float64))


def triangle_nodes(order):
    """(a, b, w): points v0 + a e1 + b e2 of a collapsed Gauss-Legendre rule on a triangle, weights summing to 1"""
    x, w = gauss01(order)
    a = np.repeat(x, order)
    b = (1.0 - a) * np.tile(x, order)
    return a, b, 2.0 * np.repeat(w, order) * np.tile(w, order) * (1.0 - a)


# ---------------------------------------------------------------- the direct gather and the photon path
def direct_mean(tri, rod_from, rod_to, length, occluders=(), order=16):
    """(share, quadrature error): the mean over the lamp of (visible solid angle of `tri`) / 4 pi, so that a launch of N photons
    leaves N * share on the triangle.  The error is the difference between Gauss-Legendre of `order` and of twice the order per
    lamp coordinate (0 for a point lamp, where nothing is integrated).  Occluders only with a point lamp, where the shadow's edge
    on the triangle is a polygon"""
    tri = np.asarray(tri, dtype=np.float64)
    point = is_point_lamp(rod_from, rod_to, length)
    assert point or not len(occluders), "a clipped reference exists for a point lamp only"

    def at(n):
        pts, w = lamp_points(rod_from, rod_to, length, n)
        if len(occluders):
            vals = np.array([regions_solid_angle(o, visible_regions(o, tri, occluders)) for o in pts])
        else:
            vals = polygon_solid_angle(pts, tri)
        return float(w @ vals) / FOUR_PI
    if point:
        return at(1), 0.0
    coarse, fine = at(order), at(2 * order)
    return fine, abs(fine - coarse)


def _central(m):
    """(mean, variance, fourth central moment) from the raw moments m1..m4"""
    m1, m2, m3, m4 = m
    return m1, m2 - m1 * m1, m4 - 4.0 * m3 * m1 + 6.0 * m2 * m1 * m1 - 3.0 * m1 ** 4


def _raw_moments(tri, regions_of, pts, w, order, integrand):
    """raw moments 1..4 of integrand(p, o) with p uniform on the triangle (0 outside the regions) and o over the lamp's nodes"""
    _, area = tri_normal(tri)
    a, b, wt = triangle_nodes(order)
    m = np.zeros(4)
    for o, wo in zip(pts, w):
        for sign, poly in regions_of(o):
            for i in range(1, poly.shape[0] - 1):
                sub = np.array([poly[0], poly[i], poly[i + 1]])
                share = tri_normal(sub)[1] / area
                p = sub[0] + a[:, None] * (sub[1] - sub[0]) + b[:, None] * (sub[2] - sub[0])
                f = integrand(p, o)
                for k in range(4):
                    m[k] += wo * sign * share * float(wt @ f ** (k + 1))
    return m


def _direct_integrand(tri, cosine=True, scale=1.0):
    n, area = tri_normal(tri)

    def f(p, o):
        D = p - o
        R2 = _dot(D, D)
        if cosine:
            return scale * area * np.abs(D @ n) / (FOUR_PI * R2 * np.sqrt(R2))
        return scale * area / (FOUR_PI * R2)
    return f


def direct_moments(tri, rod_from, rod_to, length, occluders=(), order=12, cosine=True):
    """dict(mean, var, mu4, err): the moments of one sample's contribution x / N = A_t |cos theta| vis / (4 pi R^2) with the point
    uniform on the triangle and the lamp point uniform on rod x sweep, by tensor quadrature (collapsed Gauss-Legendre on the
    triangle or on the fans of its visible and hidden parts, Gauss-Legendre on the lamp).  err: the largest relative change of
    mean and variance against twice the order.  cosine = False is the "no cosine" variant"""
    tri = np.asarray(tri, dtype=np.float64)
    assert is_point_lamp(rod_from, rod_to, length) or not len(occluders), "a clipped reference exists for a point lamp only"
    f = _direct_integrand(tri, cosine)

    def at(n):
        pts, w = lamp_points(rod_from, rod_to, length, n)
        return _central(_raw_moments(tri, lambda o: visible_regions(o, tri, occluders), pts, w, n, f))
    return _with_error(at, order)


def _with_error(at, order):
    c, fine = at(order), at(2 * order)
    err = 0.0
    for k in (0, 1):
        if fine[k] != 0:
            err = max(err, abs(fine[k] - c[k]) / abs(fine[k]))
    return dict(mean=fine[0], var=max(fine[1], 0.0), mu4=max(fine[2], 0.0), err=err)


# ---------------------------------------------------------------- form factors and the bounce
def lambert(points, n, poly):
    """Lambert's contour formula: the form factor from the points (m, 3), facing along the unit normal n, to a polygon that lies
    wholly on n's side of their plane: (1 / 2 pi) |sum_i beta_i  n . Gamma_i|"""
    poly = np.asarray(poly, dtype=np.float64)
    R = poly[None, :, :] - points[:, None, :]
    R2 = np.roll(R, -1, axis=1)
    c = np.cross(R, R2)
    cn = _norm(c)
    beta = np.arctan2(cn, _dot(R, R2))
    with np.errstate(invalid="ignore", divide="ignore"):
        g = np.where(cn > 0, (c @ n) / cn, 0.0)
    return np.abs(np.sum(beta * g, axis=1)) / (2.0 * PI)


def point_form_factor(p, n, poly):
    """the form factor from one point facing along n to any planar polygon: clipped at the point's horizon, then Lambert"""
    p = np.asarray(p, dtype=np.float64)
    n = np.asarray(n, dtype=np.float64)
    part = clip_halfspace(poly, n, n @ p)
    if part.shape[0] < 3 or polygon_area(part) == 0.0 or np.all((part - p) @ n < 1e-12):      # (nothing above the horizon)
        return 0.0
    return float(lambert(p[None, :], n, part)[0])


def form_factor(tri, face, poly, n=64, uniform=False):
    """(F, error): the mean over the triangle's points of the form factor from its face (0: the side cross(e1, e2) points to,
    1: the other) to the polygon, by the collapsed Gauss-Legendre rule of order n and of 2 n; the error is their difference.
    (Next to a shared edge the integrand goes like d log d in the distance d to the edge.  A rule on congruent sub-triangles
    converges as h^2 there; Gauss-Legendre, whose nodes crowd towards every edge of the triangle, as n^-4: 1e-6 takes
    order 64 of the one and some 10^5 points of the other.)  Every point of a planar triangle has the same horizon, so the
    polygon is clipped once.  uniform = True is the "uniform hemisphere" variant: the polygon's solid angle over 2 pi in place of
    Lambert's cosine-weighted share"""
    tri = np.asarray(tri, dtype=np.float64)
    nrm, _ = tri_normal(tri)
    if face:
        nrm = -nrm
    part = clip_halfspace(poly, nrm, nrm @ tri[0])
    if part.shape[0] < 3 or polygon_area(part) < 1e-15 or np.all((part - tri[0]) @ nrm < 1e-12):      # (nothing above the horizon)
        return 0.0, 0.0

    def at(k):
        a, b, w = triangle_nodes(k)
        pts = tri[0] + a[:, None] * (tri[1] - tri[0]) + b[:, None] * (tri[2] - tri[0])
        vals = polygon_solid_angle(pts, part) / (2.0 * PI) if uniform else lambert(pts, nrm, part)
        return float(w @ vals)
    coarse, fine = at(n), at(2 * n)
    return fine, abs(fine - coarse)


def form_factor_tables(tris, n=64, uniform=False):
    """(F[2][T][T], err[2][T][T], arrive[T][T]): F[f][t][h] from face f of triangle t to triangle h (0 for h == t), and the face
    of h that light from t arrives on (0: the side n_h points to), taken at t's centroid.  No occlusion: for scenes whose
    triangles all lie on the boundary of one convex body (on_convex_boundary)"""
    tris = np.asarray(tris, dtype=np.float64)
    T = tris.shape[0]
    F = np.zeros((2, T, T))
    E = np.zeros((2, T, T))
    arrive = np.zeros((T, T), dtype=np.int64)
    for t in range(T):
        ct = tris[t].mean(axis=0)
        for h in range(T):
            if h == t:
                continue
            nh, _ = tri_normal(tris[h])
            arrive[t, h] = 0 if nh @ (ct - tris[h][0]) > 0 else 1
            for f in (0, 1):
                F[f, t, h], E[f, t, h] = form_factor(tris[t], f, tris[h], n, uniform)
    return F, E, arrive


def on_convex_boundary(tris, tol=1e-12):
    """every triangle's plane has all the scene's vertices on one closed side: the triangles lie on the boundary of a convex body,
    and no one of them stands between two others"""
    tris = np.asarray(tris, dtype=np.float64)
    verts = tris.reshape(-1, 3)
    for tri in tris:
        n, _ = tri_normal(tri)
        s = (verts - tri[0]) @ n
        if s.min() < -tol and s.max() > tol:
            return False
    return True


def bounce(tris, radiosity, tables):
    """(mu[T], sigma[T], eps[T]) of one bounce: mu_t = A_t sum_f sum_h F^f_{t->h} r[a][h] with r[a][h] what face a of h sends back
    per unit area (reflectance times irradiance, f64[2][T]) and a the face of h that t sees; sigma_t the standard deviation of
    ONE sample's contribution, counted so that the mean of S samples has sigma / sqrt(S): the samples alternate between the two
    faces, S / 2 each, which gives sigma^2 = 2 A_t^2 sum_f (sum_h F r^2 - (sum_h F r)^2); eps the form factors' quadrature
    error carried through"""
    tris = np.asarray(tris, dtype=np.float64)
    F, E, arrive = tables
    T = tris.shape[0]
    area = np.array([tri_normal(t)[1] for t in tris])
    r = np.asarray(radiosity, dtype=np.float64)[arrive, np.arange(T)[None, :]]          # r[t][h] = radiosity[arrive[t][h]][h]
    mu, var, eps = np.zeros(T), np.zeros(T), np.zeros(T)
    for f in (0, 1):
        m1 = np.sum(F[f] * r, axis=1)
        m2 = np.sum(F[f] * r * r, axis=1)
        mu += area * m1
        var += 2.0 * area * area * np.maximum(m2 - m1 * m1, 0.0)
        eps += area * np.sum(E[f] * np.abs(r), axis=1)
    return mu, np.sqrt(var), eps


# ---------------------------------------------------------------- K bounces over recorded links
# In a scene on the boundary of one convex body a sample that leaves face f of triangle t lands on triangle h with probability
# F[f][t][h], on the face arrive[t][h], and misses with what remains.  Each face draws S' samples, so a set of links is one
# independent multinomial per row r = (f, t), and a linked call is  A_t sum_{b = 1..K} (M^b e0)  summed over the two faces, with
# M[r, c] = rho[c] n[r, c] / S', n the row's counts, c = (a, h) the emitting face, and e0 the irradiance the source planes hold.
# The rows and columns are numbered f * T + t.
def link_model(tables, area, rho, planes):
    """(P[R, R], rho[R], e0[R], A[R]), R = 2 T: the rows' landing probabilities, the reflectance of every emitting face (`rho` one
    number or f64[2][T]), the irradiance planes / area (`planes` f64[2][T], photons; 0 where the area is 0) and the rows' areas"""
    F, _, arrive = tables
    area = np.asarray(area, dtype=np.float64)
    T = area.size
    P = np.zeros((2 * T, 2 * T))
    cols = arrive * T + np.arange(T)[None, :]
    for f in (0, 1):
        P[f * T + np.arange(T)[:, None], cols] = F[f]
    assert np.all(np.diag(P) == 0.0) and np.all(P >= 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        e0 = np.where(area > 0, np.asarray(planes, dtype=np.float64) / area, 0.0).reshape(2 * T)
    rho = np.broadcast_to(np.asarray(rho, dtype=np.float64), (2, T)).reshape(2 * T)
    return P, rho.copy(), e0, np.tile(area, 2)


def fold_faces(v):
    """[.., 2 T] -> [.., T]: the two faces of every triangle added"""
    v = np.asarray(v)
    T = v.shape[-1] // 2
    return v[..., :T] + v[..., T:]


def series(P, rho, e0, A, K):
    """mu[K][R]: mu_b = A Mbar^b e0 with Mbar = rho P, the mean of M.  What the calls would give if a path never used a row twice"""
    m = P * rho[None, :]
    out, v = [], e0
    for _ in range(K):
        v = m @ v
        out.append(A * v)
    return np.array(out)


def series_exact(P, rho, e0, A, K, Sp):
    """E[A M^b e0][K][R] for K <= 4, exact: the sum over the paths r0 -> c1 -> .. -> cb.  Step i takes a count of row c_{i-1}; two
    steps that take counts of the same multinomial have E[n_a n_b] = S'(S' - 1) p_a p_b + delta_ab S' p_a in place of
    S'^2 p_a p_b.  P's diagonal is 0, so neighbouring steps never share a row and for b <= 4 no row is used three times; rows
    are independent, so the factors of the pairs multiply.  The whole tensor of paths over the active rows (<= 16) is formed"""
    assert 1 <= K <= 4
    R = P.shape[0]
    act = np.nonzero((P.sum(axis=1) > 0) | (P.sum(axis=0) > 0))[0]
    n = act.size
    assert n <= 16, "at most 16 active rows"
    p = P[np.ix_(act, act)]
    m = p * rho[act][None, :]
    eye = np.eye(n, dtype=bool)
    out = np.zeros((K, R))

    def on(M, i, j, b):                    # the matrix M[x_i, x_j] laid along the axes i and j of the path tensor
        shape = [1] * (b + 1)
        shape[i], shape[j] = n, n
        return M.reshape(shape) if i < j else M.T.reshape(shape)

    for b in range(1, K + 1):
        shape = [1] * (b + 1)
        shape[b] = n
        term = e0[act].reshape(shape)
        for i in range(1, b + 1):
            term = term * on(m, i - 1, i, b)
        for i in range(1, b + 1):
            for j in range(i + 2, b + 1):                            # steps i and j read the rows x_{i-1} and x_{j-1}
                pi = on(p, i - 1, i, b)
                with np.errstate(divide="ignore"):
                    twice = np.where(on(eye, i, j, b) & (pi > 0), 1.0 / (Sp * pi), 0.0)
                term = term * np.where(on(eye, i - 1, j - 1, b), (1.0 - 1.0 / Sp) + twice, 1.0)
        out[b - 1, act] = A[act] * term.reshape(n, -1).sum(axis=1)
    return out


def series_sigma(P, rho, e0, area, Sp, bounces):
    """sigma_call[T] of sum_{b in bounces} (g_b of a triangle, both faces), to first order in 1 / S': a change dM of row r moves
    M^b e0 by sum_k Mbar^k dM Mbar^(b-1-k) e0, so with w_r = sum_b sum_{k < b} (Mbar^k)[t, r] Mbar^(b-1-k) e0 and x = rho w_r the
    row contributes the variance of the mean of S' draws of x_j with probabilities p_rj (a miss is a draw of 0)"""
    m = P * rho[None, :]
    R = P.shape[0]
    top = max(bounces)
    pw = [np.eye(R)]
    for _ in range(top):
        pw.append(pw[-1] @ m)
    w = np.zeros((R // 2, R, R))
    for b in bounces:
        for k in range(b):
            w += fold_faces(pw[k].T).T[:, :, None] * (pw[b - 1 - k] @ e0)[None, None, :]
    x = rho[None, None, :] * w
    m1 = np.einsum("rj,trj->tr", P, x)
    m2 = np.einsum("rj,trj->tr", P, x * x)
    return np.asarray(area) * np.sqrt(np.maximum(m2 - m1 * m1, 0.0).sum(axis=1) / Sp)


def series_wrong(P, rho, e0, A, K, which):
    """g[K][R] under a wrong recursion: "no area" forgets the division by the area between bounces (e_b = g_b), "rho once"
    applies the reflectance to the first bounce only, "receiver's rho" takes, from the second bounce on, the reflectance of
    the receiving face"""
    out, v = [], e0
    for b in range(K):
        if which == "rho once" and b > 0:
            v = P @ v
        elif which == "receiver's rho" and b > 0:
            v = rho * (P @ v)
        else:
            v = (P * rho[None, :]) @ v
        out.append(A * v)
        if which == "no area":
            v = A * v
    return np.array(out)


# ---------------------------------------------------------------- the mirror
def mirror_image(p, plane_point, plane_normal):
    """the mirror image of the point p in the plane"""
    p = np.asarray(p, dtype=np.float64)
    m = np.asarray(plane_normal, dtype=np.float64)
    m = m / _norm(m)
    return p - 2.0 * ((p - np.asarray(plane_point, dtype=np.float64)) @ m) * m


def mirror_regions(tri, lamp, plane_point, plane_normal, windows):
    """[(+1, polygon)]: the parts of the triangle, on the lamp's side of the mirror's plane, that the lamp's image sees through the
    panel -- `windows` are the panel's convex pieces (its member triangles), their interiors disjoint"""
    m = np.asarray(plane_normal, dtype=np.float64)
    m = m / _norm(m)
    q = np.asarray(plane_point, dtype=np.float64)
    assert (np.asarray(lamp, dtype=np.float64) - q) @ m > 0, "the lamp stands in front of the panel"
    image = mirror_image(lamp, q, m)
    front = clip_halfspace(tri, m, m @ q)
    out = []
    if front.shape[0] < 3 or polygon_area(front) == 0.0 or np.all(np.abs((front - q) @ m) < 1e-12):
        return out
    for win in windows:
        part = clip_to_cone(front, image, win)
        if part.shape[0] >= 3 and polygon_area(part) > 0:
            out.append((1.0, part))
    return out


def mirror_mean(tri, lamp, plane_point, plane_normal, rho, windows):
    """the share of a point lamp's photons that reaches `tri` by way of the panel: rho * (solid angle of the seen part from the
    lamp's image) / 4 pi; exact, no quadrature"""
    image = mirror_image(lamp, plane_point, plane_normal)
    return rho * regions_solid_angle(image, mirror_regions(tri, lamp, plane_point, plane_normal, windows)) / FOUR_PI


def mirror_moments(tri, lamp, plane_point, plane_normal, rho, windows, order=12, cosine=True, at_mirror_point=False):
    """direct_moments for the mirror gather of a point lamp: x / N = rho A_t |cos theta| seen / (4 pi R^2) with R the unfolded
    distance |p - image|.  at_mirror_point = True is the variant that weighs with the distance from the lamp to the mirror
    point instead, tau R with tau = d_lamp / (d_lamp + d_p)"""
    tri = np.asarray(tri, dtype=np.float64)
    m = np.asarray(plane_normal, dtype=np.float64)
    m = m / _norm(m)
    q = np.asarray(plane_point, dtype=np.float64)
    image = mirror_image(lamp, q, m)
    regions = mirror_regions(tri, lamp, q, m, windows)
    base = _direct_integrand(tri, cosine, rho)
    d_o = (np.asarray(lamp, dtype=np.float64) - q) @ m

    def f(p, o):
        x = base(p, o)
        if at_mirror_point:
            tau = d_o / (d_o + (p - q) @ m)
            x = x / (tau * tau)
        return x

    def at(n):
        return _central(_raw_moments(tri, lambda o: regions, image[None, :], np.ones(1), n, f))
    return _with_error(at, order)


# ---------------------------------------------------------------- the acceptance rule
def tolerance(sigma, eps, mu, samples):
    """|mean of `samples` samples - mu| <= 6 sigma / sqrt(samples) + eps + 1e-5 mu  (six sigma for a few hundred
    comparisons, the reference's own quadrature error, the kernels' f32 sample points)"""
    return 6.0 * np.asarray(sigma) / np.sqrt(float(samples)) + np.asarray(eps) + 1e-5 * np.abs(np.asarray(mu))


def variance_tolerance(var, mu4, S, K, eps_rel):
    """for the mean over K calls of variance[t] = s^2 / S, s^2 the sample variance of S samples: the sample variance has
    sd ~ sqrt((mu4 - sigma^4) / S), so the mean over K has 6 sqrt((mu4 - sigma^4) / (S K)) / S; plus the reference's quadrature
    error and the f32 term"""
    var, mu4 = np.asarray(var), np.asarray(mu4)
    return 6.0 * np.sqrt(np.maximum(mu4 - var * var, 0.0) / (S * K)) / S + (eps_rel + 1e-5) * var / S


def binomial_tolerance(N, p):
    """|count - N p| <= 6 sqrt(N p (1 - p))"""
    p = np.asarray(p)
    return 6.0 * np.sqrt(N * p * (1.0 - p))
