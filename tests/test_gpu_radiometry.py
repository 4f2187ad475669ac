"""GPU: the gathers and the photon path against closed-form radiometry (tests/radiometry_reference.py).  Nothing
here is compared with a restatement: every figure a kernel leaves is held against a solid angle, a form factor or a clipped
polygon, under the acceptance rule

    |mean over the K S samples - mu_ref| <= 6 sigma_ref / sqrt(K S) + eps_quad + 1e-5 mu_ref

with sigma_ref and eps_quad from the reference, K = 8 calls with seeds of their own and S = 4096 samples each; photon counts
against Binomial(N, p_ref) with |count - N p| <= 6 sqrt(N p (1 - p)); K bounces over links against the exact mean over link
sets with sigma_call of one call and the K = 8 link seeds; the refine against its merge for a fixed first pass.
tests/test_radiometry_cpu.py runs the same cases through
the restatements and shows that each would notice each wrong formula.  The oracle library is used for the BVH alone.

With UVRT_RADIOMETRY_MARGINS=FILE the margins of every case are written into FILE under "gpu"."""
import numpy as np
import pytest

import gather_edge_scene as ge
import radiometry_reference as rr
import radiometry_scenes as rs

pytestmark = pytest.mark.gpu

N, K, S, SEEDS = rs.N, rs.K, rs.S, rs.SEEDS
f32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def _margins():
    yield
    rs.dump_margins("gpu")


def new_ctx(pkg, orc, rows, cap, fl=0, mode=0):
    scene = ge.HandScene(orc, np.array(rows, dtype=f32))
    c = pkg.capi.Ctx(0)
    c.set_scene(scene.tris, scene.nodes, scene.triIdx)
    c.resize_rays(cap)
    c.set_flavour(fl)
    c.set_gather_sampling(mode)
    return c


def done(c):
    c.sync()
    c.close()


# ---------------------------------------------------------------- the direct gather
@pytest.mark.parametrize("fl", (0, 1))
@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("name", tuple(rs.DIRECT_CASES))
def test_the_direct_gather(pkg, orc, name, mode, fl):
    """the mean of expected[t] over the seeds against the lamp's mean of (visible solid angle) / 4 pi: a point lamp over the plate
    (partly shadowed floor triangles, the clipped reference), a 1.2 m rod and a sweep of it; the triangle seen edge-on and the one
    wholly in the shadow are exactly 0 in every call.  A rod in the closed cube: the twelve means add up to N"""
    _, frm, to, length = rs.DIRECT_CASES[name]
    rs.check_direct_scene(name)
    rows = rs.direct_rows(name)
    ref = rs.direct_reference(name)
    c = new_ctx(pkg, orc, rows, rows.shape[0] * S, fl, mode)
    got = []
    for seed in SEEDS:
        c.gather_direct(frm, to, length, S, seed, N)
        got.append(c.read_expected())
    done(c)
    got = np.array(got)
    rs.accept("direct, %s, mode %d, flavour %d" % (name, mode, fl), got.mean(axis=0), ref, K * S)
    dark = ref["mu"] == 0
    assert dark.sum() == rs.direct_dark(name) and np.all(got[:, dark] == 0.0)
    if name == "rod in the closed cube":
        rs.accept_total("direct, %s, mode %d, flavour %d" % (name, mode, fl), got.mean(axis=0), ref, K * S, N)


@pytest.mark.parametrize("fl", (0, 1))
@pytest.mark.parametrize("name", tuple(rs.DIRECT_CASES))
def test_the_variance_plane(pkg, orc, name, fl):
    """independent sampling: the mean over the seeds of variance[t] against Var(x) / S, x one sample's contribution; the
    tolerance from its fourth moment -- a sample variance has sd sqrt((mu4 - sigma^4) / S)"""
    _, frm, to, length = rs.DIRECT_CASES[name]
    rows = rs.direct_rows(name)
    ref = rs.direct_reference(name)
    c = new_ctx(pkg, orc, rows, rows.shape[0] * S, fl, 0)
    c.set_gather_variance(1)
    got = []
    for seed in SEEDS:
        c.gather_direct(frm, to, length, S, seed, N)
        got.append(c.read_variance())
    done(c)
    tol = rr.variance_tolerance(ref["var"], ref["mu4"], S, K, ref["mom_err"])
    rs.accept("variance, %s, flavour %d" % (name, fl), np.mean(got, axis=0), dict(mu=ref["var"] / S), K * S, tol)


# ---------------------------------------------------------------- the photon path
def photon_counts(pkg, orc, rows, lamp, length, to=None):
    c = new_ctx(pkg, orc, rows, N)
    c.reset(True)
    c.seed = 0
    if to is None:
        c.generate(lamp, length, 0, N)
    else:
        c.generate_sweep(lamp, to, length, 0, N)
    c.extend(N)
    counts = c.read_counts()
    done(c)
    return counts


@pytest.mark.parametrize("name", ("point lamp, plate", "rod", "sweep"))
def test_the_photon_counts(pkg, orc, name):
    """generate -> extend with N = 2^20: tempPhotonMap[t] against Binomial(N, p_t), p_t the share the direct gather's reference
    gives.  With test_the_direct_gather this holds "`expected` is the expected photon count" on both of its sides -- for a lamp
    that stands and, with generate_sweep -> extend, for one that drives while it radiates"""
    _, frm, to, length = rs.DIRECT_CASES[name]
    ref = rs.direct_reference(name)
    p = ref["share"]
    want = dict(mu=N * p, variants={k: v for k, v in ref["variants"].items() if k != "no cosine"})
    counts = photon_counts(pkg, orc, rs.direct_rows(name), frm, length, to if name == "sweep" else None)
    rs.accept("photons, " + name, counts, want, N, rr.binomial_tolerance(N, p) + ref["eps"])


@pytest.mark.parametrize("length", (0.0, rs.ROD))
def test_no_photon_leaves_the_closed_cube(pkg, orc, length):
    counts = photon_counts(pkg, orc, rs.cube_rows(), rs.CUBE_LAMP, length)
    assert counts.sum() == N
    if length == 0:
        p = rs.cube_shares()
        rs.accept("photons, cube", counts, dict(mu=N * p), N, rr.binomial_tolerance(N, p))


# ---------------------------------------------------------------- one bounce
def write_planes(write, planes):
    write(0, planes[0])
    write(1, planes[1])


def one_bounce(c, call, seed):
    if call == "traced":
        c.gather_indirect(rs.BOUNCE_RHO, S, seed)
    elif call == "linked":
        c.indirect_links_build(S, seed)
        c.gather_indirect_linked(rs.BOUNCE_RHO, 1)
    else:
        c.indirect_links_build_sided(S, seed)
        if call == "sided":
            c.gather_indirect_linked_sided(rs.BOUNCE_RHO, 1)
        else:
            c.gather_indirect_linked_mapped(1)
    return c.read_expected()


@pytest.mark.parametrize("fl", (0, 1))
@pytest.mark.parametrize("call", rs.BOUNCE_CALLS)
def test_one_bounce(pkg, orc, call, fl):
    """uvrt_gather_indirect, _linked, _linked_sided and _linked_mapped (K = 1) on the two facing squares and the corner, a
    hand-written source: per triangle against rho A_t sum_h F_{t->h} e_h with Lambert's form factors.  The two-sided calls take
    both faces' form factors; the sided ones read, of every emitter, the face that looks at the receiver -- the other faces hold
    light too, which must not arrive -- and the mapped one a reflectance of its own on each emitting face.  The links' seeds vary
    over the K runs.  Light on the faces turned away alone: exactly 0 everywhere"""
    rows = rs.squares_rows()
    c = new_ctx(pkg, orc, rows, rows.shape[0] * S, fl)
    if call in ("traced", "linked"):
        c.write_indirect_source(rs.SOURCE)
    else:
        write_planes(c.write_gather_faces, rs.face_planes(rs.SOURCE, rs.OUTER))
    if call == "mapped":
        write_planes(c.write_reflectance, rs.face_planes(rs.RHO_INNER, rs.RHO_OUTER))
    got = np.array([one_bounce(c, call, seed) for seed in SEEDS])
    away = None
    if call in ("sided", "mapped"):
        write_planes(c.write_gather_faces, rs.face_planes(np.zeros(6), rs.OUTER))
        c.write_expected(np.full(6, -3.25))
        away = one_bounce(c, call, SEEDS[0])
    done(c)
    rs.accept("bounce, %s, flavour %d" % (call, fl), got.mean(axis=0), rs.bounce_reference(call), K * S)
    assert away is None or (np.all(away == 0.0) and not np.signbit(away).any())


# ---------------------------------------------------------------- K bounces over links
def series_calls(c, call, seed):
    """(totals[4][T], the links' targets): one links build, then the call with 1, 2, 3 and 4 bounces on those links, add = 0"""
    if call == "linked":
        c.indirect_links_build(S, seed)
        links = c.read_indirect_links()
        target = links
    else:
        c.indirect_links_build_sided(S, seed)
        links = c.read_indirect_links()
        target = np.where(links >= 0, links >> 1, -1)
    totals = []
    for k in range(1, rs.SERIES_K + 1):
        c.write_expected(np.full(c.T, -3.25))
        if call == "linked":
            c.gather_indirect_linked(rs.BOUNCE_RHO, k)
        elif call == "sided":
            c.gather_indirect_linked_sided(rs.BOUNCE_RHO, k)
        else:
            c.gather_indirect_linked_mapped(k)
        totals.append(c.read_expected())
    return np.array(totals), target


@pytest.mark.parametrize("fl", (0, 1))
@pytest.mark.parametrize("name", rs.SERIES_SCENES)
@pytest.mark.parametrize("call", rs.SERIES_CALLS)
def test_the_bounce_series(pkg, orc, call, name, fl):
    """uvrt_gather_indirect_linked, _linked_sided and _linked_mapped with 1..4 bounces, on the three squares (open: many links
    miss) and on the uneven box (closed; areas from 0.25 to 3, a triangle without area, hand-written unequal sources and
    reflectances).  A set of links is one multinomial per leaving face, and a call is A sum_b M^b e0 with M = rho n / S': the
    mean over the K link seeds of the total, and of every single bounce g_b = total(b) - total(b - 1) on the same links, is held
    against the exact mean over link sets (form factors; paths that use a row twice counted) with 6 sigma_call / sqrt(K) +
    eps_quad + 1e-5 mu.  The triangle without area is +0.0 in every call and no link points at it; light on the faces turned
    away alone gives +0.0 everywhere, in every bounce"""
    rs.check_series_scene(name)
    rows = rs.series_rows(name)
    T = rows.shape[0]
    src = rs.series_inputs(name)[0]
    faces, rho = rs.series_planes(name)
    c = new_ctx(pkg, orc, rows, T * S, fl)
    if call == "linked":
        c.write_indirect_source(src)
    else:
        write_planes(c.write_gather_faces, faces)
    if call == "mapped":
        write_planes(c.write_reflectance, rho)
    got, flat_linked = [], False
    for seed in SEEDS:
        totals, target = series_calls(c, call, seed)
        got.append(totals)
        flat_linked |= name == "uneven box" and (bool(np.any(target == rs.BOX_FLAT)) or bool(np.any(target[rs.BOX_FLAT] != -1)))
    away = None
    if call != "linked":
        write_planes(c.write_gather_faces, rs.series_planes(name, np.zeros(T))[0])
        away, _ = series_calls(c, call, SEEDS[0])
    done(c)
    assert not flat_linked, "no link points at the triangle without area, and it has none"
    rs.accept_series("series, %s, %s, flavour %d" % (call, name, fl), got, rs.series_reference(call, name))
    assert away is None or (np.all(away == 0.0) and not np.signbit(away).any())


# ---------------------------------------------------------------- the refine, conditional on its first pass
@pytest.mark.parametrize("fl", (0, 1))
@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("setting", tuple(rs.REFINE_SETTINGS))
def test_the_refine(pkg, orc, setting, mode, fl):
    """uvrt_gather_refine on the point lamp over the plate, first pass of 16 samples with a fixed seed: for that fixed first pass
    the merged planes are linear in the extra samples, so over the refine seeds the mean of expected is (a X0 + b mu) / (a + b)
    and, in the independent mode, that of variance (a^2 V0 + b Var(x)) / (a + b)^2, with a = 16, b = n_t and mu, Var(x) the
    direct gather's closed forms -- once with every refinable triangle at the cap of 4096, once with counts of their own up to
    64.  A refine forgets the gather, so every seed gathers again (the same bits).  n_t = 0 keeps every bit of both planes"""
    _, frm, to, length = rs.DIRECT_CASES[rs.REFINE_CASE]
    rel_error, max_extra, seeds = rs.REFINE_SETTINGS[setting]
    rows = rs.direct_rows(rs.REFINE_CASE)
    c = new_ctx(pkg, orc, rows, rows.shape[0] * max_extra, fl, mode)
    c.set_gather_variance(1)
    first, e, v, n = [], [], [], []
    for seed in seeds:
        c.gather_direct(frm, to, length, rs.REFINE_S0, rs.REFINE_FIRST_SEED, N)
        first.append((c.read_expected(), c.read_variance()))
        c.gather_refine(rel_error, max_extra, seed)
        e.append(c.read_expected())
        v.append(c.read_variance())
        n.append(c.read_gather_extra())
    done(c)
    X0, V0 = first[0]
    assert all(np.array_equal(x, X0) and np.array_equal(y, V0) for x, y in first), "the first pass is deterministic"
    rs.accept_refine("mode %d, flavour %d" % (mode, fl), setting, X0, V0, e, v, n, mode == 0)


# ---------------------------------------------------------------- the mirror
@pytest.mark.parametrize("fl", (0, 1))
@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("name", tuple(rs.MIRROR_CASES))
def test_the_mirror_gather(pkg, orc, name, mode, fl):
    """uvrt_gather_mirror of a point lamp in the closed cube: with the whole wall x = 4 as the panel, rho times the solid angle of
    every triangle from the lamp's image, over 4 pi; with one of the wall's two triangles, the part of every triangle that the
    image sees through that triangle (the clipped reference).  The wall itself is exactly 0"""
    rows = rs.cube_rows()
    q, m, rho = rs.wall_panel()
    c = new_ctx(pkg, orc, rows, 12 * S, fl, mode)
    c.set_mirrors([pkg.capi.mirror(q, m, rho)], rs.wall_members(name))
    got = []
    for seed in SEEDS:
        c.write_expected(np.full(12, -3.25))
        c.gather_mirror(rs.CUBE_LAMP, rs.CUBE_LAMP, 0.0, S, seed, N)
        got.append(c.read_expected())
    done(c)
    got = np.array(got)
    rs.accept("mirror, %s, mode %d, flavour %d" % (name, mode, fl), got.mean(axis=0), rs.mirror_reference(name), K * S)
    assert np.all(got[:, list(rs.WALL)] == 0.0)
