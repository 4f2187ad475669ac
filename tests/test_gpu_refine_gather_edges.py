"""GPU: the gather and refine kernels (csrc/uvrt_occlude.hip k_gather_generate / k_gather_reduce / k_gather_reduce_var,
csrc/uvrt_refine.hip) on hand-made geometry and hand-made planes (tests/gather_edge_scene.py), bit for bit against the
restatements: triangles without area (the nn == 0 branches), samples whose f32 distance under- or overflows while the f64 one
does not (the "no direction" branch), more than 64 extra samples per triangle, the count rule at every power of two and on
values no gather leaves (through the test hook uvrt_refine_counts), the prefix sum where a range ends at, before and behind a
block of 1024 positions, and its carry into a second tile of 256 block sums.  The room of the other gather tests reaches none
of these.

The file's name sorts it behind tests/test_gpu_reference_kernels.py on purpose.  The reference's generate.cl races on SEED,
and how the race resolves on a fresh module depends on what the process did on the GPU before: with this file -- or, alone,
with test_gpu_hotset.py's soup or test_gpu_adversarial.py's degenerate triangles -- directly in front of it, an eighth of the
work-items of the first launch read SEED after work-item 0's store, and test_whole_reference_kernel_chain_on_this_gpu_against_
the_product skips itself.  The suite's order in front of that test is therefore left as it was."""
import ctypes as C

import numpy as np
import pytest

import gather_edge_scene as ge
import gather_refine_restate as gf
import gather_restate as gr
import gather_stratified_restate as gs
import gather_variance_restate as gv

pytestmark = pytest.mark.gpu

N = 1 << 20
SEED = 3
RSEED = ~SEED & 0xFFFFFFFF
BOUNDARY_SEED = 123       # both ranges of the block-boundary refine start and end with a refined triangle, in both modes
MODES = (("independent", gv.INDEPENDENT), ("stratified", gv.STRATIFIED))
GEOMETRIES = (("stop, length 0", ge.LAMP, ge.LAMP, 0.0), ("stop, length 1", ge.LAMP, ge.LAMP, 1.0),
              ("segment", ge.LAMP, ge.SEGMENT_TO, 1.0))
POWERS = [2 << k for k in range(12)]            # 2 ... 4096
f32 = np.float32


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def new_ctx(pkg, scene, cap, mode=0, variance=1):
    c = pkg.capi.Ctx(0)
    c.set_scene(scene.tris, scene.nodes, scene.triIdx)
    c.resize_rays(cap)
    c.set_gather_sampling(mode)
    c.set_gather_variance(variance)
    return c


@pytest.fixture(scope="module")
def edge(orc):
    gr.check_rng(orc, 256)
    scene = ge.edge_scene(orc)
    _, _, _, nn = gr.tri_normals(scene.tris)
    assert np.array_equal(np.flatnonzero(nn == 0.0), scene.no_area)
    assert scene.sub_range[0] == scene.hand["point"] and sum(scene.sub_range) == scene.T == scene.hand["point, last"] + 1
    return scene


def check_refined(c, want_e, want_v, want_n, what, first=0):
    """n_t and both planes over [first, first + len(want_n)), and n_t = 0 outside"""
    got_n, got_e, got_v = c.read_gather_extra(), c.read_expected(), c.read_variance()
    k = want_n.size
    assert same(got_n[first:first + k], want_n), "%s: %d n_t differ" % (what, int((got_n[first:first + k] != want_n).sum()))
    assert not got_n[:first].any() and not got_n[first + k:].any(), what
    assert same(got_e[first:first + k], want_e), "%s: %d expected entries differ" % (what, int((got_e[first:first + k] != want_e).sum()))
    assert same(got_v[first:first + k], want_v), "%s: %d variance entries differ" % (what, int((got_v[first:first + k] != want_v).sum()))


# ---------------------------------------------------------------- the gather
def test_gather_on_the_edge_scene(pkg, orc, edge):
    """Both modes, the three geometries, flavours 0 and 1, S = 3 and 4, the variance on and off, one chunk and chunks of 101
    rays: `expected`, `variance` and every occlusion byte.  The restatement says that the untested branches are taken -- rays
    without a direction from underflow (the 1e-25 triangle at the foot of a lamp without length) and from overflow (the
    triangle at 3e19), NaN weights (0/0 on the triangles without area) -- and that both planes stay finite, +0.0 where there is
    no area."""
    T = edge.T
    tiny, huge, foot = edge.hand["tiny at the foot"], edge.hand["far and huge"], edge.hand["point at the foot"]
    sent_e, sent_v = np.full(T, 7.0), np.full(T, np.nan)
    big, small = new_ctx(pkg, edge, T * 4), new_ctx(pkg, edge, 101)
    for name, mode in MODES:
        for tag, frm, to, length in GEOMETRIES:
            for fl in (0, 1):
                for S in (3, 4):
                    what = "%s, %s, flavour %d, S = %d" % (name, tag, fl, S)
                    rays, w = gs.samples(orc, edge.tris, frm, to, length, S, SEED, 0, None, mode)
                    occ = gr.occluded(orc, edge, rays, fl)
                    want_e, want_v = gv.reduce_var(edge.tris, w, occ, S, N, mode)
                    assert same(want_e, gr.reduce(edge.tris, w, occ, S, N)), what
                    untraced = ((rays["dist"] == 0) & (rays["diry"] == 1)).reshape(T, S).sum(axis=1)
                    assert untraced[huge] == S and untraced[tiny] == (S if length == 0.0 else 0), what      # overflow, underflow
                    assert untraced[foot] == (S if length == 0.0 else 0) and untraced.sum() == untraced[[tiny, huge, foot]].sum(), what
                    assert np.isnan(w).sum() >= S and np.isnan(w.reshape(T, S)[edge.no_area]).sum() == np.isnan(w).sum(), what
                    assert np.isfinite(want_e).all() and np.isfinite(want_v).all(), what
                    assert not want_e[edge.no_area].view(np.uint64).any() and not want_v[edge.no_area].view(np.uint64).any(), what
                    assert 0.15 < occ.mean() < 0.6 and (want_e > 0).sum() > 0.8 * T and (want_v > 0).sum() > 0.8 * T, what
                    if tag.startswith("stop"):
                        assert want_e[edge.hand["plane through the rod"]] == 0.0, what
                    for c in (big, small):
                        c.set_flavour(fl)
                        c.set_gather_sampling(mode)
                        for var in (1, 0):
                            c.set_gather_variance(var)
                            c.write_expected(sent_e)
                            c.write_variance(sent_v)
                            c.gather_direct(frm, to, length, S, SEED, N)
                            got_e, got_v = c.read_expected(), c.read_variance()
                            assert same(got_e, want_e), "%s, variance %d: %d expected entries differ" % (what, var, int((got_e != want_e).sum()))
                            assert same(got_v, want_v if var else sent_v), "%s, variance %d: the variance plane" % (what, var)
                    assert np.array_equal(big.occluded(rays), occ), what
    big.close()
    small.close()


def test_accumulate_and_shade_on_the_edge_scene(pkg, orc, edge):
    """uvrt_accumulate_expected and uvrt_shade behind gathers of the edge scene: no NaN reaches the maps; the dose has the
    oracle's NaN (0 / 0 on a triangle whose f32 area is 0) in the oracle's positions and its bits everywhere else"""
    T = edge.T
    scaled = f32(f32(450.0) * f32(0.1))
    pm, mx = np.zeros(T), np.zeros(T)
    c = new_ctx(pkg, edge, T * 4)
    c.reset(True)
    for (tag, frm, to, length), step, (name, mode) in zip(GEOMETRIES, (60.0, 7.25, 3.5), (MODES[0], MODES[1], MODES[0])):
        e, _, _ = gv.gather(orc, edge, frm, to, length, 4, SEED, N, mode)
        c.set_gather_sampling(mode)
        c.gather_direct(frm, to, length, 4, SEED, N)
        c.accumulate_expected(step)
        gr.accumulate_expected(pm, mx, e, step)
        assert not c.read_expected().any() and not c.read_variance().any(), tag
        assert same(c.read_photon_map(0), pm) and same(c.read_photon_map(1), mx), tag
        assert np.isfinite(pm).all() and np.isfinite(mx).all(), tag
        c.shade(0, N, scaled, 100.0, 0)
        want = orc.compute_dosage(pm, edge.tris, N, scaled)
        got = c.read_dosage()
        assert np.isnan(want[edge.no_area]).all() and np.isnan(want).sum() < 10, tag
        assert np.array_equal(np.isnan(got), np.isnan(want)), tag
        ok = ~np.isnan(want)
        assert same(got[ok], want[ok]), "%s: %d dose entries differ" % (tag, int((got[ok].view(np.uint32) != want[ok].view(np.uint32)).sum()))
    assert (want[ok] > 0).sum() > 0.8 * T
    c.close()


# ---------------------------------------------------------------- the refine
def test_refine_on_the_whole_edge_scene(pkg, orc, edge):
    """tau = 0.1, at most 64 extra samples, S0 = 3 and 4, both modes, the three geometries: n_t, both planes and the report,
    from one chunk and from chunks of at most 100 rays.  Every value 0, 2 ... 64 occurs in each of the twelve cases; the
    triangles without area are never refined and keep +0.0."""
    T = edge.T
    big, small = new_ctx(pkg, edge, T * 64), new_ctx(pkg, edge, 100)
    for name, mode in MODES:
        for tag, frm, to, length in GEOMETRIES:
            for S0 in (3, 4):
                what = "%s, %s, S0 = %d" % (name, tag, S0)
                e, v, n, e0, v0 = gf.gather_and_refine(orc, edge, frm, to, length, S0, SEED, N, mode, 0.1, 64)
                assert sorted(set(n.tolist())) == [0, 2, 4, 8, 16, 32, 64], what
                assert np.isfinite(e).all() and np.isfinite(v).all() and not n[edge.no_area].any(), what
                assert not e[edge.no_area].view(np.uint64).any() and not v[edge.no_area].view(np.uint64).any(), what
                for c in (big, small):
                    c.set_gather_sampling(mode)
                    c.gather_direct(frm, to, length, S0, SEED, N)
                    assert same(c.read_expected(), e0) and same(c.read_variance(), v0), what
                    assert c.gather_refine(0.1, 64, RSEED) == (int(n.sum()), int((n > 0).sum())), what
                    check_refined(c, e, v, n, what)
    big.close()
    small.close()


@pytest.mark.parametrize("name,mode,tau", [("stratified", gv.STRATIFIED, 0.05), ("independent", gv.INDEPENDENT, 0.02)])
def test_refine_up_to_4096_samples_per_triangle(pkg, orc, edge, name, mode, tau):
    """The sub-range of the edge scene that starts and ends with a hand-made triangle, S0 = 4, at most 4096 extra samples: every
    power of two from 2 to 4096 occurs as an n_t.  Capacity 4096 makes every capped triangle a chunk of its own; a capacity
    above the total makes one chunk."""
    first, count = edge.sub_range
    frm, to, length = ge.LAMP, ge.LAMP, 1.0
    e, v, n, e0, v0 = gf.gather_and_refine(orc, edge, frm, to, length, 4, SEED, N, mode, tau, 4096, first=first, count=count)
    total = int(n.sum())
    print("%s, tau = %g: %d extra rays on %d of %d triangles" % (name, tau, total, int((n > 0).sum()), count))
    assert sorted(set(n.tolist())) == [0] + POWERS and total < 300000
    assert np.isfinite(e).all() and np.isfinite(v).all()
    sent_e, sent_v = np.linspace(1.0, 2.0, edge.T), np.linspace(3.0, 4.0, edge.T)
    for cap in (4096, 1 << 19):
        c = new_ctx(pkg, edge, cap, mode)
        c.write_expected(sent_e)
        c.write_variance(sent_v)
        c.gather_direct(frm, to, length, 4, SEED, N, first, count)
        assert c.gather_refine(tau, 4096, RSEED, first_tri=first, tri_count=count) == (total, int((n > 0).sum())), cap
        check_refined(c, e, v, n, "%s, capacity %d" % (name, cap), first)
        assert same(c.read_expected(0, first), sent_e[:first]) and same(c.read_variance(0, first), sent_v[:first]), cap
        c.close()


# ---------------------------------------------------------------- the count rule and the scan through the hook
def check_counts(c, scene_nn, E, V, S0, tau, min_expected, max_extra, first, count, what):
    """uvrt_refine_counts over [first, first + count) of planes that hold (E, V): n_t against the restated count rule, 0 outside
    the range, the offsets against the exact cumulative sum; returns n_t of the range"""
    want = gf.count_rule(E[first:first + count], V[first:first + count], scene_nn[first:first + count], S0, tau, min_expected, max_extra)
    offs = c.refine_counts(S0, tau, max_extra, min_expected, first, count)
    got = c.read_gather_extra()
    assert same(got[first:first + count], want), "%s: %d n_t differ" % (what, int((got[first:first + count] != want).sum()))
    assert not got[:first].any() and not got[first + count:].any(), what + ": n_t outside the range"
    exact = np.concatenate([[0], np.cumsum(want, dtype=np.int64)])
    assert exact[-1] < 1 << 31 and offs.dtype == np.int32 and offs.shape == (count + 1,), what
    assert np.array_equal(offs, exact), "%s: %d offsets differ, the first at position %d" % (
        what, int((offs != exact).sum()), int(np.flatnonzero(offs != exact)[0]))
    return want


@pytest.mark.parametrize("max_extra", [2, 64, 4096])
@pytest.mark.parametrize("S0", [2, 3, 16])
def test_the_count_rule_on_crafted_planes(pkg, orc, edge, S0, max_extra):
    """Planes written by hand (gather_edge_scene.count_rule_rows) so that `want` is 0 ... 4, 2^k - 1, 2^k and 2^k + 1 up to
    4097, max_extra and its neighbours, 1e300, inf and NaN, and X0 and V0 are zeros, subnormals, inf, NaN and negatives; on the
    triangles without area a row that wants the cap.  min_expected 0 and X0 itself; the whole scene and its sub-range.  The
    planes keep every bit."""
    T = edge.T
    _, _, _, nn = gr.tri_normals(edge.tris)
    X, V, pinned = ge.count_rule_rows(S0, max_extra)
    w = ge.restated_want(X, V, S0)
    for k, p in enumerate(pinned):
        assert p is None or w[k] == p, (k, X[k], V[k], w[k], p)
    assert np.isnan(w).sum() >= 3 and np.isposinf(w).sum() >= 3 and (w >= 1e299).sum() >= 5
    E, W = ge.crafted_planes(edge, S0, max_extra)
    assert gf.count_rule(E[edge.no_area], W[edge.no_area], np.ones(edge.no_area.size), S0, ge.ROW_TAU, 0.0, max_extra).tolist() \
        == [max_extra] * edge.no_area.size
    c = new_ctx(pkg, edge, 16)                          # (a capacity below max_extra: the hook stores no ray)
    c.write_expected(E)
    c.write_variance(W)
    for min_expected in (0.0, ge.ROW_X0):
        for first, count in ((0, T), edge.sub_range):
            what = "S0 = %d, max_extra = %d, min_expected = %g, range (%d, %d)" % (S0, max_extra, min_expected, first, count)
            n = check_counts(c, nn, E, W, S0, ge.ROW_TAU, min_expected, max_extra, first, count, what)
            assert not n[edge.no_area - first].any(), what
            assert set(n.tolist()) == {0} | {p for p in POWERS if p <= max_extra}, what
    assert same(c.read_expected(), E) and same(c.read_variance(), W)
    c.close()


def test_the_hook_leaves_a_gather_refinable_and_refuses_like_the_refine(pkg, orc, edge):
    """uvrt_refine_counts between a gather and its refine: the planes, the remembered gather, SEED and the maps are as they
    were, and the refine gives the restatement's bits.  Every refusal leaves the n_t plane, both planes and the remembered
    gather alone.  On a fresh scene the hook makes the planes and the per-triangle records itself."""
    Err = pkg.capi.UvrtError
    T = edge.T
    _, _, _, nn = gr.tri_normals(edge.tris)
    frm, to, length = ge.LAMP, ge.SEGMENT_TO, 1.0
    mode = gv.STRATIFIED
    e, v, n, e0, v0 = gf.gather_and_refine(orc, edge, frm, to, length, 4, SEED, N, mode, 0.1, 64)
    c = new_ctx(pkg, edge, T * 64, mode)
    # a scene that has gathered nothing: zero planes, so nothing is wanted, and the hook works without g_tris from a gather
    assert not check_counts(c, nn, np.zeros(T), np.zeros(T), 4, 0.1, 0.0, 64, 0, T, "fresh scene").any()
    c.write_expected(np.full(T, 4.0))
    c.write_variance(np.full(T, 1e6))
    got = check_counts(c, nn, np.full(T, 4.0), np.full(T, 1e6), 4, 0.1, 0.0, 64, 0, T, "before any gather")
    assert (got == 64).sum() == T - edge.no_area.size and not got[edge.no_area].any()
    c.reset(True)
    c.seed = 5
    c.gather_direct(frm, to, length, 4, SEED, N)
    pm0, mx0 = c.read_photon_map(0), c.read_photon_map(1)
    check_counts(c, nn, e0, v0, 16, 0.5, 0.0, 8, 3, 100, "another rule on a part")
    n1 = c.read_gather_extra()
    L = c._L
    offs = np.full(T + 1, -7, dtype=np.int32)
    prm = pkg.capi.RefineParams(0.1, 0.0, 64, RSEED)

    def raw(S0=4, p=prm, first=0, count=T, out=offs):
        return L.uvrt_refine_counts(c._h, S0, C.byref(p) if p is not None else None, first, count,
                                    out.ctypes.data_as(C.c_void_p) if out is not None else None)

    bad = [dict(S0=1), dict(S0=0), dict(S0=-4), dict(S0=4097), dict(first=-1), dict(first=1), dict(count=T + 1), dict(count=-1),
           dict(first=T, count=1), dict(p=None), dict(out=None)]
    for field, values in (("rel_error", (0.0, -0.25, float("nan"), float("inf"))), ("min_expected", (-1.0, float("nan"), float("inf"))),
                          ("max_extra", (0, 1, 3, 24, 8192, -16))):
        for val in values:
            p = pkg.capi.RefineParams(0.1, 0.0, 64, RSEED)
            setattr(p, field, val)
            bad.append(dict(p=p))
    reserved = pkg.capi.RefineParams(0.1, 0.0, 64, RSEED)
    reserved.reserved[0] = 1
    bad.append(dict(p=reserved))
    for kw in bad:
        assert raw(**kw) == -1 and b"uvrt_refine_counts" in L.uvrt_last_error(), kw
    assert L.uvrt_refine_counts(None, 4, C.byref(prm), 0, T, offs.ctypes.data_as(C.c_void_p)) == -1
    c.set_flavour(2)
    with pytest.raises(Err, match="error -1.*flavours 0 and 1"):
        c.refine_counts(4, 0.1, 64)
    c.set_flavour(0)
    assert np.all(offs == -7) and same(c.read_gather_extra(), n1)
    # what the refine refuses and the hook does not: the gather's own seed, a max_extra above the capacity (it stores no ray)
    c.resize_rays(8)
    check_counts(c, nn, e0, v0, 4, 0.1, 0.0, 64, 0, T, "seed and capacity")
    c.resize_rays(T * 64)
    assert c.refine_counts(4, 0.1, 64, seed=SEED)[-1] == int(n.sum())
    assert same(c.read_gather_extra(), n)
    # nothing else moved, and the gather is still there to refine
    assert same(c.read_expected(), e0) and same(c.read_variance(), v0) and c.seed == 5
    assert same(c.read_photon_map(0), pm0) and same(c.read_photon_map(1), mx0)
    assert c.gather_refine(0.1, 64, RSEED) == (int(n.sum()), int((n > 0).sum()))
    check_refined(c, e, v, n, "refine after the hook")
    # the hook needs no remembered gather: the refine has forgotten it
    with pytest.raises(Err, match="error -1.*no remembered gather"):
        c.gather_refine(0.1, 64, RSEED)
    check_counts(c, nn, e, v, 4, 0.1, 0.0, 64, 0, T, "after the refine")
    c.close()


@pytest.fixture(scope="module")
def boundary(orc):
    return ge.soup_scene(orc, ge.BOUNDARY_T)


def test_the_scan_where_a_range_meets_a_block(pkg, orc, boundary):
    """4200 triangles, seeded planes (a third of the rows want samples), the hook: ranges that are empty, one triangle, one
    short of a block of 1024 positions, a block, one more (the total opens a block of its own), two blocks, the scene"""
    T = boundary.T
    _, _, _, nn = gr.tri_normals(boundary.tris)
    assert not (nn == 0.0).any()
    E, V = ge.random_planes(T, 11)
    c = new_ctx(pkg, boundary, 64)
    c.write_expected(E)
    c.write_variance(V)
    for first, count in ((0, 0), (5, 1), (0, 1023), (3, 1023), (0, 1024), (1, 1024), (0, 1025), (7, 2047), (0, 2048), (0, T), (T - 1, 1)):
        n = check_counts(c, nn, E, V, 4, 0.25, 0.0, 64, first, count, "range (%d, %d)" % (first, count))
        if count >= 1023:
            assert 0.25 * count < (n > 0).sum() < 0.42 * count and set(n.tolist()) == {0, 2, 4, 8, 16, 32, 64}
            assert n[-8:].any(), "the last positions count"
    assert same(c.read_expected(), E) and same(c.read_variance(), V)
    c.close()


@pytest.mark.parametrize("first,count", [(1, 1024), (0, 1023)])
def test_a_refine_whose_total_sits_at_a_block_boundary(pkg, orc, boundary, first, count):
    """One real gather + refine (S0 = 2, tau = 0.5, at most 4 extra samples) of a range of 1024 triangles -- position 1024, the
    total that k_refine_generate's and k_refine_reduce's last triangle reads, is the only entry of the scan's second block --
    and of 1023, whose total is the last entry of the first block; chunks of at most 1000 rays"""
    rseed = ~BOUNDARY_SEED & 0xFFFFFFFF
    for name, mode in MODES:
        e, v, n, e0, v0 = gf.gather_and_refine(orc, boundary, ge.LAMP, ge.LAMP, 1.0, 2, BOUNDARY_SEED, N, mode, 0.5, 4, first=first, count=count)
        assert sorted(set(n.tolist())) == [0, 2, 4] and n[0] > 0 and n[-1] > 0 and n.sum() > 1000, name
        c = new_ctx(pkg, boundary, 1000, mode)
        c.gather_direct(ge.LAMP, ge.LAMP, 1.0, 2, BOUNDARY_SEED, N, first, count)
        assert c.gather_refine(0.5, 4, rseed, first_tri=first, tri_count=count) == (int(n.sum()), int((n > 0).sum())), name
        check_refined(c, e, v, n, "%s, range (%d, %d)" % (name, first, count), first)
        c.close()


def test_the_scan_carries_into_a_second_tile_of_block_sums(pkg, orc):
    """263 200 triangles, the hook only (no ray is traced at this size): k_refine_scan_sums scans 256 block sums per tile, so a
    range of more than 262 143 triangles needs the first tile's total in the second.  The whole scene; 262 143 triangles (256
    blocks exactly); 262 144 (the total alone in block 256); 262 145 from triangle 1055 on, which ends with the scene."""
    scene = ge.soup_scene(orc, ge.CARRY_T)
    T = scene.T
    _, _, _, nn = gr.tri_normals(scene.tris)
    assert not (nn == 0.0).any()
    E, V = ge.random_planes(T, 12)
    E[-8:], V[-8:] = 1.0, 1e6                           # the last triangles want the cap
    c = new_ctx(pkg, scene, 64)
    c.write_expected(E)
    c.write_variance(V)
    for first, count in ((0, T), (0, 262143), (0, 262144), (1055, 262145)):
        what = "range (%d, %d)" % (first, count)
        n = check_counts(c, nn, E, V, 4, 0.25, 0.0, 64, first, count, what)
        assert 0.3 * count < (n > 0).sum() < 0.37 * count, what
        assert n[:262144].sum() > 0 and (count <= 262144 or n[262144:].any()), what + ": a carry, and an n_t behind it"
    assert same(c.read_expected(), E) and same(c.read_variance(), V)
    c.close()
