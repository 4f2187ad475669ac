"""GPU: rays with origins of their own (uvrt_write_free_rays -> uvrt_extend = the free-origin kernel of
csrc/uvrt_extend_free.hip) against the oracle's generic extend, bit for bit over ALL rays and triangles, in flavours 0 and
1: uniform rays, rays that start on the geometry, the lamp's own rays through both kernels, hand-made rays outside the
packed division's proof conditions, the reference's own extend.cl as a second checker, and the error / isolation rules."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def unit_dirs(rng, n):
    a = rng.normal(size=(n, 3))
    return (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)


def make_rays(orc, dirs, origins):
    r = np.zeros(len(dirs), dtype=orc.RAY_DT)
    d = np.asarray(dirs, dtype=np.float32)
    o = np.asarray(origins, dtype=np.float32)
    r["dirx"], r["diry"], r["dirz"] = d[:, 0], d[:, 1], d[:, 2]
    r["origx"], r["origy"], r["origz"] = o[:, 0], o[:, 1], o[:, 2]
    r["dist"] = np.float32(1e30)
    return r


def scene_bounds(oscene):
    v = oscene.tris[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]].reshape(-1, 3)
    return v.min(0), v.max(0)


def uniform_rays(orc, oscene, n, seed):
    rng = np.random.default_rng(seed)
    lo, hi = scene_bounds(oscene)
    o = rng.uniform(lo, hi, size=(n, 3)).astype(np.float32)
    return make_rays(orc, unit_dirs(rng, n), o)


def oracle_extend(orc, oscene, rays, flavour):
    o = rays.copy()
    o["dist"] = np.float32(1e30)
    o["triID"] = 0
    temp = np.zeros(oscene.T, dtype=np.int32)
    orc.set_flavour(flavour)
    try:
        st = orc.extend(temp, oscene.tris, o, oscene.nodes, oscene.triIdx)
    finally:
        orc.set_flavour(0)
    return o, temp, st


def new_ctx(pkg, oscene, cap, dev=False):
    c = pkg.capi.Ctx(0, dev=dev)
    c.set_scene(oscene.tris, oscene.nodes, oscene.triIdx)
    c.resize_rays(cap)
    return c


def trace_free(c, rays, record=True):
    c.set_record_hits(record)
    c.reset(False)
    c.write_free_rays(rays)
    c.extend(rays.size)
    c.sync()
    got = c.read_rays(0, rays.size) if record else None
    return got, c.read_counts()


def assert_same(got, counts, o_rays, o_counts, what):
    assert np.array_equal(bits(got["dist"]), bits(o_rays["dist"])), what
    assert np.array_equal(got["triID"], o_rays["triID"]), what
    assert np.array_equal(counts, o_counts), what
    for f in ("dirx", "diry", "dirz", "origx", "origy", "origz"):      # the read-back keeps every ray's own origin
        assert np.array_equal(bits(got[f]), bits(o_rays[f])), what + " " + f


@pytest.fixture(scope="module")
def uniform(orc, oscene):
    return uniform_rays(orc, oscene, 1 << 20, 11)


def test_uniform_rays_equal_the_oracle(pkg, orc, oscene, uniform):
    """2^20 rays, origins uniform in the bounds, directions uniform on the sphere: every (dist bits, triID) and every count,
    flavours 0 and 1, launch pipelining on and off, with and without hit records."""
    rays = uniform
    for fl in (0, 1):
        o_rays, o_counts, st = oracle_extend(orc, oscene, rays, fl)
        print("flavour %d: hit share %.3f, deepest stack %s" % (fl, st["hits"] / rays.size, st.get("max_stack")))
        assert 0.3 * rays.size < st["hits"] < 0.9 * rays.size          # both deposit branches run
        for pipe in (True, False):
            c = new_ctx(pkg, oscene, rays.size)
            c.set_flavour(fl)
            c.set_pipeline(pipe)
            got, counts = trace_free(c, rays)
            assert_same(got, counts, o_rays, o_counts, "flavour %d pipeline %s" % (fl, pipe))
            _, counts = trace_free(c, rays, record=False)
            assert np.array_equal(counts, o_counts), "flavour %d pipeline %s, no hit records" % (fl, pipe)
            c.close()


def test_rays_from_hit_points_equal_the_oracle(pkg, orc, oscene, uniform):
    """Second-bounce rays: origins o + d * dist (f32) of a first pass, new directions.  They lie on triangles and on
    leaf-box planes: t > 0.0001f and zero numerators decide."""
    first, _, _ = oracle_extend(orc, oscene, uniform, 0)
    hit = first["dist"] != np.float32(1e30)
    h = first[hit]
    o = np.stack([h["origx"] + h["dirx"] * h["dist"], h["origy"] + h["diry"] * h["dist"],
                  h["origz"] + h["dirz"] * h["dist"]], axis=1).astype(np.float32)
    rays = make_rays(orc, unit_dirs(np.random.default_rng(12), o.shape[0]), o)
    for fl in (0, 1):
        o_rays, o_counts, st = oracle_extend(orc, oscene, rays, fl)
        assert 0.2 * rays.size < st["hits"] < 0.9 * rays.size
        for pipe in (True, False):
            c = new_ctx(pkg, oscene, rays.size)
            c.set_flavour(fl)
            c.set_pipeline(pipe)
            got, counts = trace_free(c, rays)
            assert_same(got, counts, o_rays, o_counts, "flavour %d pipeline %s" % (fl, pipe))
            c.close()


def test_lamp_rays_through_both_kernels(pkg, orc, oscene, oroute):
    """The rays of uvrt_generate read back and written as free rays: hits and counts equal the fixed-lamp kernel's."""
    n = 1 << 18
    comp = orc.Computation(oscene, oroute["lamps"], n, oroute["lightHeight"], oroute["lightLength"], oroute["lightIntensity"])
    lp = comp.lamp_world_pos(oroute["lamps"][0])
    for fl in (0, 1):
        c = new_ctx(pkg, oscene, n)
        c.set_flavour(fl)
        c.set_record_hits(True)
        c.reset(False)
        c.generate(lp, oroute["lightLength"], 0, n)
        c.extend(n)
        c.sync()
        lamp = c.read_rays(0, n)
        lamp_counts = c.read_counts()
        rays = lamp.copy()
        rays["dist"] = np.float32(1e30)
        rays["triID"] = 0
        got, counts = trace_free(c, rays)
        c.close()
        assert (lamp["dist"] != np.float32(1e30)).sum() > 0.9 * n
        assert_same(got, counts, lamp, lamp_counts, "flavour %d" % fl)


def adversarial_rays(orc, oscene):
    """The generators of tests/test_gpu_adversarial.py with an origin per ray."""
    nodes = oscene.nodes
    inner = nodes[nodes["triCount"] == 0]
    rng = np.random.default_rng(3)
    lo, hi = scene_bounds(oscene)
    dirs, orgs = [], []
    axes = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    verts = oscene.tris[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]].reshape(-1, 3)
    for k in range(6000):                      # zero and +-0 direction components; origins on node planes and vertices
        kind = k % 6
        if kind == 0:
            d = axes[rng.integers(6)]
        elif kind == 1:
            a = rng.normal(size=3); a[rng.integers(3)] = 0.0; d = a / np.linalg.norm(a)
        elif kind == 2:
            a = rng.normal(size=3); a[rng.integers(3)] = -0.0; d = a / np.linalg.norm(a)
        elif kind == 3:
            a = rng.normal(size=3); d = a / np.linalg.norm(a)
        elif kind == 4:
            a = rng.normal(size=3); a[1] = 0.0; d = a / np.linalg.norm(a)
        else:
            d = (0.0, rng.choice([-1.0, 1.0]), 0.0)
        dirs.append(d)
        o = rng.uniform(lo, hi)
        where = k % 4
        if where == 0:                         # every component on a plane of some inner node's box
            nd = inner[rng.integers(min(inner.size, 400), size=3)]
            o = (nd["minx"][0], nd["maxy"][1], nd["minz"][2])
        elif where == 1:                       # one component on a plane
            o[rng.integers(3)] = inner[("maxx", "miny", "maxz")[k % 3]][rng.integers(min(inner.size, 400))]
        elif where == 2:                       # a vertex
            o = verts[rng.integers(verts.shape[0])]
        orgs.append(o)
    d1 = np.asarray(dirs, dtype=np.float32)
    o1 = np.asarray(orgs, dtype=np.float32)
    n = 4096                                   # |d| > 1, |d| < 2^-60, origin components 1e-35, 2e9 and 0, a NaN direction
    d2 = unit_dirs(rng, n)
    d2[0::7] *= np.float32(3.5)
    d2[1::7, 0] = np.float32(1e-41)
    d2[2::7, 2] = np.float32(-3e-39)
    d2[3::7, 1] = np.float32(1e-30)
    d2[4::7, rng.integers(3)] = np.float32(2.0 ** -70)
    o2 = rng.uniform(lo, hi, size=(n, 3)).astype(np.float32)
    for j, val in enumerate((1e-35, 2e9, 0.0, -1e-35, -0.0, 2.0 ** -120)):
        o2[5 + j::41, j % 3] = np.float32(val)
    o2[9::53] = np.float32(0.0)
    d2[10::97, 0] = np.float32(np.nan)
    d2[11::389] = np.float32(np.nan)
    return make_rays(orc, np.concatenate([d1, d2]), np.concatenate([o1, o2]))


def test_adversarial_rays_equal_the_oracle(pkg, orc, oscene):
    """Rays outside the packed division's proof conditions take the IEEE-division step; the result equals the oracle, and
    variant 500 of the developer library (IEEE divisions everywhere) gives the same bits."""
    rays = adversarial_rays(orc, oscene)
    for fl in (0, 1):
        o_rays, o_counts, st = oracle_extend(orc, oscene, rays, fl)
        assert st["hits"] > 0.2 * rays.size
        for dev, variant in ((False, 0), (True, 0), (True, 500)):
            c = new_ctx(pkg, oscene, rays.size, dev=dev)
            c.set_flavour(fl)
            c.set_variant(variant)
            got, counts = trace_free(c, rays)
            c.close()
            assert_same(got, counts, o_rays, o_counts, "flavour %d dev %s variant %d" % (fl, dev, variant))


def test_exact_step_everywhere_equals_the_fast_step(pkg, orc, oscene, uniform):
    """variant 500 on ordinary rays: the IEEE-division step and the packed one agree on every ray"""
    rays = uniform[:1 << 18]
    o_rays, o_counts, _ = oracle_extend(orc, oscene, rays, 0)
    c = new_ctx(pkg, oscene, rays.size, dev=True)
    c.set_variant(500)
    got, counts = trace_free(c, rays)
    c.close()
    assert_same(got, counts, o_rays, o_counts, "variant 500")


def test_reference_extend_kernel_agrees_on_free_rays(pkg, orc, oscene, uniform):
    """Second checker: the reference's own extend.cl, compiled unmodified for gfx950, on the uniform rays; flavour 1 is its
    arithmetic."""
    if orc.refgpu() is None:
        pytest.skip("oracle/_ref/*.co not built (needs /root/reference at build time)")
    rays = uniform
    ref_rays = rays.copy()
    ref_counts, ms = orc.refgpu_extend(ref_rays, oscene.tris, oscene.nodes, oscene.triIdx)
    print("reference extend.cl on gfx950: %.3f ms for %d free rays" % (ms, rays.size))
    c = new_ctx(pkg, oscene, rays.size)
    c.set_flavour(1)
    got, counts = trace_free(c, rays)
    c.close()
    assert_same(got, counts, ref_rays, ref_counts, "flavour 1 against extend.cl")


def test_errors_and_isolation(pkg, orc, oscene, oroute):
    n = 1 << 16
    rays = uniform_rays(orc, oscene, n, 21)
    comp = orc.Computation(oscene, oroute["lamps"], n, oroute["lightHeight"], oroute["lightLength"], oroute["lightIntensity"])
    lp = comp.lamp_world_pos(oroute["lamps"][0])
    lp1 = comp.lamp_world_pos(oroute["lamps"][1])

    def plain(c):                        # generate / extend / accumulate / shade from SEED 0
        c.seed = 0
        c.reset(True)
        c.generate(lp, oroute["lightLength"], 0, n)
        c.extend(n)
        c.accumulate(60.0)
        c.shade(0, n, 45.0, 100.0, 0)
        c.sync()
        return c.read_dosage(), c.read_photon_map(0), c.read_color()

    fresh = new_ctx(pkg, oscene, n)
    want = plain(fresh)
    fresh.close()
    c = new_ctx(pkg, oscene, n)
    with pytest.raises(pkg.capi.UvrtError, match="capacity"):
        c.write_free_rays(uniform_rays(orc, oscene, n + 64, 22))
    with pytest.raises(pkg.capi.UvrtError, match="capacity"):
        c.generate_sweep(lp, lp1, oroute["lightLength"], 0, n + 64)
    c.write_free_rays(rays)
    c.set_flavour(2)
    with pytest.raises(pkg.capi.UvrtError, match="flavours 0 and 1"):
        c.extend(n)
    c.set_flavour(0)
    c.set_seed_mode(1)
    with pytest.raises(pkg.capi.UvrtError, match="seed mode"):
        c.generate_sweep(lp, lp1, oroute["lightLength"], 0, n)
    c.set_seed_mode(0)
    with pytest.raises(pkg.capi.UvrtError, match="different orig"):
        c.write_rays(rays)
    # a free launch and a sweep, with the walk / ordering knobs that free rays ignore, then the plain sequence again
    c.set_wide_bvh(True)
    c.set_sort_bits(8)
    o_rays, o_counts, _ = oracle_extend(orc, oscene, rays, 0)
    got, counts = trace_free(c, rays)
    assert_same(got, counts, o_rays, o_counts, "wide walk / sort bits set")
    c.set_record_hits(False)
    c.set_wide_bvh(False)
    c.set_sort_bits(0)
    c.generate_sweep(lp, lp1, oroute["lightLength"], 0, n)
    c.extend(n)
    c.accumulate(3.0)
    got = plain(c)
    c.close()
    for a, b in zip(got, want):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert want[0].astype(np.float64).sum() > 0
