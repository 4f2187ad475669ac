"""GPU: shadow rays (uvrt_occluded = k_occlude_free of csrc/uvrt_occlude.hip) against the oracle's extend with every ray's
`dist` preset to its tmax, every ray, flavours 0 and 1: uniform rays at several counts, the boundaries of tmax, hand-made rays
outside the packed division's proof conditions (also through the developer library's variant 500), and the isolation rules."""
import numpy as np
import pytest

import gather_restate as gr

pytestmark = pytest.mark.gpu

f32 = np.float32
MISS = f32(1e30)
# 98 299 rays: at 65 521 the unoccluded rays of seed 23 stop at 8 stack entries, the LDS rows; here they reach 10.  The
# other counts are prefixes of the same rays: a wave with one live lane, a full 64-ray batch less one, the batch, the batch
# plus one lane, one ray in a second workgroup's share, and an odd count over many workgroups.
COUNTS = (98299, 65521, 1, 63, 64, 65, 257, 4099)


def unit_dirs(rng, n):
    a = rng.normal(size=(n, 3))
    return (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)


def make_rays(orc, dirs, origins):
    r = np.zeros(len(dirs), dtype=orc.RAY_DT)
    d = np.asarray(dirs, dtype=np.float32)
    o = np.asarray(origins, dtype=np.float32)
    r["dirx"], r["diry"], r["dirz"] = d[:, 0], d[:, 1], d[:, 2]
    r["origx"], r["origy"], r["origz"] = o[:, 0], o[:, 1], o[:, 2]
    r["dist"] = MISS
    return r


def scene_bounds(oscene):
    v = oscene.tris[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]].reshape(-1, 3)
    return v.min(0), v.max(0)


def closest_hits(orc, oscene, rays, flavour):
    """the closest-hit distance of every ray (1e30f: none)"""
    o = rays.copy()
    o["dist"] = MISS
    o["triID"] = 0
    temp = np.zeros(oscene.T, dtype=np.int32)
    orc.set_flavour(flavour)
    try:
        orc.extend(temp, oscene.tris, o, oscene.nodes, oscene.triIdx)
    finally:
        orc.set_flavour(0)
    return o["dist"].copy()


def with_tmax(rays, tmax):
    r = rays.copy()
    r["dist"] = np.asarray(tmax, dtype=np.float32)
    return r


def scaled_tmax(hit, rng):
    """closest-hit distance x U(0.5, 1.5), 1e30f for a miss"""
    t = (hit * rng.uniform(0.5, 1.5, size=hit.size).astype(np.float32)).astype(np.float32)
    return np.where(hit == MISS, MISS, t).astype(np.float32)


def boundary_tmax(hit):
    """the tmax arrays of test_tmax_boundaries by name, for rays whose closest-hit distances are `hit`"""
    return {"exact": hit,
            "nextafter": np.nextafter(hit, f32(np.inf)).astype(np.float32),
            "small": np.resize(np.array([1e-4, 0.0, -0.0, -1.0, 5e-5, 1e-38, -1e30], dtype=np.float32), hit.size),
            "nan": np.full(hit.size, np.nan, dtype=np.float32),
            "1e30": np.full(hit.size, MISS)}


def uniform_shadow_rays(orc, oscene, n, seed, flavour):
    rng = np.random.default_rng(seed)
    lo, hi = scene_bounds(oscene)
    o = rng.uniform(lo, hi, size=(n, 3)).astype(np.float32)
    rays = make_rays(orc, unit_dirs(rng, n), o)
    hit = closest_hits(orc, oscene, rays, flavour)
    return with_tmax(rays, scaled_tmax(hit, rng)), hit


def adversarial_rays(orc, oscene):
    """The hand-made rays of tests/test_gpu_free_rays.py, rebuilt here: zero and +-0 direction components, origins on node
    planes and vertices, |d| > 1, |d| < 2^-60, origin components 1e-35, 2e9 and 0, NaN directions."""
    nodes = oscene.nodes
    inner = nodes[nodes["triCount"] == 0]
    rng = np.random.default_rng(3)
    lo, hi = scene_bounds(oscene)
    dirs, orgs = [], []
    axes = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    verts = oscene.tris[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]].reshape(-1, 3)
    for k in range(6000):
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
        if where == 0:
            nd = inner[rng.integers(min(inner.size, 400), size=3)]
            o = (nd["minx"][0], nd["maxy"][1], nd["minz"][2])
        elif where == 1:
            o[rng.integers(3)] = inner[("maxx", "miny", "maxz")[k % 3]][rng.integers(min(inner.size, 400))]
        elif where == 2:
            o = verts[rng.integers(verts.shape[0])]
        orgs.append(o)
    d1 = np.asarray(dirs, dtype=np.float32)
    o1 = np.asarray(orgs, dtype=np.float32)
    n = 4096
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


def new_ctx(pkg, oscene, cap, dev=False):
    c = pkg.capi.Ctx(0, dev=dev)
    c.set_scene(oscene.tris, oscene.nodes, oscene.triIdx)
    c.resize_rays(cap)
    return c


@pytest.fixture(scope="module")
def uniform(orc, oscene):
    """per flavour: (rays with tmax, closest-hit distances, the oracle's answer, its statistics on the unoccluded rays)"""
    out = {}
    for fl in (0, 1):
        rays, hit = uniform_shadow_rays(orc, oscene, COUNTS[0], 23, fl)
        want = gr.occluded(orc, oscene, rays, fl)
        st = {}
        gr.occluded(orc, oscene, rays[want == 0], fl, stats=st)
        out[fl] = (rays, hit, want, st)
    return out


def test_uniform_rays_equal_the_oracle(pkg, orc, oscene, uniform):
    """n = 98 299, 65 521 and the counts around a wave: every byte equals the oracle's; the unoccluded rays -- the ones that walk their
    whole tree -- take the stack beyond the LDS rows, so the overflow rows run."""
    for fl in (0, 1):
        rays, hit, want, st = uniform[fl]
        share = want.mean()
        print("flavour %d: %.3f occluded, deepest stack of the unoccluded rays %d" % (fl, share, st["max_stack"]))
        assert 0.2 < share < 0.5
        assert st["max_stack"] > 8, "the unoccluded rays must leave the LDS stack rows (PS6 = 8)"
        c = new_ctx(pkg, oscene, COUNTS[0])
        c.set_flavour(fl)
        for n in COUNTS:
            got = c.occluded(rays[:n])
            assert np.array_equal(got, want[:n]), "flavour %d n %d: %d bytes differ" % (fl, n, int((got != want[:n]).sum()))
        c.sync()            # (reports a traversal stack overflow)
        c.close()


def test_tmax_boundaries(pkg, orc, oscene, uniform):
    """tmax exactly the hit distance: no ray occluded (t < dist is strict); the next float above it: every hit ray occluded;
    tmax <= 1e-4f and NaN: never; 1e30f: every ray that hits anything.  The oracle agrees on every one."""
    for fl in (0, 1):
        rays, hit, _, _ = uniform[fl]
        rays, hit = rays[:16384], hit[:16384]
        is_hit = hit != MISS
        assert 0.3 * hit.size < is_hit.sum() < hit.size
        tm = boundary_tmax(hit)
        cases = [("exact", tm["exact"], lambda g: not g.any()),
                 ("nextafter", tm["nextafter"], lambda g: g[is_hit].all() and not g[~is_hit].any()),
                 ("small", tm["small"], lambda g: not g.any()),
                 ("nan", tm["nan"], lambda g: not g.any()),
                 ("1e30", tm["1e30"], lambda g: np.array_equal(g != 0, is_hit))]
        c = new_ctx(pkg, oscene, hit.size)
        c.set_flavour(fl)
        for name, tmax, holds in cases:
            r = with_tmax(rays, tmax)
            want = gr.occluded(orc, oscene, r, fl)
            got = c.occluded(r)
            assert holds(want), "oracle, flavour %d %s" % (fl, name)
            assert np.array_equal(got, want), "flavour %d %s" % (fl, name)
        c.close()


def test_adversarial_rays_equal_the_oracle(pkg, orc, oscene):
    """Rays outside the proof conditions take the IEEE-division step; variant 500 of the developer library (IEEE divisions
    everywhere) gives the same bytes."""
    rays0 = adversarial_rays(orc, oscene)
    for fl in (0, 1):
        hit = closest_hits(orc, oscene, rays0, fl)
        rays = with_tmax(rays0, scaled_tmax(hit, np.random.default_rng(5)))
        want = gr.occluded(orc, oscene, rays, fl)
        assert 0.05 * rays.size < want.sum() < 0.9 * rays.size
        for dev, variant in ((False, 0), (True, 0), (True, 500)):
            c = new_ctx(pkg, oscene, rays.size, dev=dev)
            c.set_flavour(fl)
            c.set_variant(variant)
            got = c.occluded(rays)
            c.close()
            assert np.array_equal(got, want), "flavour %d dev %s variant %d" % (fl, dev, variant)


def test_errors_and_isolation(pkg, orc, oscene, oroute, uniform):
    """tempPhotonMap and SEED are what they were; the last generate is dropped; the refusals."""
    n = 1 << 15
    rays, _, want, _ = uniform[0]
    comp = orc.Computation(oscene, oroute["lamps"], n, oroute["lightHeight"], oroute["lightLength"], oroute["lightIntensity"])
    lp = comp.lamp_world_pos(oroute["lamps"][0])

    def launch(c, shadow):
        c.seed = 0
        c.reset(True)
        c.generate(lp, oroute["lightLength"], 0, n)
        c.extend(n)
        if shadow:
            counts, seed = c.read_counts(), c.seed
            got = c.occluded(rays[:n])
            assert np.array_equal(got, want[:n])
            assert np.array_equal(c.read_counts(), counts) and c.seed == seed
            assert counts.sum() > 0.9 * n
            with pytest.raises(pkg.capi.UvrtError, match="last generate"):
                c.extend(n)
            with pytest.raises(pkg.capi.UvrtError, match="last generate"):
                c.read_rays(0, 1)
        c.accumulate(60.0)
        c.shade(0, n, 45.0, 100.0, 0)
        c.sync()
        return c.read_dosage(), c.read_photon_map(0), c.read_photon_map(1)

    fresh = new_ctx(pkg, oscene, n)
    plain = launch(fresh, False)
    fresh.close()
    c = new_ctx(pkg, oscene, n)
    mixed = launch(c, True)
    for a, b in zip(mixed, plain):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert plain[0].astype(np.float64).sum() > 0
    with pytest.raises(pkg.capi.UvrtError, match="capacity"):
        c.occluded(rays[:n + 1])
    c.set_flavour(2)
    with pytest.raises(pkg.capi.UvrtError, match="flavours 0 and 1"):
        c.occluded(rays[:64])
    c.set_flavour(0)
    L = pkg.capi.lib()
    out = np.zeros(4, dtype=np.uint8)
    assert L.uvrt_occluded(c._h, None, 4, out.ctypes.data) == -1
    assert L.uvrt_occluded(c._h, rays.ctypes.data, 4, None) == -1
    c.close()
    bare = pkg.capi.Ctx(0)
    with pytest.raises(pkg.capi.UvrtError, match="no scene"):
        bare.occluded(rays[:4])
    bare.close()
