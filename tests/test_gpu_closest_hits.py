"""GPU: closest hits (uvrt_closest_hits = k_closest_free of csrc/uvrt_indirect.hip) against the oracle's extend with every ray's
`dist` preset to its tmax and `triID` read back (tests/gather_indirect_restate.py), every ray, dist bits and triangle, flavours
0 and 1: the uniform rays of tests/test_gpu_shadow_rays.py at its counts, the boundaries of tmax, the hand-made rays outside
the packed division's proof conditions (also through the developer library's variant 500), and the isolation rules."""
import numpy as np
import pytest

import gather_indirect_restate as gi
import gather_restate as gr
import test_gpu_shadow_rays as sr

pytestmark = pytest.mark.gpu

f32 = np.float32
MISS = gi.MISS
COUNTS = sr.COUNTS


def same(got, want):
    return np.array_equal(gr.bits(got[0]), gr.bits(want[0])) and np.array_equal(got[1], want[1])


@pytest.fixture(scope="module")
def uniform(orc, oscene):
    """per flavour: (rays with tmax, closest-hit distances at tmax = 1e30f, the restated (dist, tri), the oracle's statistics)"""
    out = {}
    for fl in (0, 1):
        rays, hit = sr.uniform_shadow_rays(orc, oscene, COUNTS[0], 23, fl)
        st = {}
        want = gi.closest(orc, oscene, rays, fl, stats=st)
        out[fl] = (rays, hit, want, st)
    return out


def test_uniform_rays_equal_the_oracle(pkg, orc, oscene, uniform):
    """n = 98 299, 65 521 and the counts around a wave: every dist and every triangle equals the oracle's; the rays walk their
    whole tree, so the stack goes beyond the LDS rows and the overflow rows run."""
    for fl in (0, 1):
        rays, hit, want, st = uniform[fl]
        share = (want[1] >= 0).mean()
        print("flavour %d: %.3f hit below tmax, deepest stack %d" % (fl, share, st["max_stack"]))
        assert 0.2 < share < 0.5
        assert st["max_stack"] > 8, "the rays must leave the LDS stack rows (PS6 = 8)"
        assert np.array_equal(gr.bits(want[0][want[1] < 0]), gr.bits(rays["dist"][want[1] < 0]))
        c = sr.new_ctx(pkg, oscene, COUNTS[0])
        c.set_flavour(fl)
        for n in COUNTS:
            got = c.closest_hits(rays[:n])
            assert same(got, (want[0][:n], want[1][:n])), "flavour %d n %d: %d dists, %d triangles differ" % (
                fl, n, int((gr.bits(got[0]) != gr.bits(want[0][:n])).sum()), int((got[1] != want[1][:n]).sum()))
        c.sync()            # (reports a traversal stack overflow)
        c.close()


def test_tmax_boundaries(pkg, orc, oscene, uniform):
    """tmax exactly the hit distance: nothing accepted (t < dist is strict); the next float above it: the hit, at its distance;
    tmax <= 1e-4f and NaN: nothing, and dist comes back with tmax's bits; 1e30f: the closest hit itself."""
    for fl in (0, 1):
        rays, hit, _, _ = uniform[fl]
        rays, hit = rays[:16384], hit[:16384]
        is_hit = hit != MISS
        assert 0.3 * hit.size < is_hit.sum() < hit.size
        tm = sr.boundary_tmax(hit)
        none = lambda tm: (lambda d, t: np.all(t == -1) and np.array_equal(gr.bits(d), gr.bits(tm)))
        found = lambda d, t: np.array_equal(t >= 0, is_hit) and np.array_equal(gr.bits(d[is_hit]), gr.bits(hit[is_hit]))
        cases = [("exact", tm["exact"], none(tm["exact"])), ("nextafter", tm["nextafter"], found),
                 ("small", tm["small"], none(tm["small"])), ("nan", tm["nan"], none(tm["nan"])), ("1e30", tm["1e30"], found)]
        c = sr.new_ctx(pkg, oscene, hit.size)
        c.set_flavour(fl)
        for name, tmax, holds in cases:
            r = sr.with_tmax(rays, tmax)
            want = gi.closest(orc, oscene, r, fl)
            got = c.closest_hits(r)
            assert holds(*want), "oracle, flavour %d %s" % (fl, name)
            assert same(got, want), "flavour %d %s" % (fl, name)
        c.close()


def test_occluded_is_a_closest_hit(pkg, oscene, uniform):
    """k_occlude_free and k_closest_free are one traversal (csrc/uvrt_query.h): over 4096 uniform rays and the rays of
    test_tmax_boundaries (tmax NaN, 0 and the exact hit distance among them), occluded[i] == (tri[i] != -1) for every ray,
    GPU against GPU.  Exact: both answers come from testing the ray's final dist bits against its tmax bits.  The oracle's
    answer for the uniform rays holds both outcomes, so the equality is not a row of zeros."""
    for fl in (0, 1):
        rays, hit, want, _ = uniform[fl]
        accepted = want[1][:4096] >= 0
        assert 0.1 * 4096 < accepted.sum() < 0.9 * 4096, "flavour %d: the oracle must see both outcomes" % fl
        edge = [sr.with_tmax(rays[:16384], tm) for tm in sr.boundary_tmax(hit[:16384]).values()]
        r = np.concatenate([rays[:4096]] + edge)
        c = sr.new_ctx(pkg, oscene, r.size)
        c.set_flavour(fl)
        occ = c.occluded(r)
        tri = c.closest_hits(r)[1]
        c.sync()
        c.close()
        assert np.array_equal(occ[:4096] != 0, accepted), "flavour %d: the uniform rays against the oracle" % fl
        bad = (occ != 0) != (tri != -1)
        assert not bad.any(), "flavour %d: %d of %d rays, first %d" % (fl, int(bad.sum()), r.size, int(np.argmax(bad)))


def test_adversarial_rays_equal_the_oracle(pkg, orc, oscene):
    """Rays outside the proof conditions take the IEEE-division step; variant 500 of the developer library (IEEE divisions
    everywhere) gives the same bits."""
    rays0 = sr.adversarial_rays(orc, oscene)
    for fl in (0, 1):
        hit = sr.closest_hits(orc, oscene, rays0, fl)
        for rays in (rays0, sr.with_tmax(rays0, sr.scaled_tmax(hit, np.random.default_rng(5)))):
            want = gi.closest(orc, oscene, rays, fl)
            assert 0.05 * rays.size < (want[1] >= 0).sum() < (0.9 if rays is not rays0 else 1.0) * rays.size
            for dev, variant in ((False, 0), (True, 0), (True, 500)):
                c = sr.new_ctx(pkg, oscene, rays.size, dev=dev)
                c.set_flavour(fl)
                c.set_variant(variant)
                got = c.closest_hits(rays)
                c.close()
                assert same(got, want), "flavour %d dev %s variant %d" % (fl, dev, variant)


def test_errors_and_isolation(pkg, orc, oscene, oroute, uniform):
    """tempPhotonMap, SEED and the dose of the launch around the call are what they were; the last generate is dropped; the
    refusals."""
    n = 1 << 15
    rays, _, want, _ = uniform[0]
    comp = orc.Computation(oscene, oroute["lamps"], n, oroute["lightHeight"], oroute["lightLength"], oroute["lightIntensity"])
    lp = comp.lamp_world_pos(oroute["lamps"][0])

    def launch(c, closest):
        c.seed = 0
        c.reset(True)
        c.generate(lp, oroute["lightLength"], 0, n)
        c.extend(n)
        if closest:
            counts, seed = c.read_counts(), c.seed
            got = c.closest_hits(rays[:n])
            assert same(got, (want[0][:n], want[1][:n]))
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

    fresh = sr.new_ctx(pkg, oscene, n)
    plain = launch(fresh, False)
    fresh.close()
    c = sr.new_ctx(pkg, oscene, n)
    mixed = launch(c, True)
    for a, b in zip(mixed, plain):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert plain[0].astype(np.float64).sum() > 0
    with pytest.raises(pkg.capi.UvrtError, match="capacity"):
        c.closest_hits(rays[:n + 1])
    c.set_flavour(2)
    with pytest.raises(pkg.capi.UvrtError, match="flavours 0 and 1"):
        c.closest_hits(rays[:64])
    c.set_flavour(0)
    L = pkg.capi.lib()
    d, t = np.zeros(4, dtype=np.float32), np.zeros(4, dtype=np.int32)
    assert L.uvrt_closest_hits(c._h, None, 4, d.ctypes.data, t.ctypes.data) == -1
    assert L.uvrt_closest_hits(c._h, rays.ctypes.data, 4, None, t.ctypes.data) == -1
    assert L.uvrt_closest_hits(c._h, rays.ctypes.data, 4, d.ctypes.data, None) == -1
    assert c.closest_hits(rays[:0])[0].size == 0
    c.close()
    bare = pkg.capi.Ctx(0)
    with pytest.raises(pkg.capi.UvrtError, match="no scene"):
        bare.closest_hits(rays[:4])
    bare.close()
