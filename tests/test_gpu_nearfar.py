"""GPU: the sign-ordered near / far block of k_extend6's hand-written stream (uvrt_extend6.hip R7_ENTER_BOX_SIGN /
R7_NEARFAR_SIGN: flavours 0 and 1 exchange the two slab numerators of a pair in the lanes whose direction component is
negative and drop the twelve v_min_f32 / v_max_f32 of the box block) against its two in-process checkers, ray by ray and
with no tolerance:

  * the developer library's stream with the min/max block (UVRT_NEARFAR_MINMAX=1, read at uvrt_create) -- the stream of
    before, instruction for instruction after the slabs;
  * the developer library's step7 form of the loop (variant 400: leaf period 1, compiled C++ with box2_fast's min/max);
  * the developer library's own copy of the sign-ordered stream (both blocks live in one asm statement there).

Compared: the bits of every ray's hit distance, every ray's triangle id, and the whole count vector."""
import numpy as np
import pytest

from test_gpu_adversarial import make_rays
from test_gpu_fuzz import random_scene

pytestmark = pytest.mark.gpu

ROOM_RAYS = 1920 * 1080        # 2 073 600: one launch of the bench's headline


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class Streams:
    """the product stream and its checkers: (name, context, variant)"""

    def __init__(self, pkg, monkeypatch, drain_merge=None):
        if drain_merge is not None:
            monkeypatch.setenv("UVRT_DRAIN_MERGE", drain_merge)
        self.ctxs = []
        try:
            monkeypatch.delenv("UVRT_NEARFAR_MINMAX", raising=False)
            prod = self._make(pkg, False)
            dev = self._make(pkg, True)
            monkeypatch.setenv("UVRT_NEARFAR_MINMAX", "1")
            dev_mm = self._make(pkg, True)
        except Exception:
            self.close()
            raise
        finally:
            monkeypatch.delenv("UVRT_NEARFAR_MINMAX", raising=False)
            if drain_merge is not None:
                monkeypatch.delenv("UVRT_DRAIN_MERGE", raising=False)
        self.cells = [("product", prod, 0), ("dev min/max stream", dev_mm, 0), ("dev step7", dev, 400), ("dev sign stream", dev, 0)]

    def _make(self, pkg, dev):
        c = pkg.capi.Ctx(0, dev=dev)
        self.ctxs.append(c)
        return c

    def set_scene(self, tris, nodes, idx):
        for c in self.ctxs:
            c.set_scene(tris, nodes, idx)

    def trace(self, flavour, n, feed, what):
        """feed(ctx) puts n rays into the context; returns the product's (dist bits, triID, counts) after comparing all"""
        first = None
        for name, c, variant in self.cells:
            c.set_flavour(flavour)
            c.set_variant(variant)
            c.set_sort_bits(0)
            c.set_record_hits(True)
            c.resize_rays(n)
            c.reset(False)
            feed(c)
            c.extend(n)
            c.sync()
            got = c.read_rays(0, n)
            res = (bits(got["dist"]).copy(), np.array(got["triID"]), c.read_counts())
            if first is None:
                first = res
                continue
            for field, a, b in zip(("dist bits", "triID", "counts"), first, res):
                bad = np.flatnonzero(a != b)
                assert bad.size == 0, "%s: product != %s in %s at %d places, first %s" % (what, name, field, bad.size, bad[:5])
        return first

    def close(self):
        for c in self.ctxs:
            c.close()
        self.ctxs = []


@pytest.fixture
def streams(pkg, monkeypatch):
    s = Streams(pkg, monkeypatch)
    yield s
    s.close()


def lamp_pos(orc, oscene, oroute, k):
    comp = orc.Computation(oscene, oroute["lamps"], 1 << 16, oroute["lightHeight"], oroute["lightLength"], oroute["lightIntensity"])
    return tuple(float(x) for x in comp.lamp_world_pos(oroute["lamps"][k]))


@pytest.mark.parametrize("flavour", [0, 1])
@pytest.mark.parametrize("lamp", [0, 3, 5])
def test_room_launch_of_the_headline_size(streams, orc, oscene, oroute, lamp, flavour):
    streams.set_scene(oscene.tris, oscene.nodes, oscene.triIdx)
    lp = lamp_pos(orc, oscene, oroute, lamp)

    def feed(c):
        c.seed = 0
        c.generate(lp, oroute["lightLength"], 0, ROOM_RAYS)

    dist, tri, counts = streams.trace(flavour, ROOM_RAYS, feed, "room lamp %d flavour %d" % (lamp, flavour))
    assert counts.sum() > 0.5 * ROOM_RAYS and int(counts.sum()) == int((dist != bits(np.float32(1e30))).sum())


@pytest.mark.parametrize("case", range(24))
def test_seeded_fuzz_scenes(streams, orc, case):
    rng = np.random.default_rng(7000 + case)
    tris, extent = random_scene(rng)
    nodes, idx = orc.build_bvh(tris)
    streams.set_scene(tris, nodes, idx)
    for launch in range(3):
        flavour = int(rng.integers(0, 2))
        n = int(rng.choice([1, 63, 65, 1000, 20001, 70000, 300000]))
        lp = tuple(float(np.float32(v)) for v in rng.uniform(-0.6 * extent, 0.6 * extent, 3))
        length = float(np.float32(rng.choice([0.0, 0.5, 2.0]) * extent))
        seed = int(rng.integers(0, 2 ** 32))

        def feed(c):
            c.seed = seed
            c.generate(lp, length, 0, n)

        streams.trace(flavour, n, feed, "fuzz case %d launch %d (T %d, n %d, flavour %d)" % (case, launch, tris.shape[0], n, flavour))


def adversarial_scene(orc, rng):
    """A caller's BVH with inverted boxes (min and max exchanged on some axes of some nodes: extend.cl's min/max take the same
    two slab distances either way) and flat ones (axis-parallel triangles, and a quarter of the leaf boxes flattened on one axis:
    min == max there).  Whatever the boxes bound, extend.cl's walk over them is defined, and every stream must take it."""
    T = 3000
    tris = np.zeros((T, 16), dtype=np.float32)
    ctr = rng.uniform(-2.0, 2.0, (T, 1, 3))
    v = ctr + rng.normal(scale=0.15, size=(T, 3, 3))
    for axis in range(3):                                  # a third of the triangles lie in a plane of a grid: flat leaf boxes
        sel = np.arange(T) % 9 == axis
        v[sel, :, axis] = np.round(ctr[sel, :, axis] * 2.0) / 2.0
    tris[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]] = v.reshape(T, 9).astype(np.float32)
    nodes, idx = orc.build_bvh(tris)
    nodes = nodes.copy()
    leaves = np.flatnonzero(nodes["triCount"] > 0)
    for a, some in zip("xyz", np.array_split(rng.permutation(leaves)[:leaves.size // 4], 3)):
        nodes["max" + a][some] = nodes["min" + a][some]            # and leaf boxes flattened by the caller
    flat = sum(int((nodes["min" + a] == nodes["max" + a]).sum()) for a in "xyz")
    assert flat > 50
    inverted = 0
    for a in "xyz":
        sel = (rng.random(nodes.size) < 0.3) & (nodes["min" + a] != nodes["max" + a])
        lo, hi = nodes["min" + a][sel].copy(), nodes["max" + a][sel].copy()
        nodes["min" + a][sel], nodes["max" + a][sel] = hi, lo
        inverted += int(sel.sum())
    assert inverted > 100
    return tris, nodes, idx


def adversarial_rays(rng, n, origin):
    """ordinary unit directions with a special one in about every sixtieth lane, so that special and ordinary lanes share some
    waves and other waves stay in the stream: +0 / -0 / tiny / subnormal components and directions longer than 1"""
    a = rng.normal(size=(n, 3))
    d = (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)
    kind = rng.integers(0, 400, n)
    axis = rng.integers(0, 3, n)
    rows = np.arange(n)
    for k, value in ((0, np.float32(0.0)), (1, np.float32(-0.0)), (2, np.float32(1e-30)), (3, np.float32(-3e-39)), (4, np.float32(-1e-20))):
        sel = kind == k
        d[rows[sel], axis[sel]] = value
    d[kind == 5] *= np.float32(2.5)
    d[kind == 6] *= np.float32(-1.0000001)
    return make_rays(d, origin, rng.uniform(-1.5, 1.5, n))


@pytest.mark.parametrize("flavour", [0, 1])
def test_inverted_and_flat_boxes_with_special_lanes_among_ordinary_ones(pkg, orc, monkeypatch, flavour):
    """... and launches of every size down to less than one ray per wave with the drain merge forced on, which moves the last
    rays of four waves into the lanes of one.  The oracle (extend.cl restated) is compared as well."""
    rng = np.random.default_rng(99 + flavour)
    tris, nodes, idx = adversarial_scene(orc, rng)
    s = Streams(pkg, monkeypatch, drain_merge="1")
    orc.set_flavour(flavour)
    try:
        s.set_scene(tris, nodes, idx)
        for n, origin in ((200000, (0.1234, -0.4321)), (70000, (0.0, 0.0)), (4097, (-1.7, 0.9)), (700, (0.5, 0.25)), (65, (0.0, 1.0))):
            rays = adversarial_rays(rng, n, origin)
            dist, tri, counts = s.trace(flavour, n, lambda c: c.write_rays(rays), "adversarial n %d flavour %d" % (n, flavour))
            o_rays = rays.copy()
            temp = np.zeros(tris.shape[0], dtype=np.int32)
            st = orc.extend(temp, tris, o_rays, nodes, idx)
            assert n < 4097 or st["hits"] > 0.2 * n
            assert np.array_equal(dist, bits(o_rays["dist"])) and np.array_equal(tri, o_rays["triID"]) and np.array_equal(counts, temp)
    finally:
        orc.set_flavour(0)
        s.close()
