"""GPU: mask classes -- one deposit per traced ray of a dedupe group (include/uvrt.h uvrt_set_dedupe_classes; csrc/uvrt_dedupe.h
"mask classes").

Every shape runs with dedupe off (the reference), with classes off (max_classes 0: the masks themselves, one deposit per
launch), with 1 and 4 classes (most rays keep their masks where the masks are many: both forms meet in one wave) and with the
default.  Each run traces the same batch four times on one context: batches 1 and 3 are folded (uvrt_read_batch_counts) and
then replayed, 2 and 4 are replayed straight from the planes; 3 and 4 reuse the buffer sets of 1 and 2, whose class planes must
have been zeroed where they were read.  Demanded: folded per-launch planes, f64 maps, dose and colour bit-identical to the
reference and to classes off; uvrt_batch_traced_rays unchanged; uvrt_batch_deposits equal to the figure of the host hook
(uvrt_dedupe_classes, held to brute force by tests/test_dedupe_classes_cpu.py) summed over the batch's groups."""
from types import SimpleNamespace

import numpy as np
import pytest

from test_gpu_dedupe import bits, bits64, env, oracle_counts  # noqa: F401 (env: a fixture)

pytestmark = pytest.mark.gpu

N = 4096
SETTINGS = (0, 1, 4, None)          # max_classes; None = the context's default


def make_ops(capi, count, n):
    ops = np.zeros(count, dtype=capi.REPLAY_OP_DT)
    for k in range(count):
        ops[k] = (5.0 + 7.0 * (k % 5), 1 if k in (count // 2, count - 1) else 0, 1 if k == count // 2 else 0, n * (k + 1), 44.0197,
                  100.0, k & 1)
    return ops


def new_ctx(env, scene, setting, flavour, mode):
    c = env["capi"].Ctx(0)
    c.set_scene(scene.tris, scene.nodes, scene.triIdx)
    c.set_flavour(flavour)
    c.set_seed_mode(mode)
    c.set_dedupe(setting != "no dedupe")
    if setting not in ("no dedupe", None):
        c.set_dedupe_classes(setting)
    c.reset(True)
    return c


def results(c):
    return {"sum": bits64(c.read_photon_map(0)).copy(), "max": bits64(c.read_photon_map(1)).copy(),
            "dose": bits(c.read_dosage()).copy(), "colour": bits(c.read_color()).copy()}


def run(env, scene, lamps, first, n, setting, flavour=0, mode=0, seed=0):
    c = new_ctx(env, scene, setting, flavour, mode)
    ops = make_ops(env["capi"], len(lamps), n)
    out = {"counts": []}
    try:
        for batch in range(4):
            c.seed = seed
            c.trace_batch(lamps, env["length"], first, n)
            if batch % 2 == 0:
                out["counts"].append([c.read_batch_counts(k) for k in range(len(lamps))])
            if batch == 0:
                out["traced"], out["deposits"] = c.batch_traced_rays(), c.batch_deposits()
            c.replay_batch(ops)
        out["seed"] = c.seed
        out.update(results(c))
    finally:
        c.close()
    return out


def groups_of(env, lamps, seed, mode):
    """the dedupe groups of a batch of stops: (lamp, seeds before, seeds after) per group, columns of more than 31 split evenly"""
    capi = env["capi"]
    cols = {}
    for lp in lamps:
        nxt = capi.seed_next(lp, env["length"], seed, mode)
        cols.setdefault(tuple(np.float32(lp).tolist()), []).append((seed, nxt))
        seed = nxt
    out = []
    for lp, chain in cols.items():
        if len(chain) < 2:
            continue
        pieces = (len(chain) + 30) // 31
        per = (len(chain) + pieces - 1) // pieces
        for k0 in range(0, len(chain), per):
            part = chain[k0:k0 + per]
            if len(part) >= 2:
                out.append((lp, [p[0] for p in part], [p[1] for p in part]))
    return out


def expected_deposits(env, lamps, first, n, setting, seed, mode):
    capi = env["capi"]
    mc = capi.dedupe_classes_default() if setting is None else setting
    return sum(capi.dedupe_classes(lp, prev, nxt, mode, first, n, mc)[1] for lp, prev, nxt in groups_of(env, lamps, seed, mode))


def check_shape(env, scene, lamps, first, n, flavour=0, mode=0, seed=0, oracle=False):
    ref = run(env, scene, lamps, first, n, "no dedupe", flavour, mode, seed)
    assert ref["traced"] == len(lamps) * n and ref["deposits"] == 0
    assert any(int(cn.sum()) > 0 for cn in ref["counts"][0]), "the shape hits nothing"
    if oracle:
        want = oracle_counts(env, lamps, first, n, flavour, mode, seed)
        for k in range(len(lamps)):
            assert np.array_equal(ref["counts"][0][k], want[k]), "launch %d differs from the oracle" % k
    off = None
    for setting in SETTINGS:
        got = run(env, scene, lamps, first, n, setting, flavour, mode, seed)
        for b in range(2):
            for k in range(len(lamps)):
                assert np.array_equal(got["counts"][b][k], ref["counts"][0][k]), "classes %r: launch %d, batch %d" % (setting, k, 1 + 2 * b)
        for what in ("sum", "max", "dose", "colour"):
            assert np.array_equal(got[what], ref[what]), "classes %r: %s differs from dedupe off" % (setting, what)
        assert got["seed"] == ref["seed"]
        if setting == 0:
            off = got
            assert got["deposits"] == sum(len(p) for _, p, _ in groups_of(env, lamps, seed, mode)) * n
        assert got["traced"] == off["traced"] <= len(lamps) * n
        assert got["deposits"] == expected_deposits(env, lamps, first, n, setting, seed, mode), "classes %r" % (setting,)
        assert off["traced"] <= got["deposits"] <= off["deposits"]
    return off


@pytest.mark.parametrize("first", [0, 1200000, 2000000])
def test_one_lamp_8_launches(env, first):
    """15 masks at gid 0, 46 at 2 000 000, where 1 and 4 classes leave most rays to the per-bit form"""
    off = check_shape(env, env["scene"], [env["lamps"][0]] * 8, first, N, oracle=True)
    assert off["traced"] < 8 * N


def test_two_launches(env):
    check_shape(env, env["scene"], [env["lamps"][0]] * 2, 1200000, N, oracle=True)


def test_column_of_33_launches(env):
    """17 + 16: two groups of one lamp column, each with classes of its own; n is no multiple of 64"""
    check_shape(env, env["scene"], [env["lamps"][0]] * 33, 1200000, 1000, oracle=True)


def test_group_of_31_launches_keeps_the_masks(env):
    """bit 30 of a ray's word is launch 30 there: no classes at any setting, every ray deposits once per launch that holds it"""
    lamps = [env["lamps"][0]] * 31
    off = check_shape(env, env["scene"], lamps, 1200000, 1000)
    assert off["deposits"] == 31 * 1000 == expected_deposits(env, lamps, 1200000, 1000, None, 0, 0)


def test_two_lamp_columns_share_the_class_planes(env):
    """A B A B ...: two groups of 5 launches, their class planes side by side behind the 10 launch planes"""
    a, b = env["lamps"]
    check_shape(env, env["scene"], [a, b] * 5, 1200000, N, oracle=True)


@pytest.mark.parametrize("flavour,mode,seed", [(1, 0, 0), (0, 1, 0x1234), (1, 1, 0x1234)])
def test_flavour_and_seed_mode(env, flavour, mode, seed):
    check_shape(env, env["scene"], [env["lamps"][0]] * 8, 1200000, N, flavour=flavour, mode=mode, seed=seed, oracle=(flavour, mode) != (1, 1))


def small_scenes(orc):
    tris3 = np.zeros((3, 16), dtype=np.float32)
    for t, (cx, cz) in enumerate(((0.0, 1.0), (1.0, 0.0), (-0.7, -0.7))):
        tris3[t, 0:3] = (cx + 0.4, -0.5, cz)
        tris3[t, 4:7] = (cx - 0.4, -0.3, cz + 0.3)
        tris3[t, 8:11] = (cx, -1.6, cz - 0.3)
    nodes3, idx3 = orc.build_bvh(tris3)
    tris2 = np.zeros((2, 16), dtype=np.float32)
    h, d, w = np.float32(-0.5), np.float32(1.0), np.float32(0.1)
    tris2[0, 0:3] = (w, h + w, d); tris2[0, 4:7] = (-w, h + w, d); tris2[0, 8:11] = (w, h - w, d)
    tris2[1, 0:3] = (-w, h - w, d); tris2[1, 4:7] = (-w, h + w, d); tris2[1, 8:11] = (w, h - w, d)
    nodes2 = np.zeros(1, dtype=orc.NODE_DT)
    nodes2[0]["leftFirst"] = 0
    nodes2[0]["triCount"] = 2
    return {"three triangles": SimpleNamespace(tris=tris3, nodes=nodes3, triIdx=idx3, T=3),
            "leaf root": SimpleNamespace(tris=tris2, nodes=nodes2, triIdx=np.array([0, 1], dtype=np.uint32), T=2)}


@pytest.mark.parametrize("which", ["three triangles", "leaf root"])
def test_small_scenes(env, which):
    """every deposit of a plane lands on two or three counters: the hottest a class plane's replicas can get"""
    scene = small_scenes(env["orc"])[which]
    lamp = (0.0, -1.0, 0.0)
    e = dict(env, scene=scene)
    check_shape(e, scene, [lamp] * 8, 2000000, 16384, oracle=True)


def test_two_contexts_over_ray_ranges(env):
    """uvrt_reduce_batch_group on one device: each context folds its own half -- launch planes and class planes -- before the
    sum, and both replay the whole"""
    capi, lamp, first, half = env["capi"], env["lamps"][0], 1200000, N // 2
    lamps = [lamp] * 8
    ops = make_ops(capi, 8, N)
    one = new_ctx(env, env["scene"], "no dedupe", 0, 0)
    try:
        one.trace_batch(lamps, env["length"], first, N)
        whole = [one.read_batch_counts(k) for k in range(8)]
        one.replay_batch(ops)
        want = results(one)
    finally:
        one.close()
    for setting in SETTINGS:
        a, b = new_ctx(env, env["scene"], setting, 0, 0), new_ctx(env, env["scene"], setting, 0, 0)
        try:
            for batch in range(3):          # the third batch meets the first one's buffer set again
                for c, lo in ((a, first), (b, first + half)):
                    c.reset(True)
                    c.seed = 0
                    c.trace_batch(lamps, env["length"], lo, half)
                dep = (a.batch_deposits(), b.batch_deposits())
                capi.reduce_batch_group([a, b])
                for c in (a, b):
                    for k in range(8):
                        assert np.array_equal(c.read_batch_counts(k), whole[k]), (setting, batch, k)
                    c.replay_batch(ops)
                    got = results(c)
                    for what in ("sum", "max", "dose", "colour"):
                        assert np.array_equal(got[what], want[what]), (setting, batch, what)
                assert dep[0] == expected_deposits(env, lamps, first, half, setting, 0, 0)
                assert dep[1] == expected_deposits(env, lamps, first + half, half, setting, 0, 0)
        finally:
            a.close()
            b.close()
