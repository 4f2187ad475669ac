"""GPU: the issue priority of the short kernels (include/uvrt.h uvrt_set_helper_priority; csrc/uvrt_device.h
helper_priority).

The level changes when the waves of generate, the dedupe passes, fold, replay, accumulate, Shade, reset and the per-launch
records issue beside a traversal grid, never what they compute: every count plane, map, dose and colour must be the same
bits at every level, and equal to the oracle where the oracle is consulted.  The setter refuses a level outside 0..3 and
leaves the old one; UVRT_HELPER_PRIO sets the level a new context starts with."""
import numpy as np
import pytest

import dedupe_tiled_cases as cases
from conftest import GLB, ROUTE

pytestmark = pytest.mark.gpu

UVRT_ERR_INVALID = -1
K8 = 8
N = 4096


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def bits64(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.fixture(scope="module")
def env(pkg, orc, oscene, oroute):
    lamp0, length = cases.lamp0_of(orc, oscene, oroute)
    comp = orc.Computation(oscene, oroute["lamps"], 1 << 16, oroute["lightHeight"], oroute["lightLength"], oroute["lightIntensity"])
    lamp5 = tuple(float(x) for x in comp.lamp_world_pos(oroute["lamps"][5]))
    return {"capi": pkg.capi, "orc": orc, "scene": oscene, "length": length, "lamp": lamp0, "lamp5": lamp5}


def new_ctx(env, prio=None, seed=0):
    """a context with the scene; prio None keeps the level the context starts with"""
    c = env["capi"].Ctx(0)
    s = env["scene"]
    c.set_scene(s.tris, s.nodes, s.triIdx)
    if prio is not None:
        c.set_helper_priority(prio)
    c.reset(True)
    c.seed = seed
    return c


_oracle = {}


def oracle_counts(env, first):
    """the oracle's per-launch counts of K8 launches x N gids from lamp 0 (computed once per first gid, read only)"""
    if first not in _oracle:
        orc, s, seed, out = env["orc"], env["scene"], 0, []
        for _ in range(K8):
            rays, seed = orc.generate(first, N, env["lamp"], env["length"], seed)
            temp = np.zeros(s.T, dtype=np.int32)
            orc.extend(temp, s.tris, rays, s.nodes, s.triIdx)
            temp.setflags(write=False)
            out.append(temp)
        _oracle[first] = out
    return _oracle[first]


@pytest.mark.parametrize("first", [0, 2000000])
def test_batch_counts_are_the_oracles_at_every_level(env, first):
    """first gid 0: work-item 0 reads the other SEED; 2 000 000: sums above 2^24 take even values only"""
    ref = oracle_counts(env, first)
    assert sum(int(r.sum()) for r in ref) > 0.5 * K8 * N
    traced = {}
    for prio in (0, 1, 3):
        c = new_ctx(env, prio)
        try:
            assert c.get_helper_priority() == prio
            c.trace_batch([env["lamp"]] * K8, env["length"], first, N)
            for k in range(K8):
                assert np.array_equal(c.read_batch_counts(k), ref[k]), "level %d, launch %d differs from the oracle" % (prio, k)
            traced[prio] = c.batch_traced_rays()
        finally:
            c.close()
    assert traced[0] == traced[1] == traced[3] < K8 * N


def three_batches(env, prio):
    """trace, replay, trace, replay, trace, replay on one context without a sync in between: from the second batch on the
    mark, scan and write passes of a chunk run while the previous batch's traversal is resident"""
    capi, n, first = env["capi"], 65536, 1200000
    ops = np.zeros(K8, dtype=capi.REPLAY_OP_DT)
    for k in range(K8):
        ops[k] = (10.0 + 5.0 * k, 1 if k in (3, 7) else 0, 1 if k == 3 else 0, n * (k + 1), 44.0197, 100.0, k & 1)
    c = new_ctx(env, prio)
    try:
        for _ in range(3):
            c.trace_batch([env["lamp"]] * K8, env["length"], first, n)
            c.replay_batch(ops)
        return (bits64(c.read_photon_map(0)), bits64(c.read_photon_map(1)), bits(c.read_dosage()), bits(c.read_color()), c.seed)
    finally:
        c.close()


def test_helpers_beside_a_traversal(env):
    a, b = three_batches(env, 0), three_batches(env, None)
    for got, want in zip(b[:4], a[:4]):
        assert np.array_equal(got, want)
    assert b[4] == a[4]
    assert a[0].any() and a[2].any()


def loop_mode(prio):
    from uvrt_amd import host
    rt = host.RayTracer(GLB, ROUTE, device=0)
    try:
        if prio is not None:
            rt.ctx.set_helper_priority(prio)
        rt.photonCount = 16384
        rt.ResetDosageMap()
        for _ in range(3):
            rt.ComputeDosageMap()
            rt.Shade()
        rt.Sync()
        return bits(rt.read_dosage()), bits(rt.ctx.read_color())
    finally:
        rt.close()


def test_loop_mode(pkg):
    """k_generate, k_accumulate_shade and k_reset: the host loop's launches rotate over the launch lanes"""
    a, b = loop_mode(0), loop_mode(None)
    assert np.array_equal(b[0], a[0]) and np.array_equal(b[1], a[1])
    assert a[0].any()


def test_a_sweep_in_a_batch(env):
    capi = env["capi"]
    launches = [capi.stop(env["lamp"]), capi.sweep(env["lamp"], env["lamp5"])]
    got = {}
    for prio in (0, 3):
        c = new_ctx(env, prio, seed=0x1234)
        try:
            c.trace_batch_launches(launches, env["length"], 1200000, N)
            got[prio] = [c.read_batch_counts(k) for k in range(2)]
        finally:
            c.close()
    for k in range(2):
        assert np.array_equal(got[3][k], got[0][k]), k
        assert got[0][k].sum() > 0.5 * N


@pytest.fixture(scope="module")
def groups(pkg, orc, oscene, oroute):
    lamp0, length = cases.lamp0_of(orc, oscene, oroute)
    return {g.name: g for g in cases.groups(pkg.capi, lamp0, length)}


@pytest.mark.parametrize("name", ["k8_first0", "ties_first9000000"])
def test_the_mark_hook_at_level_3(pkg, groups, name):
    capi, g = pkg.capi, groups[name]
    want = cases.plan(capi, g)
    block = capi.DEDUPE_BLOCK_GIDS
    nb = (g.n + block - 1) // block
    padded = np.zeros((g.K, nb * block), dtype=bool)
    padded[:, :g.n] = want != 0
    c = capi.Ctx(0)
    try:
        c.set_helper_priority(3)
        masks, owners = c.dedupe_mark_device(*g.args())
        assert np.array_equal(masks, want), "a mask differs"
        assert np.array_equal(owners, padded.reshape(g.K, nb, block).sum(axis=2).astype(np.uint32)), "the owners of a block differ"
    finally:
        c.close()


def test_the_setter_refuses_a_level_outside_0_to_3(pkg):
    c = pkg.capi.Ctx(0)
    try:
        c.set_helper_priority(2)
        for bad in (-1, 4):
            assert c._L.uvrt_set_helper_priority(c._h, bad) == UVRT_ERR_INVALID
            with pytest.raises(pkg.capi.UvrtError):
                c.set_helper_priority(bad)
            assert c.get_helper_priority() == 2
        for ok in (0, 1, 2, 3):
            c.set_helper_priority(ok)
            assert c.get_helper_priority() == ok
    finally:
        c.close()


def test_the_environment_sets_the_starting_level(pkg, monkeypatch):
    monkeypatch.setenv("UVRT_HELPER_PRIO", "2")
    c = pkg.capi.Ctx(0)
    try:
        assert c.get_helper_priority() == 2
    finally:
        c.close()
