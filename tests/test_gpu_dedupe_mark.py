"""GPU: k_dedupe_mark, the owner test of a deduped chunk as one pass per key tile (csrc/uvrt_dedupe.h, csrc/uvrt_kernels.hip).

uvrt_dedupe_mark_device runs the kernel alone for a group and a chunk of its range: every occurrence's mask must equal
uvrt_dedupe_plan's (held to brute force by tests/test_dedupe_cpu.py), and the owners it adds up per launch and block of 2 048
gids -- what the scan pass turns into the compaction order -- must be the non-zero masks of that block.  The groups are those
of tests/test_dedupe_tiled_cpu.py.  One batch goes end to end through three chunks, twice in one context: the owner counters
must be zero again after every chunk."""
import numpy as np
import pytest

import dedupe_tiled_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def groups(pkg, orc, oscene, oroute):
    lamp0, length = cases.lamp0_of(orc, oscene, oroute)
    return {g.name: g for g in cases.groups(pkg.capi, lamp0, length)}


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.capi.Ctx(0)
    yield c
    c.close()


def block_owners(masks, block):
    K, n = masks.shape
    nb = (n + block - 1) // block
    padded = np.zeros((K, nb * block), dtype=bool)
    padded[:, :n] = masks != 0
    return padded.reshape(K, nb, block).sum(axis=2).astype(np.uint32)


@pytest.mark.parametrize("chunking", cases.CHUNKINGS)
@pytest.mark.parametrize("name", cases.NAMES)
def test_mark_gives_the_plans_masks_and_owner_counts(pkg, ctx, groups, name, chunking):
    capi, g = pkg.capi, groups[name]
    want = cases.plan(capi, g)
    parts = []
    for first, n in g.chunks()[chunking]:
        ref = want[:, first - g.first:first - g.first + n]
        for again in range(2):          # (the second run finds the counters as the first left them)
            masks, owners = ctx.dedupe_mark_device(*g.args(), chunk_first=first, chunk_n=n)
            assert np.array_equal(masks, ref), "a mask differs"
            assert np.array_equal(owners, block_owners(ref, capi.DEDUPE_BLOCK_GIDS)), "the owners of a block differ"
        parts.append(masks)
    if chunking == "meet":
        assert np.array_equal(np.concatenate(parts, axis=1), want)


def test_a_batch_through_three_chunks_twice(pkg, orc, oscene, oroute, monkeypatch):
    """8 x 20 000 from lamp 0 with 1 MB chunks: each launch's range is cut into three chunks (two lanes, so a lane's owner
    counters serve two chunks of one call); the per-launch counts equal dedupe off, the traced rays are the plan's owners,
    and the same call again in the same context gives the same bits"""
    monkeypatch.setenv("UVRT_BATCH_CHUNK_MB", "1")
    capi = pkg.capi
    lamp, length = cases.lamp0_of(orc, oscene, oroute)
    K, n, first = 8, 20000, 0
    prev, nxt = cases.seed_chain(capi, lamp, length, K, 0, 0)
    want = int((capi.dedupe_plan(lamp, prev, nxt, 0, first, n) != 0).sum())
    assert want < K * n
    got = {}
    for dedupe in (True, False):
        c = capi.Ctx(0)
        try:
            c.set_scene(oscene.tris, oscene.nodes, oscene.triIdx)
            c.set_dedupe(dedupe)
            c.reset(True)
            runs = []
            for again in range(2 if dedupe else 1):
                c.seed = 0
                c.trace_batch([lamp] * K, length, first, n)
                runs.append(([c.read_batch_counts(k) for k in range(K)], c.batch_traced_rays(), c.seed))
                c.replay_batch(np.zeros(K, dtype=capi.REPLAY_OP_DT))          # (the next batch wants this one replayed)
            got[dedupe] = runs
        finally:
            c.close()
    off_counts, off_traced, off_seed = got[False][0]
    assert off_traced == K * n
    for counts, traced, seed in got[True]:
        assert traced == want and seed == off_seed == nxt[-1]
        for k in range(K):
            assert np.array_equal(counts[k], off_counts[k]), "launch %d: dedupe on / off differ" % k
    assert sum(int(p.sum()) for p in off_counts) > 0.5 * K * n
