"""GPU: the generate of a deduped chunk (csrc/uvrt_kernels.hip k_dedupe_mark, k_dedupe_scan, k_dedupe_write; DESIGN.md
section 15): the mark pass walks strips of narrow key tiles with one wave each and carries the run bounds from tile to tile;
the scan turns its owner counts into the workgroups' first slots and the write pass leaves the counts zero for the lane's
next chunk.

* Mark against the definition: uvrt_dedupe_mark_device's masks and owners per launch and block of 2 048 gids against
  uvrt_dedupe_plan (held to brute force by tests/test_dedupe_cpu.py), for the groups of tests/dedupe_tiled_cases.py through a
  chunk that starts and ends inside a tile and inside a block, and for those of tests/dedupe_strip_cases.py (31 launches, the
  ties over 4 096 gids, keys that straddle 2^24 and 2^25, a launch without an owner) through every chunking.
* Strip seams: the occurrences whose keys lie next to a tile's or a strip's first key, on both sides of it.
* The owner counts from chunk to chunk: batches of many, few, many blocks per chunk in one context, with and without
  pipelining (without it every chunk runs on lane 0) and with chunks small enough for several per call: traced rays = the
  plan's owners, the dose equal to dedupe off bit for bit, no residue after a replay.
* A launch with no owner in a chunk.  Where SEED >> 15 of a later launch differs from an earlier one's by a multiple of 17,
  below 2^24 the later launch's key at gid g is the earlier one's at g + d / 17, and away from the ends of the range every
  occurrence of it is absorbed: lamp 0's own chain from SEED 0 has such a launch.  With 1 MB chunks it owns nothing in whole
  chunks of a batch, and the traced count, the deposits and every launch's plane, its own included, must be the plan's and
  the undeduped trace's.  Through the mark hook the same for two launches with EQUAL SEED pairs (masks and counts).
* The compaction.  No hook exposes the compacted list itself, so the per-launch planes of a group with many blocks per
  launch are held against the undeduped trace instead, together with the traced count and the deposit count: a workgroup that
  started at a wrong slot would overwrite another's rays or leave slots of the list unwritten, and a plane would differ.
A chunk without any owner does not exist: no occurrence of a group's first launch is absorbed."""
import numpy as np
import pytest

import dedupe_strip_cases as strips
import dedupe_tiled_cases as cases
from test_gpu_dedupe import bits  # noqa: F401
from test_gpu_dedupe_mark import block_owners

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lamp0(orc, oscene, oroute):
    return cases.lamp0_of(orc, oscene, oroute)


@pytest.fixture(scope="module")
def groups(pkg, lamp0):
    out = {g.name: g for g in cases.groups(pkg.capi, *lamp0)}
    out.update({g.name: g for g in strips.groups(pkg.capi, *lamp0)})
    return out


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.capi.Ctx(0)
    yield c
    c.close()


def expected(capi, g):
    return strips.plan(capi, g) if g.name in strips.NAMES else cases.plan(capi, g)


def check_mark(capi, ctx, g, first, n):
    ref = expected(capi, g)[:, first - g.first:first - g.first + n]
    masks, owners = ctx.dedupe_mark_device(*g.args(), chunk_first=first, chunk_n=n)
    assert np.array_equal(masks, ref), "a mask differs"
    assert np.array_equal(owners, block_owners(ref, capi.DEDUPE_BLOCK_GIDS)), "the owners of a block differ"
    return masks


MARK_CASES = [(name, "odd") for name in cases.NAMES] + [(name, ch) for name in strips.NAMES for ch in strips.CHUNKINGS]


@pytest.mark.parametrize("name,chunking", MARK_CASES)
def test_mark_against_the_definition(pkg, ctx, groups, name, chunking):
    capi, g = pkg.capi, groups[name]
    parts = [check_mark(capi, ctx, g, first, n) for first, n in strips.chunks(g, chunking)]
    if chunking == "meet":
        assert np.array_equal(np.concatenate(parts, axis=1), expected(capi, g))


@pytest.mark.parametrize("name", ["k2_equal_seeds"])
def test_mark_of_a_launch_without_an_owner(pkg, ctx, groups, name):
    capi, g = pkg.capi, groups[name]
    masks, owners = ctx.dedupe_mark_device(*g.args())
    assert not masks[1].any() and not owners[1].any() and int(owners[0].sum()) == g.n


@pytest.mark.parametrize("name", ["k8_first1200000", "straddle_2_24", "k8_first0"])
def test_strip_seams(pkg, ctx, groups, name):
    """a chunk that begins inside the range, so that the chunk's first tile is not the range's.  check_mark compares every
    mask of the chunk; what this test adds is the proof that the chunk holds occurrences within a gid's step of a tile's
    first key, below it and at or above it, at tile seams and at strip seams.  (Strips of capi.DEDUPE_STRIP_TILES tiles:
    what mark_tiles in csrc/uvrt_batch_plan.h picks for chunks of fewer than 5 x 4 096 tiles, as these are; with longer
    strips every strip seam is still a tile seam.)"""
    capi, g = pkg.capi, groups[name]
    first, n = (g.first, g.n) if g.first == 0 else (g.first + 300, g.n - 600)
    check_mark(capi, ctx, g, first, n)
    gids = np.arange(first, first + n)
    keys = np.stack([strips.keys_of(capi, g, k, gids) for k in range(g.K)])
    # the chunk's first tile starts at its smallest key (dedupe_tile_range)
    rel = keys - int(keys.min())
    assert rel.max() // capi.DEDUPE_MARK_KEYS + 1 < 5 * 4096          # (mark_tiles: strips of DEDUPE_STRIP_TILES)
    for every, what in ((1, "tile"), (capi.DEDUPE_STRIP_TILES, "strip")):
        seam = capi.DEDUPE_MARK_KEYS * every
        assert int(rel.max()) > 3 * seam, "the chunk holds no %s seam" % what
        above = (rel >= seam) & (rel % seam < 17)                    # (not the chunk's own first key)
        below = (rel % seam >= seam - 17) & (rel < rel.max() // seam * seam)
        assert above.any() and below.any(), what


def chain(capi, lamp, length, K, seed):
    return cases.seed_chain(capi, lamp, length, K, seed, 0)


_owner_counts = {}


def plan_owners(capi, lamp, length, K, seed, first, n):
    key = (lamp, K, seed, first, n)
    if key not in _owner_counts:
        prev, nxt = chain(capi, lamp, length, K, seed)
        _owner_counts[key] = (int((capi.dedupe_plan(lamp, prev, nxt, 0, first, n) != 0).sum()), nxt[-1])
    return _owner_counts[key]


SEQUENCE = (300000, 5000, 300000, 70000)      # many, few, many blocks per chunk, then some


def run_sequence(capi, scene, lamp, length, dedupe, pipeline):
    """the batches of SEQUENCE on one context, the SEED chain going on from batch to batch: per batch (traced rays, residue
    after the replay, dose bits)"""
    K, first = 8, 1200000
    c = capi.Ctx(0)
    out = []
    try:
        c.set_scene(scene.tris, scene.nodes, scene.triIdx)
        c.set_dedupe(dedupe)
        c.set_pipeline(pipeline)
        c.reset(True)
        c.seed = 0
        ops = np.zeros(K, dtype=capi.REPLAY_OP_DT)
        for k in range(K):
            ops[k] = (5.0 + 3.0 * k, 1 if k == K - 1 else 0, 0, 1000 * (k + 1), 44.0197, 100.0, k & 1)
        for n in SEQUENCE:
            seed = c.seed
            c.trace_batch([lamp] * K, length, first, n)
            traced = c.batch_traced_rays()
            c.replay_batch(ops)
            out.append((seed, traced, c.batch_residue(), bits(c.read_dosage()).copy()))
    finally:
        c.close()
    return out


_reference = {}


@pytest.mark.parametrize("chunk_mb", [None, 4])
@pytest.mark.parametrize("pipeline", [True, False])
def test_owner_counts_from_chunk_to_chunk(pkg, oscene, lamp0, monkeypatch, pipeline, chunk_mb):
    """chunk_mb 4: 32 768 gids per chunk at most, so the four batches run 10, 1, 10 and 3 chunks: a lane's counts meet
    chunks of 16, 3 and 12 blocks per launch in every order"""
    capi = pkg.capi
    lamp, length = lamp0
    if chunk_mb is not None:
        monkeypatch.setenv("UVRT_BATCH_CHUNK_MB", str(chunk_mb))
    if "off" not in _reference:
        _reference["off"] = run_sequence(capi, oscene, lamp, length, False, True)
    got = run_sequence(capi, oscene, lamp, length, True, pipeline)
    for n, (seed, traced, residue, dose), (seed_off, traced_off, residue_off, dose_off) in zip(SEQUENCE, got, _reference["off"]):
        want, _ = plan_owners(capi, lamp, length, 8, seed, 1200000, n)
        assert seed == seed_off and traced_off == 8 * n and residue_off == 0
        assert traced == want < 8 * n, "n = %d" % n
        assert residue == 0, "n = %d" % n
        assert np.array_equal(dose, dose_off), "n = %d: the dose differs from dedupe off" % n


def counts_of(capi, scene, lamps, length, first, n, dedupe, seed):
    c = capi.Ctx(0)
    try:
        c.set_scene(scene.tris, scene.nodes, scene.triIdx)
        c.set_dedupe(dedupe)
        c.reset(True)
        c.seed = seed
        c.trace_batch(lamps, length, first, n)
        counts = [c.read_batch_counts(k) for k in range(len(lamps))]
        return counts, c.batch_traced_rays(), c.batch_deposits()
    finally:
        c.close()


def test_a_launch_with_no_owner_in_a_chunk(pkg, oscene, lamp0, monkeypatch):
    """8 launches of 60 000 gids from gid 100 000 (keys below 2^24) with 1 MB chunks: 8 192 gids per chunk at most, the range
    dealt evenly over 8 chunks of 7 552.  The plan must show a later launch without an owner in at least two whole chunks,
    one of them an inner one; then total, deposits and planes are held for the batch"""
    capi = pkg.capi
    lamp, length = lamp0
    K, first, n = 8, 100000, 60000
    prev, nxt = chain(capi, lamp, length, K, 0)
    masks = capi.dedupe_plan(lamp, prev, nxt, 0, first, n)
    per = ((n + 7) // 8 + 63) // 64 * 64
    assert (n + per - 1) // per == 8 and per <= 8192
    empty = [(k, c) for k in range(1, K) for c in range(8) if not masks[k, c * per:(c + 1) * per].any()]
    assert len(empty) >= 2 and any(0 < c < 7 for _, c in empty), "no launch without an owner in a whole chunk: %r" % (empty,)
    for k, c in empty:          # (the chunk is not empty: the launches before it own its photons)
        assert masks[:k, c * per:(c + 1) * per].any()
    monkeypatch.setenv("UVRT_BATCH_CHUNK_MB", "1")
    on, traced, deposits = counts_of(capi, oscene, [lamp] * K, length, first, n, True, 0)
    off, traced_off, _ = counts_of(capi, oscene, [lamp] * K, length, first, n, False, 0)
    assert traced_off == K * n and traced == int((masks != 0).sum()) < K * n
    assert deposits == capi.dedupe_classes(lamp, prev, nxt, 0, first, n, capi.dedupe_classes_default())[1]
    for k in range(K):
        assert np.array_equal(on[k], off[k]), "launch %d: dedupe on / off differ" % k
        assert int(off[k].sum()) > 0.5 * n
    # the same with pipelining off: every chunk on lane 0
    c = capi.Ctx(0)
    try:
        c.set_scene(oscene.tris, oscene.nodes, oscene.triIdx)
        c.set_pipeline(False)
        c.reset(True)
        c.seed = 0
        c.trace_batch([lamp] * K, length, first, n)
        assert c.batch_traced_rays() == traced and c.batch_deposits() == deposits
        for k in range(K):
            assert np.array_equal(c.read_batch_counts(k), off[k]), "no pipelining, launch %d" % k
    finally:
        c.close()


@pytest.mark.parametrize("K,n", [(17, 20000), (2, 2049), (8, 4099)])
def test_the_compaction(pkg, oscene, lamp0, K, n):
    """10 blocks x 17 launches, a second block of one gid, and a last block that is not full: the planes of every launch against the undeduped trace (see the module's docstring)"""
    capi = pkg.capi
    lamp, length = lamp0
    first = 1200000
    prev, nxt = chain(capi, lamp, length, K, 0)
    want, _ = plan_owners(capi, lamp, length, K, 0, first, n)
    on, traced, deposits = counts_of(capi, oscene, [lamp] * K, length, first, n, True, 0)
    off, _, _ = counts_of(capi, oscene, [lamp] * K, length, first, n, False, 0)
    assert traced == want <= K * n          # (two launches of 2 049 gids share no photon: their copies lie further apart)
    assert deposits == capi.dedupe_classes(lamp, prev, nxt, 0, first, n, capi.dedupe_classes_default())[1]
    for k in range(K):
        assert np.array_equal(on[k], off[k]), "launch %d: dedupe on / off differ" % k
    assert sum(int(p.sum()) for p in off) > 0.5 * K * n
