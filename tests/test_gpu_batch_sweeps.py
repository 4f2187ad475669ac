"""GPU: batched tracing with sweeps (include/uvrt.h uvrt_trace_batch_launches) -- stops and the segments between them
in one batch, one count plane per launch.  The checkers: the per-launch sequence (uvrt_generate / uvrt_generate_sweep,
uvrt_extend, uvrt_accumulate, uvrt_shade) on a second context for both flavours, and for flavour 0 the oracle's extend
over the restated sweep rays (tests/sweep_restate.py).  Every comparison is over all triangles, bit for bit."""
import numpy as np
import pytest

from conftest import GLB, ROUTE
from sweep_restate import segment_duration, sweep

pytestmark = pytest.mark.gpu

f32 = np.float32
SEED0 = 0x1234


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def bits64(a):
    return np.ascontiguousarray(a).view(np.uint64)


def lamp_pos(orc, oscene, oroute, k):
    comp = orc.Computation(oscene, oroute["lamps"], 1 << 16, oroute["lightHeight"], oroute["lightLength"],
                           oroute["lightIntensity"])
    return tuple(float(x) for x in comp.lamp_world_pos(oroute["lamps"][k]))


def make_ops(pkg, durations, shade_at, ppl):
    ops = np.zeros(len(durations), dtype=pkg.capi.REPLAY_OP_DT)
    for k, d in enumerate(durations):
        ops[k] = (d, 1 if k in shade_at else 0, shade_at.get(k, 0), ppl * (k + 1), 44.0197, 100.0, k & 1)
    return ops


def new_ctx(pkg, oscene, n, flavour=0, dev=False, seed=SEED0):
    c = pkg.capi.Ctx(0, dev=dev)
    c.set_scene(oscene.tris, oscene.nodes, oscene.triIdx)
    c.resize_rays(n)
    c.set_flavour(flavour)
    c.reset(True)
    c.seed = seed
    return c


def is_sweep(pkg, launch):
    return launch[2] == pkg.capi.LAUNCH_SWEEP


def one_launch(pkg, c, launch, length, first, n):
    """generate or generate_sweep, then extend: the per-launch path of one logical launch"""
    if is_sweep(pkg, launch):
        c.generate_sweep(launch[0], launch[1], length, first, n)
    else:
        c.generate(launch[0], length, first, n)
    c.extend(n)


def per_launch_counts(pkg, c, launches, length, first, n):
    out = []
    for launch in launches:
        one_launch(pkg, c, launch, length, first, n)
        out.append(c.read_counts())
        c.accumulate(0.0)           # (takes the deposits out of tempPhotonMap; adds 0 to the sum map)
    return out


def seed_chain(pkg, launches, length, seed):
    """SEED before every launch, and after the last"""
    chain = [seed]
    for launch in launches:
        if is_sweep(pkg, launch):
            seed = pkg.capi.seed_next_sweep(launch[0], length, seed)
        else:
            seed = pkg.capi.seed_next(launch[0], length, seed)
        chain.append(seed)
    return chain


def oracle_sweep_counts(orc, oscene, launch, length, first, n, seed):
    rays, _ = sweep(orc, first, n, launch[0], launch[1], length, seed)
    temp = np.zeros(oscene.T, dtype=np.int32)
    orc.extend(temp, oscene.tris, rays, oscene.nodes, oscene.triIdx)
    return temp


def mixed_launches(pkg, orc, oscene, oroute):
    """stop A; sweep A -> B' (B raised by 0.37: orig.y moves too); stop B; sweep B' -> C; stop A (a repeated column);
    sweep C -> C (degenerate)"""
    A, B, C = (lamp_pos(orc, oscene, oroute, k) for k in (0, 5, 9))
    B1 = (B[0], float(f32(f32(B[1]) + f32(0.37))), B[2])
    stop, swp = pkg.capi.stop, pkg.capi.sweep
    return [stop(A), swp(A, B1), stop(B), swp(B1, C), stop(A), swp(C, C)]


DURATIONS = [60.0, 8.5, 30.0, 6.0, 45.0, 0.0]
SHADE_AT = {2: 1, 5: 0}           # a Shade after launch 2 (max map) and after launch 5 (sum map)

_oracle_planes = {}               # n -> the oracle's planes of launches 1 and 3 of the mixed batch: computed once


def mixed_oracle_planes(pkg, orc, oscene, oroute, n):
    if n not in _oracle_planes:
        launches = mixed_launches(pkg, orc, oscene, oroute)
        length = oroute["lightLength"]
        chain = seed_chain(pkg, launches, length, SEED0)
        _oracle_planes[n] = {k: oracle_sweep_counts(orc, oscene, launches[k], length, 3, n, chain[k]) for k in (1, 3)}
    return _oracle_planes[n]


@pytest.mark.parametrize("flavour", [0, 1])
@pytest.mark.parametrize("n", [100001, 1000])
def test_mixed_batch_equals_the_per_launch_sequence_and_the_oracle(pkg, orc, oscene, oroute, n, flavour):
    """n = 100001 is no multiple of 64 and its three sweep planes hold 3 x 1563 64-ray batches, more than half of the
    8192 persistent waves of a full grid: waves cross plane boundaries.  At n = 1000 a wave holds one batch or none."""
    length = oroute["lightLength"]
    launches = mixed_launches(pkg, orc, oscene, oroute)
    ops = make_ops(pkg, DURATIONS, SHADE_AT, n)
    a = new_ctx(pkg, oscene, n, flavour)
    b = new_ctx(pkg, oscene, n, flavour)
    try:
        per_launch, snap = [], {}
        for k, launch in enumerate(launches):
            one_launch(pkg, a, launch, length, 3, n)
            per_launch.append(a.read_counts())
            a.accumulate(DURATIONS[k])
            if k in SHADE_AT:
                a.shade(int(ops[k]["which_map"]), int(ops[k]["photons_per_light"]), float(ops[k]["scaled_power"]),
                        float(ops[k]["min_value"]), int(ops[k]["threshold_view"]))
                snap[k] = (a.read_dosage(), a.read_color())
        b.trace_batch_launches(launches, length, 3, n)
        assert b.seed == a.seed == seed_chain(pkg, launches, length, SEED0)[-1]
        for k in range(len(launches)):
            got = b.read_batch_counts(k)
            print("launch %d: %d of %d triangles differ from the per-launch path" % (k, int((got != per_launch[k]).sum()), got.size))
            assert np.array_equal(got, per_launch[k]), k
        b.replay_batch(ops)
        assert np.array_equal(bits64(b.read_photon_map(0)), bits64(a.read_photon_map(0)))
        assert np.array_equal(bits64(b.read_photon_map(1)), bits64(a.read_photon_map(1)))
        assert np.array_equal(bits(b.read_dosage()), bits(snap[5][0])) and np.array_equal(bits(b.read_color()), bits(snap[5][1]))
        if flavour == 0:
            want = mixed_oracle_planes(pkg, orc, oscene, oroute, n)
            for k in (1, 3):
                assert np.array_equal(per_launch[k], want[k]) and want[k].sum() > 0.5 * n, k
        # a second batch on the same context, replayed WITHOUT a fold: two sweeps over another global-id range
        two = [launches[1], launches[3]]
        b.trace_batch_launches(two, length, 7, 1000)
        b.replay_batch(make_ops(pkg, DURATIONS[:2], {1: 0}, 1000))
        for k, launch in enumerate(two):
            one_launch(pkg, a, launch, length, 7, 1000)
            a.accumulate(DURATIONS[k])
        assert np.array_equal(bits64(b.read_photon_map(0)), bits64(a.read_photon_map(0)))
        assert np.array_equal(bits64(b.read_photon_map(1)), bits64(a.read_photon_map(1)))
        assert b.seed == a.seed
    finally:
        a.close()
        b.close()


def test_plane_offset_and_exact_step_bit_share_one_register(pkg, orc, oscene, oroute):
    """Sweeps 1 and 2 run along x = 1e-35f, below the 2^-100 window of the packed division: every one of their rays takes the
    exact step while its plane offset is non-zero.  Variant 500 of the developer library puts every ray on the exact step."""
    n = 4097
    length = oroute["lightLength"]
    A, B, C = (lamp_pos(orc, oscene, oroute, k) for k in (0, 5, 9))
    tiny = float(f32(1e-35))
    launches = [pkg.capi.sweep(A, B), pkg.capi.sweep((tiny, A[1], A[2]), (tiny, B[1], B[2])),
                pkg.capi.sweep((tiny, B[1], B[2]), (tiny, C[1], C[2]))]
    chain = seed_chain(pkg, launches, length, SEED0)
    want = [oracle_sweep_counts(orc, oscene, launches[k], length, 0, n, chain[k]) for k in range(3)]
    a = new_ctx(pkg, oscene, n)
    b = new_ctx(pkg, oscene, n)
    d = new_ctx(pkg, oscene, n, dev=True)
    try:
        per_launch = per_launch_counts(pkg, a, launches, length, 0, n)
        b.trace_batch_launches(launches, length, 0, n)
        d.set_variant(500)
        d.trace_batch_launches(launches, length, 0, n)
        for k in range(3):
            got, got_exact = b.read_batch_counts(k), d.read_batch_counts(k)
            print("sweep %d: %d hits; differ from the per-launch path on %d, the oracle on %d, variant 500 on %d triangles"
                  % (k, int(got.sum()), int((got != per_launch[k]).sum()), int((got != want[k]).sum()), int((got != got_exact).sum())))
            assert np.array_equal(got, per_launch[k]) and np.array_equal(got, want[k]) and np.array_equal(got, got_exact), k
        assert want[0].sum() > 0.5 * n
        assert a.seed == b.seed == d.seed == chain[-1]
    finally:
        a.close()
        b.close()
        d.close()


def test_sweep_chunks_alternate_over_the_lanes(pkg, orc, oscene, oroute, monkeypatch):
    """UVRT_BATCH_CHUNK_MB=1 (read once in uvrt_create): 1 MB / (20032 slots x 24 B) = 2 sweep planes per chunk, so seven
    sweeps make four chunks over both side lanes; two stops share the batch."""
    n = 20000
    length = oroute["lightLength"]
    p = [lamp_pos(orc, oscene, oroute, k) for k in range(8)]
    launches = [pkg.capi.sweep(p[k], p[k + 1]) for k in range(7)]
    launches[2:2] = [pkg.capi.stop(p[3])]
    launches.append(pkg.capi.stop(p[0]))
    monkeypatch.delenv("UVRT_BATCH_CHUNK_MB", raising=False)
    whole = new_ctx(pkg, oscene, n)
    monkeypatch.setenv("UVRT_BATCH_CHUNK_MB", "1")
    chunked = new_ctx(pkg, oscene, n)
    try:
        whole.trace_batch_launches(launches, length, 0, n)
        chunked.trace_batch_launches(launches, length, 0, n)
        for k in range(len(launches)):
            want = whole.read_batch_counts(k)
            assert np.array_equal(chunked.read_batch_counts(k), want) and want.sum() > 0.5 * n, k
        assert chunked.seed == whole.seed == seed_chain(pkg, launches, length, SEED0)[-1]
    finally:
        whole.close()
        chunked.close()


def test_ray_range_shards_of_a_mixed_batch_equal_the_whole(pkg, orc, oscene, oroute):
    from uvrt_amd import sharding
    n, world = 100001, 3
    length = oroute["lightLength"]
    launches = mixed_launches(pkg, orc, oscene, oroute)
    ops = make_ops(pkg, DURATIONS, SHADE_AT, n)
    one = new_ctx(pkg, oscene, n)
    shards = [new_ctx(pkg, oscene, n) for _ in range(world)]
    try:
        one.trace_batch_launches(launches, length, 0, n)
        want = [one.read_batch_counts(k) for k in range(len(launches))]
        one.replay_batch(ops)
        for r, c in enumerate(shards):
            first, count = sharding.ray_range(r, world, n)
            c.trace_batch_launches(launches, length, first, count)
        pkg.capi.reduce_batch_group(shards)
        for c in shards:
            for k in range(len(launches)):
                assert np.array_equal(c.read_batch_counts(k), want[k]), k
            c.replay_batch(ops)
            assert np.array_equal(bits(c.read_dosage()), bits(one.read_dosage()))
            assert np.array_equal(bits64(c.read_photon_map(1)), bits64(one.read_photon_map(1)))
            assert c.seed == one.seed
        assert one.read_dosage().any()
    finally:
        one.close()
        for c in shards:
            c.close()


def test_a_batch_of_stops_is_uvrt_trace_batch(pkg, orc, oscene, oroute):
    n = 30001
    length = oroute["lightLength"]
    lamps = [lamp_pos(orc, oscene, oroute, k) for k in (0, 5, 0, 9, 5)]
    ops = make_ops(pkg, [60.0, 30.0, 45.0, 10.0, 25.0], {2: 1, 4: 0}, n)
    a = new_ctx(pkg, oscene, n)
    b = new_ctx(pkg, oscene, n)
    try:
        a.trace_batch(lamps, length, 3, n)
        b.trace_batch_launches([pkg.capi.stop(lp) for lp in lamps], length, 3, n)
        assert a.seed == b.seed
        for k in range(len(lamps)):
            want = a.read_batch_counts(k)
            assert np.array_equal(b.read_batch_counts(k), want) and want.sum() > 0.5 * n, k
        a.replay_batch(ops)
        b.replay_batch(ops)
        for w in (0, 1):
            assert np.array_equal(bits64(a.read_photon_map(w)), bits64(b.read_photon_map(w)))
        assert np.array_equal(bits(a.read_dosage()), bits(b.read_dosage())) and np.array_equal(bits(a.read_color()), bits(b.read_color()))
    finally:
        a.close()
        b.close()


def test_refusals_leave_the_seed_and_the_batch_alone(pkg, orc, oscene, oroute):
    n = 5000
    length = oroute["lightLength"]
    launches = mixed_launches(pkg, orc, oscene, oroute)
    a = new_ctx(pkg, oscene, n)
    c = new_ctx(pkg, oscene, n)
    invalid = r"uvrt error -1"              # UVRT_ERR_INVALID
    try:
        c.set_seed_mode(1)
        with pytest.raises(pkg.capi.UvrtError, match=invalid + ".*seed mode 1"):
            c.trace_batch_launches(launches, length, 0, n)
        c.set_seed_mode(0)
        assert c.seed == SEED0
        c.set_flavour(2)
        with pytest.raises(pkg.capi.UvrtError, match=invalid + ".*flavours 0 and 1"):
            c.trace_batch_launches(launches, length, 0, n)
        c.set_flavour(0)
        assert c.seed == SEED0
        bad = np.array(launches, dtype=pkg.capi.LAUNCH_DT)
        bad["kind"][3] = 2
        with pytest.raises(pkg.capi.UvrtError, match=invalid + ".*kind"):
            c.trace_batch_launches(bad, length, 0, n)
        assert c.seed == SEED0
        with pytest.raises(pkg.capi.UvrtError, match=invalid + r".*\[1,64\]"):
            c.trace_batch_launches((launches * 11)[:65], length, 0, n)
        assert c.seed == SEED0
        c.set_record_hits(True)
        with pytest.raises(pkg.capi.UvrtError, match=invalid + ".*per-launch features"):
            c.trace_batch_launches(launches, length, 0, n)
        c.set_record_hits(False)
        assert c.seed == SEED0
        c.trace_batch_launches(launches[:2], length, 0, n)
        after = c.seed
        assert after == seed_chain(pkg, launches[:2], length, SEED0)[-1]
        with pytest.raises(pkg.capi.UvrtError, match=invalid + ".*not been replayed"):
            c.trace_batch_launches(launches, length, 0, n)
        assert c.seed == after
        c.replay_batch(make_ops(pkg, DURATIONS[:2], {}, n))
        # a correct mixed batch on the same context
        c.seed = SEED0
        want = per_launch_counts(pkg, a, launches, length, 0, n)
        c.trace_batch_launches(launches, length, 0, n)
        for k in range(len(launches)):
            assert np.array_equal(c.read_batch_counts(k), want[k]), k
        assert c.seed == a.seed and want[1].sum() > 0.5 * n
        c.replay_batch(make_ops(pkg, DURATIONS, SHADE_AT, n))
    finally:
        a.close()
        c.close()


# ---- RayTracer::driveSpeed through ComputeIterationsBatched ----

def _tracer(host, lamps_n, photons, iterations, speed):
    rt = host.RayTracer(GLB, ROUTE, device=0)
    rt.set_lamps(rt.lamps()[:lamps_n])
    rt.photonCount = photons
    rt.maxIterations = iterations
    rt.driveSpeed = speed
    rt.ResetDosageMap()
    rt.viewMode = host.VIEW_DOSAGE
    return rt


def _state(rt):
    rt.Sync()
    return (rt.read_dosage(), rt.ctx.read_photon_map(0), rt.ctx.read_photon_map(1), rt.ctx.read_color())


def test_host_batches_of_stops_and_segments_equal_the_loop(pkg):
    """lange_route's 12 positions: 3 x (12 stops + 11 segments) = 69 launches cross the 64-launch limit, so the batches
    hold 46 and 23."""
    from uvrt_amd import host
    iterations = 3
    a = _tracer(host, 12, 12 << 12, iterations, 0.1)
    b = _tracer(host, 12, 12 << 12, iterations, 0.1)
    try:
        for _ in range(iterations):
            a.ComputeDosageMap()
            a.Shade()
            a.currIterations = a.currIterations + 1
        b.ComputeIterationsBatched(iterations)
        for got, want in zip(_state(b), _state(a)):
            assert np.array_equal(got.view(np.uint8), want.view(np.uint8))
        assert a.ctx.seed == b.ctx.seed and a.read_dosage().any()
        assert b.photonMapSize == a.photonMapSize == iterations * 12 * a.photonsPerLight
        assert b.currIterations == a.currIterations == iterations
    finally:
        a.close()
        b.close()


def oracle_route_with_driving(orc, oscene, oroute, lamps, photon_count, iterations, speed):
    comp = orc.Computation(oscene, lamps, photon_count, oroute["lightHeight"], oroute["lightLength"], oroute["lightIntensity"])
    comp.reset()
    for _ in range(iterations):
        comp.iteration()                                     # the stops, as orc.Computation does them
        for a, b in zip(lamps[:-1], lamps[1:]):              # then every segment: sweep -> extend -> accumulate(len / speed)
            rays, comp.SEED = sweep(orc, 0, comp.photonsPerLight, comp.lamp_world_pos(a), comp.lamp_world_pos(b),
                                    comp.lightLength, comp.SEED)
            orc.extend(comp.temp, oscene.tris, rays, oscene.nodes, oscene.triIdx)
            orc.accumulate(comp.photonMap, comp.maxPhotonMap, comp.temp, segment_duration(a, b, speed))
    return comp


GROUP = dict(lamps_n=3, photons=3 << 16, iterations=2, speed=0.1)


@pytest.fixture(scope="module")
def driving_reference(pkg, orc, oscene, oroute):
    """(the oracle's dose and SEED, the single instance's dose and SEED) of the group's computation: made once"""
    from uvrt_amd import host
    comp = oracle_route_with_driving(orc, oscene, oroute, oroute["lamps"][:GROUP["lamps_n"]], GROUP["photons"],
                                     GROUP["iterations"], GROUP["speed"])
    one = _tracer(host, **GROUP)
    try:
        one.ComputeIterationsBatched(GROUP["iterations"])
        one.Sync()
        return comp.dose(), comp.SEED, one.read_dosage(), one.ctx.seed
    finally:
        one.close()


def test_host_group_of_ray_ranges_drives(pkg, driving_reference):
    from uvrt_amd import host
    want, want_seed, single, single_seed = driving_reference
    assert np.array_equal(bits(single), bits(want)) and single_seed == want_seed
    shards = [_tracer(host, **GROUP) for _ in range(2)]
    try:
        for r, rt in enumerate(shards):
            rt.SetRayRange(r, 2)
        host.compute_iterations_batched_group(shards, GROUP["iterations"])
        for rt in shards:
            rt.Sync()
            assert np.array_equal(bits(rt.read_dosage()), bits(want))
            assert rt.ctx.seed == want_seed and rt.currIterations == GROUP["iterations"]
        assert want.any()
    finally:
        for rt in shards:
            rt.close()


def test_host_reduce_over_a_single_rank_communicator_drives(pkg, driving_reference):
    from uvrt_amd import host
    ok, why = pkg.capi.comm_available()
    if not ok:
        pytest.skip("no RCCL: " + why)
    want, want_seed, _, _ = driving_reference
    rt = _tracer(host, **GROUP)
    try:
        rt.ctx.comm_init_rank(pkg.capi.comm_unique_id(), 0, 1)
        rt.set_reduce_over_comm(True)
        rt.ComputeIterationsBatched(GROUP["iterations"])
        rt.Sync()
        assert np.array_equal(bits(rt.read_dosage()), bits(want)) and rt.ctx.seed == want_seed
        rt.ctx.comm_destroy()
    finally:
        rt.close()
