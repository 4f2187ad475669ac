"""GPU: a batch traces every distinct photon of a lamp once (include/uvrt.h uvrt_set_dedupe; csrc/uvrt_dedupe.h).

uvrt_read_batch_counts per launch with dedupe on must equal the same batch with dedupe off and the oracle's per-launch
counts, bit for bit; and uvrt_batch_traced_rays must equal the number of owners the host-side plan (uvrt_dedupe_plan, held to
brute force by tests/test_dedupe_cpu.py) gives, so a dedupe that is silently off fails here."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K8 = 8
N = 4096


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def bits64(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.fixture(scope="module")
def env(pkg, orc, oscene, oroute):
    comp = orc.Computation(oscene, oroute["lamps"], 1 << 16, oroute["lightHeight"], oroute["lightLength"], oroute["lightIntensity"])
    lamps = [tuple(float(x) for x in comp.lamp_world_pos(oroute["lamps"][k])) for k in (0, 5)]
    return {"capi": pkg.capi, "orc": orc, "scene": oscene, "length": oroute["lightLength"], "lamps": lamps}


def new_ctx(env, dedupe, flavour=0, mode=0, seed=0):
    c = env["capi"].Ctx(0)
    s = env["scene"]
    c.set_scene(s.tris, s.nodes, s.triIdx)
    c.set_flavour(flavour)
    c.set_seed_mode(mode)
    c.set_dedupe(dedupe)
    c.reset(True)
    c.seed = seed
    return c


def trace(env, lamps, first, n, dedupe, flavour=0, mode=0, seed=0):
    """(per-launch counts, rays traced, SEED afterwards) of one batch of stops"""
    c = new_ctx(env, dedupe, flavour, mode, seed)
    try:
        c.trace_batch(lamps, env["length"], first, n)
        counts = [c.read_batch_counts(k) for k in range(len(lamps))]
        return counts, c.batch_traced_rays(), c.seed
    finally:
        c.close()


def oracle_counts(env, lamps, first, n, flavour=0, mode=0, seed=0):
    orc, s = env["orc"], env["scene"]
    out = []
    orc.set_flavour(flavour)
    try:
        for lp in lamps:
            if mode == 0:
                rays, nxt = orc.generate(first, n, lp, env["length"], seed)
            else:
                rays, _ = orc.generate_fixed_seed(first, n, lp, env["length"], seed, saturate=True)
                nxt = env["capi"].seed_next(lp, env["length"], seed, 1)
            temp = np.zeros(s.T, dtype=np.int32)
            orc.extend(temp, s.tris, rays, s.nodes, s.triIdx)
            out.append(temp)
            seed = nxt
    finally:
        orc.set_flavour(0)
    return out


def owners(env, lamp, count, seed, mode, first, n):
    """(owners of a dedupe group of `count` launches from `lamp` that starts at SEED `seed`, the SEED after it)"""
    capi = env["capi"]
    prev, nxt = [], []
    for _ in range(count):
        prev.append(seed)
        seed = capi.seed_next(lamp, env["length"], seed, mode)
        nxt.append(seed)
    return int((capi.dedupe_plan(lamp, prev, nxt, mode, first, n) != 0).sum()), seed


def check(env, lamps, first, n, want_traced, flavour=0, mode=0, seed=0, oracle=True, min_hits=0.5):
    on, traced, seed_on = trace(env, lamps, first, n, True, flavour, mode, seed)
    off, traced_off, seed_off = trace(env, lamps, first, n, False, flavour, mode, seed)
    assert traced_off == len(lamps) * n and seed_on == seed_off
    assert traced == want_traced
    for k in range(len(lamps)):
        assert np.array_equal(on[k], off[k]), "launch %d: dedupe on / off differ" % k
    if oracle:
        ref = oracle_counts(env, lamps, first, n, flavour, mode, seed)
        for k in range(len(lamps)):
            assert np.array_equal(on[k], ref[k]), "launch %d differs from the oracle" % k
        assert sum(int(r.sum()) for r in ref) > min_hits * len(lamps) * n
    return on


@pytest.mark.parametrize("first", [0, 1200000, 2000000, 16000000])
def test_one_lamp_8_launches(env, first):
    lamp = env["lamps"][0]
    want, _ = owners(env, lamp, K8, 0, 0, first, N)
    assert want < K8 * N
    check(env, [lamp] * K8, first, N, want)


@pytest.mark.parametrize("first", [9000000, 15000000])
@pytest.mark.parametrize("lx8", [False, True])
def test_sums_in_2_27_to_2_28(env, first, lx8):
    """ulp 16 against a step of 17: an add that ties gives two neighbouring gids one key (a lamp with lx = 8 ties in every
    launch, SEED >> 15 = 8 mod 16 in one of sixteen): such occurrences are traced alone, every launch keeps its own counts"""
    lamp = env["lamps"][0]
    if lx8:
        lamp = (8.0, lamp[1], lamp[2])          # (outside the room: fewer hits, the same rule)
    want, _ = owners(env, lamp, K8, 0x02468ace, 0, first, N)
    check(env, [lamp] * K8, first, N, want, seed=0x02468ace, min_hits=0.0)


@pytest.fixture(scope="module")
def rcp_table(orc):
    orc.set_rcp_table(orc.refgpu_rcp_table())          # the oracle's flavour 2 evaluates v_rcp_f32 through this GPU's table


@pytest.mark.parametrize("flavour", [1, 2])
def test_flavours(env, flavour, request):
    if flavour == 2:
        request.getfixturevalue("rcp_table")
    lamp = env["lamps"][0]
    want, _ = owners(env, lamp, K8, 0, 0, 1200000, N)
    check(env, [lamp] * K8, 1200000, N, want, flavour=flavour)


def test_seed_mode_1(env):
    lamp = env["lamps"][0]
    want, _ = owners(env, lamp, K8, 0x1234, 1, 1200000, N)
    assert want < K8 * N
    check(env, [lamp] * K8, 1200000, N, want, mode=1, seed=0x1234)


def test_two_lamps_interleaved(env):
    """A B A B A B: two groups of three, each with its own places in the SEED chain"""
    a, b = env["lamps"]
    lamps = [a, b, a, b, a, b]
    capi = env["capi"]
    seeds = [0]
    for lp in lamps:
        seeds.append(capi.seed_next(lp, env["length"], seeds[-1], 0))
    want = 0
    for col in (0, 1):
        ks = [k for k in range(6) if k % 2 == col]
        plan = capi.dedupe_plan(lamps[col], [seeds[k] for k in ks], [seeds[k + 1] for k in ks], 0, 1200000, N)
        want += int((plan != 0).sum())
    assert want < 6 * N
    check(env, lamps, 1200000, N, want)


def test_column_of_33_launches_is_split(env):
    """33 launches of one lamp: two groups, 17 + 16 (a mask holds 31 launches); n is no multiple of 64"""
    lamp, n = env["lamps"][0], 1000
    w17, seed = owners(env, lamp, 17, 0, 0, 1200000, n)
    w16, _ = owners(env, lamp, 16, seed, 0, 1200000, n)
    assert w17 + w16 < 33 * n
    check(env, [lamp] * 33, 1200000, n, w17 + w16)


def test_n_not_a_multiple_of_64(env):
    lamp, n = env["lamps"][0], 4001
    want, _ = owners(env, lamp, K8, 0, 0, 0, n)
    check(env, [lamp] * K8, 0, n, want)


def test_group_of_one_launch_is_traced_as_it_is(env):
    check(env, [env["lamps"][0]], 1200000, N, N)
    a, b = env["lamps"]
    check(env, [a, b], 1200000, N, 2 * N)


def test_a_batch_with_a_sweep_in_it(env):
    """four stops, a sweep, four stops: the eight stops are one group (their SEEDs run through the sweep's), the sweep is traced
    as it is"""
    capi, n, first = env["capi"], N, 1200000
    a, b = env["lamps"]
    launches = [capi.stop(a)] * 4 + [capi.sweep(a, b)] + [capi.stop(a)] * 4
    stops = [k for k in range(9) if k != 4]
    seeds = [0]
    for k in range(9):
        seeds.append(capi.seed_next_sweep(a, env["length"], seeds[-1]) if k == 4 else capi.seed_next(a, env["length"], seeds[-1], 0))
    plan = capi.dedupe_plan(a, [seeds[k] for k in stops], [seeds[k + 1] for k in stops], 0, first, n)
    got = {}
    for dedupe in (True, False):
        c = new_ctx(env, dedupe)
        try:
            c.trace_batch_launches(launches, env["length"], first, n)
            got[dedupe] = ([c.read_batch_counts(k) for k in range(9)], c.batch_traced_rays(), c.seed)
        finally:
            c.close()
    assert got[True][1] == int((plan != 0).sum()) < 8 * n and got[False][1] == 8 * n
    assert got[True][2] == got[False][2] == seeds[9]
    for k in range(9):
        assert np.array_equal(got[True][0][k], got[False][0][k]), k
    # the stops against the oracle, each at its place in the chain
    s = env["scene"]
    for k in stops:
        rays, _ = env["orc"].generate(first, n, a, env["length"], seeds[k])
        temp = np.zeros(s.T, dtype=np.int32)
        env["orc"].extend(temp, s.tris, rays, s.nodes, s.triIdx)
        assert np.array_equal(got[True][0][k], temp), k
    assert got[True][0][4].sum() > 0.5 * n


def test_two_contexts_trace_the_halves_of_a_range(env):
    """each half dedupes within its own range; the folded planes of the halves sum to the whole's"""
    lamp, first, half = env["lamps"][0], 1200000, N // 2
    whole = oracle_counts(env, [lamp] * K8, first, N)
    lo, traced_lo, _ = trace(env, [lamp] * K8, first, half, True)
    hi, traced_hi, _ = trace(env, [lamp] * K8, first + half, half, True)
    assert traced_lo == owners(env, lamp, K8, 0, 0, first, half)[0]
    assert traced_hi == owners(env, lamp, K8, 0, 0, first + half, half)[0]
    for k in range(K8):
        assert np.array_equal(lo[k] + hi[k], whole[k]), k


def test_replay_after_a_deduped_trace_gives_the_loops_maps(env):
    """generate -> extend -> accumulate (-> Shade) launch by launch against trace_batch + replay_batch: maps, dose, colour"""
    capi, lamp, n, first = env["capi"], env["lamps"][0], N, 1200000
    durations = [60.0, 30.0, 45.0, 10.0, 25.0, 5.0, 15.0, 20.0]
    ops = np.zeros(K8, dtype=capi.REPLAY_OP_DT)
    for k, d in enumerate(durations):
        ops[k] = (d, 1 if k in (3, 7) else 0, 1 if k == 3 else 0, n * (k + 1), 44.0197, 100.0, k & 1)
    a, b = new_ctx(env, False), new_ctx(env, True)
    try:
        a.resize_rays(n)
        for k in range(K8):
            a.generate(lamp, env["length"], first, n)
            a.extend(n)
            a.accumulate(durations[k])
            if ops[k]["shade"]:
                a.shade(int(ops[k]["which_map"]), int(ops[k]["photons_per_light"]), float(ops[k]["scaled_power"]),
                        float(ops[k]["min_value"]), int(ops[k]["threshold_view"]))
        b.trace_batch([lamp] * K8, env["length"], first, n)
        assert b.batch_traced_rays() < K8 * n
        b.replay_batch(ops)
        assert b.seed == a.seed
        for which in (0, 1):
            assert np.array_equal(bits64(b.read_photon_map(which)), bits64(a.read_photon_map(which)))
        assert np.array_equal(bits(b.read_dosage()), bits(a.read_dosage())) and a.read_dosage().any()
        assert np.array_equal(bits(b.read_color()), bits(a.read_color()))
    finally:
        a.close()
        b.close()
