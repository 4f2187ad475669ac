"""No GPU: the host-only parts of the gather sampling mode (include/uvrt.h uvrt_set_gather_sampling) -- the
symbols in both libraries, the refusals that need no device, the route file's <gather_sampling>, the CLI's refusals, the
building blocks of the restatement (tests/gather_stratified_restate.py) -- and the estimator itself: both modes against the
oracle's photon counts, at a stop and on a sweep."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gather_restate as gr
import gather_stratified_restate as gs
from conftest import GLB, GOLDEN
from plan_options_pin import check_plan_option

NEW = ("uvrt_set_gather_sampling", "uvrt_get_gather_sampling")
f32 = np.float32


def test_symbols_are_bound_and_resolve_in_both_libraries(pkg):
    names = [name for name, _, _ in pkg.capi.SYMBOLS]
    for n in NEW:
        assert names.count(n) == 1
        for path in (pkg.capi.LIB_PATH, pkg.capi.LIB_DEV_PATH):
            assert hasattr(C.CDLL(path), n), (path, n)
        for dev in (False, True):
            assert getattr(pkg.capi.lib(dev), n).restype is C.c_int
    for m in ("set_gather_sampling", "get_gather_sampling"):
        assert hasattr(pkg.capi.Ctx, m)
    from uvrt_amd import host
    assert "gatherSampling" in host._FIELDS and "gatherSampling" in host._INT_FIELDS
    check_plan_option(host, "gather_sampling", C.c_int, 0)


def test_a_null_context_is_refused_without_a_gpu(pkg):
    mode = C.c_int32(7)
    for dev in (False, True):
        L = pkg.capi.lib(dev)
        calls = (("uvrt_set_gather_sampling", lambda: L.uvrt_set_gather_sampling(None, 1)),
                 ("uvrt_get_gather_sampling", lambda: L.uvrt_get_gather_sampling(None, C.byref(mode))))
        for name, call in calls:
            assert call() == -1 and name.encode() in L.uvrt_last_error(), name          # UVRT_ERR_INVALID
    assert mode.value == 7


def test_route_file_keeps_the_gather_sampling(pkg, tmp_path):
    """<gather_sampling> is written only when it and <gather_samples> are > 0, right after <gather_samples>; a route saved at 0
    is byte for byte what the tag-less writer saved; an absent tag loads as 0."""
    from uvrt_amd import host
    golden = open(os.path.join(GOLDEN, "lange_route.xml"), "rb").read()
    rt = host.RayTracer(init=False)
    rt.set_route_dir(GOLDEN + os.sep)
    rt.LoadRoute("lange_route")
    assert rt.gatherSamples == 0 and rt.gatherSampling == 0
    rt.set_route_dir(str(tmp_path) + os.sep)
    rt.SaveRoute("photons")
    assert (tmp_path / "photons.xml").read_bytes() == golden
    rt.gatherSampling = 1                       # without samples: no gather, no tag
    rt.SaveRoute("mode_only")
    assert (tmp_path / "mode_only.xml").read_bytes() == golden
    rt.gatherSamples, rt.gatherSampling = 16, 0
    rt.SaveRoute("independent")
    independent = (tmp_path / "independent.xml").read_bytes()
    samples_line = b"    <gather_samples>16</gather_samples>\n"
    assert b"gather_sampling" not in independent and independent.replace(samples_line, b"") == golden
    rt.gatherSampling = 1
    rt.driveSpeed = 0.125
    rt.SaveRoute("stratified")
    stratified = (tmp_path / "stratified.xml").read_bytes()
    line = b"    <gather_sampling>1</gather_sampling>\n"
    assert stratified.count(line) == 1
    assert stratified.index(line) == stratified.index(samples_line) + len(samples_line)
    assert stratified.index(b"<rijsnelheid>") < stratified.index(samples_line) < stratified.index(b"<lamp_lengte>")
    rt2 = host.RayTracer(init=False)
    rt2.set_route_dir(str(tmp_path) + os.sep)
    rt2.LoadRoute("stratified")
    assert rt2.gatherSamples == 16 and rt2.gatherSampling == 1 and rt2.lamps() == rt.lamps()
    rt2.SaveRoute("again")
    assert (tmp_path / "again.xml").read_bytes() == stratified
    rt2.LoadRoute("independent")                # absent: back to 0
    assert rt2.gatherSamples == 16 and rt2.gatherSampling == 0
    rt2.LoadRoute("stratified")
    rt2.LoadRoute("photons")
    assert rt2.gatherSamples == 0 and rt2.gatherSampling == 0
    rt.close(); rt2.close()


def test_cli_refuses_gather_sampling_on_its_own_and_unknown_words(pkg):
    cli = os.path.join(os.path.dirname(pkg.capi.LIB_PATH), "uvrt_cli")
    base = [cli, "--room", GLB, "--route-dir", GOLDEN, "--route", "lange_route"]
    for extra in (["--gather-sampling", "stratified"], ["--gather-sampling", "independent"],
                  ["--gather", "0", "--gather-sampling", "stratified"], ["--plan", "--gather-sampling", "stratified"],
                  ["--gather", "4", "--gather-sampling", "sobol"], ["--plan-gather", "4", "--gather-sampling", "1"]):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2, (extra, r.stdout, r.stderr)
        assert "--gather-sampling" in r.stderr and "--gather S" in r.stderr and "--plan-gather S" in r.stderr, (extra, r.stderr)
    r = subprocess.run(base + ["--gather-sampling"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2


# ---------------------------------------------------------------- the restatement's building blocks
def _wang(x):
    x &= 0xFFFFFFFF
    x = (x ^ 61) ^ (x >> 16)
    x = (x * 9) & 0xFFFFFFFF
    x ^= x >> 4
    x = (x * 0x27d4eb2d) & 0xFFFFFFFF
    return x ^ (x >> 15)


def test_u_m_against_python_integers():
    """the uint32 Weyl sequence against plain Python integers on 6 000 (t, s, seed), among them every s whose product with
    0x9E3779B9 passes 2^32 (all s >= 2) and the largest t, s and seed of the interface"""
    rng = np.random.default_rng(1)
    t = np.concatenate([rng.integers(0, 1 << 22, 1990), [0, 1, (1 << 31) // 4096 - 1, (1 << 31) - 1, 0xFFFFFFFF]
                        + list(range(5))]).astype(np.uint32)
    s = np.concatenate([rng.integers(0, 4096, 1990), [0, 1, 2, 4095, 4095, 0, 1, 2, 3, 4]]).astype(np.uint32)
    assert t.size == s.size == 2000
    wraps = 0
    for seed in (0, 7, 0xFFFFFFFF):
        got = gs.u_m_sequence(t, s, seed)
        assert got.dtype == f32
        for ti, si, g in zip(t.tolist(), s.tolist(), got):
            h_t = _wang(ti ^ _wang(seed ^ 0x9E3779B9))
            full = si * 0x9E3779B9 + h_t
            wraps += full >= 1 << 32
            k = full & 0xFFFFFFFF
            want = (k >> 8) / float(1 << 24)                    # 24 bits: exact in f32 and in f64
            assert float(g) == want and 0.0 <= want < 1.0, (ti, si, seed)
    assert wraps > 4000
    # per triangle the sequence is the golden-ratio rotation: consecutive samples are 0x9E3779B9 / 2^32 apart (mod 1)
    u = gs.u_m_sequence(np.full(64, 1234, dtype=np.uint32), np.arange(64, dtype=np.uint32), 5).astype(np.float64)
    step = np.mod(np.diff(u), 1.0)
    assert np.all(np.abs(step - 0x9E3779B9 / 2.0 ** 32) <= 2.0 ** -24)


@pytest.mark.parametrize("S", [1, 3, 4, 5, 16, 4096])
def test_u_h_stays_in_its_stratum(S):
    count = max(1, 20000 // S)
    u_h, u_m, a, b = gs.lamp_coordinates(100, count, S, 3)
    s = np.tile(np.arange(S), count)
    assert u_h.dtype == f32 and u_h.size == count * S
    # against the exact bounds s/S and (s+1)/S in f64: fl(x / S) of an x in [s, s + 1] is monotone in x, and both ends are
    # roundings of the exact bounds, so the f32 value lies between the f32 roundings of the bounds
    lo, hi = (s / S).astype(f32), ((s + 1) / S).astype(f32)
    assert np.all(u_h >= lo) and np.all(u_h <= hi)
    assert np.all((u_m >= 0) & (u_m < 1))
    if S > 1:                                   # jittered: not the stratum's centre or edge
        frac = u_h.astype(np.float64) * S - s
        assert 0.2 < frac.mean() < 0.8 and frac.std() > 0.2


def test_one_sample_at_a_stop_is_the_independent_sample(orc, oscene, oroute):
    """S = 1 at a stop: u_h = fl(fl(0 + xi_h) / 1) = xi_h and u_m multiplies a zero segment -- rays and weights bit for bit"""
    comp = orc.Computation(oscene, oroute["lamps"], 1 << 16, oroute["lightHeight"], oroute["lightLength"], oroute["lightIntensity"])
    lp = comp.lamp_world_pos(oroute["lamps"][0])
    for seed in (0, 9):
        r0, w0 = gr.samples(orc, oscene.tris, lp, lp, oroute["lightLength"], 1, seed)
        r1, w1 = gs.samples(orc, oscene.tris, lp, lp, oroute["lightLength"], 1, seed)
        assert r0.tobytes() == r1.tobytes() and w0.tobytes() == w1.tobytes()
    # and the mode argument: 0 is gather_restate.samples itself
    r0, w0 = gr.samples(orc, oscene.tris, lp, lp, oroute["lightLength"], 4, 2, 50, 70)
    r1, w1 = gs.samples(orc, oscene.tris, lp, lp, oroute["lightLength"], 4, 2, 50, 70, mode=gs.INDEPENDENT)
    r2, _ = gs.samples(orc, oscene.tris, lp, lp, oroute["lightLength"], 4, 2, 50, 70)
    assert r0.tobytes() == r1.tobytes() and w0.tobytes() == w1.tobytes() and r0.tobytes() != r2.tobytes()
    # (a, b) are the same draws: the points on the triangle do not move, so origin + dir * r lands where it did
    assert np.array_equal(r0["origx"], r2["origx"]) and np.array_equal(r0["origz"], r2["origz"])


# ---------------------------------------------------------------- the estimator
N = 1 << 21
S = 16
SEEDS = (0, 1, 2)
BAND = 3 * 0.0235               # tests/test_gather_cpu.py: three times the largest recorded deviation of a median from 1
# 5th-95th width of expected / count, stratified over independent, as tests/tools/gather_quality.py measures it
# (profiles/r13/r13_gather_quality.json, S = 16, seeds 0-7):
#   stop:  0.31-0.34 per seed; the bound 0.5 is the issue's: it leaves room for seed noise, an estimator that is not
#          stratified sits at 1
#   sweep: 0.575-0.628 per seed, mean 0.606 = SWEEP_RATIO; the bound is that ratio plus half the distance to 1, 0.803
STOP_BOUND = 0.5
SWEEP_RATIO = 0.606
SWEEP_BOUND = SWEEP_RATIO + 0.5 * (1.0 - SWEEP_RATIO)


@pytest.fixture(scope="module")
def places(orc, oscene, oroute):
    comp = orc.Computation(oscene, oroute["lamps"], N, oroute["lightHeight"], oroute["lightLength"], oroute["lightIntensity"])
    return comp.lamp_world_pos(oroute["lamps"][0]), comp.lamp_world_pos(oroute["lamps"][1])


def _both_modes(orc, oscene, oroute, frm, to, counts):
    out = []
    for seed in SEEDS:
        row = {}
        for name, mode in (("independent", gs.INDEPENDENT), ("stratified", gs.STRATIFIED)):
            e, _, _ = gs.gather(orc, oscene, frm, to, oroute["lightLength"], S, seed, N, mode=mode)
            row[name] = gs.quality(e, counts)
        print("seed %d: independent %.3f / %.3f / %.3f rms %.3f lit %d; stratified %.3f / %.3f / %.3f rms %.3f lit %d" % (
            (seed,) + row["independent"] + row["stratified"]))
        out.append(row)
    return out


def test_the_stratified_estimator_at_a_stop(orc, oscene, oroute, places):
    """Route position 0, N = 2^21 oracle photons, the triangles with >= 400 of them, S = 16, gather seeds 0-2: the stratified
    median sits on 1, its 5th-95th band is at most half as wide as the independent one of the same seed, and more of the
    zero-photon triangles get an estimate."""
    gr.check_rng(orc)
    counts = gs.photon_counts(orc, oscene, places[0], places[0], oroute["lightLength"], N)
    assert (counts >= 400).sum() > 500 and (counts == 0).sum() > 0.4 * oscene.T
    for seed, row in zip(SEEDS, _both_modes(orc, oscene, oroute, places[0], places[0], counts)):
        i5, _, i95, _, ilit = row["independent"]
        s5, s50, s95, _, slit = row["stratified"]
        assert abs(s50 - 1.0) <= BAND, "seed %d: stratified median %.4f" % (seed, s50)
        assert (s95 - s5) <= STOP_BOUND * (i95 - i5), "seed %d: widths %.4f against %.4f" % (seed, s95 - s5, i95 - i5)
        assert slit > ilit, "seed %d: %d zero-photon triangles with an estimate against %d" % (seed, slit, ilit)


def test_the_stratified_estimator_on_a_sweep(orc, oscene, oroute, places):
    """The sweep from position 0 to 1 against 2^21 oracle photons with origins shifted along the segment: the lamp moves, so
    u_m matters as well; the stratified band is narrower than the independent one of the same seed by the recorded ratio."""
    counts = gs.photon_counts(orc, oscene, places[0], places[1], oroute["lightLength"], N)
    assert (counts >= 400).sum() > 500
    for seed, row in zip(SEEDS, _both_modes(orc, oscene, oroute, places[0], places[1], counts)):
        i5, _, i95, _, _ = row["independent"]
        s5, _, s95, _, _ = row["stratified"]
        assert (s95 - s5) < (i95 - i5)
        assert (s95 - s5) <= SWEEP_BOUND * (i95 - i5), "seed %d: widths %.4f against %.4f" % (seed, s95 - s5, i95 - i5)
