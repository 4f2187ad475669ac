"""No GPU: the host-only parts of the gather's variance plane and of planning for a lower confidence bound (include/uvrt.h
uvrt_set_gather_variance, uvrt_plan_lower_confidence) -- the symbols in both libraries and in the bindings, the
refusals that need no device, the CLI's refusals of --plan-confidence, the rule on hand-made samples
(tests/gather_variance_restate.py) -- and the estimator itself against the oracle's photon counts.

Measured by test_the_bound_covers_the_truth (S = 16, 2^21 oracle photons, the triangles with >= 400 of them, gather seeds 0
and 1; tests/tools/gather_confidence.py gives the same figures for seeds 0-7, profiles/r14/r14_gather_confidence.json):

    case   mode         cover z=0        cover z=2        median lo/count z=2   (stratified samples, sample variance)
    stop   independent  0.5190 0.5305    0.9655 0.9724    0.4630 0.4571
    stop   stratified   0.5017 0.5121    0.9919 0.9965    0.7883 0.7926         0.4444 0.4497
    sweep  independent  0.5783 0.5619    0.9903 0.9913    0.3931 0.3528
    sweep  stratified   0.5590 0.5667    0.9952 0.9932    0.4937 0.4890         0.3330 0.3329
"""
import ctypes as C
import inspect
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import gather_restate as gr
import gather_stratified_restate as gs
import gather_variance_restate as gv
from conftest import GLB, GOLDEN
from plan_options_pin import check_plan_option

NEW = ("uvrt_set_gather_variance", "uvrt_get_gather_variance", "uvrt_read_variance", "uvrt_write_variance",
       "uvrt_plan_begin_expected_variance", "uvrt_plan_read_exposure_variance", "uvrt_plan_lower_confidence")
f32 = np.float32


def test_symbols_are_bound_and_resolve_in_both_libraries(pkg):
    names = [name for name, _, _ in pkg.capi.SYMBOLS]
    for n in NEW:
        assert names.count(n) == 1
        for path in (pkg.capi.LIB_PATH, pkg.capi.LIB_DEV_PATH):
            assert hasattr(C.CDLL(path), n), (path, n)
        for dev in (False, True):
            assert getattr(pkg.capi.lib(dev), n).restype is C.c_int
    by_name = {n: a for n, _, a in pkg.capi.SYMBOLS}
    assert by_name["uvrt_plan_lower_confidence"][1] is C.c_double
    for m in ("set_gather_variance", "get_gather_variance", "read_variance", "write_variance", "plan_begin_expected_variance",
              "plan_read_exposure_variance", "plan_lower_confidence"):
        assert hasattr(pkg.capi.Ctx, m)
    from uvrt_amd import host
    check_plan_option(host, "gather_confidence", C.c_double, 0.0)


def test_null_arguments_are_refused_without_a_gpu(pkg):
    buf = np.full(4, 7.0, dtype=np.float64)
    on = C.c_int32(7)
    for dev in (False, True):
        L = pkg.capi.lib(dev)
        calls = (("uvrt_set_gather_variance", lambda: L.uvrt_set_gather_variance(None, 1)),
                 ("uvrt_get_gather_variance", lambda: L.uvrt_get_gather_variance(None, C.byref(on))),
                 ("uvrt_read_variance", lambda: L.uvrt_read_variance(None, buf.ctypes.data, 0, 4)),
                 ("uvrt_write_variance", lambda: L.uvrt_write_variance(None, buf.ctypes.data, 0, 4)),
                 ("uvrt_plan_begin_expected_variance", lambda: L.uvrt_plan_begin_expected_variance(None, 3)),
                 ("uvrt_plan_read_exposure_variance", lambda: L.uvrt_plan_read_exposure_variance(None, 0, buf.ctypes.data, 0, 4)),
                 ("uvrt_plan_lower_confidence", lambda: L.uvrt_plan_lower_confidence(None, 2.0)))
        for name, call in calls:
            assert call() == -1 and name.encode() in L.uvrt_last_error(), name          # UVRT_ERR_INVALID
    assert on.value == 7 and np.all(buf == 7.0)


def test_plan_durations_refuses_a_confidence_it_cannot_plan_for(pkg):
    """gather_confidence is PlanDurations' last argument, 0 by default; the binding refuses what PlanOptions calls fatal before
    it reaches the library"""
    from uvrt_amd import host
    sig = inspect.signature(host.RayTracer.PlanDurations)
    assert list(sig.parameters)[-1] == "gather_confidence" and sig.parameters["gather_confidence"].default == 0.0
    assert sig.parameters["gather_samples"].default == 0 and sig.parameters["gather_sampling"].default == 0
    rt = host.RayTracer(init=False)
    try:
        for kw in (dict(gather_confidence=2.0), dict(gather_samples=1, gather_confidence=2.0),
                   dict(gather_samples=16, gather_confidence=-1.0), dict(gather_samples=16, gather_confidence=float("nan")),
                   dict(gather_samples=16, gather_confidence=float("inf"))):
            with pytest.raises(ValueError, match="gather_confidence"):
                rt.PlanDurations(**kw)
    finally:
        rt.close()


def test_cli_refuses_plan_confidence_without_a_gather_plan_it_can_bound(pkg):
    cli = os.path.join(os.path.dirname(pkg.capi.LIB_PATH), "uvrt_cli")
    base = [cli, "--room", GLB, "--route-dir", GOLDEN, "--route", "lange_route"]
    for extra in (["--plan-confidence", "2"], ["--plan", "50", "--plan-confidence", "2"], ["--gather", "16", "--plan-confidence", "2"],
                  ["--plan-gather", "1", "--plan-confidence", "2"], ["--plan-confidence", "2", "--plan-gather", "1"],
                  ["--plan-gather", "16", "--plan-confidence", "-1"], ["--plan-gather", "16", "--plan-confidence", "-0.5"],
                  ["--plan-gather", "16", "--plan-confidence", "nan"], ["--plan-gather", "16", "--plan-confidence", "inf"],
                  ["--plan-gather", "16", "--plan-confidence", "two"], ["--plan-gather", "16", "--plan-confidence", "2x"]):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2, (extra, r.stdout, r.stderr)
        assert "--plan-confidence" in r.stderr and "--plan-gather S" in r.stderr, (extra, r.stderr)
    r = subprocess.run(base + ["--plan-gather", "16", "--plan-confidence"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2


# ---------------------------------------------------------------- the rule on hand-made samples
def _v(x, mode):
    x = np.asarray(x, dtype=np.float64).reshape(1, -1)
    _, _, q = gv.mean_and_q(x, mode)
    return float(gv.v_of_q(q, x.shape[1], mode)[0])


@pytest.mark.parametrize("S", [2, 3, 16, 64])
def test_equal_samples_have_no_variance(S):
    """exactly 0 by successive differences whatever the value; exactly 0 by the sample variance where S * w is exact (then m is
    w itself), else what the rounding of the sum leaves: (x - m)^2 <= (S * 2^-53 * w)^2 per sample, so v below that"""
    for w in (0.0, 0.375, 3.0, 1.0 / 3.0, 0.1, 1e-300, 1e150):
        assert _v([w] * S, gv.STRATIFIED) == 0.0, (S, w)
        v = _v([w] * S, gv.INDEPENDENT)
        if w in (0.0, 0.375, 3.0):
            assert v == 0.0, (S, w)
        else:
            assert 0.0 <= v <= (S * 2.0 ** -53 * w) ** 2, (S, w, v)


@pytest.mark.parametrize("S", [2, 3, 5, 16, 4096])
def test_one_visibility_edge_in_the_stratified_rule(S):
    """x = w on one side of the edge and 0 on the other: q = w^2, so v = w^2 / (2 S (S-1)), against exact fractions (w has few
    bits, so w*w is exact and the one division is the one rounding)"""
    for w in (0.375, 3.0, 2.0 ** -40, 1.0 + 2.0 ** -20):
        want = float(Fraction(w) ** 2 / (2 * S * (S - 1)))
        for k in sorted({1, S // 2, S - 1} - {0}):                    # where the edge sits does not matter
            assert _v([w] * k + [0.0] * (S - k), gv.STRATIFIED) == want, (S, w, k)
            assert _v([0.0] * (S - k) + [w] * k, gv.STRATIFIED) == want, (S, w, k)
    # conservative against the largest true variance of one sample per stratum, w^2 / (4 S^2)
    assert Fraction(1, 2 * S * (S - 1)) >= Fraction(1, 4 * S * S)


def test_two_samples():
    """S = 2: both rules give (a - b)^2 / 4; exact for values with few bits"""
    for a, b in ((0.5, 0.25), (0.0, 3.0), (1.5, 1.5), (2.0 ** -30, 0.0)):
        want = float((Fraction(a) - Fraction(b)) ** 2 / 4)
        assert _v([a, b], gv.INDEPENDENT) == want and _v([a, b], gv.STRATIFIED) == want, (a, b)
        assert _v([b, a], gv.INDEPENDENT) == want and _v([b, a], gv.STRATIFIED) == want, (a, b)


def test_the_independent_rule_against_fractions():
    """S = 4, x = (1, 0, 0, 1) / 4 + (0, 1, 2, 3) / 8: every step exact in f64 but the last division"""
    x = [0.25, 0.125, 0.25, 0.625]
    m = sum(Fraction(v) for v in x) / 4
    want = float(sum((Fraction(v) - m) ** 2 for v in x) / 12)
    assert _v(x, gv.INDEPENDENT) == want
    want_s = float(sum((Fraction(x[s]) - Fraction(x[s - 1])) ** 2 for s in range(1, 4)) / 24)
    assert _v(x, gv.STRATIFIED) == want_s and want_s != want


def test_reduce_var_scales_with_the_triangle_and_skips_one_without_area():
    """variance = (c*c) * v with c = photons_equiv * (0.5*nn); a triangle without area has neither estimate nor variance, and
    the expected plane is gather_restate.reduce's bit for bit"""
    tris = np.zeros((2, 16), dtype=f32)
    tris[0, 4:7] = (2.0, 0.0, 0.0)              # e1 = (2, 0, 0), e2 = (0, 1, 0): nn = 2
    tris[0, 8:11] = (0.0, 1.0, 0.0)
    S, N = 4, 1 << 10
    w = np.array([0.5, 0.5, 0.25, 0.25, np.nan, np.nan, np.nan, np.nan])       # (0 / 0 weights of the degenerate triangle)
    occ = np.array([0, 1, 0, 0, 0, 0, 0, 0], dtype=np.uint8)
    for mode in (gv.INDEPENDENT, gv.STRATIFIED):
        e, v = gv.reduce_var(tris, w, occ, S, N, mode)
        assert e.tobytes() == gr.reduce(tris, w, occ, S, N).tobytes()
        c = float(N) * (0.5 * 2.0)
        assert e[0] == c * (1.0 / 4.0) and v[0] == (c * c) * _v([0.5, 0.0, 0.25, 0.25], mode) and v[0] > 0
        assert e[1] == 0.0 and v[1] == 0.0
    lo = gv.lower_confidence([4.0, 1.0, 0.0, 9.0], [1.0, 4.0, 0.0, 0.0], 2.0)
    assert lo.tolist() == [2.0, 0.0, 0.0, 9.0]
    X = np.array([4.0, 1.0, 0.0])
    assert gv.lower_confidence(X, [1.0, 4.0, 0.0], 0.0).tobytes() == X.tobytes()


# ---------------------------------------------------------------- the estimator against the oracle
N = 1 << 21
S = 16
SEEDS = (0, 1)
COVER_Z2 = 0.95                 # the issue's: the CPU prototype's lowest cover at z = 2 is 0.9655 (independent, at the stop)
COVER_GAIN = 0.2                # cover(z = 2) - cover(z = 0): without a bound about half the rows sit below their estimate
TIGHTER = 0.15                  # stratified, at the stop: median lo / count above what the sample variance gives (0.79 vs 0.45)


@pytest.fixture(scope="module")
def places(orc, oscene, oroute):
    comp = orc.Computation(oscene, oroute["lamps"], N, oroute["lightHeight"], oroute["lightLength"], oroute["lightIntensity"])
    return comp.lamp_world_pos(oroute["lamps"][0]), comp.lamp_world_pos(oroute["lamps"][1])


@pytest.mark.parametrize("case", ["stop", "sweep"])
def test_the_bound_covers_the_truth(orc, oscene, oroute, places, case):
    """Route position 0 (stop) and the sweep 0 -> 1 against 2^21 oracle photons, the triangles with >= 400 of them, S = 16,
    gather seeds 0 and 1, both sampling modes: the count is >= expected - 2 sqrt(variance) on at least 95 % of them, at
    least 0.2 more than are >= the estimate itself; at the stop the stratified bound's median over the count is at least 0.15
    above what the sample variance would give on the same samples.  The figures are in the module's docstring."""
    gr.check_rng(orc)
    frm, to = places[0], places[0] if case == "stop" else places[1]
    counts = gs.photon_counts(orc, oscene, frm, to, oroute["lightLength"], N)
    assert (counts >= 400).sum() > 500
    _, _, _, nn = gr.tri_normals(np.ascontiguousarray(oscene.tris, dtype=f32))
    c = np.float64(N) * (0.5 * nn)
    for seed in SEEDS:
        for name, mode in (("independent", gv.INDEPENDENT), ("stratified", gv.STRATIFIED)):
            e, v, x = gv.gather(orc, oscene, frm, to, oroute["lightLength"], S, seed, N, mode)
            assert np.all(np.isfinite(v)) and np.all(v >= 0.0)
            cover0, _, _ = gv.cover_and_tightness(e, v, counts, 0.0)
            cover2, tight2, _ = gv.cover_and_tightness(e, v, counts, 2.0)
            line = "%s seed %d %s: cover z=0 %.4f, z=2 %.4f, median lo/count z=2 %.4f" % (case, seed, name, cover0, cover2, tight2)
            if mode == gv.STRATIFIED:
                vs = np.where(nn == 0.0, 0.0, (c * c) * gv.sample_variance_v(x))
                _, tight_sv, _ = gv.cover_and_tightness(e, vs, counts, 2.0)
                line += "; with the sample variance %.4f" % tight_sv
            print(line)
            assert cover2 >= COVER_Z2, line
            assert cover2 - cover0 >= COVER_GAIN, line
            if mode == gv.STRATIFIED and case == "stop":
                assert tight2 >= tight_sv + TIGHTER, line
