"""No GPU: the host-only parts of the adaptive gather (include/uvrt.h uvrt_gather_refine) -- the symbols in both
libraries and in the bindings, the layouts of both structs against a C compiler's, the refusals that need no device, the
CLI's and the binding's refusals, the count rule and the merge on hand-made values against exact fractions
(tests/gather_refine_restate.py) -- and the estimator itself against the oracle's photon counts.

Measured by test_the_refined_estimate_against_photons (S0 = 16, tau = 0.1, at most 64 extra samples, 2^21 oracle photons, the
triangles with >= 400 of them, gather seeds 0 and 1, z = 2; tests/tools/gather_refine_quality.py gives the same figures for seeds
0-7 and tau = 0.2 / 0.1 / 0.05): see the table in DESIGN.md 16."""
import ctypes as C
import inspect
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import gather_edge_scene as ge
import gather_refine_restate as gf
import gather_restate as gr
import gather_stratified_restate as gs
import gather_variance_restate as gv
from conftest import GLB, GOLDEN, ROOT
from plan_options_pin import check_plan_option

NEW = ("uvrt_gather_refine", "uvrt_read_gather_extra", "uvrt_refine_counts")
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
    assert len(by_name["uvrt_gather_refine"]) == 5 and len(by_name["uvrt_read_gather_extra"]) == 4
    assert len(by_name["uvrt_refine_counts"]) == 6 and by_name["uvrt_refine_counts"][1] is C.c_int32
    for m in ("gather_refine", "read_gather_extra", "refine_counts"):
        assert hasattr(pkg.capi.Ctx, m)
    from uvrt_amd import host
    hosts = {n: a for n, _, a in host.SYMBOLS}
    n = "uvrt_host_rt_set_gather_refine"
    assert [k for k, _, _ in host.SYMBOLS].count(n) == 1 and hasattr(host.lib(), n)
    check_plan_option(host, "gather_rel_error", C.c_double, 0.0)
    check_plan_option(host, "gather_max_extra", C.c_int, 64)
    assert hosts["uvrt_host_rt_set_gather_refine"][1:] == [C.c_double, C.c_int]
    assert hasattr(host.RayTracer, "set_gather_refine")


def test_struct_layouts_match_the_c_compiler(pkg, tmp_path):
    """sizeof and every offsetof of uvrt_refine_params and uvrt_refine_report, from a program compiled against include/uvrt.h"""
    src = tmp_path / "layout.c"
    src.write_text("""#include <stddef.h>
#include <stdio.h>
#include "uvrt.h"
int main(void)
{
    printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(uvrt_refine_params), offsetof(uvrt_refine_params, rel_error),
           offsetof(uvrt_refine_params, min_expected), offsetof(uvrt_refine_params, max_extra), offsetof(uvrt_refine_params, seed),
           offsetof(uvrt_refine_params, reserved));
    printf("%zu %zu %zu %zu\\n", sizeof(uvrt_refine_report), offsetof(uvrt_refine_report, extra_rays),
           offsetof(uvrt_refine_report, refined), offsetof(uvrt_refine_report, reserved));
    return 0;
}
""")
    exe = tmp_path / "layout"
    subprocess.run([os.environ.get("CC", "cc"), "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    P, R = pkg.capi.RefineParams, pkg.capi.RefineReport
    assert [int(v) for v in lines[0].split()] == [C.sizeof(P), P.rel_error.offset, P.min_expected.offset, P.max_extra.offset,
                                                  P.seed.offset, P.reserved.offset] == [32, 0, 8, 16, 20, 24]
    assert [int(v) for v in lines[1].split()] == [C.sizeof(R), R.extra_rays.offset, R.refined.offset, R.reserved.offset] == [16, 0, 8, 12]


def test_null_arguments_are_refused_without_a_gpu(pkg):
    buf = np.full(4, 7, dtype=np.int32)
    prm = pkg.capi.RefineParams(0.1, 0.0, 64, 1)
    rep = pkg.capi.RefineReport(7, 7, 7)
    for dev in (False, True):
        L = pkg.capi.lib(dev)
        calls = (("uvrt_gather_refine", lambda: L.uvrt_gather_refine(None, C.byref(prm), 0, 4, C.byref(rep))),
                 ("uvrt_gather_refine", lambda: L.uvrt_gather_refine(None, None, 0, 4, None)),
                 ("uvrt_read_gather_extra", lambda: L.uvrt_read_gather_extra(None, buf.ctypes.data, 0, 4)),
                 ("uvrt_refine_counts", lambda: L.uvrt_refine_counts(None, 4, C.byref(prm), 0, 3, buf.ctypes.data)),
                 ("uvrt_refine_counts", lambda: L.uvrt_refine_counts(None, 4, None, 0, 3, None)))
        for name, call in calls:
            assert call() == -1 and name.encode() in L.uvrt_last_error(), name          # UVRT_ERR_INVALID
    assert np.all(buf == 7) and (rep.extra_rays, rep.refined, rep.reserved) == (7, 7, 7)


def test_plan_durations_refuses_a_refine_it_cannot_run(pkg):
    """PlanDurationsRefined takes the refine's two options in front of PlanDurations' own, which keeps its signature; the
    binding refuses what PlanOptions calls fatal before it reaches the library"""
    from uvrt_amd import host
    sig = inspect.signature(host.RayTracer.PlanDurationsRefined)
    assert list(sig.parameters)[1:3] == ["gather_rel_error", "gather_max_extra"] and sig.parameters["gather_max_extra"].default == 64
    assert list(inspect.signature(host.RayTracer.PlanDurations).parameters)[-1] == "gather_confidence"
    rt = host.RayTracer(init=False)
    try:
        assert rt.gatherRelError == 0.0 and rt.gatherMaxExtra == 64
        rt.set_gather_refine(0.125, 32)
        assert rt.gatherRelError == 0.125 and rt.gatherMaxExtra == 32
        rt.gatherRelError = 0.0
        rt.gatherMaxExtra = 64
        assert rt.gatherRelError == 0.0 and rt.gatherMaxExtra == 64
        for tau, kw in ((0.1, {}), (0.1, dict(gather_samples=1)), (-0.1, dict(gather_samples=16)), (float("nan"), dict(gather_samples=16)),
                        (float("inf"), dict(gather_samples=16))):
            with pytest.raises(ValueError, match="gather_rel_error"):
                rt.PlanDurationsRefined(tau, **kw)
        for extra in (0, 1, 3, 48, 8192, -64):
            with pytest.raises(ValueError, match="gather_max_extra"):
                rt.PlanDurationsRefined(0.1, extra, gather_samples=16)
        with pytest.raises(TypeError, match="unknown arguments"):
            rt.PlanDurationsRefined(0.1, gather_sample=16)
    finally:
        rt.close()


def test_cli_refuses_a_refine_without_a_gather_it_can_refine(pkg):
    cli = os.path.join(os.path.dirname(pkg.capi.LIB_PATH), "uvrt_cli")
    base = [cli, "--room", GLB, "--route-dir", GOLDEN, "--route", "lange_route"]
    for extra in (["--gather-refine", "0.1"], ["--plan", "50", "--gather-refine", "0.1"], ["--gather", "1", "--gather-refine", "0.1"],
                  ["--plan-gather", "1", "--gather-refine", "0.1"], ["--gather-refine", "0.1", "--gather", "0"],
                  ["--gather", "16", "--gather-refine", "0"], ["--gather", "16", "--gather-refine", "-0.1"],
                  ["--gather", "16", "--gather-refine", "nan"], ["--gather", "16", "--gather-refine", "inf"],
                  ["--gather", "16", "--gather-refine", "tenth"], ["--gather", "16", "--gather-refine", "0.1x"],
                  ["--gather", "16", "--gather-refine", "0.1,"], ["--gather", "16", "--gather-refine", "0.1,3"],
                  ["--gather", "16", "--gather-refine", "0.1,1"], ["--gather", "16", "--gather-refine", "0.1,8192"],
                  ["--plan-gather", "16", "--gather-refine", "0.1,64x"]):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2, (extra, r.stdout, r.stderr)
        assert "--gather-refine" in r.stderr and "--plan-gather S" in r.stderr, (extra, r.stderr)
    r = subprocess.run(base + ["--gather", "16", "--gather-refine"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2


# ---------------------------------------------------------------- the count rule and the merge on hand-made values
def _n(X0, V0, S0=16, tau=0.25, min_expected=0.0, max_extra=64, nn=1.0):
    return int(gf.count_rule([X0], [V0], [nn], S0, tau, min_expected, max_extra)[0])


def _want(X0, V0, S0, tau, max_extra):
    """the rule in exact arithmetic, for values at which every f64 step of it is exact"""
    r = Fraction(tau) * Fraction(X0)
    want = Fraction(S0) * (Fraction(V0) / (r * r) - 1)
    want = -(-want.numerator // want.denominator)           # ceil
    if want < 1:
        return 0
    if want >= max_extra:
        return max_extra
    n = 2
    while n < max(want, 2):
        n *= 2
    return n


def test_the_count_rule_against_fractions():
    """X0 = 4 and tau = 0.25 make r = 1, so want = S0 * (V0 - 1) exactly: want exactly 1, below it, a power of two and one above
    it, at and above the cap; and other exact settings"""
    cases = {1.0: 0, 1.0 + 1.0 / 32: 2, 1.0 + 1.0 / 16: 2, 1.0 + 2.0 / 16: 2, 1.0 + 3.0 / 16: 4, 1.5: 8, 1.0 + 9.0 / 16: 16, 2.0: 16,
             1.0 + 17.0 / 16: 32, 1.0 + 63.0 / 16: 64, 5.0: 64, 100.0: 64, 0.5: 0}
    for V0, n in cases.items():
        assert _n(4.0, V0) == n == _want(4.0, V0, 16, 0.25, 64), V0
    for X0, V0, S0, tau, cap in ((8.0, 3.0, 4, 0.125, 16), (8.0, 3.0, 4, 0.125, 4), (2.0, 0.75, 2, 0.5, 8), (3.0, 2.25, 16, 0.5, 4096),
                                 (1.0, 2.0 ** 20, 16, 1.0, 4096), (1.0, 2.0 ** -20, 16, 2.0 ** -12, 64)):
        assert _n(X0, V0, S0, tau, 0.0, cap) == _want(X0, V0, S0, tau, cap), (X0, V0, S0, tau, cap)
    for cap in (2, 4, 4096):
        assert _n(4.0, 1000.0, max_extra=cap) == cap
        assert _n(4.0, 1.0 + 1.0 / 16, max_extra=cap) == 2


def test_the_count_rule_at_its_edges():
    inf, nan, tiny = float("inf"), float("nan"), 5e-324
    assert _n(4.0, inf) == 64                               # want = inf: the cap
    assert _n(tiny, 1.0) == 64                              # r * r underflows to 0: V0 / 0 = inf
    assert _n(tiny, tiny) == 64
    assert _n(1e200, 1.0) == 0                              # r * r overflows: V0 / inf = 0, want = -S0
    assert _n(1e200, inf) == 0                              # inf / inf: NaN, not >= 1
    assert _n(nan, 1.0) == 0 and _n(4.0, nan) == 0 and _n(inf, inf) == 0
    assert _n(0.0, 1.0) == 0 and _n(-4.0, 100.0) == 0 and _n(4.0, 0.0) == 0 and _n(4.0, -1.0) == 0
    assert _n(4.0, 100.0, nn=0.0) == 0                      # a triangle without area
    assert _n(4.0, 100.0, min_expected=4.0) == 64 and _n(4.0, 100.0, min_expected=4.000001) == 0
    n = gf.count_rule([4.0, 4.0, 0.0], [1.5, 100.0, 1.0], [1.0, 1.0, 1.0], 16, 0.25, 0.0, 64)
    assert n.dtype == np.int32 and n.tolist() == [8, 64, 0]


def test_crafted_rows_pin_the_count_rule():
    """gather_edge_scene.count_rule_rows, the planes tests/test_gpu_refine_gather_edges.py writes: where a row pins `want`, the restated
    f64 `want`, the exact one and the rule's n_t agree with it; the rows of zeros, subnormals, inf, NaN and negatives give what
    the header's rule says by hand"""
    for S0 in (2, 3, 16):
        for cap in (2, 64, 4096):
            X, V, pinned = ge.count_rule_rows(S0, cap)
            w = ge.restated_want(X, V, S0)
            n = gf.count_rule(X, V, np.ones(X.size), S0, ge.ROW_TAU, 0.0, cap)
            assert sorted({p for p in pinned if p is not None}) == sorted(set(ge.ROW_WANTS[:-1]) | {cap - 1, cap, cap + 1})
            for k, p in enumerate(pinned):
                if p is None:
                    continue
                exact = Fraction(S0) * (Fraction(V[k]) - 1)
                assert w[k] == p == -(-exact.numerator // exact.denominator), (S0, cap, k, V[k])
                want_n = 0 if p < 1 else cap if p >= cap else 1 << (max(p, 2) - 1).bit_length()
                assert n[k] == want_n == _want(X[k], V[k], S0, ge.ROW_TAU, cap), (S0, cap, k, p)
            big = np.flatnonzero((w > 1e299) & np.isfinite(w))  # want = 1e300, both forms
            assert big.size == 2 and n[big].tolist() == [cap, cap]
            tail = n[-20:].tolist()
            assert tail[:8] == [0, 0, cap, cap, 0, 0, 0, 0], tail         # X0: +0, -0, subnormal, 1e-200, inf, NaN, negative, 1e200
            assert tail[8:14] == [0, 0, 0, 0, cap, 0], tail               # V0: +0, -0, subnormal, negative, inf, NaN
            assert tail[14:17] == [0, 0, cap] and np.isnan(w[-6:-4]).all() and np.isposinf(w[-4]), tail
            assert all(v > 0 for v in tail[17:]), tail                    # X0 about min_expected, none set
            assert gf.count_rule(X[-3:], V[-3:], np.ones(3), S0, ge.ROW_TAU, ge.ROW_X0, cap).tolist() == [0] + tail[18:]
            assert gf.count_rule(X, V, np.zeros(X.size), S0, ge.ROW_TAU, 0.0, cap).tolist() == [0] * X.size


def test_the_edge_scene_reaches_what_the_room_does_not(orc):
    """gather_edge_scene.edge_scene on the restatements: the triangles without area are the named ones, a stop without length
    leaves rays without a direction by underflow and by overflow, weights are NaN and no plane entry is; the refined sub-range
    holds every n_t from 2 to 4096 in both modes with fewer than 300 000 extra rays"""
    sc = ge.edge_scene(orc)
    _, _, _, nn = gr.tri_normals(sc.tris)
    assert np.array_equal(np.flatnonzero(nn == 0.0), sc.no_area) and sc.no_area.size == 5 and sc.T == ge.EDGE_SOUP + len(ge.HAND)
    assert sc.sub_range[0] in sc.hand.values() and sum(sc.sub_range) - 1 in sc.hand.values() and sum(sc.sub_range) == sc.T
    rays, w = gs.samples(orc, sc.tris, ge.LAMP, ge.LAMP, 0.0, 4, 3, 0, None, gs.INDEPENDENT)
    untraced = (rays["dist"] == 0).reshape(sc.T, 4).sum(axis=1)
    assert untraced[sc.hand["tiny at the foot"]] == 4 and nn[sc.hand["tiny at the foot"]] > 0        # underflow: r = 0, R > 0
    assert untraced[sc.hand["far and huge"]] == 4 and np.isfinite(nn[sc.hand["far and huge"]])       # overflow: r = inf
    assert np.isnan(w).sum() >= 4
    first, count = sc.sub_range
    for mode, tau in ((gv.STRATIFIED, 0.05), (gv.INDEPENDENT, 0.02)):
        e, v, n, _, _ = gf.gather_and_refine(orc, sc, ge.LAMP, ge.LAMP, 1.0, 4, 3, 1 << 20, mode, tau, 4096, first=first, count=count)
        assert sorted(set(n.tolist())) == [0] + [2 << k for k in range(12)] and n.sum() < 300000, (mode, int(n.sum()))
        assert np.isfinite(e).all() and np.isfinite(v).all() and not n[sc.no_area - first].any()


def test_the_merge_against_fractions():
    """values with few bits: every product and sum exact, the two divisions the only roundings"""
    for X0, V0, X1, V1, S0, n in ((4.0, 1.5, 3.0, 0.75, 16, 8), (1.0, 0.25, 0.0, 0.0, 4, 16), (0.375, 2.0 ** -20, 0.5, 2.0 ** -22, 2, 2),
                                  (7.0, 3.0, 9.0, 5.0, 16, 64), (2.0 ** 40, 2.0 ** 60, 2.0 ** 39, 2.0 ** 58, 3, 4)):
        e, v = gf.merge(np.float64(X0), np.float64(V0), np.float64(X1), np.float64(V1), S0, n)
        tot = S0 + n
        assert float(e) == float((S0 * Fraction(X0) + n * Fraction(X1)) / tot), (X0, X1, S0, n)
        assert float(v) == float((S0 * S0 * Fraction(V0) + n * n * Fraction(V1)) / (tot * tot)), (V0, V1, S0, n)
    # equal estimates stay; the variance of two equally certain halves halves
    e, v = gf.merge(np.float64(3.0), np.float64(2.0), np.float64(3.0), np.float64(2.0), 16, 16)
    assert float(e) == 3.0 and float(v) == 1.0


def test_refine_on_the_room_is_a_gather_of_its_own(orc, oscene, oroute):
    """the whole restated refine on a small range: a triangle with n_t extra samples holds the merge of its first pass with a
    plain gather of n_t samples at the refine's seed; one with none keeps every bit; the range's cut into calls shows nowhere"""
    comp = orc.Computation(oscene, oroute["lamps"], 1 << 20, oroute["lightHeight"], oroute["lightLength"], oroute["lightIntensity"])
    frm, to = comp.lamp_world_pos(oroute["lamps"][0]), comp.lamp_world_pos(oroute["lamps"][1])
    length, N, first, count = oroute["lightLength"], 1 << 20, 100, 400
    for mode in (gv.INDEPENDENT, gv.STRATIFIED):
        e, v, n, e0, v0 = gf.gather_and_refine(orc, oscene, frm, to, length, 4, 3, N, mode, 0.25, 16, first=first, count=count)
        assert set(n.tolist()) >= {0, 16} and len(set(n.tolist())) >= 3 and same_bits(e[n == 0], e0[n == 0]) and same_bits(v[n == 0], v0[n == 0])
        for k in sorted(set(n.tolist()) - {0}):
            e1, v1, _ = gv.gather(orc, oscene, frm, to, length, k, ~3 & 0xFFFFFFFF, N, mode, first=first, count=count)
            we, wv = gf.merge(e0, v0, e1, v1, 4, k)
            assert same_bits(e[n == k], we[n == k]) and same_bits(v[n == k], wv[n == k]), (mode, k)
        # two calls over the halves of the range
        E, V = np.zeros(oscene.T), np.zeros(oscene.T)
        E[first:first + count], V[first:first + count] = e0, v0
        a = gf.refine(orc, oscene, frm, to, length, 4, mode, N, E, V, 0.25, 16, ~3 & 0xFFFFFFFF, first=first, count=150)
        b = gf.refine(orc, oscene, frm, to, length, 4, mode, N, a[0], a[1], 0.25, 16, ~3 & 0xFFFFFFFF, first=first + 150, count=count - 150)
        assert same_bits(b[0][first:first + count], e) and same_bits(b[1][first:first + count], v)
        assert same_bits((a[2] + b[2])[first:first + count], n) and not b[2][:first + 150].any()


def same_bits(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


# ---------------------------------------------------------------- the estimator against the oracle
N = 1 << 21
S0 = 16
TAU = 0.1
MAX_EXTRA = 64
SEEDS = (0, 1)
MEDIAN_RATIO = 0.0705           # the project's bound on |median(expected / count) - 1|
COVER_Z2 = 0.95                 # tests/test_gather_variance_cpu.py's condition
GAIN_STRATIFIED_STOP = 0.02     # median lo / count at z = 2 above the unrefined one: the stratified stop is tight already
GAIN_ELSEWHERE = 0.15


@pytest.fixture(scope="module")
def places(orc, oscene, oroute):
    comp = orc.Computation(oscene, oroute["lamps"], N, oroute["lightHeight"], oroute["lightLength"], oroute["lightIntensity"])
    return comp.lamp_world_pos(oroute["lamps"][0]), comp.lamp_world_pos(oroute["lamps"][1])


@pytest.mark.parametrize("case", ["stop", "sweep"])
def test_the_refined_estimate_against_photons(orc, oscene, oroute, places, case):
    """Route position 0 (stop) and the sweep 0 -> 1 against 2^21 oracle photons, the triangles with >= 400 of them, S0 = 16,
    tau = 0.1, at most 64 extra samples, gather seeds 0 and 1 (the extra samples' seed is ~seed), both modes: the median of
    expected / count stays within 0.0705 of 1, the count is >= expected - 2 sqrt(variance) on at least 95 % of the triangles, and
    the median of that bound over the count rises by at least 0.02 at the stratified stop and by at least 0.15 elsewhere."""
    gr.check_rng(orc)
    frm, to = places[0], places[0] if case == "stop" else places[1]
    counts = gs.photon_counts(orc, oscene, frm, to, oroute["lightLength"], N)
    sel = counts >= 400
    assert sel.sum() > 500
    for seed in SEEDS:
        for name, mode in (("independent", gv.INDEPENDENT), ("stratified", gv.STRATIFIED)):
            e, v, n, e0, v0 = gf.gather_and_refine(orc, oscene, frm, to, oroute["lightLength"], S0, seed, N, mode, TAU, MAX_EXTRA)
            assert np.all(np.isfinite(v)) and np.all(v >= 0.0) and np.all(np.isfinite(e))
            _, tight0, zero0 = gv.cover_and_tightness(e0, v0, counts, 2.0)
            cover, tight, zero = gv.cover_and_tightness(e, v, counts, 2.0)
            ratio = float(np.median(e[sel] / counts[sel]))
            line = "%s seed %d %s: %d extra rays (mean %.1f); median expected/count %.4f; cover z=2 %.4f; median lo/count %.4f -> %.4f; " \
                   "zero bounds %.4f -> %.4f" % (case, seed, name, int(n.sum()), n.sum() / oscene.T, ratio, cover, tight0, tight, zero0, zero)
            print(line)
            assert abs(ratio - 1.0) <= MEDIAN_RATIO, line
            assert cover >= COVER_Z2, line
            gain = GAIN_STRATIFIED_STOP if (mode == gv.STRATIFIED and case == "stop") else GAIN_ELSEWHERE
            assert tight >= tight0 + gain, line
