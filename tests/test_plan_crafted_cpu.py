"""No GPU: the crafted planning cases (tests/plan_crafted_cases.py) hold what they are for, judged on the restatement
(tests/plan_restate.py) alone; HiGHS agrees with the closed forms; the restricted LP of csrc/uvrt_plan_lp.h, alone in a g++
program, solves the row-scaled matrices of the closed-form cases -- those whose entries span more than 1e12 included, which a
pivot floor taken from the largest entry of the whole matrix called unbounded; the hook's symbol and its host-only refusals."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import plan_crafted_cases as cc
import plan_restate as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "small-project-uv-robot-ray-tracer_amd", "csrc")


def _classes(case, tag):
    _, lower, fixed = [s for s in case["solves"] if s[0] == tag][0]
    area = pr.areas(cc.make_tris(case["area_log2"]))
    return pr.classify(case["E"], area, mask=case["mask"], lower=lower, fixed=fixed, **case["prm"])


def test_the_scenes_have_the_areas_they_claim(orc):
    for case in [cc.case_A(), cc.case_C(17, 257)] + cc.closed_cases():
        tris, nodes, idx = cc.scene(orc, case)
        area = pr.areas(tris)
        for t, e in enumerate(case["area_log2"]):
            assert area[t] == (0.0 if e is None else np.float32(2.0 ** e)), (case["name"], t, e, area[t])
        assert sorted(int(i) for i in idx) == list(range(len(area)))
    assert any(e is None for e in cc.case_A()["area_log2"]) and any(e is None for e in cc.case_C(17, 257)["area_log2"])


def test_every_class_occurs_in_every_full_block_of_A():
    """T = 513 is two blocks of 256 and one of a single triangle: the full blocks hold every class, the last an active row"""
    case = cc.case_A()
    assert case["E"].shape == (4, cc.A_T)
    for tag, classes in (("plain", range(4)), ("bounded", range(6))):
        c = _classes(case, tag)
        for first in (0, 256):
            have = set(c["cls"][first:first + 256].tolist())
            assert have == set(classes), (tag, first, have)
        assert c["cls"][512] == 0
    c = _classes(case, "bounded")
    # the rows where more than one test fires: masked rows that would be any other class, rows without area that hold photons
    unmasked = pr.classify(case["E"], c["area"], mask=None, lower=cc.A_LOWER, fixed=cc.A_FIXED, **case["prm"])["cls"]
    assert set(unmasked[c["cls"] == 3].tolist()) == {0, 1, 2, 4, 5}
    tot = pr.row_sums(case["E"])
    assert np.any((c["cls"] == 1) & (tot >= 8)) and np.any((c["cls"] == 1) & (tot == 0) & (c["area"] > 0))
    b = c["base"] * c["r"]
    assert np.any((c["cls"] == 4) & (b == 1.0)) and np.any((c["cls"] == 4) & (b > 1.0))
    assert np.any((c["cls"] == 5) & (b < 1.0)) and np.any((c["cls"] == 2) & (b >= 1.0))
    # rho: clamped up to 1e-9 on one kind of row, kept at 2^-29 on the other
    kinds = np.array(case["kinds"])
    assert np.all(c["rho"][kinds == "rho clamped"] == 1e-9) and np.all(1.0 - b[kinds == "rho clamped"] == 2.0 ** -30)
    assert np.all(c["rho"][kinds == "rho not clamped"] == 2.0 ** -29)
    # the expected plan's row one ulp below min_photons is unresolved, as its 7 in the counts plan
    ulp = np.flatnonzero(kinds == "one ulp below min_photons (expected plan)")
    X = cc.matrix(case, True)
    cx = pr.classify(X, c["area"], mask=case["mask"], lower=cc.A_LOWER, fixed=cc.A_FIXED, **case["prm"])
    assert ulp.size > 0 and np.all(X[0, ulp] < 8.0) and np.all(X[0, ulp] > 7.999999) and np.all(cx["cls"][ulp] == 2)
    assert np.array_equal(cx["cls"], c["cls"])


def test_B_needs_the_64_bit_row_sum():
    for case in (cc.case_B2(), cc.case_B256()):
        c = _classes(case, "plain")
        tot = pr.row_sums(case["E"])
        assert c["cls"][0] == 0 and int(tot[0]) >= 2 ** 32
        wrapped = tot.astype(np.uint32)
        assert wrapped[0] == 0 or case["name"] == "B256"
    c, tot = _classes(cc.case_B256(), "plain"), pr.row_sums(cc.case_B256()["E"])
    assert int(tot[0]) == 256 * (2 ** 32 - 1) and int(tot[1]) == 2 ** 32 and list(c["cls"]) == [0, 0, 2]


def _highs(A):
    from scipy.optimize import linprog
    P = A.shape[1]
    r = linprog(np.ones(P), A_ub=-A, b_ub=-np.ones(A.shape[0]), bounds=[(0, None)] * P, method="highs")
    assert r.status == 0
    return r


def test_D_stays_under_the_old_floor_and_E_goes_beyond_it():
    for case in cc.closed_cases():
        tag = case["solves"][0][0]
        A, cols, c = cc.scaled_lp(case, tag, pr)
        span = A.max() / A[A > 0].min()
        assert (span > 1e12) == case["name"].startswith("E-"), (case["name"], span)
    # at D-range's optimum the small duration is below repair()'s 1e-7 d_max: it is zeroed, and the row check raises it again
    d = cc.case_D_range()["exact"]["plain"]
    assert d[0] / d.max() <= 1e-7


def test_highs_equals_the_closed_forms_of_D_and_solves_C():
    for case in cc.closed_cases():
        if not case["name"].startswith("D-"):
            continue
        A, cols, c = cc.scaled_lp(case, "plain", pr)
        r = _highs(A)
        exact = case["exact"]["plain"]
        total = 16.0 if case["name"] == "D-ones" else float(exact.sum())
        assert abs(r.fun - total) <= 1e-7 * total, (case["name"], r.fun, total)
        if case["name"] != "D-ones":
            assert np.all(A @ exact >= 1.0 - 1e-15)
    for P, T in cc.C_SIZES:
        case = cc.case_C(P, T)
        A, cols, c = cc.scaled_lp(case, "plain", pr)
        assert A.shape[0] > 0, (P, T)
        r = _highs(A)
        assert r.fun > 0
        if T >= 255:
            cb = _classes(case, "bounded")
            assert set(cb["cls"].tolist()) >= {0, 1, 4}, (P, T)


LP_MAIN = """#include "uvrt_plan_lp.h"
#include <cstdio>
#include <cstdlib>
#include <vector>
int main(int argc, char** argv) {
    const int P = atoi(argv[2]); FILE* f = fopen(argv[1], "rb"); std::vector<double> A; double v;
    while (fread(&v, 8, 1, f) == 1) A.push_back(v);
    const long n = (long)A.size() / P; uvrt_plan_lp::RestrictedLP lp(P); int64_t piv = 0;
    lp.add_rows(A.data(), n);
    const bool ok = lp.solve(50 * (lp.rows() + P) + 1000, &piv);
    std::vector<double> y, d; lp.solution(&y, &d);
    printf("%d %lld", ok ? 1 : 0, (long long)piv); for (double x : d) printf(" %.17g", x);
    printf("\\n"); return 0; }
"""


@pytest.fixture(scope="module")
def lp_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("lp")
    (d / "lp.cpp").write_text(LP_MAIN)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC, str(d / "lp.cpp"), "-o", str(d / "lp")])
    return d


@pytest.mark.parametrize("name", [c["name"] for c in cc.closed_cases()])
def test_restricted_lp_solves_the_closed_forms_in_one_round(lp_exe, name):
    """RestrictedLP alone on the row-scaled matrix of each closed-form case, all rows in one round: solved, every row covered
    to 1 - 1e-9, and the total equal to the closed form to within the right-hand side's perturbation (delta < 2e-9)."""
    case = [c for c in cc.closed_cases() if c["name"] == name][0]
    tag = case["solves"][0][0]
    A, cols, c = cc.scaled_lp(case, tag, pr)
    (lp_exe / (name + ".bin")).write_bytes(A.tobytes())
    out = subprocess.check_output([str(lp_exe / "lp"), str(lp_exe / (name + ".bin")), str(A.shape[1])], timeout=120).split()
    ok, piv = int(out[0]), int(out[1])
    d = np.array([float(x) for x in out[2:]])
    exact = case["exact"][tag][cols] - c["lower"][cols].astype(np.float64)
    total = 16.0 if name == "D-ones" else float(exact.sum())
    print(name, "solved", ok, "pivots", piv, "total", repr(float(d.sum())), "closed form", repr(total))
    assert ok == 1, "RestrictedLP::solve gave up (unbounded or the pivot cap)"
    assert np.all(A @ d >= 1.0 - 1e-9)
    assert total * (1 - 1e-12) <= d.sum() <= total * (1 + 2e-9) * (1 + 1e-12)
    if name != "D-ones":
        keep = exact > 0
        assert np.all(np.abs(d[keep] - exact[keep]) <= 2.1e-9 * exact[keep])


def test_the_overflow_scene_is_hit(orc):
    """the scene of the GPU overflow test: a launch of 4096 photons from its lamp hits the large triangle (the oracle's tracer)"""
    case = cc.overflow_scene()
    tris, nodes, idx = cc.scene(orc, case)
    rays, _ = orc.generate(0, 4096, cc.OVERFLOW_LAMP, 1.0, 0)
    temp = np.zeros(len(case["area_log2"]), dtype=np.int32)
    orc.extend(temp, tris, rays, nodes, idx)
    assert temp[0] > 100 and temp.sum() <= 4096


def test_the_hook_is_bound_and_refuses_a_null_context(pkg):
    names = [name for name, _, _ in pkg.capi.SYMBOLS]
    assert names.count("uvrt_plan_write_exposure") == 1 and hasattr(pkg.capi.Ctx, "plan_write_exposure")
    buf = np.zeros(4, dtype=np.uint32)
    for path in (pkg.capi.LIB_PATH, pkg.capi.LIB_DEV_PATH):
        assert hasattr(C.CDLL(path), "uvrt_plan_write_exposure"), path
    for dev in (False, True):
        L = pkg.capi.lib(dev)
        assert L.uvrt_plan_write_exposure.restype is C.c_int
        assert L.uvrt_plan_write_exposure(None, 0, buf.ctypes.data, 0, 4) == -1          # UVRT_ERR_INVALID
        assert b"uvrt_plan_write_exposure" in L.uvrt_last_error()
