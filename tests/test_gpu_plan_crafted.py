"""GPU: the duration planner on hand-made exposure matrices (tests/plan_crafted_cases.py), written into a counts plan through
uvrt_plan_write_exposure and into an expected plan through uvrt_write_expected + uvrt_plan_capture_expected.  Classes, both
reports (counts, and areas in the kernel's order of summation) and min_dose_ratio equal the numpy restatement
(tests/plan_restate.py) bit for bit; the two kinds of plan agree on the same integers; the optimum checks out against HiGHS
and against closed forms, beyond the dynamic range the restricted LP's old pivot floor took; the overflow flag at its
boundary, the model dose on ranges, the hook's refusals.  Every scene has at most 513 triangles and 256 positions."""
import numpy as np
import pytest

import plan_crafted_cases as cc
import plan_restate as pr

pytestmark = pytest.mark.gpu

f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.capi.Ctx(0)
    yield c
    c.close()


def _set_scene(ctx, orc, case):
    tris, nodes, idx = cc.scene(orc, case)
    ctx.set_scene(tris, nodes, idx)
    ctx.resize_rays(4096)
    ctx.reset(True)
    return pr.areas(tris)               # of the array handed to set_scene


def _fill(ctx, case, expected):
    M = cc.matrix(case, expected)
    P = M.shape[0]
    if expected:
        ctx.plan_begin_expected(P)
        for p in range(P):
            ctx.write_expected(M[p])
            ctx.plan_capture_expected(p)
        ctx.write_expected(np.zeros(M.shape[1]))
        assert np.array_equal(bits64(ctx.plan_read_exposure_expected(P - 1)), bits64(M[P - 1]))
    else:
        ctx.plan_begin(P)
        for p in range(P):
            ctx.plan_write_exposure(p, M[p].astype(np.uint32))
        assert np.array_equal(ctx.plan_read_exposure(P - 1), M[P - 1].astype(np.uint32))
    return M


def _solve(ctx, case, lower, fixed):
    prm = case["prm"]
    kw = dict(min_photons=prm["min_photons"], margin=prm["margin"], rel_gap=cc.REL_GAP, mask=case["mask"],
              positions=case["E"].shape[0])
    if lower is None and fixed is None:
        out, rep = ctx.plan_solve(prm["m"], prm["s"], prm["N"], **kw)
        brep = None
    else:
        out, rep, brep = ctx.plan_solve_bounded(prm["m"], prm["s"], prm["N"], lower=lower, fixed=fixed, **kw)
    return dict(out=out, rep=rep, brep=brep, cls=ctx.plan_read_classes(), req=ctx.plan_read_required())


_cache = {}


def _solved(ctx, orc, case, expected):
    """every solve of the case on a plan of the given kind: {tag: result}, the matrix and the areas; solved once per module"""
    key = (case["name"], expected)
    if key not in _cache:
        area = _set_scene(ctx, orc, case)
        M = _fill(ctx, case, expected)
        _cache[key] = ({tag: _solve(ctx, case, lower, fixed) for tag, lower, fixed in case["solves"]}, M, area)
    return _cache[key]


def _against_the_restatement(case, M, area, tag, lower, fixed, got):
    c = pr.classify(M, area, mask=case["mask"], lower=lower, fixed=fixed, **case["prm"])
    want_rep, want_brep = pr.report(c)
    n = [int((c["cls"] == k).sum()) for k in range(6)]
    ratio = pr.min_dose_ratio(M, c, got["out"])
    print("%s %s: classes %r differing %d; min_dose_ratio %r restated %r; total %r rounds %d gap %.3g" % (
        case["name"], tag, n, int((got["cls"] != c["cls"]).sum()), got["rep"]["min_dose_ratio"], ratio,
        got["rep"]["total_duration"], got["rep"]["iterations"], got["rep"]["gap"]))
    assert np.array_equal(got["cls"], c["cls"])
    assert np.array_equal(got["req"], (c["cls"] == 0) | (c["cls"] == 4))
    for k, v in want_rep.items():
        if k.startswith("area"):
            assert bits64(got["rep"][k]) == bits64(v), (k, got["rep"][k], v)
        else:
            assert got["rep"][k] == v, (k, got["rep"][k], v)
    if got["brep"] is not None:
        fix = np.zeros(len(c["lower"]), dtype=bool) if fixed is None else np.asarray(fixed) != 0
        assert got["brep"]["fixed_columns"] == int(fix.sum()) and got["brep"]["free_columns"] == int((~fix).sum())
        assert bits64(got["brep"]["lower_total"]) == bits64(pr.seq_sum(c["lower"]))
        if c["bounded"]:
            for k, v in want_brep.items():
                if k.startswith("area"):
                    assert bits64(got["brep"][k]) == bits64(v), (k, got["brep"][k], v)
                else:
                    assert got["brep"][k] == v, (k, got["brep"][k], v)
    assert got["rep"]["positions"] == M.shape[0] and got["rep"]["used_positions"] == int((got["out"] > 0).sum())
    assert bits64(got["rep"]["min_dose_ratio"]) == bits64(ratio), (got["rep"]["min_dose_ratio"], ratio)
    assert got["rep"]["min_dose_ratio"] >= 1.0
    assert bits64(got["rep"]["total_duration"]) == bits64(pr.seq_sum(got["out"]))
    return c


ABC = [cc.case_A, cc.case_B2, cc.case_B256] + [lambda P=P, T=T: cc.case_C(P, T) for P, T in cc.C_SIZES]
ABC_IDS = ["A", "B2", "B256"] + ["C%dx%d" % s for s in cc.C_SIZES]


@pytest.mark.parametrize("make", ABC, ids=ABC_IDS)
def test_classes_reports_and_dose_ratio_equal_the_restatement(ctx, orc, make):
    case = make()
    for expected in ((False,) if case["counts_only"] else (False, True)):
        res, M, area = _solved(ctx, orc, case, expected)
        for tag, lower, fixed in case["solves"]:
            c = _against_the_restatement(case, M, area, tag, lower, fixed, res[tag])
            if case["name"] == "A":
                assert set(c["cls"].tolist()) == set(range(6 if tag == "bounded" else 4))
            if case["name"].startswith("B"):
                assert c["cls"][0] == 0 and res[tag]["cls"][0] == 0


@pytest.mark.parametrize("make", [ABC[0]] + ABC[3:], ids=[ABC_IDS[0]] + ABC_IDS[3:])
def test_counts_and_expected_plans_of_the_same_integers_agree(ctx, orc, make):
    case = make()
    a, b = _solved(ctx, orc, case, False)[0], _solved(ctx, orc, case, True)[0]
    for tag, _, _ in case["solves"]:
        assert np.array_equal(bits(a[tag]["out"]), bits(b[tag]["out"])), tag
        assert a[tag]["rep"] == b[tag]["rep"], (tag, a[tag]["rep"], b[tag]["rep"])
        assert a[tag]["brep"] == b[tag]["brep"], tag
        assert np.array_equal(a[tag]["cls"], b[tag]["cls"]) and np.array_equal(a[tag]["req"], b[tag]["req"]), tag


@pytest.mark.parametrize("size", cc.C_SIZES, ids=ABC_IDS[3:])
def test_C_is_optimal_against_highs(ctx, orc, size):
    """the criterion of tests/test_gpu_plan.py: lower_bound <= opt <= total <= opt (1 + 2 rel_gap), converged, feasible in f64"""
    from scipy.optimize import linprog
    case = cc.case_C(*size)
    res, M, area = _solved(ctx, orc, case, False)
    got = res["plain"]
    den, mprime, r = pr.row_scale(area, **{k: case["prm"][k] for k in ("s", "N", "m", "margin")})
    req = got["req"]
    A = M[:, req].astype(np.float64)                         # [P][R]
    b = (mprime * den / float(f32(case["prm"]["s"])))[req]
    P = A.shape[0]
    lp = linprog(np.ones(P), A_ub=-A.T, b_ub=-b, bounds=[(0, None)] * P, method="highs")
    assert lp.status == 0 and req.sum() > 0
    opt, rep = float(lp.fun), got["rep"]
    total = float(np.sum(got["out"].astype(np.float64)))
    print("C%dx%d: HiGHS %.9g, total %.9g, lower bound %.9g, gap %.3g, rounds %d" % (
        size + (opt, total, rep["lower_bound"], rep["gap"], rep["iterations"])))
    assert rep["lower_bound"] <= opt * (1 + 1e-9) and opt <= total * (1 + 1e-9)
    assert total <= opt * (1 + 2 * cc.REL_GAP)
    assert rep["converged"] and rep["gap"] <= cc.REL_GAP
    assert np.all(got["out"].astype(np.float64) @ A >= b * (1 - 1e-12))


CLOSED = cc.closed_cases()


@pytest.mark.parametrize("case", CLOSED, ids=[c["name"] for c in CLOSED])
def test_closed_forms_per_column(pkg, ctx, orc, case):
    """D and E: exact_p <= d_p <= round_trip_up(smallest f32 >= exact_p (1 + 4e-9)) on every column whose optimum is unique"""
    tag, lower, fixed = case["solves"][0]
    for expected in (False, True):
        res, M, area = _solved(ctx, orc, case, expected)
        got = res[tag]
        out, rep = got["out"], got["rep"]
        _against_the_restatement(case, M, area, tag, lower, fixed, got)
        exact = case["exact"][tag]
        print("%s %s: out %r exact %r status %d gap %.3g rounds %d" % (
            case["name"], "expected" if expected else "counts", out[:4].tolist(), exact[:4].tolist(), rep["status"], rep["gap"],
            rep["iterations"]))
        for p in range(out.size):
            if np.isnan(exact[p]):
                continue
            hi = cc.duration_bound(exact[p], pkg.capi.round_trip_up)
            assert exact[p] <= float(out[p]) <= float(hi), (case["name"], p, repr(float(out[p])), repr(exact[p]), repr(float(hi)))
        assert rep["converged"] and rep["gap"] <= cc.REL_GAP
        if case["name"] == "D-tie":
            assert out[1] == 0.0 and out[0] > 0           # the uncovered row goes to its largest E, lowest index on ties
        if case["name"] == "D-ones":                      # no column is told apart: the total decides
            total = float(np.sum(out.astype(np.float64)))
            assert 16.0 <= total <= 16.0 * (1 + 2 * cc.REL_GAP)
        if fixed is not None:
            for p in np.flatnonzero(np.asarray(fixed)):
                assert bits(out[p:p + 1])[0] == bits(lower[p:p + 1])[0], p


def test_overflow_flag_at_its_boundary(pkg, ctx, orc):
    """a captured plane on top of 2^32 - 1 - c: every sum is 2^32 - 1 or below and the solve runs; on top of 2^32 - c_t on one
    triangle the sum leaves uint32 by one and the solve refuses"""
    case = cc.overflow_scene()
    _set_scene(ctx, orc, case)
    T = len(case["area_log2"])
    top = np.uint64(2 ** 32 - 1)
    ctx.seed = 0
    ctx.trace_batch([cc.OVERFLOW_LAMP], 1.0, 0, 4096)
    c = ctx.read_batch_counts(0).astype(np.uint64)
    assert c[0] > 0 and c.sum() <= 4096
    ctx.plan_begin(1)
    ctx.plan_write_exposure(0, (top - c).astype(np.uint32))
    ctx.plan_capture_batch([0])
    ctx.replay_batch(np.zeros(1, dtype=pkg.capi.REPLAY_OP_DT))
    out, rep = ctx.plan_solve(1.0, 1.0, 2, min_photons=1, margin=0.0, positions=1)
    got = ctx.plan_read_exposure(0)
    assert np.all(got == np.uint32(top)) and out[0] > 0 and rep["required"] == int((pr.areas(cc.make_tris(case["area_log2"])) > 0).sum())
    ctx.trace_batch([cc.OVERFLOW_LAMP], 1.0, 0, 4096)
    c = ctx.read_batch_counts(0).astype(np.uint64)
    assert c[0] > 0
    ctx.plan_begin(1)
    row = np.zeros(T, dtype=np.uint32)
    row[0] = np.uint32(np.uint64(2 ** 32) - c[0])
    ctx.plan_write_exposure(0, row)
    ctx.plan_capture_batch([0])
    ctx.replay_batch(np.zeros(1, dtype=pkg.capi.REPLAY_OP_DT))
    with pytest.raises(pkg.capi.UvrtError, match="error -1.*overflow"):
        ctx.plan_solve(1.0, 1.0, 2, min_photons=1, margin=0.0, positions=1)
    ctx.plan_end()


@pytest.mark.parametrize("expected", [False, True], ids=["counts", "expected"])
def test_model_dose_on_ranges(ctx, orc, expected):
    """after A's plain solve: bits equal the restatement on every range, NaN at the same places (rows without area and without
    exposure), inf where a row without area holds some"""
    case = cc.case_A()
    area = _set_scene(ctx, orc, case)
    M = _fill(ctx, case, expected)
    got = _solve(ctx, case, None, None)
    T = M.shape[1]
    prm = case["prm"]
    vectors = [np.zeros(4), np.full(4, 2.0 ** -100), np.ones(4), np.full(4, 1e30), np.array([0, 2.0 ** -100, 1, 1e30]),
               np.array([1e30, 1, 2.0 ** -100, 0]), got["out"]]
    seen_nan = seen_inf = 0
    for d in vectors:
        d = np.asarray(d, dtype=np.float32)
        for first, count in ((0, T), (1, 1), (255, 2), (256, 1), (T - 1, 1), (0, 0)):
            have = ctx.plan_model_dose(d, first, count)
            want = pr.model_dose(M, area, prm["s"], prm["N"], d, first, count)
            assert have.shape == want.shape == (count,)
            assert np.array_equal(np.isnan(have), np.isnan(want)), (d.tolist(), first, count)
            ok = ~np.isnan(want)
            assert np.array_equal(bits(have[ok]), bits(want[ok])), (d.tolist(), first, count)
            seen_nan += int(np.isnan(want).sum())
            seen_inf += int(np.isinf(want).sum())
    assert seen_nan > 0 and seen_inf > 0
    full = pr.model_dose(M, area, prm["s"], prm["N"], got["out"])
    assert np.all(full[got["req"]] >= f32(prm["m"]))
    ctx.plan_end()


def test_the_hook_refuses_and_a_refused_write_changes_nothing(pkg, ctx, orc):
    Err = pkg.capi.UvrtError
    case = cc.case_B2()
    _set_scene(ctx, orc, case)
    T = case["E"].shape[1]
    L = ctx._L
    row = np.array([7, 8, 9], dtype=np.uint32)
    with pytest.raises(Err, match="error -1.*uvrt_plan_write_exposure"):
        ctx.plan_write_exposure(0, row)                               # no plan
    ctx.plan_begin_expected(2)
    with pytest.raises(Err, match="error -1.*uvrt_plan_write_exposure"):
        ctx.plan_write_exposure(0, row)                               # an expected plan
    assert not ctx.plan_read_exposure_expected(0).any()
    with pytest.raises(Err, match="error -1.*nothing captured"):
        ctx.plan_solve(1.0, 1.0, 2, min_photons=1, margin=0.0, positions=2)       # a refused write is no capture
    ctx.plan_begin(2)
    with pytest.raises(Err, match="error -1.*nothing captured"):
        ctx.plan_solve(1.0, 1.0, 2, min_photons=1, margin=0.0, positions=2)
    ctx.plan_write_exposure(0, row)
    ctx.plan_write_exposure(1, row[:2][::-1], 1)                      # a range: E[1][1..3) = 8, 7
    before = [ctx.plan_read_exposure(p) for p in range(2)]
    assert before[0].tolist() == [7, 8, 9] and before[1].tolist() == [0, 8, 7]
    for call in (lambda: ctx.plan_write_exposure(-1, row), lambda: ctx.plan_write_exposure(2, row),
                 lambda: ctx.plan_write_exposure(0, row, 1), lambda: ctx.plan_write_exposure(0, row, -1),
                 lambda: ctx.plan_write_exposure(1, np.zeros(T + 1, dtype=np.uint32)),
                 lambda: ctx.plan_write_exposure(1, row[:1], T)):
        with pytest.raises(Err, match="error -1.*uvrt_plan_write_exposure"):
            call()
    assert L.uvrt_plan_write_exposure(ctx._h, 0, None, 0, 3) == -1
    assert L.uvrt_plan_write_exposure(ctx._h, 0, row.ctypes.data, 0, -1) == -1
    for p in range(2):
        assert np.array_equal(ctx.plan_read_exposure(p), before[p]), p
    out, rep = ctx.plan_solve(1.0, 1.0, 2, min_photons=1, margin=0.0, positions=2)    # the writes count as captures
    assert rep["required"] == 3 and rep["min_dose_ratio"] >= 1.0 and out.sum() > 0
    ctx.plan_end()
