"""GPU: planning from the direct gather (include/uvrt.h "planning from the direct gather", RayTracer::PlanDurations with
PlanOptions::gatherSamples, uvrt_cli --plan-gather).  One solver serves both element types of the exposure matrix: an
expected plan filled with (double)E of a counts plan solves to the same bits.  The gather feeds it: every row of X is the f64
sum of the restated launches (tests/gather_restate.py), the classes equal a numpy restatement, the optimum checks out against
HiGHS, the plan holds in the pipeline and capture changes nothing.  Test room, positions 0-2 of lange_route."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import gather_restate as gr
import plan_restate as pr
from conftest import GLB, GOLDEN, ROOT, ROUTE
from sweep_restate import segment_duration

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "small-project-uv-robot-ray-tracer_amd", "uvrt_cli")
PPL = 1 << 18          # photons per launch (counts plan) / photons_equiv per launch (gather plan)
ITER = 2
S = 4                  # shadow rays per triangle and launch
SPEED = 0.05
MARGIN, REL_GAP = 1e-6, 1e-3
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _comp(orc, oscene, oroute):
    return orc.Computation(oscene, oroute["lamps"][:3], 3 * PPL, oroute["lightHeight"], oroute["lightLength"],
                           oroute["lightIntensity"])


# ---------------------------------------------------------------- 1. one solver, two element types
def _solve_all(c, s, N, min_photons):
    """the plain solve and two bounded ones (column 2 fixed at 1 s; lower bounds only) with everything they report"""
    out = {}
    kw = dict(min_photons=min_photons, margin=MARGIN, rel_gap=REL_GAP, positions=3)
    d, rep = c.plan_solve(100.0, s, N, **kw)
    out["plain"] = (d, rep, None, c.plan_read_classes(), c.plan_read_required(), c.plan_model_dose(d))
    for tag, lower, fixed in (("fixed", [0.0, 0.0, 1.0], [0, 0, 1]), ("lower", [1.0, 0.0, 0.5], None)):
        d, rep, brep = c.plan_solve_bounded(100.0, s, N, lower=lower, fixed=fixed, **kw)
        out[tag] = (d, rep, brep, c.plan_read_classes(), c.plan_read_required(), c.plan_model_dose(d))
    return out


def _fill_expected(c, rows):
    """rows[p] into row p of a fresh expected plan: the first half of the triangles in one capture, the rest in a second"""
    P, T = rows.shape
    c.plan_begin_expected(P)
    half = T // 2
    for p in range(P):
        first = rows[p].copy()
        first[half:] = 0.0
        c.write_expected(first)
        c.plan_capture_expected(p)
        assert np.array_equal(bits64(c.read_expected()), bits64(first)), "capture leaves the plane as it is"
        rest = rows[p].copy()
        rest[:half] = 0.0
        c.write_expected(rest)
        c.plan_capture_expected(p)
    c.write_expected(np.zeros(T))
    for p in range(P):
        assert np.array_equal(bits64(c.plan_read_exposure_expected(p)), bits64(rows[p])), p


def test_one_solver_two_element_types(pkg, orc, oscene, oroute):
    comp = _comp(orc, oscene, oroute)
    world = [tuple(float(x) for x in comp.lamp_world_pos(l)) for l in oroute["lamps"][:3]]
    s = f32(f32(oroute["lightIntensity"]) * f32(0.1))
    N = ITER * PPL
    c = pkg.capi.Ctx(0)
    try:
        c.set_scene(oscene.tris, oscene.nodes, oscene.triIdx)
        c.resize_rays(PPL)
        c.reset(True)
        c.plan_begin(3)
        c.trace_batch(world * ITER, oroute["lightLength"], 0, PPL)
        c.plan_capture_batch([0, 1, 2] * ITER)
        c.replay_batch(np.zeros(3 * ITER, dtype=pkg.capi.REPLAY_OP_DT))
        E = np.stack([c.plan_read_exposure(p) for p in range(3)])
        counts = _solve_all(c, s, N, 16)
        assert counts["plain"][1]["required"] > 0 and counts["plain"][0].sum() > 0
        assert counts["fixed"][2]["fixed_columns"] == 1 and counts["lower"][2]["lower_total"] == 1.5
        assert (counts["plain"][3] == 2).sum() > 0                     # some unresolved rows: the min_photons test is live

        _fill_expected(c, E.astype(np.float64))
        expected = _solve_all(c, s, N, 16)
        for tag in ("plain", "fixed", "lower"):
            a, b = counts[tag], expected[tag]
            assert np.array_equal(bits(a[0]), bits(b[0])), tag
            assert a[1] == b[1], (tag, a[1], b[1])
            assert a[2] == b[2], (tag, a[2], b[2])
            assert np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4]), tag
            assert np.array_equal(bits(a[5]), bits(b[5])), tag

        # quarters: every scaling is by an exact power of two
        _fill_expected(c, E.astype(np.float64) / 4.0)
        X = np.stack([c.plan_read_exposure_expected(p) for p in range(3)])
        assert np.any(X != np.floor(X))
        quarter = _solve_all(c, s, N // 4, 4)
        for tag in ("plain", "fixed", "lower"):
            a, b = counts[tag], quarter[tag]
            assert np.array_equal(bits(a[0]), bits(b[0])), tag
            assert np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4]), tag
    finally:
        c.close()


# ---------------------------------------------------------------- 2. the gather feeds it
@pytest.fixture(scope="module")
def restated(orc, oscene, oroute):
    """the launches of a gatherSamples = S run over positions 0-2, restated: `stops[k]` is launch k of a stops-only run
    (seed k, position k % 3; the first three are also the stops of a driving iteration), `segs[k]` the segment k -> k + 1
    of a driving run's first iteration (seed 3 + k)"""
    comp = _comp(orc, oscene, oroute)
    assert comp.photonsPerLight == PPL
    world = [comp.lamp_world_pos(l) for l in oroute["lamps"][:3]]
    ll = comp.lightLength
    stops = [gr.gather(orc, oscene, world[k % 3], world[k % 3], ll, S, k, PPL)[0] for k in range(3 * ITER)]
    segs = [gr.gather(orc, oscene, world[k], world[k + 1], ll, S, 3 + k, PPL)[0] for k in range(2)]
    for a in stops + segs:
        a.setflags(write=False)
    return {"stops": stops, "segs": segs}


def _rt(iterations, speed):
    from uvrt_amd import host
    rt = host.RayTracer(GLB, ROUTE, device=0)
    rt.set_lamps(rt.lamps()[:3])
    rt.photonCount = 3 * PPL
    rt.maxIterations = iterations
    rt.driveSpeed = speed
    rt.viewMode = host.VIEW_DOSAGE
    return rt


def _gather_run(rt):
    """the plain pipeline with gatherSamples = S from ResetDosageMap; (dose, colours, photonMap, maxPhotonMap)"""
    rt.gatherSamples = S
    rt.ResetDosageMap()
    for _ in range(rt.maxIterations):
        rt.ComputeDosageMap()
        rt.Shade()
        rt.currIterations = rt.currIterations + 1
    rt.Sync()
    return _maps(rt)


def _maps(rt):
    return rt.read_dosage(), rt.ctx.read_color(), rt.ctx.read_photon_map(0), rt.ctx.read_photon_map(1)


def _restate_classes(X, area, lower, fixed, s, N, m, min_photons, bounded):
    """the classes of include/uvrt.h from X, every sum in f64 in ascending p; also den, m', r_t and rho_t"""
    T = X.shape[1]
    tot, fre, base = np.zeros(T), np.zeros(T), np.zeros(T)
    for p in range(X.shape[0]):
        tot = tot + X[p]
        if not fixed[p]:
            fre = fre + X[p]
        base = base + X[p] * float(f32(lower[p]))
    den = (area * f32(N)).astype(np.float64)                 # f32 product, then f64
    mprime = float(f32(m)) * (1.0 + MARGIN)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = float(f32(s)) / (den * mprime)
        b = base * r
        inner = np.where(b >= 1.0, 4, np.where(fre == 0, 5, 0)) if bounded else 0
        cls = np.where((tot == 0) | ~(area > 0), 1, np.where(tot < float(max(1, min_photons)), 2, inner))
        rho = np.maximum(1.0 - b, 1e-9)
    return cls.astype(np.uint8), den, mprime, r, rho


def _check_optimum(A, b, x, total, lower_total, rep):
    """tests/test_gpu_plan.py _check_optimality on the LP  min 1.x  s.t.  x A >= b, x >= 0, whose optimum the solver's excess
    over lower_total must match (A: [columns][rows])"""
    from scipy.optimize import linprog
    P = A.shape[0]
    r = linprog(np.ones(P), A_ub=-A.T, b_ub=-b, bounds=[(0, None)] * P, method="highs")
    assert r.status == 0
    opt = float(r.fun)
    excess = total - lower_total
    print("HiGHS optimum %.9g, solver %.9g (+ %.9g fixed), lower bound %.9g, gap %.3g, rounds %d" % (
        opt, excess, lower_total, rep["lower_bound"], rep["gap"], rep["iterations"]))
    assert abs(total - rep["total_duration"]) <= 1e-9 * total
    assert rep["lower_bound"] - lower_total <= opt * (1 + 1e-9) and opt <= excess * (1 + 1e-9)
    assert excess <= opt * (1 + 2 * REL_GAP)
    assert rep["converged"] and rep["gap"] <= REL_GAP
    assert np.all(x @ A >= b * (1 - 1e-12))                  # feasible in the model, in f64


@pytest.mark.parametrize("mode", ["stops", "drive"])
def test_the_gather_feeds_the_plan(pkg, oscene, oroute, restated, mode):
    drive = mode == "drive"
    iters = 1 if drive else ITER
    lamps = oroute["lamps"][:3]
    rt, plain = _rt(iters, SPEED if drive else 0.0), _rt(iters, SPEED if drive else 0.0)
    try:
        T = rt.mesh.triangleCount
        m = float(f32(rt.minDosage))
        s = f32(f32(rt.lightIntensity) * f32(0.1))
        d, rep = rt.PlanDurations(gather_samples=S)
        N = iters * rt.photonsPerLight
        assert rt.photonsPerLight == PPL and rt.gatherSamples == 0 and rt.photonMapSize == 3 * N
        P = 5 if drive else 3
        assert rep["positions"] == P and d.size == 3

        # capture changes nothing: the maps are those of a plain gatherSamples = S run with the route's durations
        got, want = _maps(rt), _gather_run(plain)
        assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1]))
        assert np.array_equal(bits64(got[2]), bits64(want[2])) and np.array_equal(bits64(got[3]), bits64(want[3]))
        assert (got[0] > 0).sum() > 0.3 * T

        # every row of X = the f64 sum, in launch order, of the restated launches
        X = np.stack([rt.ctx.plan_read_exposure_expected(p) for p in range(P)])
        for p in range(3):
            row = np.zeros(T)
            for it in range(iters):
                row = row + restated["stops"][3 * it + p]
            assert np.array_equal(bits64(X[p]), bits64(row)), p
        for k in range(2 if drive else 0):
            assert np.array_equal(bits64(X[3 + k]), bits64(np.zeros(T) + restated["segs"][k])), k
        with pytest.raises(pkg.capi.UvrtError, match="error -1"):
            rt.ctx.plan_read_exposure(0)                     # the matrix holds no counts

        # the classes against numpy
        seg = np.array([segment_duration(lamps[k][:2], lamps[k + 1][:2], SPEED) for k in range(2)], dtype=np.float32)
        lower = np.concatenate([np.zeros(3, dtype=np.float32), seg]) if drive else np.zeros(3, dtype=np.float32)
        fixed = np.array([0, 0, 0, 1, 1][:P], dtype=bool)
        area = pr.areas(oscene.tris)
        cls, den, mprime, r, rho = _restate_classes(X, area, lower, fixed, s, N, m, 16, drive)
        got_cls = rt.ctx.plan_read_classes()
        n = [int((cls == k).sum()) for k in range(6)]
        print("%s: active %d unreachable %d unresolved %d met %d short %d; differing %d" % (
            mode, n[0], n[1], n[2], n[4], n[5], int((got_cls != cls).sum())))
        assert np.array_equal(got_cls, cls)
        req = rt.ctx.plan_read_required()
        assert np.array_equal(req, (cls == 0) | (cls == 4))
        assert rep["required"] == n[0] + n[4] and rep["unreachable"] == n[1] and rep["unresolved"] == n[2]
        assert n[0] > 0 and n[1] > 0 and n[2] > 0
        a64 = area.astype(np.float64)
        assert abs(rep["area_required"] - float(a64[req].sum())) <= 1e-9 * float(a64.sum())

        # the optimum against HiGHS
        x = np.concatenate([d, rep["segment_durations"]]).astype(np.float64) if drive else d.astype(np.float64)
        total = float(x.sum())
        if drive:
            assert np.array_equal(bits(rep["segment_durations"]), bits(seg))
            assert rep["fixed_columns"] == 2 and rep["free_columns"] == 3
            assert rep["met_by_lower"] == n[4] > 0 and rep["short_rows"] == n[5]
            act = cls == 0
            A = X[:3][:, act] * r[act]                       # the residual LP: free columns, active rows, rhs rho_t
            lower_total = float(seg.astype(np.float64).sum())
            assert abs(lower_total - rep["lower_total"]) <= 1e-9 * lower_total
            _check_optimum(A, rho[act], d.astype(np.float64), total, lower_total, rep)
        else:
            _check_optimum(X[:, req], (mprime * den / float(s))[req], x, total, 0.0, rep)
        assert rep["min_dose_ratio"] >= 1.0
        assert np.array_equal(np.array([l[2] for l in rt.lamps()], dtype=np.float32), d)

        # two more solves: the same bits
        kw = dict(min_photons=16, margin=MARGIN, rel_gap=REL_GAP, positions=P)
        for _ in range(2):
            if drive:
                again = rt.ctx.plan_solve_bounded(m, s, N, lower=lower, fixed=fixed, **kw)[0]
            else:
                again = rt.ctx.plan_solve(m, s, N, **kw)[0]
            assert np.array_equal(bits(again), bits(x.astype(np.float32)))

        # the plan holds in the pipeline
        model = rt.ctx.plan_model_dose(x.astype(np.float32))
        dose = _gather_run(rt)[0]
        assert np.all(dose[req] >= m), int((dose[req] < m).sum())
        nz = (dose > 0) & np.isfinite(dose)
        assert np.all(np.abs(model[nz].astype(np.float64) - dose[nz]) <= 1e-6 * dose[nz])
    finally:
        rt.close()
        plain.close()


# ---------------------------------------------------------------- 3. errors
def test_errors(pkg, oscene):
    Err = pkg.capi.UvrtError
    T = oscene.T
    c = pkg.capi.Ctx(0)
    L = c._L
    try:
        c.set_scene(oscene.tris, oscene.nodes, oscene.triIdx)
        c.resize_rays(4096)
        c.reset(True)
        good = np.linspace(0.0, 50.0, T)
        for bad in (float("inf"), float("nan"), -1.0):
            c.plan_begin_expected(2)
            for p in range(2):
                v = good.copy()
                if p == 1:
                    v[T // 3] = bad
                c.write_expected(v)
                c.plan_capture_expected(p)
            with pytest.raises(Err, match="error -1.*not finite or is negative"):
                c.plan_solve(100.0, 45.0, 4096, min_photons=1, positions=2)
            with pytest.raises(Err, match="error -1"):
                c.plan_solve_bounded(100.0, 45.0, 4096, min_photons=1, positions=2, lower=[0, 1], fixed=[0, 1])
        # kind mismatches and range errors on an expected plan: refused, the matrix and the plane unchanged
        c.plan_begin_expected(2)
        with pytest.raises(Err, match="error -1.*nothing captured"):
            c.plan_solve(100.0, 45.0, 4096, positions=2)
        c.write_expected(good)
        c.plan_capture_expected(0)
        c.write_expected(good[::-1])
        rows = [c.plan_read_exposure_expected(p) for p in range(2)]
        plane = c.read_expected()
        assert np.array_equal(rows[0], good) and not rows[1].any() and np.array_equal(plane, good[::-1])
        buf = np.zeros(4)
        for call in (lambda: c.plan_capture_batch([0]), lambda: c.plan_read_exposure(0),
                     lambda: c.plan_capture_expected(-1), lambda: c.plan_capture_expected(2),
                     lambda: c.plan_read_exposure_expected(2), lambda: c.plan_read_exposure_expected(-1),
                     lambda: c.plan_read_exposure_expected(0, T - 1, 2), lambda: c.write_expected(buf, T - 3)):
            with pytest.raises(Err, match="error -1"):
                call()
        assert L.uvrt_plan_read_exposure_expected(c._h, 0, None, 0, 4) == -1
        assert L.uvrt_write_expected(c._h, None, 0, 4) == -1
        for p in range(2):
            assert np.array_equal(bits64(c.plan_read_exposure_expected(p)), bits64(rows[p])), p
        assert np.array_equal(bits64(c.read_expected()), bits64(plane))
        d, rep = c.plan_solve(100.0, 45.0, 4096, min_photons=1, positions=2)
        assert rep["min_dose_ratio"] >= 1.0 and d[0] > 0 and d[1] == 0
        # on a counts plan, and without a plan
        c.plan_begin(2)
        for call in (lambda: c.plan_capture_expected(0), lambda: c.plan_read_exposure_expected(0)):
            with pytest.raises(Err, match="error -1"):
                call()
        assert not c.plan_read_exposure(0).any() and not c.plan_read_exposure(1).any()
        assert np.array_equal(bits64(c.read_expected()), bits64(plane))
        c.plan_end()
        for call in (lambda: c.plan_capture_expected(0), lambda: c.plan_read_exposure_expected(0)):
            with pytest.raises(Err, match="error -1"):
                call()
        for p in (0, 257):
            with pytest.raises(Err, match="error -1"):
                c.plan_begin_expected(p)
        # uvrt_set_scene drops an expected plan
        c.plan_begin_expected(2)
        c.plan_capture_expected(0)
        c.set_scene(oscene.tris, oscene.nodes, oscene.triIdx)
        with pytest.raises(Err, match="error -1"):
            c.plan_read_exposure_expected(0)
        with pytest.raises(Err, match="error -1"):
            c.plan_solve(100.0, 45.0, 4096, positions=2)
    finally:
        c.close()


# ---------------------------------------------------------------- 4. the CLI
def test_cli_plan_gather_verify_and_replay_of_the_saved_route(pkg, tmp_path):
    from uvrt_amd import host
    shutil.copy(os.path.join(GOLDEN, "lange_route.xml"), tmp_path / "lange_route.xml")
    vd, dd = tmp_path / "verify.f32", tmp_path / "again.f32"
    base = [CLI, "--room", GLB, "--route-dir", str(tmp_path)]
    out = subprocess.run(base + ["--route", "lange_route", "--lamps", "3", "--photons", str(3 * PPL), "--iterations", str(ITER),
                                 "--plan-gather", str(S), "--plan", "50", "--plan-verify", "--save-route", "planned",
                                 "--verify-dump", str(vd)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "plan-verify: 0 below minimum" in out.stdout and "direct gather" in out.stdout
    assert "<gather_samples>%d</gather_samples>" % S in (tmp_path / "planned.xml").read_text()
    saved = host.RayTracer(init=False)
    saved.set_route_dir(str(tmp_path) + os.sep)
    saved.LoadRoute("planned")
    cli_d = np.array([l[2] for l in saved.lamps()], dtype=np.float32)
    saved.close()
    rt = _rt(ITER, 0.0)
    try:
        d, rep = rt.PlanDurations(min_dose=50.0, gather_samples=S)
    finally:
        rt.close()
    assert d.sum() > 0 and np.array_equal(bits(cli_d), bits(d))
    again = subprocess.run(base + ["--route", "planned", "--dump", str(dd)], capture_output=True, text=True, timeout=300)
    assert again.returncode == 0, again.stderr
    v, a = np.fromfile(vd, dtype="<f4"), np.fromfile(dd, dtype="<f4")
    assert v.size == a.size > 0 and np.array_equal(bits(v), bits(a))
