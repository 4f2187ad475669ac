"""Planning a route that radiates while it drives, on the GPU: prints one JSON line with the capture overhead per batch,
the time of the bounded solve, the solver's rounds and gap, the drive time and the rows the drive meets or leaves short.

    python tests/tools/plan_drive_bench.py [--candidates route|grid:NX,NZ] [--speed V] [--ppl N] [--iterations I] [--reps R]

capture overhead = (PlanDurations - the same batched computation without a plan - one bounded solve) / batches; the
solve is timed on its own through uvrt_plan_solve_bounded with the bounds PlanDurations gives it (the stops free from 0,
every segment fixed at its drive time) and must return the planned durations bit for bit.
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", default="route", help="route, or grid:NX,NZ (inset 0.5 m; at most 128 positions)")
    ap.add_argument("--speed", type=float, default=0.1, help="driveSpeed, m/s")
    ap.add_argument("--ppl", type=int, default=1 << 20, help="photons per launch")
    ap.add_argument("--iterations", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    try:
        import torch
        if torch.cuda.is_available():
            torch.cuda.init()
    except Exception:
        pass
    import numpy as np
    import __graft_entry__ as g
    g.load_package()
    from uvrt_amd import host
    route_xml = os.path.join(ROOT, "tests", "golden", "lange_route.xml")
    rt = host.RayTracer(os.path.join(ROOT, "tests", "golden", "testroomopt.glb"), route_xml, device=0)
    if args.candidates.startswith("grid:"):
        nx, nz = (int(v) for v in args.candidates[5:].split(","))
        rt.SetCandidateGrid(nx, nz, 0.5)
    L = len(rt.lamps())
    P = 2 * L - 1
    rt.photonCount = args.ppl * L
    rt.maxIterations = args.iterations
    rt.driveSpeed = args.speed
    T = rt.mesh.triangleCount
    batches = math.ceil(args.iterations * P / 64)
    plain, plan, solve = [], [], []
    rep = None
    for _ in range(args.reps):
        rt.ctx.seed = 0
        rt.ResetDosageMap()
        t0 = time.perf_counter()
        rt.ComputeIterationsBatched(args.iterations)
        rt.Sync()
        plain.append(time.perf_counter() - t0)
        rt.ctx.seed = 0
        t0 = time.perf_counter()
        d, rep = rt.PlanDurations()
        plan.append(time.perf_counter() - t0)
        seg = rep["segment_durations"]
        lower = np.concatenate([np.zeros(L, dtype=np.float32), seg])
        fixed = np.concatenate([np.zeros(L, dtype=np.uint8), np.ones(L - 1, dtype=np.uint8)])
        t0 = time.perf_counter()
        d2, rep2, _ = rt.ctx.plan_solve_bounded(rt.minDosage, np.float32(rt.lightIntensity) * np.float32(0.1),
                                                args.iterations * rt.photonsPerLight, positions=P, lower=lower, fixed=fixed)
        solve.append(time.perf_counter() - t0)
        assert np.array_equal(d2[:L].view(np.uint32), d.view(np.uint32)) and np.array_equal(d2[L:].view(np.uint32), seg.view(np.uint32))
    med = lambda v: sorted(v)[len(v) // 2]
    out = {
        "scene": "testroomopt.glb", "triangles": T, "positions": L, "columns": P, "drive_speed": args.speed,
        "iterations": args.iterations, "photons_per_launch": rt.photonsPerLight, "batches": batches, "E_bytes": P * T * 4,
        "computation_s": med(plain), "plan_total_s": med(plan), "solve_s": med(solve),
        "capture_overhead_per_batch_ms": 1e3 * (med(plan) - med(plain) - med(solve)) / batches,
        "rounds": rep["iterations"], "gap": rep["gap"], "converged": rep["converged"],
        "used_positions": rep["used_positions"], "total_duration": rep["total_duration"],
        "lower_bound": rep["lower_bound"], "drive_time": rep["lower_total"], "required": rep["required"],
        "met_by_drive": rep["met_by_lower"], "area_met_by_drive": rep["area_met_by_lower"],
        "short_rows": rep["short_rows"], "area_short": rep["area_short"],
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
