"""Duration planning on the GPU: prints one JSON line with the capture overhead per batch, the solve time, the solver's
rounds and gap, and the bytes of the exposure matrix E the solve reads per second.

    python tests/tools/plan_bench.py [--scene soup:T] [--candidates route|grid:NX,NZ] [--ppl N] [--iterations I] [--reps R]

capture overhead = (PlanDurations - the same batched computation without a plan - one solve) / batches.  The solve reads
E once per pass over the rows: classification, row compaction, the uniform start and one row check per cutting-plane
round plus the three of the repair (E bytes read / s counts those passes).
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
    ap.add_argument("--scene", default=None, help="soup:T for a synthetic T-triangle scene (default: the test room)")
    ap.add_argument("--candidates", default="route", help="route, or grid:NX,NZ (inset 0.5 m)")
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
    if args.scene and args.scene.startswith("soup:"):
        import bench
        mesh = host.Mesh(tris=bench.soup_triangles(int(args.scene[5:])))
        rt = host.RayTracer(None, route_xml, device=0, mesh=mesh)
    else:
        rt = host.RayTracer(os.path.join(ROOT, "tests", "golden", "testroomopt.glb"), route_xml, device=0)
    if args.candidates.startswith("grid:"):
        nx, nz = (int(v) for v in args.candidates[5:].split(","))
        rt.SetCandidateGrid(nx, nz, 0.5)
    P = len(rt.lamps())
    rt.photonCount = args.ppl * P
    rt.maxIterations = args.iterations
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
        prm = dict(min_dose=rt.minDosage, scaled_power=np.float32(rt.lightIntensity) * np.float32(0.1),
                   photons_per_position=args.iterations * rt.photonsPerLight, positions=P)
        t0 = time.perf_counter()
        d2, rep2 = rt.ctx.plan_solve(**prm)
        solve.append(time.perf_counter() - t0)
        assert np.array_equal(d2.view(np.uint32), d.view(np.uint32))
    med = lambda v: sorted(v)[len(v) // 2]
    e_bytes = P * T * 4
    passes = 3 + rep["iterations"] + 1 + 3
    out = {
        "scene": args.scene or "testroomopt.glb", "triangles": T, "positions": P, "iterations": args.iterations,
        "photons_per_launch": rt.photonsPerLight, "batches": batches, "E_bytes": e_bytes,
        "computation_s": med(plain), "plan_total_s": med(plan), "solve_s": med(solve),
        "capture_overhead_per_batch_ms": 1e3 * (med(plan) - med(plain) - med(solve)) / batches,
        "rounds": rep["iterations"], "gap": rep["gap"], "converged": rep["converged"],
        "used_positions": rep["used_positions"], "total_duration": rep["total_duration"],
        "lower_bound": rep["lower_bound"], "required": rep["required"],
        "E_bytes_read_per_s": passes * e_bytes / med(solve),
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
