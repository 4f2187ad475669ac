"""Planning from the direct gather against planning from photon counts, on the GPU: prints one JSON line.

    python tests/tools/plan_gather_bench.py [--candidates route|grid:NX,NZ] [--ppl N] [--iterations I] [--samples 16,64]
                                            [--holdout-seed SEED]

Three plans over the same positions of the test room: a counts plan (PlanDurations, ppl photons per launch) and one gather plan
per sample count S (PlanDurations(gather_samples=S), photons_equiv = ppl).  Per plan: the required / unreachable / unresolved /
short rows and their areas, the total duration, the solver's rounds, the solve time, the time of the whole PlanDurations and,
for a gather plan, the capture time per launch = (PlanDurations - the same gather launches without a plan - one solve) /
launches.  Two cross-checks, reported as they come out:
  counts_plan_under_gather: the counts plan's durations recomputed by the gather at the largest S; the share of that gather
      plan's required area whose dose lies below the minimum (what a counts plan leaves under-dosed where no photon arrives);
  gather_plan_under_photons[S]: the gather plan's durations recomputed with photons from another SEED; the share of the counts
      plan's required area at or above the minimum (how far the estimator at S samples can be trusted where photons resolve).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", default="route", help="route, or grid:NX,NZ (inset 0.5 m)")
    ap.add_argument("--ppl", type=int, default=1 << 20, help="photons per launch (photons_equiv of a gather launch)")
    ap.add_argument("--iterations", type=int, default=4)
    ap.add_argument("--samples", default="16,64", help="the gather plans' sample counts")
    ap.add_argument("--holdout-seed", type=int, default=12345)
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
    rt = host.RayTracer(os.path.join(ROOT, "tests", "golden", "testroomopt.glb"),
                        os.path.join(ROOT, "tests", "golden", "lange_route.xml"), device=0)
    if args.candidates.startswith("grid:"):
        nx, nz = (int(v) for v in args.candidates[5:].split(","))
        rt.SetCandidateGrid(nx, nz, 0.5)
    route = rt.lamps()
    P = len(route)
    rt.photonCount = args.ppl * P
    rt.maxIterations = args.iterations
    rt.viewMode = host.VIEW_DOSAGE
    T = rt.mesh.triangleCount
    m = float(np.float32(rt.minDosage))
    launches = args.iterations * P
    t = rt.mesh.tris()
    a, b = t[:, 0:3] - t[:, 4:7], t[:, 0:3] - t[:, 8:11]
    area = (np.sqrt(np.sum(np.cross(a, b).astype(np.float32) ** 2, axis=1, dtype=np.float32)) / np.float32(2.0)).astype(np.float64)
    prm = dict(min_dose=rt.minDosage, scaled_power=np.float32(rt.lightIntensity) * np.float32(0.1),
               photons_per_position=args.iterations * rt.photonsPerLight, positions=P)

    def with_durations(d):
        rt.set_lamps([(x, z, float(v)) for (x, z, _), v in zip(route, d)])
        rt.photonCount = args.ppl * P

    def recompute(samples, seed):
        """the pipeline from ResetDosageMap: the gather with `samples` per triangle, or photons from `seed`"""
        rt.gatherSamples = samples
        rt.ctx.seed = seed
        rt.ResetDosageMap()
        if samples:
            for _ in range(args.iterations):
                rt.ComputeDosageMap()
                rt.Shade()
                rt.currIterations = rt.currIterations + 1
        else:
            rt.ComputeIterationsBatched(args.iterations)
        rt.Sync()
        rt.gatherSamples = 0
        return rt.read_dosage()

    def plan(samples):
        with_durations([l[2] for l in route])
        rt.ctx.seed = 0
        t0 = time.perf_counter()
        d, rep = rt.PlanDurations(gather_samples=samples)
        total = time.perf_counter() - t0
        t0 = time.perf_counter()
        d2, _ = rt.ctx.plan_solve(**prm)
        solve = time.perf_counter() - t0
        assert np.array_equal(d2.view(np.uint32), d.view(np.uint32))
        out = {k: rep[k] for k in ("required", "unreachable", "unresolved", "area_required", "area_unreachable",
                                   "area_unresolved", "total_duration", "used_positions", "gap", "converged")}
        out.update(short_rows=rep.get("short_rows", 0), area_short=rep.get("area_short", 0.0), rounds=rep["iterations"],
                   solve_s=solve, plan_total_s=total)
        return d, rt.ctx.plan_read_required(), out

    samples = [int(v) for v in args.samples.split(",")]
    recompute(0, 0)                              # (allocations and first launches stay out of the counts plan's time)
    d_counts, req_counts, counts = plan(0)
    out = {"scene": "testroomopt.glb", "triangles": T, "candidates": args.candidates, "positions": P,
           "iterations": args.iterations, "photons_per_launch": rt.photonsPerLight, "min_dose": m, "area_total": float(area.sum()),
           "counts": counts, "gather": {}, "gather_plan_under_photons": {}}
    plans = {}
    for s in samples:
        with_durations([l[2] for l in route])
        t0 = time.perf_counter()
        recompute(s, 0)
        plain = time.perf_counter() - t0
        d, req, r = plan(s)
        r["gather_run_s"] = plain
        r["capture_per_launch_ms"] = 1e3 * (r["plan_total_s"] - plain - r["solve_s"]) / launches
        r["required_not_in_counts_plan"] = int((req & ~req_counts).sum())
        out["gather"][str(s)] = r
        plans[s] = (d, req)
        with_durations(d)
        dose = recompute(0, args.holdout_seed)
        out["gather_plan_under_photons"][str(s)] = {
            "seed": args.holdout_seed,
            "counts_required_area_at_or_above_min": float(area[req_counts & (dose >= m)].sum() / area[req_counts].sum())}
    s = max(samples)
    with_durations(d_counts)
    dose = recompute(s, 0)
    req = plans[s][1]
    out["counts_plan_under_gather"] = {
        "samples": s, "gather_required_area_below_min": float(area[req & ~(dose >= m)].sum() / area[req].sum())}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
