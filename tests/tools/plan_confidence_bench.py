"""Developer tool (not the bench), on the GPU: what planning for the gather's lower confidence bound buys and costs (include/uvrt.h
uvrt_plan_lower_confidence, PlanOptions::gatherConfidence).  One JSON line.

    python tests/tools/plan_confidence_bench.py [--ppl N] [--iterations I] [--samples S] [--z 0,2] [--holdout-seed SEED] [--rounds R]

tests/tools/plan_gather_bench.py's set-up: the test room, the 12 positions of lange_route, S = 16 stratified shadow rays per
triangle and launch, 4 iterations, photons_equiv = ppl.  One plan per z (0: the plan without a bound); each plan's durations are
then recomputed with PHOTONS from another SEED, and reported per plan:
  required / unreachable / unresolved rows and areas, total duration, rounds;
  rows_lost_against_z0: required rows of the z = 0 plan that the bound turned unresolved or unreachable;
  own_required_area_at_or_above_min: the share of the plan's own required area whose photon dose reaches the minimum;
  z0_required_area_at_or_above_min: the same over the z = 0 plan's required set (one yardstick for every z).
No threshold: nobody has measured this before.

And the time of the whole uvrt_gather_direct over the room at a stop (route position 0) with the variance plane on and off, between
two device events on the context's stream, both states interleaved round by round in one process, the median of ROUNDS (default
7) after a warm-up round -- tests/tools/gather_sampling_bench.py's method -- for S = 16 and S = 64, stratified.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def gather_times(pkg, orc, torch, rounds):
    s = orc.Scene(os.path.join(ROOT, "tests/golden/testroomopt.glb"))
    route = orc.load_route(os.path.join(ROOT, "tests/golden/lange_route.xml"))
    comp = orc.Computation(s, route["lamps"], 1 << 16, route["lightHeight"], route["lightLength"], route["lightIntensity"])
    p0 = comp.lamp_world_pos(route["lamps"][0])
    out = {}
    for S in (16, 64):
        c = pkg.capi.Ctx(0)
        c.set_scene(s.tris, s.nodes, s.triIdx)
        c.resize_rays(s.T * S)         # one chunk: one shadow-ray launch per call
        c.set_pipeline(False)
        c.set_gather_sampling(1)
        st = torch.cuda.Stream()
        c.set_stream(st.cuda_stream)
        ms = {"off": [], "on": []}
        for rnd in range(rounds + 1):  # round 0 warms up (code objects, records, buffers, the plane)
            for name, on in (("off", 0), ("on", 1)):
                c.set_gather_variance(on)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                c.gather_direct(p0, p0, route["lightLength"], S, 0, 1 << 21)
                e1.record(st)
                e1.synchronize()
                if rnd:
                    ms[name].append(e0.elapsed_time(e1))
        c.sync()
        c.set_stream(None)
        c.close()
        rec = {k: {"ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}
               for k, v in ms.items()}
        rec["on_over_off"] = round(rec["on"]["ms_median"] / rec["off"]["ms_median"], 3)
        out[str(S)] = rec
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ppl", type=int, default=1 << 20, help="photons_equiv of a gather launch, photons of a recompute launch")
    ap.add_argument("--iterations", type=int, default=4)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--z", default="0,2")
    ap.add_argument("--holdout-seed", type=int, default=12345)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    import torch               # torch's HIP runtime first where torch is used in the same process (tests/conftest.py)
    torch.cuda.init()
    import numpy as np
    import __graft_entry__ as g
    pkg, orc = g.load_package(), g.load_oracle()
    from uvrt_amd import host
    rt = host.RayTracer(os.path.join(ROOT, "tests", "golden", "testroomopt.glb"),
                        os.path.join(ROOT, "tests", "golden", "lange_route.xml"), device=0)
    route = rt.lamps()
    P = len(route)
    rt.photonCount = args.ppl * P
    rt.maxIterations = args.iterations
    rt.viewMode = host.VIEW_DOSAGE
    T = rt.mesh.triangleCount
    m = float(np.float32(rt.minDosage))
    t = rt.mesh.tris()
    a, b = t[:, 0:3] - t[:, 4:7], t[:, 0:3] - t[:, 8:11]
    area = (np.sqrt(np.sum(np.cross(a, b).astype(np.float32) ** 2, axis=1, dtype=np.float32)) / np.float32(2.0)).astype(np.float64)

    def with_durations(d):
        rt.set_lamps([(x, z, float(v)) for (x, z, _), v in zip(route, d)])
        rt.photonCount = args.ppl * P

    def photons(seed):
        rt.gatherSamples = 0
        rt.ctx.seed = seed
        rt.ResetDosageMap()
        rt.ComputeIterationsBatched(args.iterations)
        rt.Sync()
        return rt.read_dosage()

    out = {"tool": "plan_confidence_bench", "scene": "testroomopt.glb", "triangles": T, "positions": P, "iterations": args.iterations,
           "photons_per_launch": args.ppl, "samples": args.samples, "sampling": "stratified", "min_dose": m,
           "area_total": float(area.sum()), "holdout_seed": args.holdout_seed, "plans": {}}
    zs = [float(v) for v in args.z.split(",")]
    assert zs[0] == 0.0, "the first z is the yardstick: the plan without a bound"
    req0 = None
    for z in zs:
        with_durations([l[2] for l in route])
        rt.ctx.seed = 0
        d, rep = rt.PlanDurations(gather_samples=args.samples, gather_sampling=1, gather_confidence=z)
        req, cls = rt.ctx.plan_read_required(), rt.ctx.plan_read_classes()
        if req0 is None:
            req0 = req
        r = {k: rep[k] for k in ("required", "unreachable", "unresolved", "area_required", "area_unreachable", "area_unresolved",
                                 "total_duration", "used_positions", "gap", "converged", "min_dose_ratio")}
        r["rounds"] = rep["iterations"]
        lost = req0 & ~req
        r["rows_lost_against_z0"] = {"unresolved": int((lost & (cls == 2)).sum()), "unreachable": int((lost & (cls == 1)).sum()),
                                     "area": float(area[lost].sum())}
        with_durations(d)
        dose = photons(args.holdout_seed)
        ok = dose >= m
        r["own_required_area_at_or_above_min"] = float(area[req & ok].sum() / area[req].sum())
        r["z0_required_area_at_or_above_min"] = float(area[req0 & ok].sum() / area[req0].sum())
        r["z0_required_rows_below_min"] = int((req0 & ~ok).sum())
        out["plans"]["z%g" % z] = r
    rt.close()
    out["gather_direct_ms"] = gather_times(pkg, orc, torch, max(args.rounds, 5))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
