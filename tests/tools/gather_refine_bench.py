"""Developer tool (not the bench), on the GPU: what the adaptive gather costs and what it does to a plan (include/uvrt.h
uvrt_gather_refine, RayTracer::gatherRelError).  One JSON line.

    python tests/tools/gather_refine_bench.py [--rounds R] [--tau 0.1] [--max-extra 64] [--only-timing]
                                              [--ppl N] [--iterations I] [--holdout-seed SEED]

Timing, over the whole test room from route position 0 (stop) and on the sweep 0 -> 1, S0 = 16 stratified, the variance plane
on, photons_equiv 2^21, one context whose capacity holds every launch in one chunk; all states interleaved round by round in
one process, the median of ROUNDS (default 7) after a warm-up round, between two device events on the context's stream
(tests/tools/gather_sampling_bench.py's method; the refine's one read-back stalls the host inside the interval):
  gather            uvrt_gather_direct alone
  gather_refine     uvrt_gather_direct + uvrt_gather_refine(tau, max_extra)
  uniform           uvrt_gather_direct at S = 16 + the refine's mean extra samples per triangle, rounded
  refine_nothing    uvrt_gather_direct + a refine at tau = 1e6: count, scan and the read-back, nothing after them
and the refine's own parts from them: count_scan_readback = refine_nothing - gather; trace = the shadow-ray kernel's device
time inside the refine (uvrt_extend_time_ms, a round of its own with the launch timing on); generate_reduce = the rest.  Per
kernel figures come from a kernel trace of `--only-timing`.

The plan (unless --only-timing): tests/tools/plan_confidence_bench.py's set-up -- the 12 positions of lange_route, S = 16
stratified, 4 iterations, photons_equiv = ppl -- at z = 0 and z = 2, each without and with the refine: required, unresolved and
unreachable rows, the rows of the unrefined z = 0 plan lost, the total duration, and the share of the plan's required area (and
of the unrefined z = 0 plan's) whose dose reaches the minimum when the durations are recomputed with PHOTONS from another SEED.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
S0 = 16
PE = 1 << 21


def summary(v):
    return {"ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}


def timing(pkg, orc, torch, rounds, tau, max_extra):
    s = orc.Scene(os.path.join(ROOT, "tests/golden/testroomopt.glb"))
    route = orc.load_route(os.path.join(ROOT, "tests/golden/lange_route.xml"))
    comp = orc.Computation(s, route["lamps"], 1 << 16, route["lightHeight"], route["lightLength"], route["lightIntensity"])
    p0, p1 = comp.lamp_world_pos(route["lamps"][0]), comp.lamp_world_pos(route["lamps"][1])
    length = route["lightLength"]
    c = pkg.capi.Ctx(0)
    c.set_scene(s.tris, s.nodes, s.triIdx)
    c.resize_rays(s.T * (S0 + max_extra))       # one chunk whatever the refine asks for
    c.set_pipeline(False)
    c.set_gather_sampling(1)
    c.set_gather_variance(1)
    st = torch.cuda.Stream()
    out = {}
    for case, frm, to in (("stop", p0, p0), ("sweep", p0, p1)):
        c.gather_direct(frm, to, length, S0, 0, PE)
        extra, refined = c.gather_refine(tau, max_extra, 0xFFFFFFFF)
        uniform_s = S0 + int(round(extra / s.T))

        def gather(S=S0):
            c.gather_direct(frm, to, length, S, 0, PE)

        states = (("gather", lambda: gather()),
                  ("gather_refine", lambda: (gather(), c.gather_refine(tau, max_extra, 0xFFFFFFFF))),
                  ("uniform", lambda: gather(uniform_s)),
                  ("refine_nothing", lambda: (gather(), c.gather_refine(1e6, max_extra, 0xFFFFFFFF))))
        ms = {name: [] for name, _ in states}
        c.set_stream(st.cuda_stream)
        for rnd in range(rounds + 1):           # round 0 warms up (code objects, records, buffers, the planes)
            for name, call in states:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                call()
                e1.record(st)
                e1.synchronize()
                if rnd:
                    ms[name].append(e0.elapsed_time(e1))
        c.sync()
        c.set_stream(None)
        # the shadow-ray kernel inside the refine: device events around the traversal launches alone
        c.set_timing(True)
        trace = []
        for rnd in range(rounds + 1):
            gather()
            c.sync()
            c.extend_time_ms()
            c.gather_refine(tau, max_extra, 0xFFFFFFFF)
            t, k = c.extend_time_ms()
            assert k == 1
            if rnd:
                trace.append(t)
        c.set_timing(False)
        rec = {name: summary(v) for name, v in ms.items()}
        rec["extra_rays"], rec["refined_triangles"] = extra, refined
        rec["mean_samples"] = round(S0 + extra / s.T, 2)
        rec["uniform_samples"] = uniform_s
        whole = rec["gather_refine"]["ms_median"] - rec["gather"]["ms_median"]
        head = rec["refine_nothing"]["ms_median"] - rec["gather"]["ms_median"]
        tr = statistics.median(trace)
        rec["refine"] = {"ms": round(whole, 4), "count_scan_readback_ms": round(head, 4), "trace_ms": round(tr, 4),
                         "generate_reduce_ms": round(whole - head - tr, 4)}
        rec["refine_over_gather"] = round(whole / rec["gather"]["ms_median"], 3)
        rec["gather_refine_over_uniform"] = round(rec["gather_refine"]["ms_median"] / rec["uniform"]["ms_median"], 3)
        out[case] = rec
    out["device_cus"] = c.device_cus()
    c.close()
    return out


def plans(args, np, host):
    rt = host.RayTracer(os.path.join(ROOT, "tests", "golden", "testroomopt.glb"),
                        os.path.join(ROOT, "tests", "golden", "lange_route.xml"), device=0)
    route = rt.lamps()
    P = len(route)
    rt.photonCount = args.ppl * P
    rt.maxIterations = args.iterations
    rt.viewMode = host.VIEW_DOSAGE
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

    out = {"triangles": rt.mesh.triangleCount, "positions": P, "iterations": args.iterations, "photons_per_launch": args.ppl,
           "samples": S0, "sampling": "stratified", "min_dose": m, "holdout_seed": args.holdout_seed, "plans": {}}
    req0 = None
    for z in (0.0, 2.0):
        for tau in (0.0, args.tau):
            with_durations([l[2] for l in route])
            rt.ctx.seed = 0
            d, rep = rt.PlanDurationsRefined(tau, args.max_extra, gather_samples=S0, gather_sampling=1, gather_confidence=z)
            req, cls = rt.ctx.plan_read_required(), rt.ctx.plan_read_classes()
            if req0 is None:
                req0 = req
            r = {k: rep[k] for k in ("required", "unreachable", "unresolved", "area_required", "area_unreachable", "area_unresolved",
                                     "total_duration", "used_positions", "gap", "converged", "min_dose_ratio")}
            lost = req0 & ~req
            r["rows_of_plain_z0_lost"] = {"unresolved": int((lost & (cls == 2)).sum()), "unreachable": int((lost & (cls == 1)).sum()),
                                          "area": float(area[lost].sum())}
            with_durations(d)
            ok = photons(args.holdout_seed) >= m
            r["own_required_area_at_or_above_min"] = float(area[req & ok].sum() / area[req].sum())
            r["plain_z0_required_area_at_or_above_min"] = float(area[req0 & ok].sum() / area[req0].sum())
            out["plans"]["z%g_%s" % (z, "refined" if tau else "plain")] = r
    rt.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--tau", type=float, default=0.1)
    ap.add_argument("--max-extra", type=int, default=64)
    ap.add_argument("--only-timing", action="store_true")
    ap.add_argument("--ppl", type=int, default=1 << 20, help="photons_equiv of a plan's gather launch, photons of a recompute launch")
    ap.add_argument("--iterations", type=int, default=4)
    ap.add_argument("--holdout-seed", type=int, default=12345)
    args = ap.parse_args()
    import torch               # torch's HIP runtime first where torch is used in the same process (tests/conftest.py)
    torch.cuda.init()
    import numpy as np
    import __graft_entry__ as g
    pkg, orc = g.load_package(), g.load_oracle()
    from uvrt_amd import host
    out = {"tool": "gather_refine_bench", "scene": "testroomopt.glb", "tau": args.tau, "max_extra": args.max_extra,
           "rounds": max(args.rounds, 5), "timing": timing(pkg, orc, torch, max(args.rounds, 5), args.tau, args.max_extra)}
    if not args.only_timing:
        out["plan"] = plans(args, np, host)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
