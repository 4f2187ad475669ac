"""Developer tool (not the bench), on the GPU: what the batched direct gather costs and saves (include/uvrt.h "batched direct
gather", RayTracer::gatherBatch).  One JSON line.

    python tests/tools/gather_batch_bench.py [--rounds R] [--launches 16] [--no-plan]

The protocol of tests/tools/gather_links_bench.py: whole calls between two device events on the context's stream, the states
interleaved round by round in one process, the median of ROUNDS (default 7) after a warm-up round; `spread` is (max - min) /
median of the rounds.  On the test room at S = 16, K = 16 launches from the route's first positions (stops and the segments
between them, alternating), seeds 0 .. K - 1:

  K x uvrt_gather_direct                                  the launch-by-launch path, the yardstick (the parent's code)
  uvrt_gather_direct_batch of K at capacity K T S         one chunk
  the same batch at a capacity of 4 launches per chunk    K / 4 chunks
  K x uvrt_gather_batch_select                            what putting the planes back costs

and, wall clock with a device sync at the end, RayTracer::PlanDurations over grid:8,8 at S = 16 (64 gather launches per
iteration of the route) with gatherBatch = 0, 16 and 64, interleaved the same way.  Before anything is timed every batch plane is compared
with its single call, bit for bit."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
S = 16
PE = 1 << 21


def summary(v):
    med = statistics.median(v)
    return {"ms_median": round(med, 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
            "spread": round((max(v) - min(v)) / med, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=16)
    ap.add_argument("--no-plan", action="store_true")
    args = ap.parse_args()
    rounds = max(args.rounds, 5)
    K = min(max(args.launches, 2), 64)
    import numpy as np
    import torch               # torch's HIP runtime first where torch is used in the same process (tests/conftest.py)
    torch.cuda.init()
    import __graft_entry__ as g
    pkg, orc = g.load_package(), g.load_oracle()
    glb, xml = os.path.join(ROOT, "tests/golden/testroomopt.glb"), os.path.join(ROOT, "tests/golden/lange_route.xml")
    s = orc.Scene(glb)
    route = orc.load_route(xml)
    comp = orc.Computation(s, route["lamps"], 1 << 16, route["lightHeight"], route["lightLength"], route["lightIntensity"])
    places = [comp.lamp_world_pos(l) for l in route["lamps"]]
    length = route["lightLength"]
    launches = []
    for k in range(K):
        a = places[(k // 2) % len(places)]
        b = a if k % 2 == 0 else places[(k // 2 + 1) % len(places)]
        launches.append(dict(frm=a, to=b, light_length=length, samples=S, seed=k, photons_equiv=PE))
    c = pkg.capi.Ctx(0)
    c.set_scene(s.tris, s.nodes, s.triIdx)
    c.set_pipeline(False)
    out = {"tool": "gather_batch_bench", "scene": "testroomopt.glb", "triangles": s.T, "samples": S, "launches": K,
           "rounds": rounds, "device_cus": c.device_cus()}
    caps = {"one_chunk": K * s.T * S, "4_launches_per_chunk": 4 * s.T * S}

    def singles():
        for l in launches:
            c.gather_direct(l["frm"], l["to"], l["light_length"], S, l["seed"], PE)

    def selects():
        for k in range(K):
            c.gather_batch_select(k)

    # the contract first: every plane is its single call's, at both capacities
    for cap in caps.values():
        c.resize_rays(cap)
        c.gather_direct_batch(launches)
        for k, l in enumerate(launches):
            c.gather_direct(l["frm"], l["to"], l["light_length"], S, l["seed"], PE)
            if c.read_gather_batch(k).tobytes() != c.read_expected().tobytes():
                raise SystemExit("plane %d differs from its single call at capacity %d" % (k, cap))
    out["planes_equal_single_calls"] = True
    st = torch.cuda.Stream()
    c.set_stream(st.cuda_stream)
    states = [("singles", caps["one_chunk"], singles), ("batch_one_chunk", caps["one_chunk"], lambda: c.gather_direct_batch(launches)),
              ("batch_4_launches_per_chunk", caps["4_launches_per_chunk"], lambda: c.gather_direct_batch(launches)),
              ("singles_at_4_launches_capacity", caps["4_launches_per_chunk"], singles),
              ("selects", caps["4_launches_per_chunk"], selects)]
    wm = {name: [] for name, _, _ in states}
    for rnd in range(rounds + 1):                   # round 0 warms up (code objects, buffers)
        for name, cap, call in states:
            c.resize_rays(cap)                      # (synchronises; outside the events)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            call()
            e1.record(st)
            e1.synchronize()
            if rnd:
                wm[name].append(e0.elapsed_time(e1))
    for name, v in wm.items():
        out[name] = summary(v)
    for name in ("batch_one_chunk", "batch_4_launches_per_chunk"):
        out[name + "_over_singles"] = round(out[name]["ms_median"] / out["singles"]["ms_median"], 4)
    c.sync()
    c.set_stream(None)
    c.clock_probe_start(2000)
    c.gather_direct_batch(launches)
    out["shader_mhz_under_load"] = round(c.clock_probe_read(), 1)
    c.close()

    if not args.no_plan:
        from uvrt_amd import host
        rt = host.RayTracer(glb, xml, device=0)
        rt.SetCandidateGrid(8, 8, 0.5)
        rt.photonCount = 64 * (1 << 15)
        lamps = rt.lamps()
        plan, first = {B: [] for B in (0, 16, 64)}, {}
        for rnd in range(rounds + 1):
            for B in plan:
                rt.set_lamps(lamps)
                rt.ResetDosageMap()
                rt.Sync()
                t0 = time.perf_counter()
                d, rep = rt.PlanDurationsBatched(B, gather_samples=S)
                rt.Sync()
                dt = (time.perf_counter() - t0) * 1e3
                rt.EndPlan()
                first.setdefault(B, np.asarray(d).tobytes())
                if np.asarray(d).tobytes() != first[0]:
                    raise SystemExit("gatherBatch = %d planned other durations" % B)
                if rnd:
                    plan[B].append(dt)
        out["plan_grid_8x8"] = {"launches": 64 * rt.maxIterations, "iterations": rt.maxIterations, "wall_clock": True,
                                "durations_equal": True}
        for B, v in plan.items():
            out["plan_grid_8x8"]["gather_batch_%d" % B] = summary(v)
        for B in (16, 64):
            out["plan_grid_8x8"]["gather_batch_%d_over_0" % B] = round(
                out["plan_grid_8x8"]["gather_batch_%d" % B]["ms_median"] / out["plan_grid_8x8"]["gather_batch_0"]["ms_median"], 4)
        rt.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
