"""Developer tool (not the bench): what the shadow-ray kernel (csrc/uvrt_occlude.hip) buys over answering the same question
with the closest-hit kernel, on the test room's own gather rays at S = 64 (2.9 M rays from route position 0).  One JSON line:

  (a) occlude      k_occlude_free: the rays with their tmax, one byte per ray
  (b) closest_hit  the same rays through k_extend_free with hit records (the comparison dist < tmax is then the host's)
  gather_direct    the whole uvrt_gather_direct call (generate, trace, reduce) between two device events on the context's stream

(a) and (b) are the median kernel time of ROUNDS (default 7, at least 5) timed launches after a warm-up launch, from
uvrt_extend_time_ms (device events around the traversal launch alone), interleaved round by round in one process so that
clock drift favours neither -- tests/tools/free_bench.py's method.  The warm-up round checks that both give the same answer
on every ray.  Lives under tests/ because it uses the oracle's scene loader and the restated rays (tests/gather_restate.py).

    python tests/tools/gather_bench.py [--samples S] [--rounds R] [--flavour 0|1]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as g  # noqa: E402
import gather_restate as gr  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--flavour", type=int, default=0)
    a = ap.parse_args()
    S, rounds = a.samples, max(a.rounds, 5)
    torch = None
    try:                       # torch's HIP runtime first where torch is used in the same process (tests/conftest.py)
        import torch
        if torch.cuda.is_available():
            torch.cuda.init()
        else:
            torch = None
    except Exception:
        torch = None
    pkg, orc = g.load_package(), g.load_oracle()
    s = orc.Scene(os.path.join(ROOT, "tests/golden/testroomopt.glb"))
    route = orc.load_route(os.path.join(ROOT, "tests/golden/lange_route.xml"))
    comp = orc.Computation(s, route["lamps"], 1 << 16, route["lightHeight"], route["lightLength"], route["lightIntensity"])
    p0 = comp.lamp_world_pos(route["lamps"][0])
    length = route["lightLength"]
    rays, _ = gr.samples(orc, s.tris, p0, p0, length, S, 0)
    n = rays.size
    closest = rays.copy()
    closest["dist"] = np.float32(1e30)

    c = pkg.capi.Ctx(0)
    c.set_scene(s.tris, s.nodes, s.triIdx)
    c.resize_rays(n)
    c.set_flavour(a.flavour)
    c.set_pipeline(False)      # one launch at a time: kernel time, not overlap
    c.set_timing(True)
    c.set_record_hits(True)

    answers, ms = {}, {"occlude": [], "closest_hit": []}
    for rnd in range(rounds + 1):                 # round 0 warms up (code objects, records, buffers) and checks the answers
        c.sync()
        c.extend_time_ms()
        occ = c.occluded(rays)
        t, k = c.extend_time_ms()
        assert k == 1
        if rnd == 0:
            answers["occlude"] = occ
        else:
            ms["occlude"].append(t)
        c.reset(False)
        c.write_free_rays(closest)
        c.sync()
        c.extend_time_ms()
        c.extend(n)
        c.sync()
        t, k = c.extend_time_ms()
        assert k == 1
        if rnd == 0:
            hit = c.read_rays(0, n)["dist"]
            answers["closest_hit"] = (hit < rays["dist"]).astype(np.uint8)        # (a miss is 1e30f; a NaN tmax compares false)
        else:
            ms["closest_hit"].append(t)
    out = {"tool": "gather_bench", "scene": "testroomopt.glb", "samples": S, "rays": int(n), "rounds": rounds,
           "flavour": a.flavour, "device_cus": c.device_cus(),
           "answers_equal": bool(np.array_equal(answers["occlude"], answers["closest_hit"])),
           "occluded_share": round(float(answers["occlude"].mean()), 4)}
    for name in ms:
        med = statistics.median(ms[name])
        out[name] = {"ms_median": round(med, 4), "ms_min": round(min(ms[name]), 4), "ms_max": round(max(ms[name]), 4),
                     "mray_s": round(n / med / 1e3, 1)}
    out["occlude_over_closest_hit"] = round(out["occlude"]["mray_s"] / out["closest_hit"]["mray_s"], 3)
    c.set_timing(False)
    c.set_record_hits(False)
    if torch is not None:
        st = torch.cuda.Stream()
        c.set_stream(st.cuda_stream)
        whole = []
        for rnd in range(rounds + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            c.gather_direct(p0, p0, length, S, rnd, 1 << 21)
            e1.record(st)
            e1.synchronize()
            if rnd:
                whole.append(e0.elapsed_time(e1))
        c.sync()
        c.set_stream(None)
        med = statistics.median(whole)
        out["gather_direct"] = {"ms_median": round(med, 4), "ms_min": round(min(whole), 4), "ms_max": round(max(whole), 4),
                                "mray_s": round(n / med / 1e3, 1), "triangles": int(s.T)}
    else:
        out["gather_direct"] = None
    c.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
