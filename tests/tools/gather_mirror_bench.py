"""Developer tool (not the bench), on the GPU: what the mirror gather costs (include/uvrt.h "specular panels",
RayTracer::mirrorMap).  One JSON line.

    python tests/tools/gather_mirror_bench.py [--rounds R] [--samples 16]
    python tests/tools/gather_mirror_bench.py --split [--rounds R]      (under a kernel trace: only mirror calls are made)

The protocol of tests/tools/gather_faces_bench.py: whole calls between two device events on the context's stream, the states
interleaved round by round in one process, the median of ROUNDS (default 7) after a warm-up round; `spread` is (max - min) /
median of the rounds.  No time is fixed in advance: the yardstick is uvrt_gather_direct at the same S in the same process, which
the mirror gather leaves untouched.  On the test room at position 0 of lange_route, one panel on the wall whose centroids have
x >= 1.2 (the plane x = 1.47 looking at the room, rho = 0.85), everything in one chunk.

  uvrt_gather_direct against uvrt_gather_mirror(add = 0) at S samples, and the two traversal launches of the mirror call
  (closest hit, shadow rays) from the context's own launch timing -- the call's other three kernels (generate, fold, reduce) are
  what is left
  a gather launch (uvrt_gather_direct, then uvrt_accumulate_expected) without and with the panel (uvrt_gather_mirror(add = 1)
  between the two)

--split makes one warm-up call and ROUNDS mirror calls and nothing else, so that a kernel trace of the process (rocprofv3
--kernel-trace --stats -- python ... --split) shows the five kernels of a call side by side."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PE = 1 << 21
PANEL = "mirror 1.2 -1e30 -1e30 1e30 1e30 1e30 0.85 plane 1.47 0 0 -1 0 0\n"


def summary(v):
    med = statistics.median(v)
    return {"ms_median": round(med, 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
            "spread": round((max(v) - min(v)) / med, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--split", action="store_true")
    args = ap.parse_args()
    rounds = max(args.rounds, 5)
    S = args.samples
    import torch               # torch's HIP runtime first where torch is used in the same process (tests/conftest.py)
    torch.cuda.init()
    import __graft_entry__ as g
    import gather_mirror_restate as gm
    pkg, orc = g.load_package(), g.load_oracle()
    s = orc.Scene(os.path.join(ROOT, "tests/golden/testroomopt.glb"))
    route = orc.load_route(os.path.join(ROOT, "tests/golden/lange_route.xml"))
    comp = orc.Computation(s, route["lamps"], 1 << 16, route["lightHeight"], route["lightLength"], route["lightIntensity"])
    p0 = comp.lamp_world_pos(route["lamps"][0])
    length = route["lightLength"]
    panels, members = gm.rules_panels(s.tris, PANEL)
    st = torch.cuda.Stream()
    c = pkg.capi.Ctx(0)
    c.set_scene(s.tris, s.nodes, s.triIdx)
    c.set_pipeline(False)
    c.resize_rays(s.T * S)                                  # every launch in one chunk
    c.set_mirrors([pkg.capi.mirror(q, m, rho) for q, m, rho in panels], members)
    out = {"tool": "gather_mirror_bench", "scene": "testroomopt.glb", "triangles": s.T, "panel_triangles": int((members == 1).sum()),
           "rounds": rounds, "device_cus": c.device_cus(), "samples": S}
    if args.split:
        for _ in range(rounds + 1):
            c.gather_mirror(p0, p0, length, S, 0, PE)
        c.sync()
        c.close()
        out["mode"] = "split: %d mirror calls for a kernel trace" % (rounds + 1)
        print(json.dumps(out))
        return
    c.gather_direct(p0, p0, length, S, 0, PE)
    c.gather_mirror(p0, p0, length, S, 0, PE)
    c.set_stream(st.cuda_stream)

    def launch(mirrored):
        c.gather_direct(p0, p0, length, S, 0, PE)
        if mirrored:
            c.gather_mirror(p0, p0, length, S, 0, PE, add=1)
        c.accumulate_expected(1.0)

    states = [("gather_direct", lambda: c.gather_direct(p0, p0, length, S, 0, PE)),
              ("gather_mirror", lambda: c.gather_mirror(p0, p0, length, S, 0, PE)),
              ("gather_launch", lambda: launch(False)), ("gather_launch_with_panel", lambda: launch(True))]
    wm = {name: [] for name, _ in states}
    traversal = []
    for rnd in range(rounds + 1):               # round 0 warms up (code objects, buffers)
        for name, call in states:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            call()
            e1.record(st)
            e1.synchronize()
            if rnd:
                wm[name].append(e0.elapsed_time(e1))
        # the two traversal launches of one mirror call, from the context's launch timing (events around each launch)
        c.set_timing(True)
        c.extend_time_ms()
        c.gather_mirror(p0, p0, length, S, 0, PE)
        ms, launches = c.extend_time_ms()
        c.set_timing(False)
        if rnd:
            assert launches == 2, launches
            traversal.append(ms)
    rec = {name: summary(v) for name, v in wm.items()}
    rec["mirror_traversals_closest_plus_shadow"] = summary(traversal)
    rec["mirror_over_direct"] = round(rec["gather_mirror"]["ms_median"] / rec["gather_direct"]["ms_median"], 4)
    rec["mirror_other_kernels_ms"] = round(rec["gather_mirror"]["ms_median"] - rec["mirror_traversals_closest_plus_shadow"]["ms_median"], 4)
    rec["launch_with_panel_over_launch"] = round(rec["gather_launch_with_panel"]["ms_median"] / rec["gather_launch"]["ms_median"], 4)
    out["states"] = rec
    c.sync()
    c.set_stream(None)
    c.clock_probe_start(2000)
    c.gather_mirror(p0, p0, length, S, 0, PE)
    out["shader_mhz_under_load"] = round(c.clock_probe_read(), 1)
    c.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
