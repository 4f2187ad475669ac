"""Developer tool (not the bench), on the GPU: what a reflectance per face costs (include/uvrt.h "per-face reflectance",
RayTracer::reflectMap).  One JSON line.

    python tests/tools/gather_reflect_map_bench.py [--rounds R] [--samples 16,64,256]

The protocol of tests/tools/gather_faces_bench.py: whole calls between two device events on the context's stream, the states
interleaved round by round in one process, the median of ROUNDS (default 7) after a warm-up round; `spread` is (max - min) /
median of the rounds.  No time is fixed in advance: the yardstick of every mapped state is its one-rho twin in the same process.
On the test room, with the face planes of a direct gather at S = 16 as the emitters, one context (both calls read the same sided
links); the map is 0.85 where the centroid has x >= 1.2 and 0.05 elsewhere.

  uvrt_gather_indirect_linked_sided against uvrt_gather_indirect_linked_mapped at S2 = 16, 64, 256 with K = 1 and 4
  a gather launch (uvrt_gather_direct at S = 16 with the faces state on, then K = 4 bounces added) without and with the map"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
S_DIRECT = 16
PE = 1 << 21
LINK_SEED = 0x85EBCA6B


def summary(v):
    med = statistics.median(v)
    return {"ms_median": round(med, 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
            "spread": round((max(v) - min(v)) / med, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--samples", default="16,64,256")
    args = ap.parse_args()
    rounds = max(args.rounds, 5)
    samples = [int(v) for v in args.samples.split(",")]
    import torch               # torch's HIP runtime first where torch is used in the same process (tests/conftest.py)
    torch.cuda.init()
    import __graft_entry__ as g
    pkg, orc = g.load_package(), g.load_oracle()
    s = orc.Scene(os.path.join(ROOT, "tests/golden/testroomopt.glb"))
    route = orc.load_route(os.path.join(ROOT, "tests/golden/lange_route.xml"))
    comp = orc.Computation(s, route["lamps"], 1 << 16, route["lightHeight"], route["lightLength"], route["lightIntensity"])
    p0 = comp.lamp_world_pos(route["lamps"][0])
    length = route["lightLength"]
    st = torch.cuda.Stream()
    c = pkg.capi.Ctx(0)
    c.set_scene(s.tris, s.nodes, s.triIdx)
    c.set_pipeline(False)
    c.resize_rays(s.T * max([S_DIRECT] + samples))          # every launch and every build in one chunk
    lined = s.tris[:, 12] >= np.float32(1.2)
    plane = np.where(lined, np.float32(0.85), np.float32(0.05)).astype(np.float32)
    c.write_reflectance(0, plane)
    c.write_reflectance(1, plane)
    out = {"tool": "gather_reflect_map_bench", "scene": "testroomopt.glb", "triangles": s.T, "lined_triangles": int(lined.sum()),
           "rounds": rounds, "device_cus": c.device_cus(), "direct_samples": S_DIRECT, "by_samples": {}}
    c.set_gather_faces(1)
    c.gather_direct(p0, p0, length, S_DIRECT, 0, PE)
    c.set_stream(st.cuda_stream)

    def launch(mapped):
        c.gather_direct(p0, p0, length, S_DIRECT, 0, PE)
        if mapped:
            c.gather_indirect_linked_mapped(4, add=1)
        else:
            c.gather_indirect_linked_sided(0.5, 4, add=1)

    for S2 in samples:
        c.indirect_links_build_sided(S2, LINK_SEED)
        states = [("linked_sided_K1", lambda: c.gather_indirect_linked_sided(0.5, 1)),
                  ("linked_mapped_K1", lambda: c.gather_indirect_linked_mapped(1)),
                  ("linked_sided_K4", lambda: c.gather_indirect_linked_sided(0.5, 4)),
                  ("linked_mapped_K4", lambda: c.gather_indirect_linked_mapped(4))]
        if S2 == samples[0]:
            states += [("gather_launch_sided", lambda: launch(False)), ("gather_launch_mapped", lambda: launch(True))]
        wm = {name: [] for name, _ in states}
        for rnd in range(rounds + 1):               # round 0 warms up (code objects, buffers)
            for name, call in states:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                call()
                e1.record(st)
                e1.synchronize()
                if rnd:
                    wm[name].append(e0.elapsed_time(e1))
        rec = {name: summary(v) for name, v in wm.items()}
        for a, b in (("linked_mapped_K1", "linked_sided_K1"), ("linked_mapped_K4", "linked_sided_K4"),
                     ("gather_launch_mapped", "gather_launch_sided")):
            if a in rec:
                rec[a + "_over_" + b] = round(rec[a]["ms_median"] / rec[b]["ms_median"], 4)
        out["by_samples"]["S2_%d" % S2] = rec
    c.sync()
    c.set_stream(None)
    c.clock_probe_start(2000)
    c.indirect_links_build_sided(samples[-1], LINK_SEED)
    out["shader_mhz_under_load"] = round(c.clock_probe_read(), 1)
    c.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
