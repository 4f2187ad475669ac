"""Developer tool (not the bench): what the free-origin traversal kernel (csrc/uvrt_extend_free.hip) costs, on the test
room at 2^21 rays.  One JSON line:

  (a) lamp         the fixed-lamp kernel on the generated rays of route position 0
  (b) free_lamp    the free-origin kernel on the same rays, written as free rays
  (c) free_sweep   the free-origin kernel on a sweep from route position 0 to position 1
  (d) reference    the reference's own extend.cl (oracle/_ref, strict build) on (c)'s rays, where it was built

Each figure is the median kernel time of ROUNDS (default 7, at least 5) timed launches after a warm-up launch, taken from
uvrt_extend_time_ms (device events around the extend launch alone); the cases are interleaved round by round, in one
process, so that clock drift does not favour one of them.  (d) is timed by oracle/ref_gpu.cpp's own events around its
kernel.  Counts are checked once: (b) against (a), (c) against the reference kernel in flavour 1.
Lives under tests/ because it uses the oracle's scene loader.

    python tests/tools/free_bench.py [--rays N] [--rounds R] [--flavour 0|1]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1 << 21)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--flavour", type=int, default=0)
    a = ap.parse_args()
    n, rounds = a.rays, max(a.rounds, 5)
    try:                       # torch's HIP runtime first where torch is used in the same process (tests/conftest.py)
        import torch
        if torch.cuda.is_available():
            torch.cuda.init()
    except Exception:
        pass
    pkg, orc = g.load_package(), g.load_oracle()
    s = orc.Scene(os.path.join(ROOT, "tests/golden/testroomopt.glb"))
    route = orc.load_route(os.path.join(ROOT, "tests/golden/lange_route.xml"))
    comp = orc.Computation(s, route["lamps"], 1 << 16, route["lightHeight"], route["lightLength"], route["lightIntensity"])
    p0, p1 = comp.lamp_world_pos(route["lamps"][0]), comp.lamp_world_pos(route["lamps"][1])
    length = route["lightLength"]

    c = pkg.capi.Ctx(0)
    c.set_scene(s.tris, s.nodes, s.triIdx)
    c.resize_rays(n)
    c.set_flavour(a.flavour)
    c.set_pipeline(False)      # one launch at a time: kernel time, not overlap
    c.set_timing(True)

    # the rays of (a) / (b) and of (c) / (d), read back once
    c.set_record_hits(True)
    c.seed = 0
    c.generate(p0, length, 0, n)
    lamp_rays = c.read_rays(0, n)
    c.seed = 0
    c.generate_sweep(p0, p1, length, 0, n)
    sweep_rays = c.read_rays(0, n)
    c.set_record_hits(False)

    def lamp():
        c.seed = 0
        c.generate(p0, length, 0, n)

    def free_lamp():
        c.write_free_rays(lamp_rays)

    def free_sweep():
        c.seed = 0
        c.generate_sweep(p0, p1, length, 0, n)

    cases = {"lamp": lamp, "free_lamp": free_lamp, "free_sweep": free_sweep}
    counts, ms = {}, {k: [] for k in cases}
    for rnd in range(rounds + 1):                 # round 0 warms up (code objects, hot records, buffers) and checks counts
        for name, make in cases.items():
            c.reset(False)
            make()
            c.sync()
            c.extend_time_ms()
            c.extend(n)
            c.sync()
            t, k = c.extend_time_ms()
            assert k == 1
            if rnd == 0:
                counts[name] = c.read_counts()
            else:
                ms[name].append(t)
    out = {"tool": "free_bench", "scene": "testroomopt.glb", "rays": n, "rounds": rounds, "flavour": a.flavour,
           "device_cus": c.device_cus()}
    out["counts_free_lamp_equal_lamp"] = bool(np.array_equal(counts["free_lamp"], counts["lamp"]))
    for name in cases:
        med = statistics.median(ms[name])
        out[name] = {"ms_median": round(med, 4), "ms_min": round(min(ms[name]), 4), "ms_max": round(max(ms[name]), 4),
                     "mray_s": round(n / med / 1e3, 1), "hit_share": round(float(counts[name].sum()) / n, 4)}
    c.close()
    if orc.refgpu() is not None and n % 256 == 0:
        ref_ms = []
        ref_counts = None
        for rnd in range(rounds + 1):
            r = sweep_rays.copy()
            r["dist"] = np.float32(1e30)
            r["triID"] = 0
            ref_counts, t = orc.refgpu_extend(r, s.tris, s.nodes, s.triIdx)
            if rnd:
                ref_ms.append(t)
        med = statistics.median(ref_ms)
        out["reference"] = {"ms_median": round(med, 4), "ms_min": round(min(ref_ms), 4), "ms_max": round(max(ref_ms), 4),
                            "mray_s": round(n / med / 1e3, 1), "hit_share": round(float(ref_counts.sum()) / n, 4)}
        if a.flavour == 1:
            out["counts_free_sweep_equal_reference"] = bool(np.array_equal(counts["free_sweep"], ref_counts))
        out["free_lamp_over_reference"] = round(out["free_lamp"]["mray_s"] / out["reference"]["mray_s"], 3)
        out["free_sweep_over_reference"] = round(out["free_sweep"]["mray_s"] / out["reference"]["mray_s"], 3)
    else:
        out["reference"] = None
    out["free_lamp_over_lamp"] = round(out["free_lamp"]["mray_s"] / out["lamp"]["mray_s"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
