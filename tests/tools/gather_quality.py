"""Developer tool (no GPU): how tight the direct gather's estimate is under both sampling modes (include/uvrt.h
uvrt_set_gather_sampling), from the CPU restatements alone.  One JSON line:

  for a stop (route position 0) and a sweep (position 0 -> 1), S = 4 / 16 / 64, gather seeds 0..7, mode independent /
  stratified: the 5th / 50th / 95th percentile and the rms of (expected / count - 1) over the triangles that N = 2^21 oracle
  photons resolve (>= 400 of them), and how many zero-photon triangles get an estimate; per (case, S) the per-seed ratio
  stratified width / independent width of the 5th-95th band, its minimum, maximum and mean.

The truth of the sweep is 2^21 oracle photons of position 0 whose origins are shifted along the segment by a uniform u each
(tests/gather_stratified_restate.py photon_counts).  The source of the table in DESIGN.md 13 and of the recorded constants in
tests/test_gather_stratified_cpu.py; takes a few minutes on one core.

    python tests/tools/gather_quality.py [--samples 4,16,64] [--seeds 8] [--photons 2097152]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as g  # noqa: E402
import gather_restate as gr  # noqa: E402
import gather_stratified_restate as gs  # noqa: E402

MODES = (("independent", gs.INDEPENDENT), ("stratified", gs.STRATIFIED))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", default="4,16,64")
    ap.add_argument("--seeds", type=int, default=8)
    ap.add_argument("--photons", type=int, default=1 << 21)
    a = ap.parse_args()
    orc = g.load_oracle()
    gr.check_rng(orc)
    s = orc.Scene(os.path.join(ROOT, "tests/golden/testroomopt.glb"))
    route = orc.load_route(os.path.join(ROOT, "tests/golden/lange_route.xml"))
    comp = orc.Computation(s, route["lamps"], 1 << 16, route["lightHeight"], route["lightLength"], route["lightIntensity"])
    p0, p1 = comp.lamp_world_pos(route["lamps"][0]), comp.lamp_world_pos(route["lamps"][1])
    length, N = route["lightLength"], a.photons
    out = {"tool": "gather_quality", "scene": "testroomopt.glb", "triangles": int(s.T), "photons": N, "min_photons": 400,
           "seeds": a.seeds, "cases": {}}
    for case, to in (("stop", p0), ("sweep", p1)):
        counts = gs.photon_counts(orc, s, p0, to, length, N)
        rec = {"resolved_triangles": int((counts >= 400).sum()), "zero_photon_triangles": int((counts == 0).sum()), "samples": {}}
        for S in (int(v) for v in a.samples.split(",")):
            rows = {name: [] for name, _ in MODES}
            for seed in range(a.seeds):
                for name, mode in MODES:
                    e, _, _ = gs.gather(orc, s, p0, to, length, S, seed, N, mode=mode)
                    p5, p50, p95, rms, lit = gs.quality(e, counts)
                    rows[name].append({"seed": seed, "p5": round(p5, 4), "p50": round(p50, 4), "p95": round(p95, 4),
                                       "width": round(p95 - p5, 4), "rms": round(rms, 4), "zero_photon_with_estimate": lit})
            ratios = [st["width"] / ind["width"] for st, ind in zip(rows["stratified"], rows["independent"])]
            rows["width_ratio"] = {"per_seed": [round(r, 4) for r in ratios], "min": round(min(ratios), 4),
                                   "max": round(max(ratios), 4), "mean": round(sum(ratios) / len(ratios), 4)}
            rec["samples"][str(S)] = rows
        out["cases"][case] = rec
    print(json.dumps(out))


if __name__ == "__main__":
    main()
