"""Developer tool (no GPU): how well the gather's variance plane covers the truth (include/uvrt.h uvrt_set_gather_variance,
DESIGN.md 14), from the CPU restatements alone.  One JSON line:

  for a stop (route position 0) and a sweep (position 0 -> 1), S = 4 / 16 / 64, gather seeds 0..7, z = 0 / 1 / 2 / 3 and the
  estimators "independent" (independent samples, sample variance of the mean), "stratified" (stratified samples, successive
  differences) and "stratified_sample_variance" (stratified samples, the sample variance: the estimator the stratified mode
  does NOT use): over the triangles that N = 2^21 oracle photons resolve (>= 400 of them), per seed the cover -- the share
  whose photon count is >= max(0, expected - z sqrt(variance)) --, the median of that bound over the count, the share of
  bounds that are 0, and "cover_with_count_noise", the share whose count is >= expected - z sqrt(variance + count): the count
  is a Poisson draw, and where the bound is tight its own scatter is what the plain cover measures; and per (case, S,
  estimator, z) the minimum and maximum over the seeds.

The truth of the sweep is tests/gather_stratified_restate.py photon_counts.  The source of the table in DESIGN.md 14 and of the
values recorded in tests/test_gather_variance_cpu.py; takes several minutes on one core.

    python tests/tools/gather_confidence.py [--samples 4,16,64] [--seeds 8] [--photons 2097152]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as g  # noqa: E402
import gather_restate as gr  # noqa: E402
import gather_stratified_restate as gs  # noqa: E402
import gather_variance_restate as gv  # noqa: E402

ZS = (0.0, 1.0, 2.0, 3.0)


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
    out = {"tool": "gather_confidence", "scene": "testroomopt.glb", "triangles": int(s.T), "photons": N, "min_photons": 400,
           "seeds": a.seeds, "z": list(ZS), "cases": {}}
    for case, to in (("stop", p0), ("sweep", p1)):
        counts = gs.photon_counts(orc, s, p0, to, length, N)
        rec = {"resolved_triangles": int((counts >= 400).sum()), "samples": {}}
        for S in (int(v) for v in a.samples.split(",")):
            rows = {"independent": [], "stratified": [], "stratified_sample_variance": []}
            for seed in range(a.seeds):
                e0, v0, _ = gv.gather(orc, s, p0, to, length, S, seed, N, gv.INDEPENDENT)
                e1, v1, x1 = gv.gather(orc, s, p0, to, length, S, seed, N, gv.STRATIFIED)
                # the sample variance on the stratified samples: (c*c) * v with c*c taken off the stratified plane's own rule
                _, _, _, nn = gr.tri_normals(np.ascontiguousarray(s.tris, dtype=np.float32))
                c = np.float64(N) * (0.5 * nn)
                v1s = np.where(nn == 0.0, 0.0, (c * c) * gv.sample_variance_v(x1))
                for name, e, v in (("independent", e0, v0), ("stratified", e1, v1), ("stratified_sample_variance", e1, v1s)):
                    row = {"seed": seed}
                    for z in ZS:
                        cover, tight, zero = gv.cover_and_tightness(e, v, counts, z)
                        # the yardstick is a photon count with Poisson scatter of its own: the share of counts that are
                        # >= expected - z sqrt(variance + count), the bound a noise-free truth would be held against
                        sel = counts >= 400
                        cn = counts[sel].astype(np.float64)
                        aware = float((cn >= e[sel] - z * np.sqrt(v[sel] + cn)).mean())
                        row["z%g" % z] = {"cover": round(cover, 4), "lo_over_count": round(tight, 4), "zero_bounds": round(zero, 4),
                                          "cover_with_count_noise": round(aware, 4)}
                    rows[name].append(row)
            summary = {}
            for name, rr in rows.items():
                summary[name] = {}
                for z in ZS:
                    k = "z%g" % z
                    summary[name][k] = {f: [min(r[k][f] for r in rr), max(r[k][f] for r in rr)]
                                        for f in ("cover", "lo_over_count", "zero_bounds", "cover_with_count_noise")}
            rows["min_max_over_seeds"] = summary
            rec["samples"][str(S)] = rows
        out["cases"][case] = rec
    print(json.dumps(out))


if __name__ == "__main__":
    main()
