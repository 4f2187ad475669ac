"""Developer tool (no GPU): what the adaptive gather buys (include/uvrt.h uvrt_gather_refine), from the CPU
restatements alone.  One JSON line:

  for a stop (route position 0) and a sweep (position 0 -> 1), both sampling modes, gather seeds 0..7 (the extra samples' seed
  is ~seed, as the host layer chooses it), S0 = 16, at most 64 extra samples and tau = 0.2 / 0.1 / 0.05: over the triangles that
  N = 2^21 oracle photons resolve (>= 400 of them), per seed
    base      the first pass alone: the median of max(0, expected - 2 sqrt(variance)) over the count, the cover (the share whose
              count is >= that bound), the share of bounds that are 0, the median of expected over the count;
    refined   the same after the refine, the extra rays, their mean per triangle, and the share of them that went to triangles
              no photon reaches;
    uniform   the same for a plain gather at S = 16 + that mean, rounded: the same rays spent evenly;
  and per (case, mode, tau) the minimum and maximum over the seeds.

The source of the table in DESIGN.md 16 and of the values recorded in tests/test_gather_refine_cpu.py; takes several minutes on
one core.

    python tests/tools/gather_refine_quality.py [--tau 0.2,0.1,0.05] [--seeds 8] [--photons 2097152] [--max-extra 64]
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
import gather_refine_restate as gf  # noqa: E402
import gather_restate as gr  # noqa: E402
import gather_stratified_restate as gs  # noqa: E402
import gather_variance_restate as gv  # noqa: E402

S0 = 16
FIELDS = ("lo_over_count", "cover", "zero_bounds", "expected_over_count")


def figures(e, v, counts):
    cover, tight, zero = gv.cover_and_tightness(e, v, counts, 2.0)
    sel = counts >= 400
    return {"lo_over_count": round(tight, 4), "cover": round(cover, 4), "zero_bounds": round(zero, 4),
            "expected_over_count": round(float(np.median(e[sel] / counts[sel])), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tau", default="0.2,0.1,0.05")
    ap.add_argument("--seeds", type=int, default=8)
    ap.add_argument("--photons", type=int, default=1 << 21)
    ap.add_argument("--max-extra", type=int, default=64)
    a = ap.parse_args()
    orc = g.load_oracle()
    gr.check_rng(orc)
    s = orc.Scene(os.path.join(ROOT, "tests/golden/testroomopt.glb"))
    route = orc.load_route(os.path.join(ROOT, "tests/golden/lange_route.xml"))
    comp = orc.Computation(s, route["lamps"], 1 << 16, route["lightHeight"], route["lightLength"], route["lightIntensity"])
    p0, p1 = comp.lamp_world_pos(route["lamps"][0]), comp.lamp_world_pos(route["lamps"][1])
    length, N, T = route["lightLength"], a.photons, int(s.T)
    taus = [float(v) for v in a.tau.split(",")]
    out = {"tool": "gather_refine_quality", "scene": "testroomopt.glb", "triangles": T, "photons": N, "min_photons": 400,
           "seeds": a.seeds, "z": 2.0, "first_samples": S0, "max_extra": a.max_extra, "cases": {}}
    for case, to in (("stop", p0), ("sweep", p1)):
        counts = gs.photon_counts(orc, s, p0, to, length, N)
        rec = {"resolved_triangles": int((counts >= 400).sum())}
        for name, mode in (("independent", gv.INDEPENDENT), ("stratified", gv.STRATIFIED)):
            rows = {"tau%g" % t: [] for t in taus}
            uniform = {}                         # S -> seed -> figures: several tau may land on one S
            for seed in range(a.seeds):
                e0, v0, _ = gv.gather(orc, s, p0, to, length, S0, seed, N, mode)
                base = figures(e0, v0, counts)
                for tau in taus:
                    e, v, n = gf.refine(orc, s, p0, to, length, S0, mode, N, e0, v0, tau, a.max_extra, ~seed & 0xFFFFFFFF)
                    extra = int(n.sum())
                    Su = S0 + int(round(extra / T))
                    if (Su, seed) not in uniform:
                        eu, vu, _ = gv.gather(orc, s, p0, to, length, Su, seed, N, mode)
                        uniform[(Su, seed)] = figures(eu, vu, counts)
                    refined = figures(e, v, counts)
                    refined.update(extra_rays=extra, mean_extra=round(extra / T, 2), refined_triangles=int((n > 0).sum()),
                                   zero_photon_share_of_extra=round(float(n[counts == 0].sum()) / max(extra, 1), 4))
                    rows["tau%g" % tau].append({"seed": seed, "base": base, "refined": refined,
                                                "uniform": dict(uniform[(Su, seed)], samples=Su)})
            summary = {}
            for k, rr in rows.items():
                summary[k] = {kind: {f: [min(r[kind][f] for r in rr), max(r[kind][f] for r in rr)] for f in FIELDS}
                              for kind in ("base", "refined", "uniform")}
                summary[k]["refined"]["extra_rays"] = [min(r["refined"]["extra_rays"] for r in rr), max(r["refined"]["extra_rays"] for r in rr)]
                summary[k]["refined"]["zero_photon_share_of_extra"] = [min(r["refined"]["zero_photon_share_of_extra"] for r in rr),
                                                                       max(r["refined"]["zero_photon_share_of_extra"] for r in rr)]
                summary[k]["uniform"]["samples"] = [min(r["uniform"]["samples"] for r in rr), max(r["uniform"]["samples"] for r in rr)]
                summary[k]["gain_lo_over_count"] = [round(min(r["refined"]["lo_over_count"] - r["base"]["lo_over_count"] for r in rr), 4),
                                                    round(max(r["refined"]["lo_over_count"] - r["base"]["lo_over_count"] for r in rr), 4)]
            rows["min_max_over_seeds"] = summary
            rec[name] = rows
        out["cases"][case] = rec
    print(json.dumps(out))


if __name__ == "__main__":
    main()
