"""Developer tool (no GPU): what a reflectance map does to the face-resolved bounces (include/uvrt.h "per-face reflectance",
DESIGN.md 22), from the CPU restatements alone.  One JSON line.  The test room at position 0 of lange_route, the direct plane at
S = 16 (seed 0, N = 2^21), the sided links with the host layer's fixed seed.  Per S2 in 64, 256 and per map

  rho == 0.05, rho == 0.85, and 0.85 where the centroid has x >= 1.2 with 0.05 elsewhere

sum_t g_b / sum_t direct for b = 1..4 and max e_b / max e_{b-1}, which never exceeds the map's largest entry.

None of the figures is an acceptance threshold.  Takes a few minutes on one core.

    python tests/tools/gather_reflect_map_quality.py [--samples 64,256] [--bounces 4]
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
import gather_faces_restate as gf  # noqa: E402
import gather_links_restate as gl  # noqa: E402
import gather_reflect_map_restate as gm  # noqa: E402
import gather_restate as gr  # noqa: E402

S_DIRECT = 16
N = 1 << 21
CHUNK = 4096            # triangles per oracle call: bounds the rays held at once
LINED = "box 1.2 -1e30 -1e30 1e30 1e30 1e30 0.85\n"


def chunked(fn, T):
    return np.concatenate([fn(first, min(CHUNK, T - first)) for first in range(0, T, CHUNK)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", default="64,256")
    ap.add_argument("--bounces", type=int, default=4)
    a = ap.parse_args()
    orc = g.load_oracle()
    gr.check_rng(orc)
    s = orc.Scene(os.path.join(ROOT, "tests/golden/testroomopt.glb"))
    route = orc.load_route(os.path.join(ROOT, "tests/golden/lange_route.xml"))
    comp = orc.Computation(s, route["lamps"], 1 << 16, route["lightHeight"], route["lightLength"], route["lightIntensity"])
    p0 = comp.lamp_world_pos(route["lamps"][0])
    T, K = int(s.T), a.bounces
    faces, direct = gf.gather_faces(orc, s, p0, p0, route["lightLength"], S_DIRECT, 0, N)
    total = float(direct.sum())
    lined = gm.rules_map(s.tris, LINED, 0.05)
    maps = (("rho_0.05", gm.as_planes(0.05, T)), ("rho_0.85", gm.as_planes(0.85, T)), ("lined_x_ge_1.2", lined))
    out = {"tool": "gather_reflect_map_quality", "scene": "testroomopt.glb", "triangles": T, "direct_samples": S_DIRECT,
           "photons_equiv": N, "link_seed": gl.LINK_SEED, "bounces": K, "lined_triangles": int((lined[0] == np.float32(0.85)).sum()),
           "direct_sum": round(total, 1), "by_samples": {}}
    for S2 in (int(v) for v in a.samples.split(",")):
        sided = chunked(lambda f, n: gf.sided_links(orc, s, S2, gl.LINK_SEED, first=f, count=n), T)
        rec = {}
        for name, rho in maps:
            gs, es = gm.bounces(s.tris, faces, sided, rho, K)
            rec[name] = {"bounce_over_direct": [round(float(x.sum()) / total, 4) for x in gs],
                         "max_e_ratio": [round(float(es[b].max() / es[b - 1].max()), 4) for b in range(1, K + 1)]}
        out["by_samples"]["S2_%d" % S2] = rec
    print(json.dumps(out))


if __name__ == "__main__":
    main()
