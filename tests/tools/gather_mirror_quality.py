"""Developer tool (no GPU): what a specular panel does to the dose (include/uvrt.h "specular panels"), from the CPU
restatements alone.  One JSON line.  The test room at position 0 of lange_route, the direct plane at S samples (seed 0, N =
2^21), one panel on the wall whose centroids have x >= 1.2 (the lining of DESIGN.md 22): the plane x = 1.47 looking at the room,
rho = 0.85.

  sum_t mirror / sum_t direct
  the triangles the panel lights that the direct gather leaves at 0
  of the samples in front of the panel with w' > 0: the share whose leg A misses the panel (it ends beside it, or nowhere), the
  share occluded on leg A (a triangle that is no member stands before the plane), the share occluded on leg B
  the same wall as a diffuse reflector of rho = 0.85 (0 elsewhere) through the reflectance map, one and four bounces, S2 = 64

None of the figures is an acceptance threshold.

    python tests/tools/gather_mirror_quality.py [--samples 16]
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
import gather_mirror_restate as gm  # noqa: E402
import gather_reflect_map_restate as grm  # noqa: E402
import gather_restate as gr  # noqa: E402

N = 1 << 21
S2 = 64
CHUNK = 4096            # triangles per oracle call of the link build: bounds the rays held at once
PANEL = "mirror 1.2 -1e30 -1e30 1e30 1e30 1e30 0.85 plane 1.47 0 0 -1 0 0\n"
LINED = "box 1.2 -1e30 -1e30 1e30 1e30 1e30 0.85\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=16)
    a = ap.parse_args()
    S = a.samples
    orc = g.load_oracle()
    gr.check_rng(orc)
    s = orc.Scene(os.path.join(ROOT, "tests/golden/testroomopt.glb"))
    route = orc.load_route(os.path.join(ROOT, "tests/golden/lange_route.xml"))
    comp = orc.Computation(s, route["lamps"], 1 << 16, route["lightHeight"], route["lightLength"], route["lightIntensity"])
    p0 = comp.lamp_world_pos(route["lamps"][0])
    T = int(s.T)
    faces, direct = gf.gather_faces(orc, s, p0, p0, route["lightLength"], S, 0, N)
    panels, members = gm.rules_panels(s.tris, PANEL)
    mirror, _, info = gm.gather(orc, s, panels, members, p0, p0, route["lightLength"], S, 0, N)
    i = info[0]
    lit = i["w"] > 0
    hit = i["h"] >= 0
    short = hit & (i["dist"] < i["ra"] * np.float32(1.0 - 2.0 ** -10))      # leg A ends before the plane
    occluded_a = lit & i["off"] & short
    beside = lit & i["lost"] & ~occluded_a
    total = float(direct.sum())
    sided = np.concatenate([gf.sided_links(orc, s, S2, gl.LINK_SEED, first=f, count=min(CHUNK, T - f)) for f in range(0, T, CHUNK)])
    g_diffuse, _ = grm.bounces(s.tris, faces, sided, grm.rules_map(s.tris, LINED, 0.0), 4)
    one = g_diffuse[0][0] + g_diffuse[0][1]
    four = one + sum(x[0] + x[1] for x in g_diffuse[1:])
    out = {"tool": "gather_mirror_quality", "scene": "testroomopt.glb", "triangles": T, "samples": S, "photons_equiv": N,
           "panel_triangles": int((members == 1).sum()), "direct_sum": round(total, 1),
           "mirror_over_direct": round(float(mirror.sum()) / total, 4),
           "lit_by_the_panel": int((mirror > 0).sum()), "lit_by_the_panel_dark_in_direct": int(((mirror > 0) & (direct == 0)).sum()),
           "dark_in_direct": int((direct == 0).sum()),
           "samples_in_front_with_weight": int(lit.sum()),
           "share_leg_a_beside_the_panel": round(float(beside.sum()) / float(lit.sum()), 4),
           "share_occluded_on_leg_a": round(float(occluded_a.sum()) / float(lit.sum()), 4),
           "share_occluded_on_leg_b": round(float((i["occluded"] & lit).sum()) / float(lit.sum()), 4),
           "share_kept": round(float((i["x"] > 0).sum()) / float(lit.sum()), 4),
           "diffuse_0.85_same_wall": {"link_samples": S2, "one_bounce_over_direct": round(float(one.sum()) / total, 4),
                                      "four_bounces_over_direct": round(float(four.sum()) / total, 4),
                                      "lit_by_one_bounce_dark_in_direct": int(((one > 0) & (direct == 0)).sum()),
                                      "floor_under_the_panel_diffuse_over_mirror": None}}
    # the floor right under the panel: the lowest tenth of the room within half a metre of the wall
    y = s.tris[:, 13]
    floor = (y <= np.percentile(y, 10)) & (s.tris[:, 12] >= np.float32(0.7)) & (members == 0)
    if floor.any() and mirror[floor].sum() > 0:
        out["diffuse_0.85_same_wall"]["floor_under_the_panel_diffuse_over_mirror"] = round(float(one[floor].sum() / mirror[floor].sum()), 3)
        out["diffuse_0.85_same_wall"]["floor_triangles"] = int(floor.sum())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
