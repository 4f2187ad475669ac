"""Developer tool (no GPU): what resolving the faces does to the linked bounces (include/uvrt.h "face-resolved gather and
bounces"), from the CPU restatements alone.  One JSON line.  The test room at position 0 of lange_route, the direct
plane at S = 16 (seed 0, N = 2^21), the links with the host layer's fixed seed:

  faces        how the direct plane splits between the two faces, and how many triangles are lit on both
  bounces      per S2 in 64, 256 and rho in 0.1, 0.5, 0.8, 1.0: sum_t g_b / sum_t direct for b = 1..6 in the two-sided model
               (uvrt_gather_indirect_linked) and in the face-resolved one (uvrt_gather_indirect_linked_sided), and for the latter
               max e_b / max e_{b-1}, which never exceeds rho

None of the figures is an acceptance threshold.  Takes a few minutes on one core.

    python tests/tools/gather_faces_quality.py [--samples 64,256] [--rho 0.1,0.5,0.8,1.0] [--bounces 6]
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
import gather_restate as gr  # noqa: E402

S_DIRECT = 16
N = 1 << 21
CHUNK = 4096            # triangles per oracle call: bounds the rays held at once


def chunked(fn, T):
    return np.concatenate([fn(first, min(CHUNK, T - first)) for first in range(0, T, CHUNK)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", default="64,256")
    ap.add_argument("--rho", default="0.1,0.5,0.8,1.0")
    ap.add_argument("--bounces", type=int, default=6)
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
    out = {"tool": "gather_faces_quality", "scene": "testroomopt.glb", "triangles": T, "direct_samples": S_DIRECT,
           "photons_equiv": N, "link_seed": gl.LINK_SEED, "bounces": K,
           "faces": {"direct_sum": round(total, 1), "face0_sum": round(float(faces[0].sum()), 1),
                     "face1_sum": round(float(faces[1].sum()), 1), "lit_on_face0": int((faces[0] > 0).sum()),
                     "lit_on_face1": int((faces[1] > 0).sum()), "lit_on_both": int(((faces[0] > 0) & (faces[1] > 0)).sum())},
           "by_samples": {}}
    for S2 in (int(v) for v in a.samples.split(",")):
        sided = chunked(lambda f, n: gf.sided_links(orc, s, S2, gl.LINK_SEED, first=f, count=n), T)
        plain = np.where(sided >= 0, sided >> 1, -1)          # (tests/test_gpu_gather_faces.py: the plain build's links)
        rec = {"links_that_point": round(float((sided >= 0).mean()), 4),
               "links_that_arrive_on_face1": round(float(((sided >= 0) & (sided & 1 == 1)).sum() / max((sided >= 0).sum(), 1)), 4)}
        for rho in (float(v) for v in a.rho.split(",")):
            two = gl.bounces(s.tris, direct, plain, rho, K)
            gs, es = gf.bounces(s.tris, faces, sided, rho, K)
            rec["rho_%g" % rho] = {
                "two_sided": [round(float(x.sum()) / total, 4) for x in two],
                "face_resolved": [round(float(x.sum()) / total, 4) for x in gs],
                "face_resolved_max_e_ratio": [round(float(es[b].max() / es[b - 1].max()), 4) for b in range(1, K + 1)]}
        out["by_samples"]["S2_%d" % S2] = rec
    print(json.dumps(out))


if __name__ == "__main__":
    main()
