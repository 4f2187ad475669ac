"""Developer tool (no GPU): what recorded hit links give and what further bounces add (include/uvrt.h "recorded hit links",
DESIGN.md 18), from the CPU restatements alone.  One JSON line.  The test room at position 0 of lange_route, the direct plane
at S = 16 (seed 0, N = 2^21) as the source:

  one_bounce   per S2 in 16, 64, 256: the linked one-bounce plane (links with the host layer's fixed seed) against the restated
               traced bounce at S2 = 1024 with another seed, per triangle |linked - reference| / reference over the triangles
               whose reference is positive: the median and the 95th percentile; and the same for the traced bounce at that S2
               with a per-launch seed, which is what a single launch had before
  energy       sum_t g_b / sum_t g_1 for b = 2..5 at rho = 0.1, 0.5, 0.8 over the links at the largest S2: what the bounces after
               the first add to the room's total

None of the figures is an acceptance threshold.  Takes minutes on one core: the reference traces 46 M rays through the oracle.

    python tests/tools/gather_links_quality.py [--samples 16,64,256] [--reference 1024] [--rho 0.1,0.5,0.8]
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
import gather_indirect_restate as gi  # noqa: E402
import gather_links_restate as gl  # noqa: E402
import gather_restate as gr  # noqa: E402

S_DIRECT = 16
N = 1 << 21
CHUNK = 4096            # triangles per oracle call: bounds the rays held at once


def rel_diff(plane, ref):
    sel = ref > 0
    d = np.abs(plane[sel] - ref[sel]) / ref[sel]
    return {"median": round(float(np.median(d)), 4), "p95": round(float(np.percentile(d, 95)), 4), "triangles": int(sel.sum())}


def chunked(fn, T):
    return np.concatenate([fn(first, min(CHUNK, T - first)) for first in range(0, T, CHUNK)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", default="16,64,256")
    ap.add_argument("--reference", type=int, default=1024)
    ap.add_argument("--rho", default="0.1,0.5,0.8")
    a = ap.parse_args()
    orc = g.load_oracle()
    gr.check_rng(orc)
    s = orc.Scene(os.path.join(ROOT, "tests/golden/testroomopt.glb"))
    route = orc.load_route(os.path.join(ROOT, "tests/golden/lange_route.xml"))
    comp = orc.Computation(s, route["lamps"], 1 << 16, route["lightHeight"], route["lightLength"], route["lightIntensity"])
    p0 = comp.lamp_world_pos(route["lamps"][0])
    T = int(s.T)
    direct, _, _ = gr.gather(orc, s, p0, p0, route["lightLength"], S_DIRECT, 0, N)
    samples = [int(v) for v in a.samples.split(",")]
    ref_seed = 0x1234567
    ref = chunked(lambda f, n: gi.indirect(orc, s, direct, 0.1, a.reference, ref_seed, first=f, count=n)[0], T)
    out = {"tool": "gather_links_quality", "scene": "testroomopt.glb", "triangles": T, "direct_samples": S_DIRECT,
           "photons_equiv": N, "reference_samples": a.reference, "reference_seed": ref_seed, "link_seed": gl.LINK_SEED,
           "triangles_without_direct": int((direct == 0).sum()), "one_bounce": {}, "energy": {}}
    lk = None
    for S2 in samples:
        lk = chunked(lambda f, n: gl.links(orc, s, S2, gl.LINK_SEED, first=f, count=n), T)
        one = gl.linked(s.tris, direct, lk, 0.1, 1)
        traced = chunked(lambda f, n: gi.indirect(orc, s, direct, 0.1, S2, 0 ^ gl.LINK_SEED ^ 1, first=f, count=n)[0], T)
        out["one_bounce"]["S2_%d" % S2] = {"linked": rel_diff(one, ref), "traced_per_launch_seed": rel_diff(traced, ref),
                                           "links_that_point": round(float((lk >= 0).mean()), 4),
                                           "sum_over_reference": round(float(one.sum() / ref.sum()), 4)}
    out["energy"]["links_samples"] = samples[-1]
    out["energy"]["g1_over_direct_at_rho_1"] = round(float(gl.bounces(s.tris, direct, lk, 1.0, 1)[0].sum() / direct.sum()), 4)
    for rho in (float(v) for v in a.rho.split(",")):
        gb = gl.bounces(s.tris, direct, lk, rho, 5)
        out["energy"]["rho_%g" % rho] = {"g%d_over_g1" % (b + 1): round(float(gb[b].sum() / gb[0].sum()), 5) for b in range(1, 5)}
        out["energy"]["rho_%g" % rho]["bounces_2_to_5_over_direct_plus_g1"] = round(
            float(sum(x.sum() for x in gb[1:]) / (direct.sum() + gb[0].sum())), 5)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
