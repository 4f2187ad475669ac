"""Developer tool (not the bench), on the GPU: what recorded hit links cost and save (include/uvrt.h "recorded hit links",
RayTracer::reflectBounces).  One JSON line.

    python tests/tools/gather_links_bench.py [--rounds R] [--samples 16,64,256]

The protocol of tests/tools/gather_indirect_bench.py: whole calls between two device events on the context's stream, the states
interleaved round by round in one process, the median of ROUNDS (default 7) after a warm-up round; `spread` is (max - min) /
median of the rounds.  On the test room, with the direct plane at S = 16 as the source:

  uvrt_gather_indirect at S2 = 16                                    the traced bounce, the yardstick
  uvrt_gather_indirect_linked at S2 = 16, 64, 256 with K = 1 and 4   the lookup-and-sum over the links
  uvrt_indirect_links_build at each S2                               the one trace per scene
  a gather launch at S = 16 with the traced bounce and with the linked one (K = 1, S2 = 16)

Every state of one S2 is timed against links of that S2, so the states go S2 by S2 with the traced call and the two launches
repeated beside each: the box's drift shows in their rows.  The shader clock is read under load (uvrt_clock_probe_start beside
a build)."""
import argparse
import json
import os
import statistics
import sys

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
    c = pkg.capi.Ctx(0)
    c.set_scene(s.tris, s.nodes, s.triIdx)
    c.set_pipeline(False)
    c.resize_rays(s.T * max([S_DIRECT] + samples))      # every launch and every build in one chunk
    out = {"tool": "gather_links_bench", "scene": "testroomopt.glb", "triangles": s.T, "rounds": rounds,
           "device_cus": c.device_cus(), "direct_samples": S_DIRECT, "by_samples": {}}
    st = torch.cuda.Stream()

    def direct():
        c.gather_direct(p0, p0, length, S_DIRECT, 0, PE)

    def launch_traced():
        direct()
        c.indirect_source_from_expected()
        c.gather_indirect(0.1, 16, 0 ^ LINK_SEED, add=1)

    def launch_linked():
        direct()
        c.indirect_source_from_expected()
        c.gather_indirect_linked(0.1, 1, add=1)

    direct()
    c.indirect_source_from_expected()
    c.set_stream(st.cuda_stream)
    for S2 in samples:
        states = [("gather_indirect_S2_16", lambda: c.gather_indirect(0.1, 16, LINK_SEED, add=0)),
                  ("links_build", lambda: c.indirect_links_build(S2, LINK_SEED)),
                  ("linked_K1", lambda: c.gather_indirect_linked(0.1, 1)),
                  ("linked_K4", lambda: c.gather_indirect_linked(0.1, 4))]
        if S2 == 16:
            states += [("gather_launch_traced_bounce", launch_traced), ("gather_launch_linked_bounce", launch_linked)]
        wm = {name: [] for name, _ in states}
        for rnd in range(rounds + 1):               # round 0 warms up (code objects, buffers, the links themselves)
            for name, call in states:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                call()
                e1.record(st)
                e1.synchronize()
                if rnd:
                    wm[name].append(e0.elapsed_time(e1))
        rec = {name: summary(v) for name, v in wm.items()}
        rec["link_bytes"] = s.T * S2 * 4
        rec["linked_K1_over_traced_S2_16"] = round(rec["linked_K1"]["ms_median"] / rec["gather_indirect_S2_16"]["ms_median"], 4)
        rec["build_over_traced_S2_16"] = round(rec["links_build"]["ms_median"] / rec["gather_indirect_S2_16"]["ms_median"], 3)
        out["by_samples"]["S2_%d" % S2] = rec
    c.sync()
    c.set_stream(None)
    c.clock_probe_start(2000)
    c.indirect_links_build(samples[-1], LINK_SEED)
    out["shader_mhz_under_load"] = round(c.clock_probe_read(), 1)
    c.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
