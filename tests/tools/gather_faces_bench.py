"""Developer tool (not the bench), on the GPU: what resolving the faces costs (include/uvrt.h "face-resolved gather and bounces",
RayTracer::reflectSided).  One JSON line.

    python tests/tools/gather_faces_bench.py [--rounds R] [--samples 16,64,256]

The protocol of tests/tools/gather_links_bench.py: whole calls between two device events on the context's stream, the states
interleaved round by round in one process, the median of ROUNDS (default 7) after a warm-up round; `spread` is (max - min) /
median of the rounds.  No time is fixed in advance: the yardstick of every sided state is its plain twin in the same process.  On
the test room, with the direct plane at S = 16 and its face planes as the emitters, two contexts side by side (a context holds one
link set): `plain` with plain links, `sided` with sided ones of the same S2 and seed.

  uvrt_gather_indirect_linked against uvrt_gather_indirect_linked_sided at S2 = 16, 64, 256 with K = 1 and 4
  uvrt_indirect_links_build against uvrt_indirect_links_build_sided at each S2
  a gather launch (uvrt_gather_direct at S = 16) with the faces state off and on"""
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
    st = torch.cuda.Stream()
    ctx = {}
    for name in ("plain", "sided"):
        c = pkg.capi.Ctx(0)
        c.set_scene(s.tris, s.nodes, s.triIdx)
        c.set_pipeline(False)
        c.resize_rays(s.T * max([S_DIRECT] + samples))      # every launch and every build in one chunk
        ctx[name] = c
    p, q = ctx["plain"], ctx["sided"]
    out = {"tool": "gather_faces_bench", "scene": "testroomopt.glb", "triangles": s.T, "rounds": rounds,
           "device_cus": p.device_cus(), "direct_samples": S_DIRECT, "by_samples": {}}
    p.gather_direct(p0, p0, length, S_DIRECT, 0, PE)
    p.indirect_source_from_expected()
    q.set_gather_faces(1)
    q.gather_direct(p0, p0, length, S_DIRECT, 0, PE)
    q.set_gather_faces(0)
    for c in (p, q):
        c.set_stream(st.cuda_stream)

    def launch(on):
        q.set_gather_faces(on)
        q.gather_direct(p0, p0, length, S_DIRECT, 0, PE)

    for S2 in samples:
        states = [("links_build", lambda: p.indirect_links_build(S2, LINK_SEED)),
                  ("links_build_sided", lambda: q.indirect_links_build_sided(S2, LINK_SEED)),
                  ("linked_K1", lambda: p.gather_indirect_linked(0.5, 1)),
                  ("linked_sided_K1", lambda: q.gather_indirect_linked_sided(0.5, 1)),
                  ("linked_K4", lambda: p.gather_indirect_linked(0.5, 4)),
                  ("linked_sided_K4", lambda: q.gather_indirect_linked_sided(0.5, 4))]
        if S2 == samples[0]:
            states += [("gather_launch_faces_off", lambda: launch(0)), ("gather_launch_faces_on", lambda: launch(1))]
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
        for a, b in (("linked_sided_K1", "linked_K1"), ("linked_sided_K4", "linked_K4"), ("links_build_sided", "links_build"),
                     ("gather_launch_faces_on", "gather_launch_faces_off")):
            if a in rec:
                rec[a + "_over_" + b] = round(rec[a]["ms_median"] / rec[b]["ms_median"], 4)
        out["by_samples"]["S2_%d" % S2] = rec
    for c in (p, q):
        c.sync()
        c.set_stream(None)
    q.clock_probe_start(2000)
    q.indirect_links_build_sided(samples[-1], LINK_SEED)
    out["shader_mhz_under_load"] = round(q.clock_probe_read(), 1)
    for c in (p, q):
        c.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
