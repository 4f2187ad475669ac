"""Developer tool (not the bench): what the gather sampling mode (include/uvrt.h uvrt_set_gather_sampling) does to the GPU time of
uvrt_gather_direct over the whole test room.  A stratified triangle's rays leave the rod in height order, which may help or hurt
the coherence of k_occlude_free; the shadow rays are the same number.  One JSON line, per case (a stop at route position 0, the
sweep 0 -> 1) and mode:

  occlude        the shadow-ray launch alone, from uvrt_extend_time_ms (device events around k_occlude_free)
  gather_direct  the whole call (generate, trace, reduce) between two device events on the context's stream

each the median of ROUNDS (default 7, at least 5) timed launches after a warm-up round, both modes interleaved round by round in
one process so that clock drift favours neither -- tests/tools/gather_bench.py's method.  The same gather seed in every round: the
rays of a round are the rays of the last.  No threshold: the mode is kept for its estimator.

    python tests/tools/gather_sampling_bench.py [--samples S] [--rounds R] [--flavour 0|1]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as g  # noqa: E402

MODES = (("independent", 0), ("stratified", 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--flavour", type=int, default=0)
    a = ap.parse_args()
    S, rounds = a.samples, max(a.rounds, 5)
    import torch               # torch's HIP runtime first where torch is used in the same process (tests/conftest.py)
    torch.cuda.init()
    pkg, orc = g.load_package(), g.load_oracle()
    s = orc.Scene(os.path.join(ROOT, "tests/golden/testroomopt.glb"))
    route = orc.load_route(os.path.join(ROOT, "tests/golden/lange_route.xml"))
    comp = orc.Computation(s, route["lamps"], 1 << 16, route["lightHeight"], route["lightLength"], route["lightIntensity"])
    p0, p1 = comp.lamp_world_pos(route["lamps"][0]), comp.lamp_world_pos(route["lamps"][1])
    length, n = route["lightLength"], s.T * S

    c = pkg.capi.Ctx(0)
    c.set_scene(s.tris, s.nodes, s.triIdx)
    c.resize_rays(n)           # one chunk: one shadow-ray launch per call
    c.set_flavour(a.flavour)
    c.set_pipeline(False)
    st = torch.cuda.Stream()
    out = {"tool": "gather_sampling_bench", "scene": "testroomopt.glb", "triangles": int(s.T), "samples": S, "rays": int(n),
           "rounds": rounds, "flavour": a.flavour, "device_cus": c.device_cus(), "cases": {}}
    for case, to in (("stop", p0), ("sweep", p1)):
        ms = {name: {"occlude": [], "gather_direct": []} for name, _ in MODES}
        lit = {}
        c.set_timing(True)
        for rnd in range(rounds + 1):              # round 0 warms up (code objects, records, buffers)
            for name, mode in MODES:
                c.set_gather_sampling(mode)
                c.sync()
                c.extend_time_ms()
                c.gather_direct(p0, to, length, S, 0, 1 << 21)
                c.sync()
                t, k = c.extend_time_ms()
                assert k == 1
                if rnd == 0:
                    lit[name] = int((c.read_expected() > 0).sum())
                else:
                    ms[name]["occlude"].append(t)
        c.set_timing(False)
        c.set_stream(st.cuda_stream)
        for rnd in range(rounds + 1):
            for name, mode in MODES:
                c.set_gather_sampling(mode)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                c.gather_direct(p0, to, length, S, 0, 1 << 21)
                e1.record(st)
                e1.synchronize()
                if rnd:
                    ms[name]["gather_direct"].append(e0.elapsed_time(e1))
        c.sync()
        c.set_stream(None)
        rec = {}
        for name, _ in MODES:
            rec[name] = {"triangles_with_estimate": lit[name]}
            for what, v in ms[name].items():
                med = statistics.median(v)
                rec[name][what] = {"ms_median": round(med, 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
                                   "mray_s": round(n / med / 1e3, 1)}
        for what in ("occlude", "gather_direct"):
            rec["stratified_over_independent_" + what] = round(rec["stratified"][what]["ms_median"] / rec["independent"][what]["ms_median"], 3)
        out["cases"][case] = rec
    c.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
