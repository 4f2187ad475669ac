"""Developer tool (not the bench), on the GPU: what the one-bounce gather costs (include/uvrt.h uvrt_gather_indirect,
RayTracer::reflectance).  One JSON line.

    python tests/tools/gather_indirect_bench.py [--rounds R] [--samples S2]

Kernel against kernel: the S2 = 64 rays of the whole test room (uvrt_gather_indirect_rays, seed 1), traced by k_closest_free
(uvrt_closest_hits) and by k_extend_free with hit records (uvrt_write_free_rays + uvrt_extend with uvrt_set_record_hits) on the
same rays, interleaved round by round in one process; the figure is the kernel's own device time between the events of the
launch timing (uvrt_extend_time_ms: uploads and read-backs are outside it), the median of ROUNDS (default 7) launches after a
warm-up round.  `spread` is (max - min) / median of the rounds: the box's run-to-run spread for that kernel.

Whole calls, between two device events on the context's stream (tests/tools/gather_refine_bench.py's method), the same
interleaving: uvrt_gather_indirect alone at S2 samples (default 16), a gather launch uvrt_gather_direct at S = 16 without the
bounce, and with it (+ uvrt_indirect_source_from_expected + uvrt_gather_indirect, add = 1).  The shader clock is read under
load (uvrt_clock_probe_start beside a closest-hit launch)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
S_DIRECT = 16
S_KERNEL = 64
PE = 1 << 21


def summary(v):
    med = statistics.median(v)
    return {"ms_median": round(med, 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
            "spread": round((max(v) - min(v)) / med, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--samples", type=int, default=16)
    args = ap.parse_args()
    rounds = max(args.rounds, 5)
    import torch               # torch's HIP runtime first where torch is used in the same process (tests/conftest.py)
    torch.cuda.init()
    import numpy as np
    import __graft_entry__ as g
    pkg, orc = g.load_package(), g.load_oracle()
    s = orc.Scene(os.path.join(ROOT, "tests/golden/testroomopt.glb"))
    route = orc.load_route(os.path.join(ROOT, "tests/golden/lange_route.xml"))
    comp = orc.Computation(s, route["lamps"], 1 << 16, route["lightHeight"], route["lightLength"], route["lightIntensity"])
    p0 = comp.lamp_world_pos(route["lamps"][0])
    length = route["lightLength"]
    n = s.T * S_KERNEL
    c = pkg.capi.Ctx(0)
    c.set_scene(s.tris, s.nodes, s.triIdx)
    c.set_pipeline(False)
    c.set_record_hits(True)
    c.resize_rays(n)
    rays = c.gather_indirect_rays(0.1, S_KERNEL, 1)
    out = {"tool": "gather_indirect_bench", "scene": "testroomopt.glb", "triangles": s.T, "rounds": rounds,
           "device_cus": c.device_cus()}

    # ---- kernel against kernel ----
    def closest():
        return c.closest_hits(rays)

    def extend():
        c.write_free_rays(rays)
        c.extend(n)

    c.set_timing(True)
    ms = {"k_closest_free": [], "k_extend_free_record": []}
    for rnd in range(rounds + 1):               # round 0 warms up (code objects, records, buffers)
        for name, call in (("k_closest_free", closest), ("k_extend_free_record", extend)):
            c.sync()
            c.extend_time_ms()
            res = call()
            t, k = c.extend_time_ms()
            assert k == 1, (name, k)
            if rnd:
                ms[name].append(t)
            if name == "k_closest_free":
                hits = int((res[1] >= 0).sum())
        c.reset(True)                           # (the deposits of the extend are not wanted)
    c.clock_probe_start(2000)
    closest()
    out["shader_mhz_under_load"] = round(c.clock_probe_read(), 1)
    c.set_timing(False)
    kk = {name: summary(v) for name, v in ms.items()}
    kk["rays"], kk["hits"] = n, hits
    kk["closest_over_extend"] = round(kk["k_closest_free"]["ms_median"] / kk["k_extend_free_record"]["ms_median"], 4)
    kk["mray_per_s_closest"] = round(n / kk["k_closest_free"]["ms_median"] / 1e3, 1)
    out["kernel"] = kk

    # ---- whole calls ----
    c.set_record_hits(False)
    S2 = args.samples
    c.resize_rays(s.T * max(S_DIRECT, S2))      # every launch in one chunk
    st = torch.cuda.Stream()

    def direct():
        c.gather_direct(p0, p0, length, S_DIRECT, 0, PE)

    def bounce(add):
        c.gather_indirect(0.1, S2, 0 ^ 0x85EBCA6B, add=add)

    def launch_with_bounce():
        direct()
        c.indirect_source_from_expected()
        bounce(1)

    direct()
    c.indirect_source_from_expected()
    states = (("gather_indirect", lambda: bounce(0)), ("gather_launch", direct), ("gather_launch_with_bounce", launch_with_bounce))
    wm = {name: [] for name, _ in states}
    c.set_stream(st.cuda_stream)
    for rnd in range(rounds + 1):
        for name, call in states:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            call()
            e1.record(st)
            e1.synchronize()
            if rnd:
                wm[name].append(e0.elapsed_time(e1))
    c.sync()
    c.set_stream(None)
    calls = {name: summary(v) for name, v in wm.items()}
    calls["direct_samples"], calls["bounce_samples"] = S_DIRECT, S2
    calls["bounce_over_launch"] = round(calls["gather_launch_with_bounce"]["ms_median"] / calls["gather_launch"]["ms_median"], 3)
    expected = c.read_expected()
    calls["triangles_with_an_estimate"] = int((expected > 0).sum())
    out["calls"] = calls
    c.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
