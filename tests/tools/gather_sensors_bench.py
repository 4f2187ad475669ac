"""Developer tool (not the bench), on the GPU: what the virtual dosimeters cost (include/uvrt.h "sensors", RayTracer::sensorMap,
DESIGN.md 26).  One JSON line.

    python tests/tools/gather_sensors_bench.py [--rounds R] [--samples 16]

The protocol of tests/tools/gather_mirror_bench.py: whole calls between two device events on the context's stream, the states
interleaved round by round in one process, the median of ROUNDS (default 7) after a warm-up round; `spread` is (max - min) /
median of the rounds.  No time is fixed in advance: the yardstick is uvrt_gather_direct on the room at the same S in the same
process.  On the test room at position 0 of lange_route, everything in one chunk.

  uvrt_gather_sensors for a 64 x 32 x 64 lattice of spherical sensors over the room's bounds at S samples (2.1 M shadow rays at
  S = 16), as time per ray against uvrt_gather_direct's time per ray; the call's traversal launch from the context's own launch
  timing -- the generate and reduce kernels are what is left
  uvrt_gather_sensors_indirect (emitter 0) at S2 = S against uvrt_gather_indirect, per ray, with its traversal launch likewise
  a gather launch (uvrt_gather_direct, then uvrt_accumulate_expected) without and with 64 sensors (uvrt_gather_sensors at S = 64
  and uvrt_accumulate_sensors between the two)"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PE = 1 << 21
GRID = (64, 32, 64)


def summary(v):
    med = statistics.median(v)
    return {"ms_median": round(med, 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
            "spread": round((max(v) - min(v)) / med, 4)}


def lattice(lo, hi, cells):
    """the cell centres of a lattice over the box, x fastest, as spherical uvrt_sensor records"""
    import gather_sensors_restate as gsr
    ax = [np.float32(lo[a]) + np.float32(hi[a] - lo[a]) * ((np.arange(cells[a], dtype=np.float32) + np.float32(0.5)) / np.float32(cells[a]))
          for a in range(3)]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    out = np.zeros(x.size, dtype=gsr.SENSOR_DT)
    out["pos"] = np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1)
    out["kind"] = gsr.SPHERICAL
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--samples", type=int, default=16)
    args = ap.parse_args()
    rounds = max(args.rounds, 5)
    S = args.samples
    import torch               # torch's HIP runtime first where torch is used in the same process (tests/conftest.py)
    torch.cuda.init()
    import __graft_entry__ as g
    pkg, orc = g.load_package(), g.load_oracle()
    s = orc.Scene(os.path.join(ROOT, "tests/golden/testroomopt.glb"))
    route = orc.load_route(os.path.join(ROOT, "tests/golden/lange_route.xml"))
    comp = orc.Computation(s, route["lamps"], 1 << 16, route["lightHeight"], route["lightLength"], route["lightIntensity"])
    p0 = comp.lamp_world_pos(route["lamps"][0])
    length = route["lightLength"]
    v = np.concatenate([s.tris[:, 0:3], s.tris[:, 4:7], s.tris[:, 8:11]])
    big = lattice(v.min(axis=0), v.max(axis=0), GRID)
    small = big[:: big.size // 64][:64].copy()
    K = big.size
    st = torch.cuda.Stream()
    c = pkg.capi.Ctx(0)
    c.set_scene(s.tris, s.nodes, s.triIdx)
    c.set_pipeline(False)
    c.resize_rays(max(s.T, K) * S)                          # every call in one chunk
    out = {"tool": "gather_sensors_bench", "scene": "testroomopt.glb", "triangles": s.T, "sensors": K, "rounds": rounds,
           "device_cus": c.device_cus(), "samples": S, "direct_rays": s.T * S, "sensor_rays": K * S}
    c.set_sensors(big)
    c.gather_direct(p0, p0, length, S, 0, PE)
    c.indirect_source_from_expected()
    c.gather_sensors(p0, p0, length, S, 0, PE)
    c.set_stream(st.cuda_stream)

    def launch(sensors):
        c.gather_direct(p0, p0, length, S, 0, PE)
        if sensors:
            c.gather_sensors(p0, p0, length, 64, 0, PE)
            c.accumulate_sensors(1.0)
        c.accumulate_expected(1.0)

    big_states = [("gather_direct", lambda: c.gather_direct(p0, p0, length, S, 0, PE)),
                  ("gather_sensors", lambda: c.gather_sensors(p0, p0, length, S, 0, PE)),
                  ("gather_indirect", lambda: c.gather_indirect(0.5, S, 1)),
                  ("gather_sensors_indirect", lambda: c.gather_sensors_indirect(0.5, S, 1, 0))]
    small_states = [("gather_launch", lambda: launch(False)), ("gather_launch_with_64_sensors", lambda: launch(True))]
    wm = {name: [] for name, _ in big_states + small_states}
    traversal = {"gather_sensors": [], "gather_sensors_indirect": [], "gather_direct": [], "gather_indirect": []}

    def timed(states, rnd):
        for name, call in states:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            call()
            e1.record(st)
            e1.synchronize()
            if rnd:
                wm[name].append(e0.elapsed_time(e1))

    for rnd in range(rounds + 1):               # round 0 warms up (code objects, buffers)
        timed(big_states, rnd)
        # the traversal launch of each call, from the context's launch timing (events around the launch)
        for name, call in big_states:
            c.set_timing(True)
            c.extend_time_ms()
            call()
            ms, launches = c.extend_time_ms()
            c.set_timing(False)
            if rnd:
                assert launches == 1, (name, launches)
                traversal[name].append(ms)
    c.sync()
    c.set_sensors(small)
    for rnd in range(rounds + 1):
        timed(small_states, rnd)
    rec = {name: summary(v) for name, v in wm.items()}
    for name, v in traversal.items():
        rec[name]["traversal_ms_median"] = round(statistics.median(v), 4)
        rec[name]["other_kernels_ms"] = round(rec[name]["ms_median"] - statistics.median(v), 4)
    rays = {"gather_direct": s.T * S, "gather_sensors": K * S, "gather_indirect": s.T * S, "gather_sensors_indirect": K * S}
    for name, n in rays.items():
        rec[name]["ns_per_ray"] = round(rec[name]["ms_median"] * 1e6 / n, 4)
        rec[name]["traversal_ns_per_ray"] = round(rec[name]["traversal_ms_median"] * 1e6 / n, 4)
    rec["sensors_over_direct_per_ray"] = round(rec["gather_sensors"]["ns_per_ray"] / rec["gather_direct"]["ns_per_ray"], 4)
    rec["sensors_indirect_over_indirect_per_ray"] = round(rec["gather_sensors_indirect"]["ns_per_ray"] / rec["gather_indirect"]["ns_per_ray"], 4)
    rec["launch_with_64_sensors_over_launch"] = round(rec["gather_launch_with_64_sensors"]["ms_median"] / rec["gather_launch"]["ms_median"], 4)
    out["states"] = rec
    c.sync()
    c.set_stream(None)
    c.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
