"""Developer probe (not the bench): interleaved A/B of the helper-kernel issue priority (uvrt_set_helper_priority) on the
bench's own step, all in ONE process -- rounds x levels, each cell = STEPS back-to-back computations bracketed by device
syncs, as tests/tools/ab_bench.py does for kernel variants.

    LEVELS=0,1,3 MODE=batched STEPS=30 ROUNDS=5 python tests/tools/ab_helper_prio.py

Prints per level the median, best and lowest Mray/s over the rounds and the dose CRC (must be the same at every level)."""
import os
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402

import torch  # noqa: E402  (HIP runtime order: torch first, see tests/conftest.py)

torch.cuda.init()
g.load_package()
from uvrt_amd import host  # noqa: E402

levels = [int(v) for v in os.environ.get("LEVELS", "0,1,3").split(",")]
mode = os.environ.get("MODE", "batched")
steps = int(os.environ.get("STEPS", "30"))
rounds = int(os.environ.get("ROUNDS", "5"))
photons = int(os.environ.get("PHOTONS", str(1920 * 1080)))
waves = int(os.environ.get("WAVES", "8"))

rt = host.RayTracer(os.path.join(ROOT, "tests", "golden", "testroomopt.glb"),
                    os.path.join(ROOT, "tests", "golden", "lange_route.xml"), device=0)
rt.set_lamps(rt.lamps()[:1])
rt.photonCount = photons
rt.maxIterations = waves
rays_per_step = waves * rt.photonsPerLight


def step():
    rt.ctx.seed = 0
    rt.ResetDosageMap()
    if mode == "batched":
        rt.ComputeIterationsBatched(waves)
    else:
        for _ in range(waves):
            rt.ComputeDosageMap()
            rt.Shade()
            rt.currIterations = rt.currIterations + 1
            if mode == "loop_sync":
                rt.Sync()


res = {lv: [] for lv in levels}
crcs = {}
for rnd in range(rounds + 1):                 # round 0 = warm-up (allocations, hot records, clocks)
    for lv in levels:
        rt.ctx.set_helper_priority(lv)
        step()
        rt.Sync()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        rt.Sync()
        el = time.perf_counter() - t0
        if rnd > 0:
            res[lv].append(rays_per_step * steps / el / 1e6)
        crcs[lv] = "%08x" % zlib.crc32(rt.read_dosage().tobytes())
base = np.median(res[levels[0]])
for lv in levels:
    a = np.array(res[lv])
    print("helper priority %d  %s  median %8.1f  best %8.1f  min %8.1f Mray/s  (%+.2f %% vs the first)  crc %s  rounds %s"
          % (lv, mode, np.median(a), a.max(), a.min(), 100.0 * (np.median(a) / base - 1.0), crcs[lv],
             " ".join("%.1f" % v for v in a)), flush=True)
if len(set(crcs.values())) != 1:
    print("DOSE MISMATCH between levels", crcs)
    sys.exit(1)
