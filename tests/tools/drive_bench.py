"""Developer tool (not the bench): what a whole driving route costs through RayTracer::ComputeIterationsBatched -- the
stops and the segments between them (RayTracer::driveSpeed).  One JSON line.

Workload: the test room, lange_route (12 positions), the reference's default photon count (2^25 over the positions) and
10 iterations at driveSpeed 0.1: 10 x (12 stops + 11 segments) launches.  A computation is ResetDosageMap +
ComputeIterationsBatched + Sync from SEED 0; the figure is the median wall time of ROUNDS (default 7, at least 5) timed
computations after a warm-up one, and rays per second over the stops plus the segments.  The dose CRC is printed so that
two builds can be told to have computed the same thing; the shader clock is measured under load during the last
computation (uvrt_clock_probe_*).

    python tests/tools/drive_bench.py [--rounds R] [--photons N] [--iterations I] [--speed V] [--pkg-dir DIR]

--pkg-dir: load the package (its Python files and built libraries) from another directory, e.g. a build of the parent
commit, for an A/B in alternating processes."""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402


def load_package_from(pkg_dir):
    """what __graft_entry__.load_package does, for a package directory of the caller's choice"""
    spec = importlib.util.spec_from_file_location(g.PKG_NAME, os.path.join(pkg_dir, "__init__.py"),
                                                  submodule_search_locations=[pkg_dir])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[g.PKG_NAME] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--photons", type=int, default=1 << 25)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--speed", type=float, default=0.1)
    ap.add_argument("--pkg-dir", default=None)
    a = ap.parse_args()
    rounds = max(a.rounds, 5)
    try:                       # torch's HIP runtime first where torch is used in the same process (tests/conftest.py)
        import torch
        if torch.cuda.is_available():
            torch.cuda.init()
    except Exception:
        pass
    if a.pkg_dir:
        load_package_from(os.path.abspath(a.pkg_dir))
    else:
        g.load_package()
    from uvrt_amd import host
    rt = host.RayTracer(os.path.join(ROOT, "tests/golden/testroomopt.glb"), os.path.join(ROOT, "tests/golden/lange_route.xml"), device=0)
    rt.photonCount = a.photons
    rt.maxIterations = a.iterations
    rt.driveSpeed = a.speed
    L = len(rt.lamps())
    launches = a.iterations * (2 * L - 1 if a.speed > 0 and L >= 2 else L)
    rays = launches * rt.photonsPerLight

    def computation():
        rt.ctx.seed = 0
        rt.ResetDosageMap()
        rt.ComputeIterationsBatched(a.iterations)
        rt.Sync()

    computation()              # warm-up: allocations, hot records, free records, clocks
    times = []
    mhz = None
    for r in range(rounds):
        if r == rounds - 1:
            try:
                rt.ctx.clock_probe_start(20000)
            except Exception:
                pass
        t0 = time.perf_counter()
        computation()
        times.append(time.perf_counter() - t0)
    try:
        mhz = rt.ctx.clock_probe_read()
    except Exception:
        pass
    dose = rt.read_dosage()
    med = statistics.median(times)
    print(json.dumps({"tool": "drive_bench", "positions": L, "iterations": a.iterations, "drive_speed": a.speed,
                      "photons_per_launch": rt.photonsPerLight, "launches": launches, "rays": rays, "rounds": rounds,
                      "seconds_median": round(med, 6), "seconds_min": round(min(times), 6), "seconds_max": round(max(times), 6),
                      "gray_per_s": round(rays / med / 1e9, 4), "shader_mhz": None if mhz is None else round(mhz, 1),
                      "dose_crc": "%08x" % zlib.crc32(dose.tobytes()), "seed": rt.ctx.seed,
                      "package": os.path.abspath(a.pkg_dir) if a.pkg_dir else "in-tree"}))
    rt.close()


if __name__ == "__main__":
    main()
