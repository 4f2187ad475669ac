"""GPU: a plain bench.py run times the headline and nothing else, and `--dump-outputs` writes what its last timed step
computed -- the same arrays, bit for bit, on every run with the same arguments."""
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def bench(args):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args,
                         capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])


def test_plain_run_dumps_the_outputs_of_its_last_timed_step(tmp_path):
    common = ["--gpus", "1", "--photons", "200000", "--waves", "4", "--steps", "3", "--warmup", "1"]
    d = bench(common + ["--dump-outputs", str(tmp_path / "a")])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(d["config"]["rays_per_step"] / (d["ms_per_step"] * 1e3), rel=2e-3)
    # nothing beside the headline
    assert d["roofline"] is None and d["cpu_baseline"] is None and d["other_modes"] == {}
    assert d["cold_start"] is None and d["route_workload"] is None and "single_computation" not in d
    T = d["config"]["triangles"]
    a = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in ("dose", "color", "photon_map", "max_photon_map")}
    assert a["dose"].dtype == np.float32 and a["dose"].shape == (T,)
    assert a["color"].dtype == np.float32 and a["color"].shape == (T, 9)
    assert a["photon_map"].dtype == np.float64 and a["max_photon_map"].dtype == np.float64
    assert "%08x" % zlib.crc32(a["dose"].tobytes()) == d["dose_crc32"]
    assert a["photon_map"].sum() > 0 and np.isfinite(a["dose"]).all()
    b = bench(common + ["--dump-outputs", str(tmp_path / "b")])
    for n, x in a.items():
        assert np.array_equal(x.view(np.uint8), np.load(tmp_path / "b" / (n + ".npy")).view(np.uint8)), n
    assert b["dose_crc32"] == d["dose_crc32"]
