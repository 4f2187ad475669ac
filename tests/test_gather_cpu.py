"""No GPU: the host-only parts of the shadow-ray / direct-gather interface (include/uvrt.h "shadow rays and the direct
gather") -- the symbols in both libraries, the binding's layout of uvrt_gather_params against a C compiler's, the refusals
that need no device, the route file's <gather_samples>, the CLI's refusals -- and the estimator itself: the restatement
(tests/gather_restate.py) against the oracle's photon counts."""
import ctypes as C
import os
import subprocess

import numpy as np

import gather_restate as gr
from conftest import GLB, GOLDEN, ROOT

NEW = ("uvrt_occluded", "uvrt_gather_direct", "uvrt_accumulate_expected", "uvrt_read_expected")


def test_symbols_are_bound_and_resolve_in_both_libraries(pkg):
    names = [name for name, _, _ in pkg.capi.SYMBOLS]
    for n in NEW:
        assert names.count(n) == 1
        for path in (pkg.capi.LIB_PATH, pkg.capi.LIB_DEV_PATH):
            assert hasattr(C.CDLL(path), n), (path, n)
        for dev in (False, True):
            assert getattr(pkg.capi.lib(dev), n).restype is C.c_int
    for m in ("occluded", "gather_direct", "accumulate_expected", "read_expected"):
        assert hasattr(pkg.capi.Ctx, m)
    from uvrt_amd import host
    assert "gatherSamples" in host._FIELDS and "gatherSamples" in host._INT_FIELDS


def test_gather_params_binding_matches_the_header(pkg, tmp_path):
    """uvrt_gather_params as the Python binding lays it out (capi.GatherParams) = as a C compiler lays out the struct of
    include/uvrt.h: same size and field offsets."""
    fields = ("from", "to", "light_length", "samples", "seed", "photons_equiv", "reserved")
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "uvrt.h"\nint main(void){printf("%zu'
                   + " %zu" * len(fields) + '\\n", sizeof(uvrt_gather_params)'
                   + "".join(", offsetof(uvrt_gather_params, %s)" % f for f in fields) + ");return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    G = pkg.capi.GatherParams
    want = [C.sizeof(G)] + [getattr(G, "from_" if f == "from" else f).offset for f in fields]
    assert got == want and C.sizeof(G) == 48
    g = G()
    g.from_ = (C.c_float * 3)(1, 2, 3)
    g.to = (C.c_float * 3)(4, 5, 6)
    g.samples, g.seed, g.photons_equiv = 16, 0xFFFFFFFF, 1 << 21
    raw = np.frombuffer(bytes(g), dtype=np.uint32)
    assert raw[:6].view(np.float32).tolist() == [1, 2, 3, 4, 5, 6] and raw[7:10].tolist() == [16, 0xFFFFFFFF, 1 << 21]


def test_null_arguments_are_refused_without_a_gpu(pkg):
    rays = np.zeros(4, dtype=pkg.capi.RAY_DT)
    out = np.zeros(4, dtype=np.uint8)
    exp = np.zeros(4, dtype=np.float64)
    prm = pkg.capi.GatherParams()
    prm.samples, prm.photons_equiv = 4, 100
    for dev in (False, True):
        L = pkg.capi.lib(dev)
        calls = (("uvrt_occluded", lambda: L.uvrt_occluded(None, rays.ctypes.data, 4, out.ctypes.data)),
                 ("uvrt_gather_direct", lambda: L.uvrt_gather_direct(None, C.byref(prm), 0, 4)),
                 ("uvrt_accumulate_expected", lambda: L.uvrt_accumulate_expected(None, 1.0, 4)),
                 ("uvrt_read_expected", lambda: L.uvrt_read_expected(None, exp.ctypes.data, 0, 4)))
        for name, call in calls:
            assert call() == -1 and name.encode() in L.uvrt_last_error(), name          # UVRT_ERR_INVALID


def test_route_file_keeps_the_gather_samples(pkg, tmp_path):
    """<gather_samples> is written only when > 0; a route saved at 0 is byte for byte what the tag-less writer saved."""
    from uvrt_amd import host
    rt = host.RayTracer(init=False)
    rt.set_route_dir(GOLDEN + os.sep)
    rt.LoadRoute("lange_route")
    assert rt.gatherSamples == 0
    rt.set_route_dir(str(tmp_path) + os.sep)
    rt.SaveRoute("photons")
    plain = (tmp_path / "photons.xml").read_bytes()
    assert plain == open(os.path.join(GOLDEN, "lange_route.xml"), "rb").read()
    assert b"gather_samples" not in plain
    rt.gatherSamples = 16
    rt.SaveRoute("gathering")
    gathering = (tmp_path / "gathering.xml").read_bytes()
    line = b"    <gather_samples>16</gather_samples>\n"
    assert gathering.count(line) == 1 and gathering.replace(line, b"") == plain
    assert gathering.index(line) == gathering.index(b"</minimale_bestralingssterkte>\n") + len(b"</minimale_bestralingssterkte>\n")
    rt.driveSpeed = 0.125                       # both additions: the speed first
    rt.SaveRoute("both")
    both = (tmp_path / "both.xml").read_bytes()
    assert both.index(b"<rijsnelheid>") < both.index(b"<gather_samples>") < both.index(b"<lamp_lengte>")
    rt2 = host.RayTracer(init=False)
    rt2.set_route_dir(str(tmp_path) + os.sep)
    rt2.LoadRoute("gathering")
    assert rt2.gatherSamples == 16 and rt2.driveSpeed == 0.0 and rt2.lamps() == rt.lamps()
    rt2.LoadRoute("both")
    assert rt2.gatherSamples == 16 and np.float32(rt2.driveSpeed) == np.float32(0.125)
    rt2.LoadRoute("photons")                    # absent: back to 0
    assert rt2.gatherSamples == 0
    rt.close(); rt2.close()


def test_cli_refuses_gather_with_batch_gpus_and_plan(pkg):
    cli = os.path.join(os.path.dirname(pkg.capi.LIB_PATH), "uvrt_cli")
    base = [cli, "--room", GLB, "--route-dir", GOLDEN, "--route", "lange_route", "--gather", "4"]
    for extra, word in ((["--batch", "2"], "--batch"), (["--gpus", "2"], "--gpus"), (["--plan"], "--plan"),
                        (["--plan", "50"], "--plan"), (["--plan-drive", "0.1"], "--plan-drive")):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2, (extra, r.stdout, r.stderr)
        assert "--gather" in r.stderr and word in r.stderr, (extra, r.stderr)
    r = subprocess.run(base[:-1] + ["5000"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--gather" in r.stderr


# median over the triangles with >= 400 photons of expected / count, S = 16, gather seeds 0..7, as measured with this
# restatement; the largest deviation from 1 is 0.0235
RECORDED = (0.9890, 0.9867, 1.0047, 0.9889, 0.9799, 1.0078, 0.9942, 0.9765)
BAND = 3 * 0.0235


def test_the_estimator_agrees_with_the_photon_counts(orc, oscene, oroute):
    """The physics: at route position 0 the gather's expected tempPhotonMap entry against the count of N = 2^21 oracle
    photons, on the triangles the photons resolve (>= 400 of them).  The median ratio of each of 8 gather seeds lies within
    three times the largest deviation from 1 that was recorded -- seed-to-seed noise; an estimator that is wrong is off by
    more than 0.1."""
    gr.check_rng(orc)
    N = 1 << 21
    comp = orc.Computation(oscene, oroute["lamps"], N, oroute["lightHeight"], oroute["lightLength"], oroute["lightIntensity"])
    lp = comp.lamp_world_pos(oroute["lamps"][0])
    rays, _ = orc.generate(0, N, lp, oroute["lightLength"], 0)
    counts = np.zeros(oscene.T, dtype=np.int32)
    orc.extend(counts, oscene.tris, rays, oscene.nodes, oscene.triIdx)
    sel = counts >= 400
    assert sel.sum() > 500 and (counts == 0).sum() > 0.4 * oscene.T
    assert max(abs(m - 1) for m in RECORDED) < 0.1
    medians = []
    for seed in range(8):
        e, _, occ = gr.gather(orc, oscene, lp, lp, oroute["lightLength"], 16, seed, N)
        medians.append(float(np.median(e[sel] / counts[sel])))
        if seed == 0:
            assert 0.2 < 1.0 - occ.mean() < 0.8
            assert ((counts == 0) & (e > 0)).sum() > 1000          # the point of it: estimates where no photon arrives
    print("medians of expected / count:", " ".join("%.4f" % m for m in medians))
    for seed, m in enumerate(medians):
        assert abs(m - 1.0) <= BAND, "gather seed %d: median %.4f" % (seed, m)
