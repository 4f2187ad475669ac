"""No GPU: the host-only parts of the recorded hit links and the multi-bounce gather (include/uvrt.h "recorded hit links",
DESIGN.md 18) -- the symbols in both libraries and in the bindings, the layouts of uvrt_links_params and uvrt_linked_params
against a C compiler's, the refusals that need no device, route files with and without <reflect_bounces>, the CLI's and the
binding's refusals -- and the restatement (tests/gather_links_restate.py) against the one-bounce restatement and against the
closed cube, where b bounces return rho^b times the source."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gather_edge_scene as ges
import gather_indirect_restate as gi
import gather_links_restate as gl
import gather_restate as gr
from conftest import GLB, GOLDEN, ROOT
from plan_options_pin import check_plan_option

NEW = ("uvrt_indirect_links_build", "uvrt_indirect_links_info", "uvrt_read_indirect_links", "uvrt_gather_indirect_linked")
f32 = np.float32


def test_symbols_are_bound_and_resolve_in_both_libraries(pkg):
    names = [name for name, _, _ in pkg.capi.SYMBOLS]
    header = open(os.path.join(ROOT, "include", "uvrt.h")).read()
    for n in NEW:
        assert names.count(n) == 1
        assert ("int %s(uvrt_ctx* ctx, " % n) in header
        for path in (pkg.capi.LIB_PATH, pkg.capi.LIB_DEV_PATH):
            assert hasattr(C.CDLL(path), n), (path, n)
        for dev in (False, True):
            assert getattr(pkg.capi.lib(dev), n).restype is C.c_int
    by_name = {n: a for n, _, a in pkg.capi.SYMBOLS}
    assert [len(by_name[n]) for n in NEW] == [2, 2, 4, 4]
    for m in ("indirect_links_build", "indirect_links_info", "read_indirect_links", "gather_indirect_linked"):
        assert hasattr(pkg.capi.Ctx, m)
    from uvrt_amd import host
    check_plan_option(host, "reflect_bounces", C.c_int, 0)
    check_plan_option(host, "reflectance", C.c_float, 0.0)                 # the option from before stays
    assert "reflectBounces" in host._FIELDS and "reflectBounces" in host._INT_FIELDS


def test_struct_layouts_match_the_c_compiler(pkg, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text("""#include <stddef.h>
#include <stdio.h>
#include "uvrt.h"
int main(void)
{
    printf("%zu %zu %zu %zu\\n", sizeof(uvrt_links_params), offsetof(uvrt_links_params, samples), offsetof(uvrt_links_params, seed),
           offsetof(uvrt_links_params, reserved));
    printf("%zu %zu %zu %zu %zu\\n", sizeof(uvrt_linked_params), offsetof(uvrt_linked_params, reflectance),
           offsetof(uvrt_linked_params, bounces), offsetof(uvrt_linked_params, add), offsetof(uvrt_linked_params, reserved));
    return 0;
}
""")
    exe = tmp_path / "layout"
    subprocess.run([os.environ.get("CC", "cc"), "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    P, Q = pkg.capi.LinksParams, pkg.capi.LinkedParams
    assert [int(v) for v in out[0].split()] == [C.sizeof(P), P.samples.offset, P.seed.offset, P.reserved.offset] == [16, 0, 4, 8]
    assert [int(v) for v in out[1].split()] == [C.sizeof(Q), Q.reflectance.offset, Q.bounces.offset, Q.add.offset,
                                                Q.reserved.offset] == [24, 0, 4, 8, 12]


def test_null_arguments_are_refused_without_a_gpu(pkg):
    buf = np.full(16, 7, dtype=np.int32)
    lp = pkg.capi.LinksParams(4, 1)
    kp = pkg.capi.LinkedParams(0.25, 1, 0)
    for dev in (False, True):
        L = pkg.capi.lib(dev)
        calls = (("uvrt_indirect_links_build", lambda: L.uvrt_indirect_links_build(None, C.byref(lp))),
                 ("uvrt_indirect_links_build", lambda: L.uvrt_indirect_links_build(None, None)),
                 ("uvrt_indirect_links_info", lambda: L.uvrt_indirect_links_info(None, buf.ctypes.data)),
                 ("uvrt_indirect_links_info", lambda: L.uvrt_indirect_links_info(None, None)),
                 ("uvrt_read_indirect_links", lambda: L.uvrt_read_indirect_links(None, buf.ctypes.data, 0, 4)),
                 ("uvrt_read_indirect_links", lambda: L.uvrt_read_indirect_links(None, None, 0, 4)),
                 ("uvrt_gather_indirect_linked", lambda: L.uvrt_gather_indirect_linked(None, C.byref(kp), 0, 4)),
                 ("uvrt_gather_indirect_linked", lambda: L.uvrt_gather_indirect_linked(None, None, 0, 4)))
        for name, call in calls:
            assert call() == -1 and name.encode() in L.uvrt_last_error(), name          # UVRT_ERR_INVALID
    assert np.all(buf == 7)


def test_route_file_keeps_the_bounces(pkg, tmp_path):
    """<reflect_bounces> is written only when reflectance > 0 and reflectBounces > 0, after <reflect_samples>; every file written
    without it is byte for byte what it was; an absent tag loads as 0."""
    from uvrt_amd import host
    golden = open(os.path.join(GOLDEN, "lange_route.xml"), "rb").read()
    rt = host.RayTracer(init=False)
    rt.set_route_dir(GOLDEN + os.sep)
    rt.LoadRoute("lange_route")
    assert rt.reflectBounces == 0
    rt.set_route_dir(str(tmp_path) + os.sep)
    rt.SaveRoute("photons")
    assert (tmp_path / "photons.xml").read_bytes() == golden
    rt.gatherSamples = 16
    rt.reflectSamples = 8
    rt.reflectBounces = 3                       # without a reflectance: no bounce, no tag
    rt.SaveRoute("direct")
    direct = (tmp_path / "direct.xml").read_bytes()
    assert b"reflect" not in direct
    rt.reflectance = 0.125
    rt.reflectBounces = 0                       # the traced bounce: the file of the parent
    rt.SaveRoute("traced")
    traced = (tmp_path / "traced.xml").read_bytes()
    assert b"reflect_bounces" not in traced and b"<reflect_samples>8</reflect_samples>" in traced
    rt.reflectBounces = 3
    rt.SaveRoute("linked")
    linked = (tmp_path / "linked.xml").read_bytes()
    tag = b"    <reflect_bounces>3</reflect_bounces>\n"
    assert linked.count(tag) == 1 and linked.replace(tag, b"") == traced
    assert linked.index(b"<reflect_samples>8</reflect_samples>\n") + len(b"<reflect_samples>8</reflect_samples>\n") == linked.index(tag)
    rt2 = host.RayTracer(init=False)
    rt2.set_route_dir(str(tmp_path) + os.sep)
    rt2.LoadRoute("linked")
    assert rt2.reflectBounces == 3 and rt2.reflectance == 0.125 and rt2.reflectSamples == 8 and rt2.lamps() == rt.lamps()
    rt2.SaveRoute("again")
    assert (tmp_path / "again.xml").read_bytes() == linked
    rt2.LoadRoute("traced")                     # absent: back to 0
    assert rt2.reflectBounces == 0 and rt2.reflectance == 0.125
    rt2.SaveRoute("traced2")
    assert (tmp_path / "traced2.xml").read_bytes() == traced
    rt.close(); rt2.close()


def test_the_binding_refuses_bounces_outside_0_to_16(pkg):
    from uvrt_amd import host
    rt = host.RayTracer(init=False)
    try:
        for k in (-1, 17):
            with pytest.raises(ValueError, match="reflectBounces"):
                rt.reflectBounces = k
            with pytest.raises(ValueError, match="reflect_bounces"):
                rt.PlanDurationsReflect(0.1, 4, gather_samples=16, reflect_bounces=k)
        with pytest.raises(ValueError, match="reflect_bounces"):
            rt.PlanDurationsReflect(0.1, 4, gather_samples=16, reflect_bounces=1.5)
        assert rt.reflectBounces == 0
        rt.reflectBounces = 16
        assert rt.reflectBounces == 16
        with pytest.raises(ValueError, match="gather_confidence"):              # the existing refusal stays
            rt.PlanDurationsReflect(0.1, 4, gather_samples=16, gather_confidence=2.0, reflect_bounces=2)
    finally:
        rt.close()


def test_cli_refuses_bounces_it_cannot_run(pkg):
    cli = os.path.join(os.path.dirname(pkg.capi.LIB_PATH), "uvrt_cli")
    base = [cli, "--room", GLB, "--route-dir", GOLDEN, "--route", "lange_route"]
    for extra in (["--gather", "16", "--reflect", "0.1", "--reflect-bounces", "-1"],
                  ["--gather", "16", "--reflect", "0.1", "--reflect-bounces", "0"],
                  ["--gather", "16", "--reflect", "0.1", "--reflect-bounces", "17"],
                  ["--gather", "16", "--reflect", "0.1", "--reflect-bounces", "three"],
                  ["--gather", "16", "--reflect", "0.1", "--reflect-bounces", "3x"],
                  ["--plan-gather", "16", "--reflect", "0.1", "--reflect-bounces", "2.5"],
                  ["--gather", "16", "--reflect-bounces", "3"],
                  ["--plan-gather", "16", "--reflect-bounces", "3"],
                  ["--reflect-bounces", "3"]):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2, (extra, r.stdout, r.stderr)
        assert "--reflect-bounces" in r.stderr, (extra, r.stderr)
    r = subprocess.run(base + ["--gather", "16", "--reflect", "0.1", "--reflect-bounces"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2
    # without a gather the bounce itself is refused, and --plan-confidence still refuses --reflect
    for extra in (["--reflect", "0.1", "--reflect-bounces", "3"],
                  ["--plan-gather", "16", "--plan-confidence", "2", "--reflect", "0.1", "--reflect-bounces", "3"],
                  ["--plan-gather", "16", "--plan-confidence", "2", "--reflect", "0.1"]):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "--reflect" in r.stderr, (extra, r.stderr)


# ---------------------------------------------------------------- the restatement against itself
def _source(T, seed):
    return np.random.default_rng(seed).uniform(0.0, 1000.0, T)


@pytest.mark.parametrize("add", (0, 1))
def test_one_linked_bounce_is_the_traced_bounce_on_the_cube_and_the_edge_scene(orc, add):
    for scene, S2, seed in ((ges.HandScene(orc, gi.cube_tris()), 4, 7), (ges.edge_scene(orc), 6, 11)):
        source = _source(scene.T, 3)
        base = _source(scene.T, 4) if add else None
        want, _, _, _ = gi.indirect(orc, scene, source, 0.3, S2, seed, base=base)
        lk = gl.links(orc, scene, S2, seed)
        got = gl.linked(scene.tris, source, lk, 0.3, 1, base=base)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
        first, count = 5, scene.T - 7
        part = gl.linked(scene.tris, source, lk, 0.3, 1, first, count, None if base is None else base[first:first + count])
        assert np.array_equal(part.view(np.uint64), want[first:first + count].view(np.uint64))


def test_the_edge_scene_links_point_at_no_triangle_without_area(orc):
    scene = ges.edge_scene(orc)
    lk = gl.links(orc, scene, 6, 11)
    assert not np.isin(lk, scene.no_area).any()
    assert np.all(lk[scene.no_area] == -1)
    got = gl.linked(scene.tris, _source(scene.T, 3), lk, 0.5, 3)
    assert np.all(got[scene.no_area] == 0.0)
    assert not (lk == np.arange(scene.T)[:, None]).any()


def test_one_linked_bounce_is_the_traced_bounce_on_2000_triangles_of_the_room(orc, oscene):
    first, count, S2, seed = 21000, 2000, 4, 5
    source = _source(oscene.T, 9)
    want, _, _, _ = gi.indirect(orc, oscene, source, 0.1, S2, seed, first=first, count=count)
    lk = gl.links(orc, oscene, S2, seed, first=first, count=count)
    got = gl.linked(oscene.tris, source, lk, 0.1, 1, first, count)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert (lk >= 0).any() and (lk < 0).any()


@pytest.mark.parametrize("S2", (2, 4, 64))
def test_the_closed_cube_returns_rho_to_the_b_times_its_source(orc, S2):
    """Every triangle of the closed cube carries the same irradiance, half of each triangle's samples see the inside: bounce b
    is rho^b x source.  At most about 6 roundings of 2^-53 per bounce: under 1e-14 after 8, so 1e-12 has two decades of margin."""
    cube = ges.HandScene(orc, gi.cube_tris())
    nn = gl.normals(cube.tris)
    assert np.all(nn == 16.0)
    source = 0.5 * nn * 1000.0
    lk = gl.links(orc, cube, S2, 7)
    assert not (lk == np.arange(12)[:, None]).any(), "no link is a self-link"
    assert (lk < 0).sum() * 2 == lk.size, "exactly half the links are -1"
    g = gl.bounces(cube.tris, source, lk, 0.5, 8)
    for b in range(1, 9):
        want = 0.5 ** b * source
        assert np.all(np.abs(g[b - 1] - want) <= 1e-12 * want), b
    total = gl.linked(cube.tris, source, lk, 0.5, 8)
    acc = g[0]
    for b in range(1, 8):
        acc = acc + g[b]
    assert np.array_equal(total.view(np.uint64), acc.view(np.uint64))
