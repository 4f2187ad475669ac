"""No GPU: the host-only parts of the face-resolved gather and bounces (include/uvrt.h "face-resolved gather and bounces",
DESIGN.md 21) -- the symbols in both libraries, the header and the bindings, the refusals that need no device, route files with
and without <reflect_sided>, the CLI's and the binding's refusals -- and the restatement (tests/gather_faces_restate.py)
against the two-sided one: the closed cube, where no light crosses a sheet and both models agree bit for bit; the plates,
where they must not; the edge scene and 2 000 triangles of the room, where the face-resolved bounce never exceeds the two-sided
one and never amplifies."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gather_edge_scene as ges
import gather_faces_restate as gf
import gather_indirect_restate as gi
import gather_links_restate as gl
import gather_restate as gr
from conftest import GLB, GOLDEN, ROOT

NEW = ("uvrt_set_gather_faces", "uvrt_get_gather_faces", "uvrt_read_gather_faces", "uvrt_write_gather_faces",
       "uvrt_indirect_links_build_sided", "uvrt_gather_indirect_linked_sided")
N = 1 << 20


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def test_symbols_are_bound_and_resolve_in_both_libraries(pkg):
    names = [name for name, _, _ in pkg.capi.SYMBOLS]
    header = open(os.path.join(ROOT, "include", "uvrt.h")).read()
    assert "face-resolved gather and bounces" in header
    for n in NEW:
        assert names.count(n) == 1
        assert ("int %s(uvrt_ctx* ctx, " % n) in header
        for path in (pkg.capi.LIB_PATH, pkg.capi.LIB_DEV_PATH):
            assert hasattr(C.CDLL(path), n), (path, n)
        for dev in (False, True):
            assert getattr(pkg.capi.lib(dev), n).restype is C.c_int
    by_name = {n: a for n, _, a in pkg.capi.SYMBOLS}
    assert [len(by_name[n]) for n in NEW] == [2, 2, 5, 5, 2, 4]
    for m in ("set_gather_faces", "get_gather_faces", "read_gather_faces", "write_gather_faces", "indirect_links_build_sided",
              "indirect_links_kind", "gather_indirect_linked_sided"):
        assert hasattr(pkg.capi.Ctx, m)
    from uvrt_amd import host
    assert "reflectSided" in host._FIELDS and "reflectSided" in host._INT_FIELDS


def test_null_arguments_are_refused_without_a_gpu(pkg):
    buf = np.full(16, 7.0)
    on = C.c_int32(5)
    lp = pkg.capi.LinksParams(4, 1)
    kp = pkg.capi.LinkedParams(0.25, 1, 0)
    for dev in (False, True):
        L = pkg.capi.lib(dev)
        calls = (("uvrt_set_gather_faces", lambda: L.uvrt_set_gather_faces(None, 1)),
                 ("uvrt_get_gather_faces", lambda: L.uvrt_get_gather_faces(None, C.byref(on))),
                 ("uvrt_get_gather_faces", lambda: L.uvrt_get_gather_faces(None, None)),
                 ("uvrt_read_gather_faces", lambda: L.uvrt_read_gather_faces(None, 0, buf.ctypes.data, 0, 4)),
                 ("uvrt_read_gather_faces", lambda: L.uvrt_read_gather_faces(None, 0, None, 0, 4)),
                 ("uvrt_write_gather_faces", lambda: L.uvrt_write_gather_faces(None, 1, buf.ctypes.data, 0, 4)),
                 ("uvrt_write_gather_faces", lambda: L.uvrt_write_gather_faces(None, 1, None, 0, 4)),
                 ("uvrt_indirect_links_build_sided", lambda: L.uvrt_indirect_links_build_sided(None, C.byref(lp))),
                 ("uvrt_indirect_links_build_sided", lambda: L.uvrt_indirect_links_build_sided(None, None)),
                 ("uvrt_gather_indirect_linked_sided", lambda: L.uvrt_gather_indirect_linked_sided(None, C.byref(kp), 0, 4)),
                 ("uvrt_gather_indirect_linked_sided", lambda: L.uvrt_gather_indirect_linked_sided(None, None, 0, 4)))
        for name, call in calls:
            assert call() == -1 and name.encode() in L.uvrt_last_error(), name          # UVRT_ERR_INVALID
    assert np.all(buf == 7.0) and on.value == 5


def test_route_file_keeps_the_sided_flag(pkg, tmp_path):
    """<reflect_sided>1</reflect_sided> is written only when the linked bounce is written and reflectSided is on, right after
    <reflect_bounces>; every file written without it is byte for byte what it was; an absent tag loads as 0."""
    from uvrt_amd import host
    golden = open(os.path.join(GOLDEN, "lange_route.xml"), "rb").read()
    rt = host.RayTracer(init=False)
    rt.set_route_dir(GOLDEN + os.sep)
    rt.LoadRoute("lange_route")
    assert rt.reflectSided == 0
    rt.set_route_dir(str(tmp_path) + os.sep)
    rt.SaveRoute("photons")
    assert (tmp_path / "photons.xml").read_bytes() == golden
    rt.gatherSamples = 16
    rt.reflectance = 0.125
    rt.reflectSamples = 8
    rt.reflectBounces = 3
    rt.SaveRoute("linked")
    linked = (tmp_path / "linked.xml").read_bytes()
    assert b"reflect_sided" not in linked and b"<reflect_bounces>3</reflect_bounces>" in linked
    rt.reflectSided = 1
    rt.SaveRoute("sided")
    sided = (tmp_path / "sided.xml").read_bytes()
    tag = b"    <reflect_sided>1</reflect_sided>\n"
    before = b"<reflect_bounces>3</reflect_bounces>\n"
    assert sided.count(tag) == 1 and sided.replace(tag, b"") == linked
    assert sided.index(before) + len(before) == sided.index(tag)
    rt2 = host.RayTracer(init=False)
    rt2.set_route_dir(str(tmp_path) + os.sep)
    rt2.LoadRoute("sided")
    assert rt2.reflectSided == 1 and rt2.reflectBounces == 3 and rt2.reflectance == 0.125 and rt2.lamps() == rt.lamps()
    rt2.SaveRoute("again")
    assert (tmp_path / "again.xml").read_bytes() == sided
    rt2.LoadRoute("linked")                     # absent: back to 0
    assert rt2.reflectSided == 0 and rt2.reflectBounces == 3
    rt2.SaveRoute("linked2")
    assert (tmp_path / "linked2.xml").read_bytes() == linked
    rt.close(); rt2.close()


def test_the_binding_refuses_a_value_other_than_0_or_1(pkg):
    from uvrt_amd import host
    rt = host.RayTracer(init=False)
    try:
        for k in (-1, 2):
            with pytest.raises(ValueError, match="reflectSided"):
                rt.reflectSided = k
        assert rt.reflectSided == 0
        rt.reflectSided = 1
        assert rt.reflectSided == 1
        for k in (-1, 2, 0.5):
            with pytest.raises(ValueError, match="reflect_sided"):
                rt.PlanDurationsReflect(0.1, 4, gather_samples=16, reflect_bounces=2, reflect_sided=k)
        with pytest.raises(ValueError, match="reflect_sided"):      # the traced single bounce has no sided form
            rt.PlanDurationsReflect(0.1, 4, gather_samples=16, reflect_bounces=0, reflect_sided=1)
    finally:
        rt.close()


def test_cli_refuses_sided_without_linked_bounces(pkg):
    cli = os.path.join(os.path.dirname(pkg.capi.LIB_PATH), "uvrt_cli")
    base = [cli, "--room", GLB, "--route-dir", GOLDEN, "--route", "lange_route"]
    for extra in (["--gather", "16", "--reflect", "0.1", "--reflect-sided"],
                  ["--gather", "16", "--reflect-sided"],
                  ["--plan-gather", "16", "--reflect", "0.1", "--reflect-sided"],
                  ["--reflect-sided"],
                  ["--gather", "16", "--gather-batch", "4", "--reflect", "0.1", "--reflect-bounces", "2", "--reflect-sided"]):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2, (extra, r.stdout, r.stderr)
        assert "--reflect-sided" in r.stderr, (extra, r.stderr)


# ---------------------------------------------------------------- the restatement against itself
@pytest.mark.parametrize("S2", (2, 4, 64))
def test_the_closed_cube_is_the_two_sided_rule_bit_for_bit(orc, S2):
    """the source on the inner faces, 0 on the outer ones: every link arrives on an inner face and the outer faces' samples all
    miss, so each sum holds the two-sided sum's non-zero terms in its order.  Every triangle carries the same irradiance: bounce b
    is rho^b x source (about 6 roundings of 2^-53 per bounce, as for the two-sided rule: 1e-12 has two decades of margin)."""
    cube = ges.HandScene(orc, gi.cube_tris())
    nn = gl.normals(cube.tris)
    source = 0.5 * nn * 1000.0
    faces = gf.cube_faces(source)
    inner = gf.inner_face(cube.tris, (gi.CUBE_SIDE / 2,) * 3)
    assert bits_equal(faces[0] + faces[1], source) and np.all(faces[1 - inner, np.arange(12)] == 0.0)
    lk = gf.sided_links(orc, cube, S2, 7)
    plain = gl.links(orc, cube, S2, 7)
    assert np.array_equal(lk < 0, plain < 0) and np.array_equal((lk >> 1)[plain >= 0], plain[plain >= 0])
    assert np.array_equal((lk & 1)[lk >= 0], inner[lk[lk >= 0] >> 1])
    for K in (1, 2, 5):
        assert bits_equal(gf.linked(cube.tris, faces, lk, 0.5, K), gl.linked(cube.tris, source, plain, 0.5, K)), K
    g, _ = gf.bounces(cube.tris, faces, lk, 0.5, 8)
    for b in range(1, 9):
        want = 0.5 ** b * source
        assert np.all(np.abs((g[b - 1][0] + g[b - 1][1]) - want) <= 1e-12 * want), b
        assert np.all(g[b - 1][1 - inner, np.arange(12)] == 0.0), "the outer faces stay dark"


@pytest.mark.parametrize("S2", (16, 64))
def test_the_plates_shade_what_the_two_sided_bounce_lights(orc, S2):
    """only A's face towards B emits: one face-resolved bounce leaves both triangles of C and B's face away from A at exactly 0 and
    lights B's facing side; the two-sided bounce over the same plane lights C from A's dark side"""
    scene = ges.HandScene(orc, gf.plates_tris())
    faces = gf.plates_faces()
    A, B, Cc = (list(gf.PLATES[k]) for k in "ABC")
    n = gr.tri_normals(np.ascontiguousarray(scene.tris[12:], dtype=np.float32))[2]
    assert np.all(n[:, 1] > 0) and np.all(n[:, [0, 2]] == 0), "face 0 of every plate looks up"
    lk = gf.sided_links(orc, scene, S2, 3)
    g, _ = gf.bounces(scene.tris, faces, lk, 1.0, 1)
    assert np.all(g[0][:, Cc] == 0.0) and np.all(g[0][0, B] == 0.0) and np.all(g[0][1, B] > 0.0)
    assert np.all(g[0][:, A] == 0.0)
    plain = gl.linked(scene.tris, faces[0] + faces[1], gl.links(orc, scene, S2, 3), 1.0, 1)
    assert np.all(plain[Cc] > 0.0) and bits_equal(plain[B], g[0][1, B])


def _direct(orc, scene, frm, length, first, count):
    return gf.gather_faces(orc, scene, frm, frm, length, 4, 7, N, first=first, count=count)


def _check_against_two_sided(tris, faces, expected, sided, plain):
    """what holds on any scene.  Each sum below has at most 4 096 terms, every one >= 0: a sum's relative rounding error is under
    4 096 x 2^-53 < 5e-13, so 1e-12 bounds the comparison of two of them.
    f0 + f1 = expected: the two face sums split the terms of expected's sum.
    sided g_1 <= two-sided g_1: face f of t sums e_0[a][h] over half the samples, the two-sided rule e_0[0][h] + e_0[1][h] over
    all of them.
    max e_b <= max e_{b-1} at rho = 1: e_b[f][t] = 2 / S2 x a sum of S2 / 2 values of e_{b-1}."""
    total = faces[0] + faces[1]
    assert np.all(np.abs(total - expected) <= 1e-12 * expected)
    g, e = gf.bounces(tris, faces, sided, 1.0, 6)
    two = gl.bounces(tris, total, plain, 1.0, 1)[0]
    assert np.all(g[0][0] + g[0][1] <= two * (1 + 1e-12))
    assert (g[0][0] + g[0][1] < 0.999 * two).any(), "the two models differ somewhere"
    for b in range(1, 7):
        assert e[b].max() <= e[b - 1].max() * (1 + 1e-12), b
    assert e[0].max() > 0


def test_the_edge_scene_never_amplifies(orc):
    scene = ges.edge_scene(orc)
    faces, expected = _direct(orc, scene, ges.LAMP, 1.0, 0, None)
    assert (faces[0] > 0).any() and (faces[1] > 0).any()
    _check_against_two_sided(scene.tris, faces, expected, gf.sided_links(orc, scene, 6, 11), gl.links(orc, scene, 6, 11))


def test_2000_triangles_of_the_room_never_amplify(orc, oscene, oroute):
    """a real direct plane at S = 4 on triangles [21000, 23000); the bounces run over those 2 000 triangles as a scene of their own
    (links that leave the range dropped in both models)"""
    first, count, S2 = 21000, 2000, 4
    comp = orc.Computation(oscene, oroute["lamps"], N, oroute["lightHeight"], oroute["lightLength"], oroute["lightIntensity"])
    place = comp.lamp_world_pos(oroute["lamps"][0])
    faces, expected = _direct(orc, oscene, place, oroute["lightLength"], first, count)
    sided = gf.sided_links(orc, oscene, S2, 5, first=first, count=count).astype(np.int64)
    plain = gl.links(orc, oscene, S2, 5, first=first, count=count).astype(np.int64)
    assert np.array_equal(sided < 0, plain < 0) and np.array_equal((sided >> 1)[plain >= 0], plain[plain >= 0])
    inside = (plain >= first) & (plain < first + count)
    sided = np.where(inside, sided - 2 * first, -1)
    plain = np.where(inside, plain - first, -1)
    assert inside.sum() > 500 and (expected > 0).sum() > 200
    _check_against_two_sided(oscene.tris[first:first + count], faces, expected, sided, plain)
