"""No GPU: the host-only parts of the specular panels (include/uvrt.h "specular panels") -- the symbols in both
libraries, the header and the bindings, uvrt_mirror as a C compiler lays it out, null arguments, the rules file through
libuvrt_host.so against its Python restatement (hand-made triangles, the room, every parse error), route files with and without
<mirror_map>, the binding's and the CLI's refusals -- and the restatement (tests/gather_mirror_restate.py) against itself: the
virtual lamp first (the mirror plane of the cube equals the direct gather of the mirrored lamp in the cube without its mirror
wall, bit for bit), then wrong sides, blockers on the plates scene, a mirror point off the panel, monotony in rho, two panels
and the face planes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gather_edge_scene as ges
import gather_faces_restate as gf
import gather_indirect_restate as gi
import gather_mirror_restate as gm
import gather_restate as gr
import gather_stratified_restate as gs
from conftest import GLB, GOLDEN, ROOT

NEW = ("uvrt_set_mirrors", "uvrt_mirror_info", "uvrt_read_mirrors", "uvrt_drop_mirrors", "uvrt_gather_mirror")
N = 1 << 20
SEED = 7
f32 = np.float32


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def test_symbols_are_bound_and_resolve_in_both_libraries(pkg):
    names = [name for name, _, _ in pkg.capi.SYMBOLS]
    header = open(os.path.join(ROOT, "include", "uvrt.h")).read()
    assert "specular panels" in header and "} uvrt_mirror;" in header and "#define UVRT_MIRROR_MAX 8" in header
    for n in NEW:
        assert names.count(n) == 1
        assert ("int %s(uvrt_ctx* ctx" % n) in header
        for path in (pkg.capi.LIB_PATH, pkg.capi.LIB_DEV_PATH):
            assert hasattr(C.CDLL(path), n), (path, n)
        for dev in (False, True):
            assert getattr(pkg.capi.lib(dev), n).restype is C.c_int
    by_name = {n: a for n, _, a in pkg.capi.SYMBOLS}
    assert [len(by_name[n]) for n in NEW] == [4, 2, 3, 1, 5]
    for m in ("set_mirrors", "mirror_info", "read_mirrors", "drop_mirrors", "gather_mirror"):
        assert hasattr(pkg.capi.Ctx, m)
    assert pkg.capi.MIRROR_MAX == gm.MIRROR_MAX == 8
    from uvrt_amd import host
    for m in ("mirrorMap", "SetMirrors"):
        assert hasattr(host.RayTracer, m)
    assert hasattr(host, "parse_mirror_rules") and hasattr(C.CDLL(host.LIB_PATH), "uvrt_host_mirror_rules")


def test_mirror_record_matches_the_header(pkg, tmp_path):
    fields = ("point", "normal", "reflectance", "reserved")
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "uvrt.h"\nint main(void){printf("%zu'
                   + " %zu" * len(fields) + ' %d\\n", sizeof(uvrt_mirror)'
                   + "".join(", offsetof(uvrt_mirror, %s)" % f for f in fields) + ", UVRT_MIRROR_MAX);return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    dt = pkg.capi.MIRROR_DT
    assert got == [dt.itemsize] + [dt.fields[f][1] for f in fields] + [pkg.capi.MIRROR_MAX] == [32, 0, 12, 24, 28, 8]
    rec = np.array([pkg.capi.mirror((1, 2, 3), (0, 0, -1), 0.5)], dtype=dt)
    assert np.frombuffer(rec.tobytes(), dtype=f32)[:7].tolist() == [1, 2, 3, 0, 0, -1, 0.5] and rec["reserved"][0] == 0


def test_null_arguments_are_refused_without_a_gpu(pkg):
    rec = np.array([pkg.capi.mirror((0, 0, 0), (1, 0, 0), 0.5)], dtype=pkg.capi.MIRROR_DT)
    pot = np.full(16, 1, dtype=np.uint8)
    info = np.full(4, 5, dtype=np.int32)
    prm = pkg.capi.GatherParams()
    prm.samples, prm.photons_equiv = 4, 100
    for dev in (False, True):
        L = pkg.capi.lib(dev)
        calls = (("uvrt_set_mirrors", lambda: L.uvrt_set_mirrors(None, rec.ctypes.data, 1, pot.ctypes.data)),
                 ("uvrt_set_mirrors", lambda: L.uvrt_set_mirrors(None, None, 1, None)),
                 ("uvrt_mirror_info", lambda: L.uvrt_mirror_info(None, info.ctypes.data)),
                 ("uvrt_mirror_info", lambda: L.uvrt_mirror_info(None, None)),
                 ("uvrt_read_mirrors", lambda: L.uvrt_read_mirrors(None, rec.ctypes.data, pot.ctypes.data)),
                 ("uvrt_read_mirrors", lambda: L.uvrt_read_mirrors(None, None, None)),
                 ("uvrt_drop_mirrors", lambda: L.uvrt_drop_mirrors(None)),
                 ("uvrt_gather_mirror", lambda: L.uvrt_gather_mirror(None, C.byref(prm), 0, 0, 4)),
                 ("uvrt_gather_mirror", lambda: L.uvrt_gather_mirror(None, None, 0, 0, 4)))
        for name, call in calls:
            assert call() == -1 and name.encode() in L.uvrt_last_error(), name          # UVRT_ERR_INVALID
    assert np.all(pot == 1) and np.all(info == 5) and rec["reflectance"][0] == f32(0.5)


# ---------------------------------------------------------------- the rules file
def _tri(v0, v1, v2):
    row = np.zeros(16, dtype=f32)
    row[0:3], row[4:7], row[8:11] = v0, v1, v2
    return row


def _hand_tris(orc):
    """four triangles: one whose centroid has x = 1 exactly (a box face), two in one box, one far away"""
    rows = np.stack([_tri((0.5, 0, 0), (1.5, 0, 0), (1.0, 0, 3.0)),
                     _tri((4, 1, 4), (5, 1, 4), (4, 1, 5)),
                     _tri((4, 1, 4), (4, 1, 5), (5, 1, 4)),
                     _tri((9, 9, 9), (9, 9, 8), (8, 9, 9))])
    return np.array(ges.HandScene(orc, rows).tris)


def _both(host, tmp_path, tris, text, name="mirror.rules"):
    path = tmp_path / name
    path.write_text(text)
    panels, members = host.parse_mirror_rules(str(path), tris)
    want_p, want_m = gm.rules_panels(tris, text)
    assert members.dtype == np.uint8 and bits_equal(members, want_m), (text, members, want_m)
    assert len(panels) == len(want_p)
    for got, (q, m, rho) in zip(panels, want_p):
        assert bits_equal(got["point"], np.array(q, dtype=f32)) and bits_equal(got["normal"], np.array(m, dtype=f32))
        assert bits_equal(got["reflectance"], f32(rho)) and got["reserved"] == 0
    return panels, members


PLANE = " plane 1 0 0 -1 0 0"


def test_rules_on_hand_made_triangles(pkg, orc, tmp_path):
    from uvrt_amd import host
    tris = _hand_tris(orc)
    cx = tris[0, 12]
    assert tris[0, 12:15].tolist() == [f32(3.0) * f32(0.3333), 0.0, f32(3.0) * f32(0.3333)]
    # the closed box: a centroid on its face is inside, one ulp outside it is not
    _, m = _both(host, tmp_path, tris, "mirror %r -1 -1 7 1 2 0.5%s\n" % (float(cx), PLANE))
    assert m.tolist() == [1, 0, 0, 0]
    _, m = _both(host, tmp_path, tris, "mirror %r -1 -1 7 1 2 0.5%s\n" % (float(np.nextafter(cx, f32(9))), PLANE))
    assert m.tolist() == [0, 0, 0, 0]
    _, m = _both(host, tmp_path, tris, "mirror -1 -1 -1 %r 1 7 0.5%s\n" % (float(cx), PLANE))
    assert m.tolist() == [1, 0, 0, 0]
    # every line is a panel, a later line takes a triangle over; comments, blank lines, tabs
    text = ("# two panels\n\nmirror -1e30 -1e30 -1e30 1e30 1e30 1e30 0.25 plane 0 0 0 0 2 0   # everything\n"
            "\tmirror 3 0 3 6 3 6 1 plane 4 1 4 0.5 0 -0.5\nmirror 100 100 100 101 101 101 0 plane 1 2 3 0 0 1e-30 # no member\n")
    p, m = _both(host, tmp_path, tris, text)
    assert m.tolist() == [1, 2, 2, 1] and len(p) == 3 and p["reflectance"].tolist() == [0.25, 1.0, 0.0]
    assert p["normal"][0].tolist() == [0, 2, 0], "the normal is kept as it is written: the context normalises"
    p, m = _both(host, tmp_path, tris, "")
    assert len(p) == 0 and not m.any()
    eight = "".join("mirror 0 0 0 1 1 1 0.5 plane %d 0 0 1 0 0\n" % k for k in range(8))
    p, m = _both(host, tmp_path, tris, eight)
    assert len(p) == 8 and p["point"][:, 0].tolist() == list(range(8))


BOX = "mirror 0 0 0 1 1 1 "
BAD_RULES = (
    ("box 0 0 0 1 1 1 0.5\n", 1, "keyword"),
    (BOX + "0.5" + PLANE + "\n" + BOX + "0.5 plane 0 0 0 1 0\n", 2, "mirror takes"),
    ("\n# c\n" + BOX + "0.5" + PLANE + " 1\n", 3, "mirror takes"),
    (BOX + "0.5 plain 0 0 0 1 0 0\n", 1, "mirror takes"),
    (BOX + "0.5\n", 1, "mirror takes"),
    ("mirror 0 0 0 1 1 x 0.5" + PLANE + "\n", 1, "number"),
    (BOX + "0.5 plane 0 0 0 1 0 y\n", 1, "number"),
    (BOX + "0.5 plane 0 inf 0 1 0 0\n", 1, "number"),
    (BOX + "0.5 plane 0 0 0 1 nan 0\n", 1, "number"),
    (BOX + "1.5" + PLANE + "\n", 1, "RHO"),
    (BOX + "-0.25" + PLANE + "\n", 1, "RHO"),
    (BOX + "inf" + PLANE + "\n", 1, "RHO"),
    (BOX + "nan" + PLANE + "\n", 1, "number"),
    (BOX + "0.5 plane 1 2 3 0 0 0\n", 1, "normal"),
    (BOX + "0.5 plane 1 2 3 0 -0 0\n", 1, "normal"),
    (BOX + "0.5" + PLANE + "\n" + BOX + "0.5" + PLANE + "\nmirror 2 0 0 1 1 1 0.5" + PLANE + "\n", 3, "lower bound"),
    ((BOX + "0.5" + PLANE + "\n") * 8 + "# still eight\n" + BOX + "0.5" + PLANE + "\n", 10, "ninth"),
)


def test_every_parse_error_names_the_file_and_the_line(pkg, orc, tmp_path):
    from uvrt_amd import host
    tris = _hand_tris(orc)
    for k, (text, line, why) in enumerate(BAD_RULES):
        path = tmp_path / ("bad%d.txt" % k)
        path.write_text(text)
        with pytest.raises(ValueError, match=why) as e:
            host.parse_mirror_rules(str(path), tris)
        assert str(e.value).startswith("%s:%d: " % (path, line)), (text, str(e.value))
        with pytest.raises(gm.RulesError, match=why) as e:
            gm.rules_panels(tris, text, name=str(path))
        assert str(e.value).startswith("%s:%d: " % (path, line)), (text, str(e.value))
    with pytest.raises(ValueError, match="cannot be read"):
        host.parse_mirror_rules(str(tmp_path / "absent.txt"), tris)


ROOM_RULES = """mirror 1.2 -1e30 -1e30 1e30 1e30 1e30 0.85 plane 1.47 0 0 -1 0 0     # the wall x >= 1.2
mirror -1e30 1.25 -1e30 1e30 1e30 1e30 0.5 plane 0 1.3 0 0 -1 0            # the ceiling takes its part of that wall over
"""


def test_rules_on_the_room(pkg, oscene, tmp_path):
    from uvrt_amd import host
    mesh = host.Mesh(GLB)
    tris = mesh.tris()
    mesh.close()
    assert bits_equal(tris, oscene.tris), "the host's triangles and centroids are the oracle's"
    p, m = _both(host, tmp_path, tris, ROOM_RULES)
    high = tris[:, 13] >= f32(1.25)
    assert len(p) == 2 and int((m == 2).sum()) == int(high.sum()) > 0
    assert int((m == 1).sum()) == int(((tris[:, 12] >= f32(1.2)) & ~high).sum()) > 100
    assert ((tris[:, 12] >= f32(1.2)) & high).sum() > 0, "the second line takes triangles over"


# ---------------------------------------------------------------- the route file, the binding, the CLI
def test_route_file_keeps_the_mirror_map(pkg, tmp_path):
    """<mirror_map>FILE</mirror_map> is written only when a file is named, as the last gather tag (right before <lamp_lengte>);
    every file written without it is byte for byte what it was; an absent tag loads as none"""
    from uvrt_amd import host
    golden = open(os.path.join(GOLDEN, "lange_route.xml"), "rb").read()
    rt = host.RayTracer(init=False)
    rt.set_route_dir(GOLDEN + os.sep)
    rt.LoadRoute("lange_route")
    assert rt.mirrorMap == ""
    rt.set_route_dir(str(tmp_path) + os.sep)
    rt.SaveRoute("photons")
    assert (tmp_path / "photons.xml").read_bytes() == golden
    rt.gatherSamples = 16
    rt.reflectance = 0.125
    rt.reflectSamples = 8
    rt.reflectBounces = 3
    rt.reflectSided = 1
    rt.reflectMap = "lining.rules"
    rt.SaveRoute("diffuse")
    diffuse = (tmp_path / "diffuse.xml").read_bytes()
    assert b"mirror_map" not in diffuse
    rt.mirrorMap = "panels.rules"
    assert rt.mirrorMap == "panels.rules"
    rt.SaveRoute("mirrored")
    mirrored = (tmp_path / "mirrored.xml").read_bytes()
    tag = b"    <mirror_map>panels.rules</mirror_map>\n"
    before, after = b"    <reflect_map>lining.rules</reflect_map>\n", b"    <lamp_lengte>"
    assert mirrored.count(tag) == 1 and mirrored.replace(tag, b"") == diffuse
    assert mirrored.index(before) + len(before) == mirrored.index(tag) and mirrored.index(tag) + len(tag) == mirrored.index(after)
    rt2 = host.RayTracer(init=False)
    rt2.set_route_dir(str(tmp_path) + os.sep)
    rt2.LoadRoute("mirrored")
    assert rt2.mirrorMap == "panels.rules" and rt2.reflectMap == "lining.rules" and rt2.gatherSamples == 16 and rt2.lamps() == rt.lamps()
    rt2.SaveRoute("again")
    assert (tmp_path / "again.xml").read_bytes() == mirrored
    rt2.LoadRoute("diffuse")                    # absent: none
    assert rt2.mirrorMap == ""
    rt2.SaveRoute("diffuse2")
    assert (tmp_path / "diffuse2.xml").read_bytes() == diffuse
    rt.reflectance = 0.0                        # without the diffuse tags the tag follows the gather's own
    rt.SaveRoute("plain")
    plain = (tmp_path / "plain.xml").read_bytes()
    assert plain.index(b"<gather_samples>16</gather_samples>\n") + len(b"<gather_samples>16</gather_samples>\n") == plain.index(tag)
    rt.mirrorMap = ""
    rt.gatherSamples = 0
    rt.SaveRoute("photons2")
    assert (tmp_path / "photons2.xml").read_bytes() == golden
    for bad in ("a&b.rules", "a<b", "b>a"):         # a name that would break the file
        with pytest.raises(ValueError, match="route file"):
            rt.mirrorMap = bad
    assert rt.mirrorMap == ""
    rt.close(); rt2.close()


def test_the_binding_refuses_panels_it_cannot_use(pkg):
    from uvrt_amd import host
    rt = host.RayTracer(init=False)
    ok = pkg.capi.mirror((4, 0, 0), (-1, 0, 0), 0.5)
    try:
        for bad, why in ((pkg.capi.mirror((np.nan, 0, 0), (1, 0, 0), 0.5), "finite"), (pkg.capi.mirror((0, 0, 0), (np.inf, 0, 0), 0.5), "finite"),
                         (pkg.capi.mirror((0, 0, 0), (1, 0, 0), 1.5), r"\[0, 1\]"), (pkg.capi.mirror((0, 0, 0), (1, 0, 0), -0.5), r"\[0, 1\]"),
                         (pkg.capi.mirror((0, 0, 0), (1, 0, 0), 0.5, 1), "reserved"), (pkg.capi.mirror((0, 0, 0), (0, 0, 0), 0.5), "normal")):
            with pytest.raises(ValueError, match=why):
                rt.SetMirrors([bad], np.ones(3, dtype=np.uint8))
        with pytest.raises(ValueError, match="1 to 8"):
            rt.SetMirrors([ok] * 9, np.ones(3, dtype=np.uint8))
        with pytest.raises(ValueError, match="1 to 8"):
            rt.SetMirrors([], np.zeros(3, dtype=np.uint8))
        with pytest.raises(ValueError, match="not there"):
            rt.SetMirrors([ok], np.array([0, 2, 1], dtype=np.uint8))
        assert not rt._has_mirrors()
        rt.SetMirrors([ok], np.array([0, 1, 1], dtype=np.uint8))
        assert rt._has_mirrors()
        for call in (rt.ComputeDosageMap, rt.ComputeSegments, lambda: rt.ComputeSingleLightDosageMap((0, 0, 1), 16, 3),
                     lambda: rt.ComputeSegmentDosageMap((0, 0), (1, 1), 16, 3)):
            with pytest.raises(ValueError, match="gatherSamples"):       # panels without the direct gather
                call()
        rt.gatherSamples = 4                            # no mesh: an error of the binding's, with panels and with a file
        with pytest.raises(ValueError, match="need a mesh"):
            rt.ComputeDosageMap()
        rt.SetMirrors(None)
        assert not rt._has_mirrors()
        rt.mirrorMap = "panels.rules"
        assert rt._has_mirrors()
        with pytest.raises(ValueError, match="need a mesh"):
            rt.ComputeDosageMap()
        rt.mirrorMap = ""
        assert not rt._has_mirrors()
        for k in (-1, 2, 0.5):
            with pytest.raises(ValueError, match="mirror_mapped"):
                rt.PlanDurationsBatched(0, min_dose=0.1, gather_samples=16, mirror_mapped=k)
        with pytest.raises(ValueError, match="specular panels"):
            rt.PlanDurationsBatched(0, min_dose=0.1, gather_samples=16, mirror_mapped=1)
        rt.SetMirrors([ok], np.array([0, 1, 1], dtype=np.uint8))
        with pytest.raises(ValueError, match="gather_samples"):
            rt.PlanDurationsBatched(0, min_dose=0.1, mirror_mapped=1)
        with pytest.raises(ValueError, match="gather_confidence"):
            rt.PlanDurationsBatched(0, min_dose=0.1, gather_samples=16, gather_confidence=2.0, mirror_mapped=1)
        with pytest.raises(ValueError, match="gather_confidence"):
            rt.PlanDurationsRefined(0.1, min_dose=0.1, gather_samples=16, gather_confidence=2.0, mirror_mapped=1)
    finally:
        rt.close()


def test_cli_refuses_a_mirror_map_it_cannot_use(pkg, tmp_path):
    cli = os.path.join(os.path.dirname(pkg.capi.LIB_PATH), "uvrt_cli")
    rules = tmp_path / "m.rules"
    rules.write_text("mirror 0 0 0 1 1 1 0.5 plane 0 0 0 1 0 0\n")
    base = [cli, "--room", GLB, "--route-dir", GOLDEN, "--route", "lange_route"]
    for extra in (["--mirror-map", str(rules)], ["--plan", "--mirror-map", str(rules)], ["--gather", "0", "--mirror-map", str(rules)]):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "--mirror-map" in r.stderr and "--gather" in r.stderr, (extra, r.stdout, r.stderr)
    r = subprocess.run(base + ["--plan-gather", "16", "--plan-confidence", "2", "--mirror-map", str(rules)], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 2 and "--mirror-map" in r.stderr and "--plan-confidence" in r.stderr, r.stderr
    r = subprocess.run(base + ["--gather", "16", "--mirror-map", "a&b"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--mirror-map" in r.stderr
    r = subprocess.run(base + ["--gather", "16", "--mirror-map"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "missing value" in r.stderr


# ---------------------------------------------------------------- the restatement against itself: the virtual lamp first
@pytest.fixture(scope="module")
def cube_a(orc):
    return ges.HandScene(orc, gi.cube_tris())


@pytest.fixture(scope="module")
def cube_b(orc):
    return ges.HandScene(orc, gm.cube_without_wall())


def check_virtual_lamp_conditions(info, occ_b, S):
    """what the identity needs of the seed, shown by the restatement itself: no sample of triangles 0..9 has d_p = 0, and none with
    w' > 0 is lost or occluded in A or occluded in B"""
    i = info[0]
    lit = i["w"][:10] > 0
    assert not (i["d_p"][:10] == 0).any() and lit.sum() > 5 * S
    assert not (i["lost"][:10] & lit).any() and not (i["occluded"][:10] & lit).any()
    assert not (occ_b.reshape(12, S)[:10][lit] != 0).any()


@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("S", (4, 16))
def test_the_virtual_lamp(orc, cube_a, cube_b, S, mode):
    """Scene A: the closed cube, panel 0 = the plane x = 4 with normal (-1, 0, 0) and rho = 1, members the wall's two triangles, the
    lamp at (1, 0.5, 2).  Scene B: the same twelve records with that wall collapsed to a point outside, the lamp at (7, 0.5, 2).
    Every coordinate is dyadic, so the mirroring is exact in f32: the mirror plane of A over triangles 0..9 is the direct gather of B
    bit for bit, and with rho = 0.5 exactly half of it.  The wall itself gets exactly 0: d_p = 0 there."""
    e, _, info = gm.gather(orc, cube_a, [gm.wall_panel()], gm.wall_members(), gm.LAMP_A, gm.LAMP_A, 1.0, S, SEED, N, mode=mode)
    direct, _, occ_b = gs.gather(orc, cube_b, gm.LAMP_B, gm.LAMP_B, 1.0, S, SEED, N, mode=mode)
    check_virtual_lamp_conditions(info, occ_b, S)
    assert np.all(e[:10] > 0) and bits_equal(e[:10], direct[:10])
    assert np.all(e[10:] == 0.0) and not np.signbit(e[10:]).any() and np.all(direct[10:] == 0.0)
    half, _, _ = gm.gather(orc, cube_a, [gm.wall_panel(0.5)], gm.wall_members(), gm.LAMP_A, gm.LAMP_A, 1.0, S, SEED, N, mode=mode)
    assert bits_equal(half, 0.5 * e)
    # add = 1 over a plane, and a sub-range
    base = np.linspace(1.0, 2.0, 12)
    added, _, _ = gm.gather(orc, cube_a, [gm.wall_panel()], gm.wall_members(), gm.LAMP_A, gm.LAMP_A, 1.0, S, SEED, N, mode=mode, base=base)
    assert bits_equal(added, base + e)
    part, _, _ = gm.gather(orc, cube_a, [gm.wall_panel()], gm.wall_members(), gm.LAMP_A, gm.LAMP_A, 1.0, S, SEED, N, mode=mode, first=3, count=5)
    assert bits_equal(part, e[3:8])


def test_the_lamp_behind_the_plane_lights_nothing(orc, cube_a):
    """the normal flipped: the lamp and every receiver are behind the panel, no sample is traced, the plane is all +0.0"""
    for mode in (0, 1):
        e, f, info = gm.gather(orc, cube_a, [gm.wall_panel(1.0, (1.0, 0.0, 0.0))], gm.wall_members(), gm.LAMP_A, gm.LAMP_A, 1.0, 16, SEED, N,
                               mode=mode, sided=True)
        assert np.all(e == 0.0) and not np.signbit(e).any() and np.all(f == 0.0)
        assert not info[0]["front"].any() and not info[0]["traced"].any()
    # the receiver alone behind it: a plane through the middle of the cube that faces the lamp's half
    e, _, info = gm.gather(orc, cube_a, [gm.panel((2.0, 0, 0), (-1, 0, 0), 1.0)], gm.wall_members(), gm.LAMP_A, gm.LAMP_A, 1.0, 16, SEED, N)
    behind = info[0]["d_p"] <= 0
    assert behind.any() and (~behind).any() and np.all(info[0]["w"][behind] == 0.0)


# ---------------------------------------------------------------- blockers, on the plates scene with the wall x = 4 as the mirror
@pytest.fixture(scope="module")
def plates(orc):
    return ges.HandScene(orc, gf.plates_tris())


PLATE_A, PLATE_B, PLATE_C = (list(gf.PLATES[k]) for k in "ABC")
UNDER_A = (2.0, 1.85, 2.0)          # a lamp of 0.1 m right under plate A (y = 2), in the middle of the plates
BESIDE = (3.5, 2.8, 2.0)            # a lamp of 0.1 m between the plates' edge x = 3 and the mirror wall


def test_a_plate_between_the_lamp_and_the_mirror(orc, plates):
    """The lamp stands right under plate A.  A path to plate B (y = 3) climbs: leg A would cross y = 2 at x = 2 + (2 - y_o)(6 - p_x) /
    (3 - y_o) <= 2 + 0.15 * 5 / 1.05 < 3, inside A's footprint [1, 3], for every lamp height in [1.85, 1.95] and every p_x in [1, 3] (z
    stays within [1, 3] as well: it moves from 2 towards p_z).  So every sample of B has w' > 0, its leg A ends on A instead of the
    panel, and B gets exactly 0.  A (reached from below, under y = 2 all the way) and C (reached from above, over y = 1 all the way)
    lie beside it and are lit."""
    for mode in (0, 1):
        e, _, info = gm.gather(orc, plates, [gm.wall_panel(0.9)], gm.wall_members(18), UNDER_A, UNDER_A, 0.1, 16, SEED, N, mode=mode)
        i = info[0]
        assert np.all(i["w"][PLATE_B] > 0) and i["lost"][PLATE_B].all() and i["off"][PLATE_B].all()
        assert set(i["h"][PLATE_B].ravel().tolist()) <= set(PLATE_A), "leg A ends on plate A"
        assert np.all(e[PLATE_B] == 0.0) and not np.signbit(e[PLATE_B]).any()
        assert np.all(e[PLATE_A] > 0) and np.all(e[PLATE_C] > 0)


def _crosses_a_plate(P, p, margin=0.02):
    """of the segments P -> p (f64 [n, 3]): (blocked, clear) bool[n] by plain geometry -- the segment crosses the plane of a plate it
    does not end on, well inside its length, well inside the plate's square / well outside it or not at all; neither: too close to
    an edge to call"""
    n = P.shape[0]
    blocked, unsure = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    for y in gf.PLATE_Y.values():
        with np.errstate(all="ignore"):
            s = (y - P[:, 1]) / (p[:, 1] - P[:, 1])
        ends_here = p[:, 1] == y
        with np.errstate(all="ignore"):
            x = P[:, 0] + s * (p[:, 0] - P[:, 0])
            z = P[:, 2] + s * (p[:, 2] - P[:, 2])
        inside = (x > gf.PLATE_LO + margin) & (x < gf.PLATE_HI - margin) & (z > gf.PLATE_LO + margin) & (z < gf.PLATE_HI - margin)
        outside = (x < gf.PLATE_LO - margin) | (x > gf.PLATE_HI + margin) | (z < gf.PLATE_LO - margin) | (z > gf.PLATE_HI + margin)
        within = (s > margin) & (s < 1 - margin) & ~ends_here
        never = ~np.isfinite(s) | (s < -margin) | (s > 1 + margin) | ends_here
        blocked |= within & inside
        unsure |= ~never & ~(within & (inside | outside))
    return blocked, ~blocked & ~unsure


def test_a_plate_between_the_mirror_and_a_receiver(orc, plates):
    """The lamp stands between the plates' edge and the mirror wall, so leg A meets no plate: no lit sample is lost.  Leg B then runs
    from the wall to the receiver, and plain geometry (the crossing of each plate's plane, in f64, with a margin at the edges) says
    which samples a plate shadows: those weigh exactly 0, the samples beside them their full w', and a triangle's entry is the
    reduction of exactly those.  (A whole triangle cannot be shadowed this way: the plates share one footprint and the image stands
    outside it, so the edge of a plate that faces the wall always sees it.  Whole triangles go dark in the test above.)"""
    S = 64
    for mode in (0, 1):
        e, _, info = gm.gather(orc, plates, [gm.wall_panel(0.9)], gm.wall_members(18), BESIDE, BESIDE, 0.1, S, SEED, N, mode=mode)
        i = info[0]
        lit = i["w"] > 0
        assert lit[:10].all() and lit[12:].all() and not (i["lost"] & lit).any()
        p, o, _, _ = gm.points(plates.tris, BESIDE, BESIDE, 0.1, S, SEED, mode=mode)
        p, o = p.astype(np.float64), o.astype(np.float64)
        image = o.copy()
        image[:, 0] = 2 * gi.CUBE_SIDE - o[:, 0]
        tau = (gi.CUBE_SIDE - o[:, 0]) / ((gi.CUBE_SIDE - o[:, 0]) + (gi.CUBE_SIDE - p[:, 0]))
        P = image + tau[:, None] * (p - image)
        blocked, clear = (m.reshape(18, S) for m in _crosses_a_plate(P, p))
        assert (blocked & lit).sum() > 100 and (clear & lit).sum() > 500 and (blocked | clear).mean() > 0.9
        assert np.all(i["x"][blocked] == 0.0) and i["occluded"][blocked & lit].all()
        assert bits_equal(i["x"][clear], i["w"][clear]) and not i["occluded"][clear].any()
        both = (blocked & lit).any(axis=1) & (clear & lit).any(axis=1)
        assert both[PLATE_A].any() or both[PLATE_B].any() or both[PLATE_C].any()
        sure = (blocked | clear).all(axis=1)
        assert sure.sum() >= 6
        want = gr.reduce(plates.tris, i["w"].reshape(-1), blocked.reshape(-1).astype(np.uint8), S, N)
        assert bits_equal(e[sure], want[sure])


def test_a_mirror_point_off_the_panel(orc, plates):
    """members = one of the wall's two triangles: exactly the samples whose leg A ends on the other one weigh 0, every other sample
    keeps its bits"""
    for mode in (0, 1):
        full, _, fi = gm.gather(orc, plates, [gm.wall_panel(0.9)], gm.wall_members(18), BESIDE, BESIDE, 0.1, 16, SEED, N, mode=mode)
        one, _, oi = gm.gather(orc, plates, [gm.wall_panel(0.9)], gm.wall_members(18, (10,)), BESIDE, BESIDE, 0.1, 16, SEED, N, mode=mode)
        other = fi[0]["h"] == 11
        assert (other & (fi[0]["x"] > 0)).sum() > 20 and ((fi[0]["h"] == 10) & (fi[0]["x"] > 0)).sum() > 20
        assert bits_equal(fi[0]["h"], oi[0]["h"])
        assert np.all(oi[0]["x"][other] == 0.0) and oi[0]["off"][other].all() and bits_equal(oi[0]["x"][~other], fi[0]["x"][~other])
        assert np.all(one <= full) and (one < full).any() and (one > 0).any()


# ---------------------------------------------------------------- monotone, two panels, faces
@pytest.fixture(scope="module")
def edge(orc):
    return ges.edge_scene(orc)


def test_raising_a_reflectance_lowers_no_entry(orc, edge, cube_a):
    """exact: w' = rho * w and every later operation is monotone on non-negative values"""
    pot = gm.edge_members(edge)
    lo = gm.gather(orc, edge, gm.edge_panels(0.3, 0.5), pot, ges.LAMP, ges.SEGMENT_TO, 1.0, 5, SEED, N)[0]
    hi = gm.gather(orc, edge, gm.edge_panels(0.6, 0.5), pot, ges.LAMP, ges.SEGMENT_TO, 1.0, 5, SEED, N)[0]
    top = gm.gather(orc, edge, gm.edge_panels(0.6, 1.0), pot, ges.LAMP, ges.SEGMENT_TO, 1.0, 5, SEED, N)[0]
    assert np.all(hi >= lo) and (hi > lo).sum() > 30 and np.all(top >= hi) and (top > hi).sum() > 30
    dark = gm.gather(orc, edge, gm.edge_panels(0.0, 0.0), pot, ges.LAMP, ges.SEGMENT_TO, 1.0, 5, SEED, N)[0]
    assert np.all(dark == 0.0) and not np.signbit(dark).any()


def test_two_panels_add_in_panel_order(orc, edge):
    """the plane is m_0 + m_1 in that order, each what its panel gives alone; with add = 1 (base + m_0) + m_1"""
    pot = gm.edge_members(edge)
    panels = gm.edge_panels()
    for mode, (frm, to) in ((0, (ges.LAMP, ges.LAMP)), (1, (ges.LAMP, ges.SEGMENT_TO))):
        e, _, info = gm.gather(orc, edge, panels, pot, frm, to, 1.0, 4, SEED, N, mode=mode)
        m0 = gm.gather(orc, edge, panels[:1], np.where(pot == 1, 1, 0), frm, to, 1.0, 4, SEED, N, mode=mode)[0]
        m1 = gm.gather(orc, edge, panels[1:], np.where(pot == 2, 1, 0), frm, to, 1.0, 4, SEED, N, mode=mode)[0]
        assert (m0 > 0).sum() > 40 and (m1 > 0).sum() > 40 and ((m0 > 0) & (m1 > 0)).sum() > 10
        assert bits_equal(info[0]["m"], m0) and bits_equal(info[1]["m"], m1) and bits_equal(e, m0 + m1)
        assert np.all(e[edge.no_area] == 0.0)
        base = np.random.default_rng(3).uniform(0.0, 50.0, edge.T)
        added = gm.gather(orc, edge, panels, pot, frm, to, 1.0, 4, SEED, N, mode=mode, base=base)[0]
        assert bits_equal(added, (base + m0) + m1)


def test_the_face_planes_split_the_plane(orc, edge, plates):
    """f0 + f1 is the plane within 1e-12 relative: the two sums visit the samples the one sum visits, at most 4 096 f64 roundings
    each; where all kept samples lie on one face that face's entry is the plane's, bit for bit"""
    pot = gm.edge_members(edge)
    for scene, panels, members, frm, to, length in ((edge, gm.edge_panels(), pot, ges.LAMP, ges.SEGMENT_TO, 1.0),
                                                    (plates, [gm.wall_panel(0.9)], gm.wall_members(18), BESIDE, BESIDE, 0.1)):
        e, f, info = gm.gather(orc, scene, panels, members, frm, to, length, 16, SEED, N, sided=True)
        assert f.shape == (2, scene.T) and (e > 0).sum() > 10
        assert np.all(np.abs((f[0] + f[1]) - e) <= 1e-12 * e) and np.array_equal((f[0] + f[1]) > 0, e > 0)
        one = (f[0] == 0) != (f[1] == 0)
        if len(panels) == 1:
            assert one.sum() > 5 and bits_equal(np.where(f[0] != 0, f[0], f[1])[one], e[one])
        fb = np.random.default_rng(4).uniform(0.0, 9.0, (2, scene.T))
        _, f2, _ = gm.gather(orc, scene, panels, members, frm, to, length, 16, SEED, N, sided=True, faces_base=fb)
        first = gm.gather(orc, scene, panels[:1], np.where(members == 1, 1, 0), frm, to, length, 16, SEED, N, sided=True)[1]
        if len(panels) == 1:
            assert bits_equal(f2, fb + first)
