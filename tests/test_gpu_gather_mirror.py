"""GPU: specular panels and the mirror gather (include/uvrt.h "specular panels").  The panels' life in both
libraries; the virtual lamp GPU against GPU -- uvrt_gather_mirror on the cube with a mirror wall against uvrt_gather_direct of the
mirrored lamp on the cube without it, in a second context, bit for bit; the edge scene with two panels against the restatement
(tests/gather_mirror_restate.py), every bit, whatever the capacity, the sampling mode, the flavour, `add` and the faces state; a
sub-range and its cut into two calls; the plates' exact zeros; the room with a panel from a rules file; every refusal with the
planes, the panels and a gather batch compared before and after; what the call leaves and forgets; RayTracer::mirrorMap and
SetMirrors through host.py over two stops and a driven segment -- behind a scene swap, with a refine in front, with sided mapped
bounces behind, gatherBatch 2 against 0 -- uvrt_cli --mirror-map and a plan's captured columns."""
import os
import subprocess

import numpy as np
import pytest

import gather_edge_scene as ge
import gather_faces_restate as gf
import gather_indirect_restate as gi
import gather_links_restate as gl
import gather_mirror_restate as gm
import gather_reflect_map_restate as grm
import gather_refine_restate as gref
import gather_restate as gr
import gather_stratified_restate as gs
from conftest import GLB, GOLDEN, ROOT, ROUTE
from sweep_restate import segment_duration

pytestmark = pytest.mark.gpu

N = 1 << 20
SEED = 7
SENTINEL = -3.25
f32 = np.float32


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def new_ctx(pkg, scene, cap, dev=False, fl=0, mode=0):
    c = pkg.capi.Ctx(0, dev=dev)
    c.set_scene(scene.tris, scene.nodes, scene.triIdx)
    c.resize_rays(cap)
    c.set_flavour(fl)
    c.set_gather_sampling(mode)
    return c


def records(pkg, panels):
    return [pkg.capi.mirror(q, m, rho) for q, m, rho in panels]


def read_faces(c, first=0, count=None):
    return np.stack([c.read_gather_faces(0, first, count), c.read_gather_faces(1, first, count)])


def write_faces(c, faces, first=0):
    c.write_gather_faces(0, faces[0], first)
    c.write_gather_faces(1, faces[1], first)


@pytest.fixture(scope="module")
def edge(orc):
    return ge.edge_scene(orc)


# ---------------------------------------------------------------- the panels' life
@pytest.mark.parametrize("dev", (False, True))
def test_the_life_of_the_panels(pkg, orc, edge, dev):
    T = edge.T
    Err = pkg.capi.UvrtError
    c = new_ctx(pkg, edge, T * 4, dev=dev)
    assert c.mirror_info() == (0, 0)
    with pytest.raises(Err, match="no panels"):
        c.read_mirrors()
    with pytest.raises(Err, match="no panels"):
        c.gather_mirror(ge.LAMP, ge.LAMP, 1.0, 4, SEED, N)
    c.drop_mirrors()                                    # nothing to do
    panels, pot = records(pkg, gm.edge_panels()), gm.edge_members(edge)
    c.set_mirrors(panels, pot)
    assert c.mirror_info() == (2, int((pot != 0).sum()))

    def unchanged(count=2):
        rec, members = c.read_mirrors()
        want = np.array(panels[:count], dtype=pkg.capi.MIRROR_DT)
        return c.mirror_info()[0] == count and same(rec, want) and same(members, pot)
    assert unchanged()
    # every other call leaves them bit for bit
    c.set_gather_faces(1)
    c.set_gather_variance(1)
    c.gather_direct(ge.LAMP, ge.SEGMENT_TO, 1.0, 4, SEED, N)
    c.gather_refine(0.5, 4, SEED + 1)
    c.fill_reflectance(0.5)
    c.indirect_links_build_sided(2, 3)
    c.gather_indirect_linked_mapped(2, add=1)
    c.gather_mirror(ge.LAMP, ge.SEGMENT_TO, 1.0, 4, SEED, N, add=1)
    c.accumulate_expected(2.0)
    c.resize_rays(T * 2)
    c.set_gather_faces(0)
    c.set_gather_variance(0)
    assert unchanged()
    # what the host refuses before anything is uploaded
    ok = panels[0]
    mk = pkg.capi.mirror
    bad_sets = (([mk((np.nan, 0, 0), (1, 0, 0), 0.5)], pot, None, "finite"), ([mk((0, 0, 0), (0, np.inf, 0), 0.5)], pot, None, "finite"),
                ([mk((0, 0, 0), (1, 0, 0), np.nan)], pot, None, "reflectance"), ([mk((0, 0, 0), (0, 0, 0), 0.5)], pot, None, "zero normal"),
                ([mk((0, 0, 0), (1, 0, 0), 1.5)], pot, None, "reflectance"), ([mk((0, 0, 0), (1, 0, 0), -0.25)], pot, None, "reflectance"),
                ([mk((0, 0, 0), (1, 0, 0), 0.5, 1)], pot, None, "reserved"), ([ok], pot, None, "names no panel"),
                ([ok, ok], np.where(pot == 2, 3, pot), None, "names no panel"), ([ok], pot, 0, "count"), ([ok] * 9, np.zeros(T, np.uint8), None, "count"),
                ([ok], pot, -1, "count"))
    for recs, members, count, why in bad_sets:
        with pytest.raises(Err, match=why):
            c.set_mirrors(recs, members, count=count)
        assert unchanged(), why
    assert c._L.uvrt_set_mirrors(c._h, None, 1, pot.ctypes.data) == -1 and c._L.uvrt_read_mirrors(c._h, None, None) == -1
    assert c._L.uvrt_mirror_info(c._h, None) == -1 and unchanged()
    # a second call replaces the first
    one = np.where(pot == 1, 1, 0).astype(np.uint8)
    c.set_mirrors(panels[1:], one)
    rec, members = c.read_mirrors()
    assert c.mirror_info() == (1, int(one.sum())) and same(rec, np.array(panels[1:], dtype=pkg.capi.MIRROR_DT)) and same(members, one)
    c.drop_mirrors()
    assert c.mirror_info() == (0, 0)
    with pytest.raises(Err, match="no panels"):
        c.gather_mirror(ge.LAMP, ge.LAMP, 1.0, 4, SEED, N)
    # uvrt_set_scene drops them
    c.set_mirrors(panels, pot)
    assert c.mirror_info()[0] == 2
    c.set_scene(edge.tris, edge.nodes, edge.triIdx)
    assert c.mirror_info() == (0, 0)
    with pytest.raises(Err, match="no panels"):
        c.read_mirrors()
    c.sync()
    c.close()
    fresh = pkg.capi.Ctx(0, dev=dev)                    # no scene
    rec = np.array(panels, dtype=pkg.capi.MIRROR_DT)
    assert fresh._L.uvrt_set_mirrors(fresh._h, rec.ctypes.data, 2, pot.ctypes.data) == -1 and b"no scene" in fresh._L.uvrt_last_error()
    assert fresh._L.uvrt_drop_mirrors(fresh._h) == -1 and fresh.mirror_info() == (0, 0)
    fresh.close()


# ---------------------------------------------------------------- the virtual lamp, GPU against GPU
@pytest.mark.parametrize("fl", (0, 1))
@pytest.mark.parametrize("mode", (0, 1))
def test_the_virtual_lamp(pkg, orc, fl, mode):
    """uvrt_gather_mirror(add = 0) on scene A (the cube, the wall x = 4 a mirror, the lamp at (1, 0.5, 2)) against uvrt_gather_direct
    on scene B (the wall taken away, the lamp at (7, 0.5, 2)) in a second context: bit for bit on triangles 0..9, whatever the
    restatement says; rho = 0.5 gives exactly half; the wall itself gets exactly 0"""
    A = ge.HandScene(orc, gi.cube_tris())
    B = ge.HandScene(orc, gm.cube_without_wall())
    for S in (4, 16):
        a = new_ctx(pkg, A, 12 * S, fl=fl, mode=mode)
        b = new_ctx(pkg, B, 12 * S, fl=fl, mode=mode)
        a.set_mirrors(records(pkg, [gm.wall_panel()]), gm.wall_members())
        a.write_expected(np.full(12, SENTINEL))
        a.gather_mirror(gm.LAMP_A, gm.LAMP_A, 1.0, S, SEED, N)
        b.gather_direct(gm.LAMP_B, gm.LAMP_B, 1.0, S, SEED, N)
        got, direct = a.read_expected(), b.read_expected()
        assert np.all(direct[:10] > 0) and same(got[:10], direct[:10]), (S, got, direct)
        assert np.all(got[10:] == 0.0) and not np.signbit(got[10:]).any()
        want, _, info = gm.gather(orc, A, [gm.wall_panel()], gm.wall_members(), gm.LAMP_A, gm.LAMP_A, 1.0, S, SEED, N, flavour=fl, mode=mode)
        assert same(got, want) and not (info[0]["lost"][:10] & (info[0]["w"][:10] > 0)).any()
        a.set_mirrors(records(pkg, [gm.wall_panel(0.5)]), gm.wall_members())
        a.gather_mirror(gm.LAMP_A, gm.LAMP_A, 1.0, S, SEED, N)
        assert same(a.read_expected()[:10], 0.5 * direct[:10])
        for c in (a, b):
            c.sync()
            c.close()


# ---------------------------------------------------------------- the edge scene with two panels
@pytest.mark.parametrize("fl", (0, 1))
@pytest.mark.parametrize("mode", (0, 1))
def test_the_edge_scene_with_two_panels(pkg, orc, edge, fl, mode):
    """S = 4 and 5, a stop and a sweep, capacity S (one triangle per chunk), 7 S + 1 (ragged chunks) and everything in one chunk, add
    0 and 1 over a real direct plane, the faces state off (`faces` keeps a sentinel) and on (both planes): the restatement's bits"""
    T = edge.T
    panels, pot = gm.edge_panels(), gm.edge_members(edge)
    for S in (4, 5):
        for frm, to in ((ge.LAMP, ge.LAMP), (ge.LAMP, ge.SEGMENT_TO)):
            dfaces, direct = gf.gather_faces(orc, edge, frm, to, 1.0, S, SEED, N, flavour=fl, mode=mode)
            want0, wantf0, info = gm.gather(orc, edge, panels, pot, frm, to, 1.0, S, SEED + 1, N, flavour=fl, mode=mode, sided=True)
            want1, wantf1, _ = gm.gather(orc, edge, panels, pot, frm, to, 1.0, S, SEED + 1, N, flavour=fl, mode=mode, sided=True,
                                         base=direct, faces_base=dfaces)
            assert (want0 > 0).sum() > 60 and all((i["m"] > 0).sum() > 30 for i in info) and np.all(want0[edge.no_area] == 0.0)
            assert any((i["lost"] & (i["w"] > 0)).sum() > 50 for i in info) and any(i["occluded"].sum() > 10 for i in info)
            for cap in (S, 7 * S + 1, T * S):
                for sided in (0, 1):
                    c = new_ctx(pkg, edge, cap, fl=fl, mode=mode)
                    c.set_mirrors(records(pkg, panels), pot)
                    c.set_gather_faces(sided)
                    where = (S, frm is to, cap, sided)
                    sentinel = np.full((2, T), SENTINEL)
                    write_faces(c, sentinel)
                    c.write_expected(np.full(T, SENTINEL))
                    c.gather_mirror(frm, to, 1.0, S, SEED + 1, N)
                    got = c.read_expected()
                    assert same(got, want0), "%r: %d entries differ" % (where, int((got != want0).sum()))
                    assert same(read_faces(c), wantf0 if sided else sentinel), where
                    # add = 1 over a real direct plane (and, with the state on, over its face planes)
                    c.gather_direct(frm, to, 1.0, S, SEED, N)
                    assert same(c.read_expected(), direct)
                    if not sided:
                        write_faces(c, sentinel)
                    c.gather_mirror(frm, to, 1.0, S, SEED + 1, N, add=1)
                    got = c.read_expected()
                    assert same(got, want1), "%r add: %d entries differ" % (where, int((got != want1).sum()))
                    assert same(read_faces(c), wantf1 if sided else sentinel), where
                    assert c.get_gather_faces() == sided
                    c.sync()
                    c.close()


def test_a_sub_range_keeps_what_lies_outside(pkg, orc, edge):
    """a sub-range that starts and ends with a hand-made triangle, in one call and cut into two: the range's entries are the whole
    scene's, the others keep a sentinel, in `expected` and in both face planes"""
    T, S = edge.T, 4
    first, count = edge.sub_range
    panels, pot = gm.edge_panels(), gm.edge_members(edge)
    want, wantf, _ = gm.gather(orc, edge, panels, pot, ge.LAMP, ge.SEGMENT_TO, 1.0, S, SEED, N, sided=True)
    part = gm.gather(orc, edge, panels, pot, ge.LAMP, ge.SEGMENT_TO, 1.0, S, SEED, N, first=first, count=count)[0]
    assert same(part, want[first:first + count])
    for cuts in (((first, count),), ((first, 61), (first + 61, count - 61))):
        c = new_ctx(pkg, edge, 7 * S + 1)
        c.set_mirrors(records(pkg, panels), pot)
        c.set_gather_faces(1)
        write_faces(c, np.full((2, T), SENTINEL))
        c.write_expected(np.full(T, SENTINEL))
        for a, n in cuts:
            c.gather_mirror(ge.LAMP, ge.SEGMENT_TO, 1.0, S, SEED, N, first_tri=a, tri_count=n)
        got, gotf = c.read_expected(), read_faces(c)
        assert same(got[first:first + count], want[first:first + count]) and same(gotf[:, first:first + count], wantf[:, first:first + count]), cuts
        assert np.all(got[:first] == SENTINEL) and np.all(got[first + count:] == SENTINEL)
        assert np.all(gotf[:, :first] == SENTINEL) and np.all(gotf[:, first + count:] == SENTINEL)
        c.sync()
        c.close()


# ---------------------------------------------------------------- the plates
def test_the_plates_exact_zeros(pkg, orc):
    """the lamp right under plate A: plate B, whose every leg A ends on A, gets exactly 0, and A and C beside it are lit; the lamp
    beside the plates with one of the wall's two triangles as the panel: the restatement's bits, below the whole wall's everywhere"""
    scene = ge.HandScene(orc, gf.plates_tris())
    A, B, Cc = (list(gf.PLATES[k]) for k in "ABC")
    under, beside = (2.0, 1.85, 2.0), (3.5, 2.8, 2.0)
    for fl in (0, 1):
        for mode in (0, 1):
            c = new_ctx(pkg, scene, 18 * 16, fl=fl, mode=mode)
            c.set_mirrors(records(pkg, [gm.wall_panel(0.9)]), gm.wall_members(18))
            c.write_expected(np.full(18, SENTINEL))
            c.gather_mirror(under, under, 0.1, 16, SEED, N)
            got = c.read_expected()
            want, _, info = gm.gather(orc, scene, [gm.wall_panel(0.9)], gm.wall_members(18), under, under, 0.1, 16, SEED, N, flavour=fl, mode=mode)
            assert same(got, want) and np.all(info[0]["w"][B] > 0)
            assert np.all(got[B] == 0.0) and not np.signbit(got[B]).any() and np.all(got[A] > 0) and np.all(got[Cc] > 0)
            c.gather_mirror(beside, beside, 0.1, 16, SEED, N)
            full = c.read_expected()
            c.set_mirrors(records(pkg, [gm.wall_panel(0.9)]), gm.wall_members(18, (10,)))
            c.gather_mirror(beside, beside, 0.1, 16, SEED, N)
            one = c.read_expected()
            want = gm.gather(orc, scene, [gm.wall_panel(0.9)], gm.wall_members(18, (10,)), beside, beside, 0.1, 16, SEED, N, flavour=fl, mode=mode)[0]
            finfo = gm.gather(orc, scene, [gm.wall_panel(0.9)], gm.wall_members(18), beside, beside, 0.1, 16, SEED, N, flavour=fl, mode=mode)[2]
            lower = ((finfo[0]["x"] > 0) & (finfo[0]["h"] == 11)).any(axis=1)       # a sample the whole wall keeps ends off the half
            assert same(one, want) and np.all(one <= full) and np.array_equal(one < full, lower) and lower.any() and (one > 0).sum() > 3
            c.sync()
            c.close()


# ---------------------------------------------------------------- the room
ROOM_RULES = "mirror 1.2 -1e30 -1e30 1e30 1e30 1e30 0.85 plane 1.47 0 0 -1 0 0   # the wall x >= 1.2 (DESIGN.md 22)\n"


@pytest.fixture(scope="module")
def place(orc, oscene, oroute):
    comp = orc.Computation(oscene, oroute["lamps"], N, oroute["lightHeight"], oroute["lightLength"], oroute["lightIntensity"])
    return comp.lamp_world_pos(oroute["lamps"][0])


@pytest.fixture(scope="module")
def room_panel(oscene):
    panels, pot = gm.rules_panels(oscene.tris, ROOM_RULES)
    assert len(panels) == 1 and 5000 < (pot == 1).sum() < 12000
    return panels, pot


def test_the_room_with_a_panel_from_a_rules_file(pkg, orc, oscene, oroute, place, room_panel, tmp_path):
    from uvrt_amd import host
    T = oscene.T
    path = tmp_path / "panel.rules"
    path.write_text(ROOM_RULES)
    recs, pot = host.parse_mirror_rules(str(path), oscene.tris)
    assert same(pot, room_panel[1])
    want, _, info = gm.gather(orc, oscene, room_panel[0], room_panel[1], place, place, oroute["lightLength"], 4, SEED, N)
    c = new_ctx(pkg, oscene, 1000 * 4 + 3)
    c.set_mirrors(recs, pot)
    c.gather_mirror(place, place, oroute["lightLength"], 4, SEED, N)
    got = c.read_expected()
    assert same(got, want), "%d entries differ" % int((got != want).sum())
    i = info[0]
    print("the room's mirror plane: %d triangles lit, sum %.6g; of %d samples with w' > 0 %d are lost off the panel, %d occluded on leg B"
          % ((got > 0).sum(), got.sum(), (i["w"] > 0).sum(), (i["lost"] & (i["w"] > 0)).sum(), i["occluded"].sum()))
    assert (got > 0).sum() > 3000
    c.sync()
    c.close()


# ---------------------------------------------------------------- refusals and state
def test_refusals_change_nothing(pkg, orc, edge):
    T = edge.T
    Err = pkg.capi.UvrtError
    c = new_ctx(pkg, edge, T * 4)
    panels, pot = records(pkg, gm.edge_panels()), gm.edge_members(edge)
    launches = [dict(frm=ge.LAMP, to=ge.LAMP, light_length=1.0, samples=4, seed=k, photons_equiv=N) for k in (3, 4)]
    c.gather_direct_batch(launches)
    batch = [c.read_gather_batch(k) for k in range(2)]
    faces = np.random.default_rng(2).uniform(0.5, 50.0, (2, T))
    write_faces(c, faces)
    c.write_expected(np.arange(T, dtype=np.float64))
    before = c.read_expected()
    with pytest.raises(Err, match="no panels"):
        c.gather_mirror(ge.LAMP, ge.LAMP, 1.0, 4, SEED, N)
    c.set_mirrors(panels, pot)
    c.set_gather_faces(1)

    def unchanged():
        rec, members = c.read_mirrors()
        return (same(c.read_expected(), before) and same(read_faces(c), faces) and same(members, pot)
                and same(rec, np.array(panels, dtype=pkg.capi.MIRROR_DT)) and c.gather_batch_info()[0] == 2
                and all(same(c.read_gather_batch(k), batch[k]) for k in range(2)))
    c.set_flavour(2)
    with pytest.raises(Err, match="flavours 0 and 1"):
        c.gather_mirror(ge.LAMP, ge.LAMP, 1.0, 4, SEED, N)
    c.set_flavour(0)
    for bad in (0, -1, 4097, T * 4 + 1):
        with pytest.raises(Err, match="samples"):
            c.gather_mirror(ge.LAMP, ge.LAMP, 1.0, bad, SEED, N)
    c.resize_rays(3)
    with pytest.raises(Err, match="capacity"):
        c.gather_mirror(ge.LAMP, ge.LAMP, 1.0, 4, SEED, N)
    c.resize_rays(T * 4)
    for bad in (0, -5):
        with pytest.raises(Err, match="photons_equiv"):
            c.gather_mirror(ge.LAMP, ge.LAMP, 1.0, 4, SEED, bad)
    for bad in (2, -1):
        with pytest.raises(Err, match="add"):
            c.gather_mirror(ge.LAMP, ge.LAMP, 1.0, 4, SEED, N, add=bad)
    for first, count in ((0, T + 1), (-1, 10), (T, 1), (5, -1)):
        with pytest.raises(Err, match="outside"):
            c.gather_mirror(ge.LAMP, ge.LAMP, 1.0, 4, SEED, N, first_tri=first, tri_count=count)
    assert c._L.uvrt_gather_mirror(c._h, None, 0, 0, 1) == -1
    assert unchanged()
    c.gather_mirror(ge.LAMP, ge.LAMP, 1.0, 4, SEED, N, first_tri=T, tri_count=0)       # an empty range at the end is a range
    c.gather_mirror(ge.LAMP, ge.LAMP, 1.0, 4, SEED, N, add=1, first_tri=0, tri_count=0)
    assert unchanged()
    c.sync()
    c.close()


def test_what_the_call_leaves_and_what_it_forgets(pkg, orc, oscene, oroute, place, room_panel):
    T, length = oscene.T, oroute["lightLength"]
    n = 1 << 14
    Err = pkg.capi.UvrtError
    c = new_ctx(pkg, oscene, T * 4)
    c.reset(True)
    c.seed = 0
    c.generate(place, length, 0, n)
    c.extend(n)
    counts, seed = c.read_counts(), c.seed
    launches = [dict(frm=place, to=place, light_length=length, samples=4, seed=k, photons_equiv=N) for k in (3, 4)]
    c.gather_direct_batch(launches, 0, 2000)
    c.set_gather_variance(1)
    c.gather_direct(place, place, length, 4, SEED, N)
    c.indirect_source_from_expected()
    c.indirect_links_build_sided(2, SEED)
    c.fill_reflectance(0.25)
    c.set_mirrors(records(pkg, room_panel[0]), room_panel[1])
    source, var, expected, lk = c.read_indirect_source(), c.read_variance(), c.read_expected(), c.read_indirect_links()
    rho = c.read_reflectance(0)
    batch = [c.read_gather_batch(k, 0, 0, 2000) for k in range(2)]
    c.gather_mirror(place, place, length, 4, SEED, N, add=1)
    want = gm.gather(orc, oscene, room_panel[0], room_panel[1], place, place, length, 4, SEED, N, base=expected)[0]
    assert same(c.read_expected(), want)
    assert c.seed == seed and np.array_equal(c.read_counts(), counts)
    assert same(c.read_indirect_source(), source) and same(c.read_variance(), var), "no variance is written"
    assert np.array_equal(c.read_indirect_links(), lk) and same(c.read_reflectance(0), rho)
    assert c.gather_batch_info()[0] == 2 and all(same(c.read_gather_batch(k, 0, 0, 2000), batch[k]) for k in range(2))
    with pytest.raises(Err, match="no remembered gather"):        # a refine cannot merge into a plane that holds specular light
        c.gather_refine(0.5, 4, SEED + 100)
    assert same(c.read_expected(), want)
    # it drops the last generate, like every shadow-ray call
    c.set_gather_variance(0)
    c.reset(True)
    c.seed = 0
    c.generate(place, length, 0, n)
    c.gather_mirror(place, place, length, 4, SEED, N)
    with pytest.raises(Err):
        c.extend(n)
    assert c.seed == seed
    c.sync()
    c.close()


# ---------------------------------------------------------------- the host layer
CLI = os.path.join(ROOT, "small-project-uv-robot-ray-tracer_amd", "uvrt_cli")
LAMPS = 2
PHOTONS = 1 << 16
S = 4           # the direct gather's samples
S2 = 2          # the bounces'
TAU, MAX_EXTRA = 0.25, 16
BASE = 0.05
LINING = "box 1.2 -1e30 -1e30 1e30 1e30 1e30 0.85\n"


def route_ends(orc, oscene, oroute):
    """(from, to, duration) of one iteration over two positions driven at 0.1 m/s: stop, stop, segment; and the computation"""
    lamps = oroute["lamps"][:LAMPS]
    comp = orc.Computation(oscene, lamps, PHOTONS, oroute["lightHeight"], oroute["lightLength"], oroute["lightIntensity"])
    ends = [(comp.lamp_world_pos(l), comp.lamp_world_pos(l), l[2]) for l in lamps]
    ends.append((comp.lamp_world_pos(lamps[0]), comp.lamp_world_pos(lamps[1]), segment_duration(lamps[0], lamps[1], 0.1)))
    return ends, comp


@pytest.fixture(scope="module")
def host_launches(orc, oscene, oroute, room_panel):
    """per launch, as RunLaunch runs it with gatherSamples = 4 (the launch counter is the seed): the direct gather's (faces,
    expected), the refined plane, what the mirror gather adds to each, and the duration"""
    ends, comp = route_ends(orc, oscene, oroute)
    out = []
    for seed, (frm, to, duration) in enumerate(ends):
        faces, expected = gf.gather_faces(orc, oscene, frm, to, comp.lightLength, S, seed, comp.photonsPerLight)
        refined = gref.gather_and_refine(orc, oscene, frm, to, comp.lightLength, S, seed, comp.photonsPerLight, 0, TAU, MAX_EXTRA)[0]
        plain, mfaces, info = gm.gather(orc, oscene, room_panel[0], room_panel[1], frm, to, comp.lightLength, S, seed, comp.photonsPerLight,
                                        base=expected, faces_base=faces, sided=True)
        out.append(dict(faces=faces, expected=expected, refined=refined, mirrored=plain, mirrored_faces=mfaces, m=info[0]["m"],
                        duration=duration))
    assert all((l["m"] > 0).sum() > 1000 for l in out)
    return out


def restated_route(orc, oscene, oroute, planes):
    """the maps after one iteration whose launches leave `planes` ((plane, duration): stop, stop, segment)"""
    lamps = oroute["lamps"][:LAMPS]
    comp = orc.Computation(oscene, lamps, PHOTONS, oroute["lightHeight"], oroute["lightLength"], oroute["lightIntensity"])
    comp.reset()
    for k, (plane, duration) in enumerate(planes):
        gr.accumulate_expected(comp.photonMap, comp.maxPhotonMap, plane, duration)
        if k < LAMPS:
            comp.photonMapSize += comp.photonsPerLight
    return comp


def run_raytracer(rules=None, panels=None, refine=False, swap=False, batch=0, bounces=0, lining=None):
    from uvrt_amd import host
    rt = host.RayTracer(GLB, ROUTE, device=0)
    rt.set_lamps(rt.lamps()[:LAMPS])
    rt.photonCount = PHOTONS
    rt.maxIterations = 1
    rt.driveSpeed = 0.1
    rt.gatherSamples = S
    rt.gatherBatch = batch
    if refine:
        rt.set_gather_refine(TAU, MAX_EXTRA)
    if bounces:
        rt.reflectance = BASE
        rt.reflectSamples = S2
        rt.reflectBounces = bounces
        rt.reflectSided = 1
        rt.reflectMap = lining
    if rules is not None:
        rt.mirrorMap = rules
    if panels is not None:
        rt.SetMirrors(*panels)
    rt.ResetDosageMap()
    rt.viewMode = host.VIEW_DOSAGE
    if swap:        # a scene swap drops the context's panels: the next launch uploads them again
        rt.ComputeSingleLightDosageMap(rt.lamps()[0], rt.photonsPerLight, rt.mesh.triangleCount)
        assert rt.ctx.mirror_info()[0] == 1
        m = rt.mesh
        rt.ctx.set_scene(m.tris(), m.nodes(), m.triIdx())
        assert rt.ctx.mirror_info() == (0, 0)
        rt.ResetDosageMap()
    rt.ComputeDosageMap()
    rt.Shade()
    rt.Sync()
    got = dict(dose=rt.read_dosage(), sum=rt.ctx.read_photon_map(0), max=rt.ctx.read_photon_map(1), seed=rt.ctx.seed, size=rt.photonMapSize,
               faces=rt.ctx.get_gather_faces(), variance=rt.ctx.get_gather_variance(), info=rt.ctx.mirror_info(),
               panels=rt.ctx.mirror_info()[0] and rt.ctx.read_mirrors())
    rt.close()
    return got


def check_route(got, comp, what):
    assert same(got["sum"], comp.photonMap) and same(got["max"], comp.maxPhotonMap) and same(got["dose"], comp.dose()), what
    assert got["seed"] == 0 and got["size"] == comp.photonMapSize and got["faces"] == 0 and got["variance"] == 0, what


def test_raytracer_and_cli_with_a_mirror_map(pkg, orc, oscene, oroute, host_launches, room_panel, tmp_path):
    """mirrorMap on gatherSamples = 4 over two stops and the drive between them: the restated route, the context's panels the
    file's; the same panels through SetMirrors, and once more behind a scene swap; gatherBatch = 2 against 0, bit for bit;
    uvrt_cli --mirror-map --dump gives host.py's dose; with no panels the route is the direct gather's, as it was"""
    rules = tmp_path / "panel.rules"
    rules.write_text(ROOM_RULES)
    comp = restated_route(orc, oscene, oroute, [(l["mirrored"], l["duration"]) for l in host_launches])
    got = run_raytracer(rules=str(rules))
    check_route(got, comp, "the file's panels")
    rec, members = got["panels"]
    assert got["info"] == (1, int((room_panel[1] != 0).sum())) and same(members, room_panel[1])
    assert same(rec, np.array(records(pkg, room_panel[0]), dtype=pkg.capi.MIRROR_DT))
    direct = run_raytracer(panels=(records(pkg, room_panel[0]), room_panel[1]))
    check_route(direct, comp, "SetMirrors")
    swapped = run_raytracer(rules=str(rules), swap=True)
    check_route(swapped, comp, "behind a scene swap")
    assert swapped["info"][0] == 1
    batched = run_raytracer(rules=str(rules), batch=2)
    check_route(batched, comp, "gatherBatch = 2")
    f = tmp_path / "dose.f32"
    cmd = [CLI, "--room", GLB, "--route-dir", GOLDEN, "--route", "lange_route", "--lamps", str(LAMPS), "--photons", str(PHOTONS),
           "--iterations", "1", "--gather", str(S), "--mirror-map", str(rules), "--drive-speed", "0.1", "--dump", str(f)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr + out.stdout
    assert np.array_equal(np.fromfile(f, dtype="<u4"), gr.bits(got["dose"])), "uvrt_cli"
    comp0 = restated_route(orc, oscene, oroute, [(l["expected"], l["duration"]) for l in host_launches])
    got0 = run_raytracer()
    check_route(got0, comp0, "no panels")
    assert got0["info"] == (0, 0) and not same(got0["dose"], got["dose"])


def test_raytracer_with_a_refine_in_front(pkg, orc, oscene, oroute, host_launches, room_panel):
    """gatherRelError = 0.25: the mirror gather is added to the refined plane"""
    comp = restated_route(orc, oscene, oroute, [(l["refined"] + l["m"], l["duration"]) for l in host_launches])
    got = run_raytracer(panels=(records(pkg, room_panel[0]), room_panel[1]), refine=True)
    check_route(got, comp, "refined")


def test_raytracer_with_sided_mapped_bounces_behind(pkg, orc, oscene, oroute, host_launches, room_panel, tmp_path):
    """reflectSided = 1 with a reflectance map: the bounces take the face planes the mirror gather has added to, so they see the
    specular light as a source"""
    K = 2
    lining = tmp_path / "lining.rules"
    lining.write_text(LINING)
    rho = grm.rules_map(oscene.tris, LINING, BASE)
    links = gf.sided_links(orc, oscene, S2, gl.LINK_SEED)
    planes = [(grm.linked(oscene.tris, l["mirrored_faces"], links, rho, K, base=l["mirrored"]), l["duration"]) for l in host_launches]
    blind = grm.linked(oscene.tris, host_launches[0]["faces"], links, rho, K, base=host_launches[0]["mirrored"])
    assert (planes[0][0] > blind).sum() > 1000, "the bounces of the specular light are there"
    comp = restated_route(orc, oscene, oroute, planes)
    got = run_raytracer(panels=(records(pkg, room_panel[0]), room_panel[1]), bounces=K, lining=str(lining))
    check_route(got, comp, "sided mapped bounces")


def test_a_plan_captures_the_mirror_gather(pkg, oscene, host_launches, room_panel, tmp_path):
    """PlanOptions::mirrorMapped: every column of the plan's exposure matrix is the restated plane of its launch"""
    from uvrt_amd import host
    rules = tmp_path / "panel.rules"
    rules.write_text(ROOM_RULES)
    rt = host.RayTracer(GLB, ROUTE, device=0)
    try:
        rt.set_lamps(rt.lamps()[:LAMPS])
        rt.photonCount = PHOTONS
        rt.maxIterations = 1
        rt.driveSpeed = 0.1
        rt.mirrorMap = str(rules)
        for batch in (0, 2):
            d, rep = rt.PlanDurationsBatched(batch, gather_samples=S, mirror_mapped=1)
            assert rep["positions"] == LAMPS + 1 and rt.gatherSamples == 0 and rt.ctx.mirror_info()[0] == 1
            for p, l in enumerate(host_launches):
                got = rt.ctx.plan_read_exposure_expected(p)
                assert same(got, l["mirrored"]), "B = %d, column %d: %d entries differ" % (batch, p, int((got != l["mirrored"]).sum()))
            rt.EndPlan()
    finally:
        rt.close()
