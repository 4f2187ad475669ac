"""GPU: the face-resolved gather and bounces (include/uvrt.h "face-resolved gather and bounces") against the
restatement (tests/gather_faces_restate.py): the direct gather's two face planes, every bit, whatever the capacity, the
sampling mode, the variance state and the cut into ranges, with `expected` and `variance` those of a context without the
state; the sided links, which are the plain links with the arrival face in bit 0; uvrt_gather_indirect_linked_sided on the
closed cube (the plain call's bits), the plates (the exact zeros an opaque sheet gives and the two-sided bounce does not), the
edge scene and the room; what the calls leave alone, the lifecycle and the refusals; RayTracer::reflectSided through host.py,
with a refine in front, through uvrt_cli --reflect-sided and through a plan."""
import os
import subprocess

import numpy as np
import pytest

import gather_edge_scene as ge
import gather_faces_restate as gf
import gather_indirect_restate as gi
import gather_links_restate as gl
import gather_refine_restate as gref
import gather_restate as gr
from conftest import GLB, GOLDEN, ROOT, ROUTE
from sweep_restate import segment_duration

pytestmark = pytest.mark.gpu

N = 1 << 20
SEED = 7
RHO = 0.1
ROOM_S2 = 16
SENTINEL = -3.25


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def new_ctx(pkg, scene, cap, dev=False):
    c = pkg.capi.Ctx(0, dev=dev)
    c.set_scene(scene.tris, scene.nodes, scene.triIdx)
    c.resize_rays(cap)
    return c


def read_faces(c, first=0, count=None):
    return np.stack([c.read_gather_faces(0, first, count), c.read_gather_faces(1, first, count)])


def write_faces(c, faces, first=0):
    c.write_gather_faces(0, faces[0], first)
    c.write_gather_faces(1, faces[1], first)


# ---------------------------------------------------------------- the direct gather's face planes
@pytest.fixture(scope="module")
def edge(orc):
    return ge.edge_scene(orc)


@pytest.mark.parametrize("fl", (0, 1))
@pytest.mark.parametrize("mode", (0, 1))
def test_face_planes_of_the_edge_scene(pkg, orc, edge, fl, mode):
    """S = 4 and 5, a stop and a sweep, the variance on and off, capacity S (one triangle per chunk), 7 S + 1 and everything in
    one chunk: both planes are the restatement's, `expected` and `variance` those of a context with the state off; where all
    visible samples lie on one face that face's entry is `expected` and the other +0.0"""
    T = edge.T
    for S in (4, 5):
        for frm, to in ((ge.LAMP, ge.LAMP), (ge.LAMP, ge.SEGMENT_TO)):
            want, want_e = gf.gather_faces(orc, edge, frm, to, 1.0, S, SEED, N, flavour=fl, mode=mode)
            assert (want[0] > 0).sum() > 20 and (want[1] > 0).sum() > 20, "both faces are lit somewhere"
            assert np.all(want[:, edge.no_area] == 0.0)
            for var in (0, 1):
                off = new_ctx(pkg, edge, T * S)
                off.set_flavour(fl)
                off.set_gather_sampling(mode)
                off.set_gather_variance(var)
                off.gather_direct(frm, to, 1.0, S, SEED, N)
                e0 = off.read_expected()
                v0 = off.read_variance() if var else None
                off.sync()
                off.close()
                assert same(e0, want_e)
                for cap in (S, 7 * S + 1, T * S):
                    c = new_ctx(pkg, edge, cap)
                    c.set_flavour(fl)
                    c.set_gather_sampling(mode)
                    c.set_gather_variance(var)
                    c.set_gather_faces(1)
                    assert c.get_gather_faces() == 1
                    c.gather_direct(frm, to, 1.0, S, SEED, N)
                    got = read_faces(c)
                    where = (S, frm is to, var, cap)
                    assert same(got, want), "%r: %d entries differ" % (where, int((got != want).sum()))
                    assert same(c.read_expected(), e0), where
                    if var:
                        assert same(c.read_variance(), v0), where
                    one = (got[0] == 0) != (got[1] == 0)          # exactly one face is lit
                    assert one.sum() > 50
                    lit = np.where(got[0] != 0, got[0], got[1])
                    assert same(lit[one], e0[one]) and not np.signbit(got[:, one]).any(), where
                    c.sync()
                    c.close()


def test_face_planes_of_a_sub_range_keep_what_lies_outside(pkg, orc, edge):
    """a sub-range that starts and ends with a hand-made triangle, in one call and cut into two: the range's entries are the whole
    scene's, the others keep a sentinel"""
    T, S = edge.T, 4
    first, count = edge.sub_range
    want, _ = gf.gather_faces(orc, edge, ge.LAMP, ge.SEGMENT_TO, 1.0, S, SEED, N)
    for cuts in (((first, count),), ((first, 61), (first + 61, count - 61))):
        c = new_ctx(pkg, edge, 7 * S + 1)
        c.set_gather_faces(1)
        write_faces(c, np.full((2, T), SENTINEL))
        for a, n in cuts:
            c.gather_direct(ge.LAMP, ge.SEGMENT_TO, 1.0, S, SEED, N, a, n)
        got = read_faces(c)
        assert same(got[:, first:first + count], want[:, first:first + count]), cuts
        assert np.all(got[:, :first] == SENTINEL) and np.all(got[:, first + count:] == SENTINEL)
        c.sync()
        c.close()


@pytest.fixture(scope="module")
def place(orc, oscene, oroute):
    comp = orc.Computation(oscene, oroute["lamps"], N, oroute["lightHeight"], oroute["lightLength"], oroute["lightIntensity"])
    return comp.lamp_world_pos(oroute["lamps"][0])


@pytest.fixture(scope="module")
def room_faces(orc, oscene, oroute, place):
    """(faces, expected) of the room at S = 4, restated once"""
    return gf.gather_faces(orc, oscene, place, place, oroute["lightLength"], 4, SEED, N)


def test_face_planes_of_the_room(pkg, oscene, oroute, place, room_faces):
    T = oscene.T
    want, want_e = room_faces
    c = new_ctx(pkg, oscene, 1000 * 4 + 3)
    c.set_gather_faces(1)
    c.gather_direct(place, place, oroute["lightLength"], 4, SEED, N)
    got = read_faces(c)
    assert same(got, want), "%d entries differ" % int((got != want).sum())
    assert same(c.read_expected(), want_e)
    both = (got[0] > 0) & (got[1] > 0)
    print("the room's direct plane: face 0 %.6g, face 1 %.6g, %d triangles lit on both faces" % (got[0].sum(), got[1].sum(), both.sum()))
    assert (got[0] > 0).sum() > 5000
    c.sync()
    c.close()


# ---------------------------------------------------------------- sided links
def check_sided_against_plain(sided, plain):
    assert np.array_equal(sided < 0, plain < 0) and np.all(sided[sided < 0] == -1)
    assert np.array_equal((sided >> 1)[plain >= 0], plain[plain >= 0])


@pytest.mark.parametrize("fl", (0, 1))
def test_sided_links_of_the_closed_cube(pkg, orc, fl):
    """S2 = 2, 4, 64: the restatement's values; >> 1 is the plain build of a second context; every link arrives on the inner face"""
    cube = ge.HandScene(orc, gi.cube_tris())
    inner = gf.inner_face(cube.tris, (gi.CUBE_SIDE / 2,) * 3)
    c = new_ctx(pkg, cube, 12 * 64)
    p = new_ctx(pkg, cube, 12 * 64)
    for x in (c, p):
        x.set_flavour(fl)
    for s2 in (2, 4, 64):
        want = gf.sided_links(orc, cube, s2, 7, flavour=fl)
        c.indirect_links_build_sided(s2, 7)
        p.indirect_links_build(s2, 7)
        got, plain = c.read_indirect_links(), p.read_indirect_links()
        assert got.shape == (12, s2) and np.array_equal(got, want), s2
        check_sided_against_plain(got, plain)
        assert np.array_equal((got & 1)[got >= 0], inner[got[got >= 0] >> 1])
        assert c.indirect_links_info() == (s2, 7, fl) and c.indirect_links_kind() == 1 and p.indirect_links_kind() == 0
    for x in (c, p):
        x.sync()
        x.close()


def test_sided_links_of_the_edge_scene(pkg, orc, edge):
    """capacity 4 S2 + 1: many chunks of four triangles and a ragged last one"""
    s2 = 4
    want = gf.sided_links(orc, edge, s2, 11)
    assert edge.T % 4 != 0 and ((want >= 0) & (want & 1 == 0)).sum() > 30 and ((want >= 0) & (want & 1 == 1)).sum() > 30
    for dev in (False, True):
        c = new_ctx(pkg, edge, 4 * s2 + 1, dev=dev)
        c.indirect_links_build_sided(s2, 11)
        got = c.read_indirect_links()
        assert np.array_equal(got, want), "%d links differ" % int((got != want).sum())
        first, count = edge.sub_range
        assert np.array_equal(c.read_indirect_links(first, count), want[first:first + count])
        check_sided_against_plain(got, gl.links(orc, edge, s2, 11))
        c.sync()
        c.close()


@pytest.fixture(scope="module")
def room_sided(orc, oscene):
    return gf.sided_links(orc, oscene, ROOM_S2, SEED)


def test_sided_links_of_the_room(pkg, oscene, room_sided):
    T = oscene.T
    c = new_ctx(pkg, oscene, 1000 * ROOM_S2 + 3)
    c.indirect_links_build_sided(ROOM_S2, SEED)
    got = c.read_indirect_links()
    assert np.array_equal(got, room_sided), "%d links differ" % int((got != room_sided).sum())
    c.indirect_links_build(ROOM_S2, SEED)
    check_sided_against_plain(got, c.read_indirect_links())
    c.sync()
    c.close()


def test_one_link_set_and_each_gather_refuses_the_other_kind(pkg, orc):
    cube = ge.HandScene(orc, gi.cube_tris())
    Err = pkg.capi.UvrtError
    c = new_ctx(pkg, cube, 12 * 8)
    assert c.indirect_links_kind() == 0
    with pytest.raises(Err, match="no links"):
        c.gather_indirect_linked_sided(RHO, 1)
    base = np.arange(12, dtype=np.float64) + 1.0
    faces = np.arange(24, dtype=np.float64).reshape(2, 12) + 100.0
    c.write_expected(base)
    write_faces(c, faces)
    c.indirect_links_build_sided(4, 3)
    sided = c.read_indirect_links()
    assert c.indirect_links_info() == (4, 3, 0) and c.indirect_links_kind() == 1
    with pytest.raises(Err, match="sided"):
        c.gather_indirect_linked(RHO, 1)
    assert same(c.read_expected(), base) and same(read_faces(c), faces) and np.array_equal(c.read_indirect_links(), sided)
    c.indirect_links_build(8, 5)                        # plain replaces sided
    assert c.indirect_links_info() == (8, 5, 0) and c.indirect_links_kind() == 0
    assert np.array_equal(c.read_indirect_links(), gl.links(orc, cube, 8, 5))
    with pytest.raises(Err, match="plain"):
        c.gather_indirect_linked_sided(RHO, 1)
    assert same(c.read_expected(), base) and same(read_faces(c), faces)
    c.gather_indirect_linked(RHO, 1)
    c.indirect_links_build_sided(4, 3)                  # ... and back
    assert c.indirect_links_kind() == 1 and np.array_equal(c.read_indirect_links(), sided)
    for bad in (0, 1, 3, -2, 4098):                     # the plain build's refusals, the links kept
        with pytest.raises(Err, match="samples"):
            c.indirect_links_build_sided(bad, 1)
    prm = pkg.capi.LinksParams(4, 1)
    prm.reserved[0] = 1
    L = pkg.capi.lib()
    assert L.uvrt_indirect_links_build_sided(c._h, pkg.capi.C.byref(prm)) == -1 and b"reserved" in L.uvrt_last_error()
    c.set_flavour(2)
    with pytest.raises(Err, match="flavours 0 and 1"):
        c.indirect_links_build_sided(4, 1)
    c.set_flavour(0)
    assert c.indirect_links_kind() == 1 and np.array_equal(c.read_indirect_links(), sided)
    c.set_scene(cube.tris, cube.nodes, cube.triIdx)
    assert c.indirect_links_info() == (0, 0, 0) and c.indirect_links_kind() == 0, "uvrt_set_scene drops the links"
    c.sync()
    c.close()


# ---------------------------------------------------------------- the face-resolved linked gather
@pytest.mark.parametrize("fl", (0, 1))
def test_the_closed_cube_is_the_plain_call_bit_for_bit(pkg, orc, fl):
    """source on the inner faces, 0 on the outer ones: no light crosses a sheet, so the sided call gives the plain call's bits,
    GPU against GPU, for K = 1, 2, 5 and both `add`"""
    cube = ge.HandScene(orc, gi.cube_tris())
    source = 0.5 * gl.normals(cube.tris) * np.random.default_rng(5).uniform(1.0, 1000.0, 12)
    base = np.random.default_rng(1).uniform(0.0, 100.0, 12)
    faces = gf.cube_faces(source)
    c = new_ctx(pkg, cube, 12 * 64)
    p = new_ctx(pkg, cube, 12 * 64)
    for x in (c, p):
        x.set_flavour(fl)
    p.write_indirect_source(source)
    write_faces(c, faces)
    for s2 in (2, 4, 64):
        c.indirect_links_build_sided(s2, 7)
        p.indirect_links_build(s2, 7)
        lk = c.read_indirect_links()
        for K in (1, 2, 5):
            for add in (0, 1):
                for x in (c, p):
                    x.write_expected(base)
                c.gather_indirect_linked_sided(0.25, K, add=add)
                p.gather_indirect_linked(0.25, K, add=add)
                got = c.read_expected()
                assert same(got, p.read_expected()), (s2, K, add)
                assert same(got, gf.linked(cube.tris, faces, lk, 0.25, K, base=base if add else None)), (s2, K, add)
        assert same(read_faces(c), faces)
    for x in (c, p):
        x.sync()
        x.close()


def test_the_plates_shade_what_the_two_sided_bounce_lights(pkg, orc):
    """only A's face towards B emits.  One sided bounce: both triangles of C get exactly 0, B gets more than 0; the plain call
    over the same plane lights C from A's dark side"""
    scene = ge.HandScene(orc, gf.plates_tris())
    faces = gf.plates_faces()
    A, B, Cc = (list(gf.PLATES[k]) for k in "ABC")
    for s2 in (16, 64):         # (eight samples a face: every triangle of B and C sees A at least once)
        c = new_ctx(pkg, scene, 18 * 64)
        write_faces(c, faces)
        c.write_expected(np.full(18, SENTINEL))
        c.indirect_links_build_sided(s2, 3)
        lk = c.read_indirect_links()
        assert np.array_equal(lk, gf.sided_links(orc, scene, s2, 3))
        c.gather_indirect_linked_sided(1.0, 1)
        got = c.read_expected()
        assert same(got, gf.linked(scene.tris, faces, lk, 1.0, 1))
        assert np.all(got[Cc] == 0.0) and not np.signbit(got[Cc]).any(), got[Cc]
        assert np.all(got[B] > 0.0) and np.all(got[A] == 0.0)
        g, _ = gf.bounces(scene.tris, faces, lk, 1.0, 1)
        assert np.all(g[0][0, B] == 0.0) and same(g[0][1, B], got[B]), "B's face away from A stays dark"
        c.write_indirect_source(faces[0] + faces[1])
        c.indirect_links_build(s2, 3)
        c.gather_indirect_linked(1.0, 1)
        plain = c.read_expected()
        assert np.all(plain[Cc] > 0.0) and same(plain[B], got[B]), "the two-sided bounce"
        c.sync()
        c.close()


def test_the_edge_scene_against_the_restatement(pkg, orc, edge):
    """S2 = 2 and 4 (the tail loop alone), 18 and 22 (two groups of the unroll and a tail of one and three pairs), 64; K = 1, 3, 16;
    add = 1; a range cut into two calls is one call; a triangle without area gets 0"""
    T = edge.T
    faces = np.random.default_rng(2).uniform(0.5, 50.0, (2, T))
    base = np.random.default_rng(3).uniform(0.0, 10.0, T)
    first, count = edge.sub_range
    for s2 in (2, 4, 18, 22, 64):
        c = new_ctx(pkg, edge, 4 * s2 + 1)
        write_faces(c, faces)
        c.indirect_links_build_sided(s2, 11)
        lk = c.read_indirect_links()
        assert np.array_equal(lk, gf.sided_links(orc, edge, s2, 11)), s2
        for K in (1, 3, 16):
            want = gf.linked(edge.tris, faces, lk, 0.5, K, base=base)
            c.write_expected(base)
            c.gather_indirect_linked_sided(0.5, K, add=1)
            one = c.read_expected()
            assert same(one, want), "S2 = %d, K = %d: %d entries differ" % (s2, K, int((one != want).sum()))
            assert same(one[edge.no_area], base[edge.no_area]), "a triangle without area gets 0"
            c.write_expected(base)
            c.gather_indirect_linked_sided(0.5, K, add=1, first_tri=first, tri_count=100)
            c.gather_indirect_linked_sided(0.5, K, add=1, first_tri=first + 100, tri_count=count - 100)
            two = c.read_expected()
            assert same(two[first:first + count], want[first:first + count]) and same(two[:first], base[:first]), (s2, K)
            assert same(two[first + count:], base[first + count:])
        assert same(read_faces(c), faces)
        c.sync()
        c.close()


def test_the_room_against_the_restatement(pkg, oscene, oroute, place, room_faces, room_sided):
    """S2 = 16, K = 3 over the face planes of a direct gather at S = 4"""
    T = oscene.T
    c = new_ctx(pkg, oscene, T * ROOM_S2)
    c.set_gather_faces(1)
    c.gather_direct(place, place, oroute["lightLength"], 4, SEED, N)
    direct = c.read_expected()
    c.indirect_links_build_sided(ROOM_S2, SEED)
    c.gather_indirect_linked_sided(0.8, 3, add=1)
    got = c.read_expected()
    want = gf.linked(oscene.tris, room_faces[0], room_sided, 0.8, 3, base=direct)
    assert same(got, want), "%d entries differ" % int((got != want).sum())
    assert ((direct == 0) & (got > 0)).sum() > 1000
    c.gather_indirect_linked_sided(0.8, 3, add=0, first_tri=0, tri_count=777)
    c.gather_indirect_linked_sided(0.8, 3, add=0, first_tri=777, tri_count=T - 777)
    assert same(c.read_expected(), gf.linked(oscene.tris, room_faces[0], room_sided, 0.8, 3)), "two ranges"
    c.sync()
    c.close()


def test_links_of_flavour_1_serve_in_flavours_0_and_2(pkg, orc, edge):
    T = edge.T
    faces = np.random.default_rng(4).uniform(0.5, 50.0, (2, T))
    c = new_ctx(pkg, edge, T * 4)
    write_faces(c, faces)
    c.set_flavour(1)
    c.indirect_links_build_sided(4, 9)
    lk = c.read_indirect_links()
    want = gf.linked(edge.tris, faces, lk, 0.5, 2)
    for fl in (1, 0, 2):
        c.set_flavour(fl)
        c.gather_indirect_linked_sided(0.5, 2)
        assert same(c.read_expected(), want), fl
        assert c.indirect_links_info() == (4, 9, 1) and c.indirect_links_kind() == 1
    c.sync()
    c.close()


# ---------------------------------------------------------------- state
def test_what_the_calls_leave_and_what_they_forget(pkg, oscene, oroute, place):
    T, length = oscene.T, oroute["lightLength"]
    n = 1 << 14
    Err = pkg.capi.UvrtError
    c = new_ctx(pkg, oscene, T * 4)
    c.reset(True)
    c.seed = 0
    c.generate(place, length, 0, n)
    c.extend(n)
    counts, seed = c.read_counts(), c.seed
    c.set_gather_variance(1)
    c.set_gather_faces(1)
    c.gather_direct(place, place, length, 4, SEED, N)
    assert c.seed == seed and np.array_equal(c.read_counts(), counts)
    c.indirect_source_from_expected()
    source, var, expected, faces = c.read_indirect_source(), c.read_variance(), c.read_expected(), read_faces(c)
    assert faces.any() and var.any()
    c.indirect_links_build_sided(4, SEED)
    assert c.seed == seed and np.array_equal(c.read_counts(), counts)
    assert same(c.read_indirect_source(), source) and same(c.read_variance(), var) and same(c.read_expected(), expected)
    assert same(read_faces(c), faces)
    with pytest.raises(Err, match="last generate"):               # the build drops the last generate
        c.extend(n)
    lk = c.read_indirect_links()
    extra, refined = c.gather_refine(0.5, 4, SEED + 100)          # the build leaves the remembered gather; the refine the planes
    assert refined > 0 and same(read_faces(c), faces), "after a refine the face planes describe the first pass"
    refined_e, refined_v = c.read_expected(), c.read_variance()
    c.gather_indirect_linked_sided(RHO, 2, add=1)
    assert c.seed == seed and np.array_equal(c.read_counts(), counts)
    assert same(c.read_indirect_source(), source) and same(c.read_variance(), refined_v) and same(read_faces(c), faces)
    assert np.array_equal(c.read_indirect_links(), lk)
    assert same(c.read_expected(), gf.linked(oscene.tris, faces, lk, RHO, 2, base=refined_e))
    c.gather_direct(place, place, length, 4, SEED, N)
    c.gather_indirect_linked_sided(RHO, 1)
    with pytest.raises(Err, match="no remembered gather"):        # the sided gather forgets it, as the plain one does
        c.gather_refine(0.5, 4, SEED + 100)
    for call in (lambda: c.gather_indirect(RHO, 4, SEED), lambda: c.write_expected(expected),
                 lambda: c.write_indirect_source(source)):
        call()
        assert same(read_faces(c), faces)
    # the sided gather leaves the last generate: generate -> sided gather -> extend counts what generate -> extend counts
    c.reset(True)
    c.seed = 0
    c.generate(place, length, 0, n)
    c.gather_indirect_linked_sided(RHO, 2)
    c.extend(n)
    assert np.array_equal(c.read_counts(), counts) and c.seed == seed
    # uvrt_accumulate_expected zeroes the face planes of the triangles it consumes
    c.accumulate_expected(1.0, 1000)
    after = read_faces(c)
    assert np.all(after[:, :1000] == 0.0) and same(after[:, 1000:], faces[:, 1000:]) and faces[:, :1000].any()
    # the state is the context's; the planes are the scene's
    c.set_scene(oscene.tris, oscene.nodes, oscene.triIdx)
    assert c.get_gather_faces() == 1 and not read_faces(c).any(), "uvrt_set_scene zeroes the planes and keeps the state"
    c.sync()
    c.close()


def test_the_state_off_makes_no_plane_and_the_batch_refuses_the_state(pkg, orc, edge):
    T, S = edge.T, 4
    Err = pkg.capi.UvrtError
    c = new_ctx(pkg, edge, T * S)
    assert c.get_gather_faces() == 0
    for bad in (2, -1):
        with pytest.raises(Err, match="uvrt_set_gather_faces"):
            c.set_gather_faces(bad)
    assert c.get_gather_faces() == 0
    c.gather_direct(ge.LAMP, ge.LAMP, 1.0, S, SEED, N)
    assert not read_faces(c).any(), "with the state off the planes, made by the read, are zero"
    launches = [dict(frm=ge.LAMP, to=ge.LAMP, light_length=1.0, samples=S, seed=SEED + k, photons_equiv=N) for k in range(2)]
    c.gather_direct_batch(launches)
    info, planes = c.gather_batch_info(), [c.read_gather_batch(k) for k in range(2)]
    c.set_gather_faces(1)
    c.gather_direct(ge.LAMP, ge.LAMP, 1.0, S, SEED, N)
    faces, expected = read_faces(c), c.read_expected()
    assert faces.any()
    with pytest.raises(Err, match="face planes"):
        c.gather_direct_batch(launches[:1])
    assert c.gather_batch_info() == info and all(same(c.read_gather_batch(k), planes[k]) for k in range(2)), "the earlier batch is kept"
    assert same(read_faces(c), faces) and same(c.read_expected(), expected)
    c.gather_batch_select(1)
    assert same(read_faces(c), faces) and same(c.read_expected(), planes[1])
    with pytest.raises(Err, match="0..8"):
        c.device_ptr(9)
    c.sync()
    c.close()


def test_refusals_change_nothing(pkg, orc, edge):
    T = edge.T
    Err = pkg.capi.UvrtError
    c = new_ctx(pkg, edge, T * 4)
    faces = np.random.default_rng(2).uniform(0.5, 50.0, (2, T))
    write_faces(c, faces)
    c.indirect_links_build_sided(4, 11)
    c.gather_indirect_linked_sided(0.5, 2)
    before = c.read_expected()
    assert before.any()
    lk = c.read_indirect_links()
    buf = np.zeros(T + 1)
    for first, count in ((0, T + 1), (-1, 10), (T, 1), (5, -1)):
        with pytest.raises(Err, match="outside"):
            c.gather_indirect_linked_sided(0.5, 2, 0, first, count)
        for f in (0, 1):
            with pytest.raises(Err, match="outside"):
                c.read_gather_faces(f, first, count)
        if count > 0:
            with pytest.raises(Err, match="outside"):
                c.write_gather_faces(0, buf[:count], first)
    for f in (2, -1):
        with pytest.raises(Err, match="face must be"):
            c.read_gather_faces(f)
        with pytest.raises(Err, match="face must be"):
            c.write_gather_faces(f, buf[:T])
    for bad in (0, -1, 17, 1 << 20):
        with pytest.raises(Err, match="bounces"):
            c.gather_indirect_linked_sided(0.5, bad)
    for bad in (-0.1, 1.5, float("nan"), float("inf")):
        with pytest.raises(Err, match="reflectance"):
            c.gather_indirect_linked_sided(bad, 2)
    for bad in (2, -1):
        with pytest.raises(Err, match="add"):
            c.gather_indirect_linked_sided(0.5, 2, add=bad)
    L = pkg.capi.lib()
    for k in range(3):
        prm = pkg.capi.LinkedParams(0.5, 2, 0)
        prm.reserved[k] = 1
        assert L.uvrt_gather_indirect_linked_sided(c._h, pkg.capi.C.byref(prm), 0, 16) == -1 and b"reserved" in L.uvrt_last_error()
    assert L.uvrt_gather_indirect_linked_sided(c._h, None, 0, 1) == -1
    assert L.uvrt_read_gather_faces(c._h, 0, None, 0, 1) == -1 and L.uvrt_write_gather_faces(c._h, 0, None, 0, 1) == -1
    assert same(c.read_expected(), before) and same(read_faces(c), faces) and np.array_equal(c.read_indirect_links(), lk)
    c.gather_indirect_linked_sided(0.5, 2, 0, T, 0)     # an empty range at the end is a range
    c.gather_indirect_linked_sided(1.0, 16, 0, 0, 0)
    assert same(c.read_expected(), before) and same(read_faces(c), faces)
    c.sync()
    c.close()
    bare = pkg.capi.Ctx(0)
    for call in (lambda: bare.indirect_links_build_sided(4, 1), lambda: bare.gather_indirect_linked_sided(RHO, 1, 0, 0, 0),
                 lambda: bare.read_gather_faces(0, 0, 0), lambda: bare.write_gather_faces(0, buf[:1])):
        with pytest.raises(Err, match="no scene"):
            call()
    bare.set_gather_faces(1)                            # a property of the context: no scene, no device work
    assert bare.get_gather_faces() == 1
    bare.close()


# ---------------------------------------------------------------- the host layer
CLI = os.path.join(ROOT, "small-project-uv-robot-ray-tracer_amd", "uvrt_cli")
LAMPS = 2
PHOTONS = 1 << 16
S = 4           # the direct gather's samples
S2 = 2          # the bounce's
TAU, MAX_EXTRA = 0.25, 16


def route_ends(orc, oscene, oroute):
    """(from, to, duration) of one iteration over two positions driven at 0.1 m/s: stop, stop, segment; and the computation"""
    lamps = oroute["lamps"][:LAMPS]
    comp = orc.Computation(oscene, lamps, PHOTONS, oroute["lightHeight"], oroute["lightLength"], oroute["lightIntensity"])
    ends = [(comp.lamp_world_pos(l), comp.lamp_world_pos(l), l[2]) for l in lamps]
    ends.append((comp.lamp_world_pos(lamps[0]), comp.lamp_world_pos(lamps[1]), segment_duration(lamps[0], lamps[1], 0.1)))
    return ends, comp


@pytest.fixture(scope="module")
def host_directs(orc, oscene, oroute):
    """per launch (faces, expected, duration) as RunLaunch gathers them with gatherSamples = 4: the launch counter is the seed"""
    ends, comp = route_ends(orc, oscene, oroute)
    out = []
    for seed, (frm, to, duration) in enumerate(ends):
        faces, expected = gf.gather_faces(orc, oscene, frm, to, comp.lightLength, S, seed, comp.photonsPerLight)
        out.append((faces, expected, duration))
    return out


@pytest.fixture(scope="module")
def host_refined(orc, oscene, oroute):
    """per launch the refined expected plane of gatherRelError = 0.25, gatherMaxExtra = 16 (refine seed ~seed)"""
    ends, comp = route_ends(orc, oscene, oroute)
    return [gref.gather_and_refine(orc, oscene, frm, to, comp.lightLength, S, seed, comp.photonsPerLight, 0, TAU, MAX_EXTRA)[0]
            for seed, (frm, to, _) in enumerate(ends)]


@pytest.fixture(scope="module")
def host_sided_links(orc, oscene):
    return gf.sided_links(orc, oscene, S2, gl.LINK_SEED)


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


def run_raytracer(K, sided, rho, refine=False):
    from uvrt_amd import host
    rt = host.RayTracer(GLB, ROUTE, device=0)
    rt.set_lamps(rt.lamps()[:LAMPS])
    rt.photonCount = PHOTONS
    rt.maxIterations = 1
    rt.driveSpeed = 0.1
    rt.gatherSamples = S
    if refine:
        rt.set_gather_refine(TAU, MAX_EXTRA)
    rt.reflectance = rho
    rt.reflectSamples = S2
    rt.reflectBounces = K
    rt.reflectSided = sided
    rt.ResetDosageMap()
    rt.viewMode = host.VIEW_DOSAGE
    rt.ComputeDosageMap()
    rt.Shade()
    rt.Sync()
    got = (rt.read_dosage(), rt.ctx.read_photon_map(0), rt.ctx.read_photon_map(1), rt.ctx.seed, rt.photonMapSize,
           rt.ctx.indirect_links_info(), rt.ctx.indirect_links_kind(), rt.ctx.get_gather_faces(), rt.ctx.get_gather_variance())
    rt.close()
    return got


def test_raytracer_and_cli_sided_bounces(pkg, orc, oscene, oroute, host_directs, host_sided_links, tmp_path):
    """reflectSided on gatherSamples = 4, reflectance = 0.8, reflectSamples = 2, reflectBounces = 3 over two stops and the drive
    between them: the restated route, the context's faces state put back; uvrt_cli --reflect-sided --dump gives host.py's dose;
    reflectSided = 0 is the two-sided route, bit for bit"""
    rho, K = 0.8, 3
    comp = restated_route(orc, oscene, oroute, [(gf.linked(oscene.tris, f, host_sided_links, rho, K, base=e), t)
                                                for f, e, t in host_directs])
    got = run_raytracer(K, 1, rho)
    assert same(got[1], comp.photonMap) and same(got[2], comp.maxPhotonMap)
    assert same(got[0], comp.dose())
    assert got[3] == 0 and got[4] == comp.photonMapSize and got[5] == (S2, gl.LINK_SEED, 0) and got[6] == 1 and got[7] == 0
    f = tmp_path / "dose.f32"
    cmd = [CLI, "--room", GLB, "--route-dir", GOLDEN, "--route", "lange_route", "--lamps", str(LAMPS), "--photons", str(PHOTONS),
           "--iterations", "1", "--gather", str(S), "--reflect", "%g,%d" % (rho, S2), "--reflect-bounces", str(K), "--reflect-sided",
           "--drive-speed", "0.1", "--dump", str(f)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr + out.stdout
    assert np.array_equal(np.fromfile(f, dtype="<u4"), gr.bits(got[0])), "uvrt_cli"
    plain_links = gl.links(orc, oscene, S2, gl.LINK_SEED)
    comp0 = restated_route(orc, oscene, oroute, [(gl.linked(oscene.tris, e, plain_links, rho, K, base=e), t) for _, e, t in host_directs])
    got0 = run_raytracer(K, 0, rho)
    assert same(got0[0], comp0.dose()) and same(got0[1], comp0.photonMap) and got0[6] == 0
    assert not same(got0[0], got[0])


def test_raytracer_sided_bounces_after_a_refine(pkg, orc, oscene, oroute, host_directs, host_refined, host_sided_links):
    """gatherRelError = 0.25 in front: the bounces take the first pass's face planes and are added to the refined plane"""
    rho, K = 0.5, 2
    comp = restated_route(orc, oscene, oroute, [(gf.linked(oscene.tris, f, host_sided_links, rho, K, base=r), t)
                                                for (f, _, t), r in zip(host_directs, host_refined)])
    got = run_raytracer(K, 1, rho, refine=True)
    assert same(got[1], comp.photonMap) and same(got[2], comp.maxPhotonMap) and same(got[0], comp.dose())
    assert got[7] == 0 and got[8] == 0, "both states are put back"


def test_a_plan_captures_the_sided_bounces(pkg, oscene, host_directs, host_sided_links):
    """PlanOptions::reflectSided with reflectBounces = 2: every column of the plan's exposure matrix is the restated plane of its
    launch"""
    from uvrt_amd import host
    rt = host.RayTracer(GLB, ROUTE, device=0)
    try:
        rt.set_lamps(rt.lamps()[:LAMPS])
        rt.photonCount = PHOTONS
        rt.maxIterations = 1
        rt.driveSpeed = 0.1
        d, rep = rt.PlanDurationsReflect(0.8, S2, gather_samples=S, reflect_bounces=2, reflect_sided=1)
        assert rep["positions"] == LAMPS + 1 and rt.reflectance == 0.0 and rt.reflectBounces == 0 and rt.reflectSided == 0
        assert rt.ctx.indirect_links_kind() == 1 and rt.ctx.get_gather_faces() == 0
        for p, (faces, expected, _) in enumerate(host_directs):
            want = gf.linked(oscene.tris, faces, host_sided_links, 0.8, 2, base=expected)
            got = rt.ctx.plan_read_exposure_expected(p)
            assert same(got, want), "column %d: %d entries differ" % (p, int((got != want).sum()))
        rt.EndPlan()
    finally:
        rt.close()
    assert d.size == LAMPS and d.sum() > 0
