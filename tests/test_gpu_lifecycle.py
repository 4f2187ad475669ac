"""GPU: a context can be destroyed in every state it can be in (uvrt_ctx.h: the context, its lanes, its batch sets and the
plan own their buffers, streams and events; uvrt_destroy waits for every stream and deletes).  A context is brought to a
stage and closed; a fresh context with the same SEED then traces one launch, and its tempPhotonMap must equal, bit for bit,
that of a first context nothing came before.  The last stage keeps the loaded context and swaps its scene instead.
Test room (44 866 triangles), 16 384 photons per launch: the smallest launch that builds a hot-record renumbering."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 16384
SEED = 12345
f32 = np.float32


@pytest.fixture(scope="module")
def lamps(orc, oscene, oroute):
    comp = orc.Computation(oscene, oroute["lamps"][:2], N, oroute["lightHeight"], oroute["lightLength"],
                           oroute["lightIntensity"])
    return [tuple(float(x) for x in comp.lamp_world_pos(l)) for l in oroute["lamps"][:2]]


def _launch(c, lamps, oroute):
    c.reset(True)
    c.seed = SEED
    c.generate(lamps[0], oroute["lightLength"], 0, N)
    c.extend(N)
    c.sync()
    return c.read_counts()


def _fresh_launch(pkg, oscene, oroute, lamps):
    c = pkg.capi.Ctx(0)
    try:
        c.set_scene(oscene.tris, oscene.nodes, oscene.triIdx)
        c.resize_rays(N)
        return _launch(c, lamps, oroute)
    finally:
        c.close()


@pytest.fixture(scope="module")
def first_counts(pkg, oscene, oroute, lamps):
    counts = _fresh_launch(pkg, oscene, oroute, lamps)
    assert counts.sum() > 0
    return counts


# ---- the steps, each on top of the ones before it
def _scene(c, pkg, oscene, oroute, lamps):
    c.set_scene(oscene.tris, oscene.nodes, oscene.triIdx)
    c.resize_rays(N)
    c.reset(True)


def _extended(c, pkg, oscene, oroute, lamps):
    c.generate(lamps[0], oroute["lightLength"], 0, N)
    c.extend(N)


def _deferred(c, pkg, oscene, oroute, lamps):
    c.accumulate(1.0)                                   # all triangles: deferred until the next call (PendingAcc)


def _timed(c, pkg, oscene, oroute, lamps):
    c.set_timing(True)
    for k in range(3):                                  # over both launch lanes; the last accumulate stays deferred
        c.generate(lamps[k % 2], oroute["lightLength"], 0, N)
        c.extend(N)
        c.accumulate(1.0)


def _batch(c, pkg, oscene, oroute, lamps):
    a, b = lamps
    up = (a[0], a[1] + 0.25, a[2])                      # a second stop on a's lamp column
    c.trace_batch_launches([pkg.capi.stop(a), pkg.capi.stop(up), pkg.capi.sweep(a, b)], oroute["lightLength"], 0, N)


def _captured(c, pkg, oscene, oroute, lamps):
    c.fold_batch()
    c.plan_begin(2)
    c.plan_capture_batch([0, 0, 1])


def _solved(c, pkg, oscene, oroute, lamps):
    s = f32(f32(oroute["lightIntensity"]) * f32(0.1))
    d, rep = c.plan_solve(100.0, s, N)
    assert rep["required"] > 0 and d.sum() > 0
    d, rep, brep = c.plan_solve_bounded(100.0, s, N, lower=[0.5, 1.0], fixed=[0, 1])
    assert brep["fixed_columns"] == 1 and d[1] == f32(1.0)
    c.plan_model_dose(d)


def _gathered(c, pkg, oscene, oroute, lamps):
    c.plan_begin_expected(1)
    c.gather_direct(lamps[0], lamps[1], oroute["lightLength"], 4, 7, N, 0, 256)
    c.plan_capture_expected(0)


STEPS = [_scene, _extended, _deferred, _timed, _batch, _captured, _solved, _gathered]
STAGES = ["created"] + [f.__name__[1:] for f in STEPS]


@pytest.mark.parametrize("stage", range(len(STAGES)), ids=STAGES)
def test_destroy_at_stage(pkg, oscene, oroute, lamps, first_counts, stage):
    c = pkg.capi.Ctx(0)
    try:
        for step in STEPS[:stage]:
            step(c, pkg, oscene, oroute, lamps)
    finally:
        c.close()
    assert np.array_equal(_fresh_launch(pkg, oscene, oroute, lamps), first_counts)


def test_scene_swap_with_everything_live(pkg, orc, oscene, oroute, lamps, first_counts):
    """every step on one context, then CalibratePower's detour: a 2-triangle scene and the room again"""
    tris = np.zeros((2, 16), dtype=np.float32)
    h, d, w = f32(-0.5), f32(1.0), f32(0.1)
    tris[0, 0:3] = (w, h + w, d); tris[0, 4:7] = (-w, h + w, d); tris[0, 8:11] = (w, h - w, d)
    tris[1, 0:3] = (-w, h - w, d); tris[1, 4:7] = (-w, h + w, d); tris[1, 8:11] = (w, h - w, d)
    nodes = np.zeros(1, dtype=orc.NODE_DT)
    nodes[0]["leftFirst"], nodes[0]["triCount"] = 0, 2
    c = pkg.capi.Ctx(0)
    try:
        for step in STEPS:
            step(c, pkg, oscene, oroute, lamps)
        c.set_scene(tris, nodes, np.array([0, 1], dtype=np.uint32))
        c.set_scene(oscene.tris, oscene.nodes, oscene.triIdx)
        assert np.array_equal(_launch(c, lamps, oroute), first_counts)
    finally:
        c.close()
