"""GPU: free rays on the small random scenes of test_gpu_fuzz.py.  The traversal step is ONE function for the fixed-lamp
kernel and the free-ray kernel (csrc/uvrt_traverse.h step6 / step7); every other free-ray test walks the test room, so these
clustered, duplicated and tiny scenes drive the free lane type through it: stacks beyond the LDS rows, leaves with several
triangles, ray counts that are not multiples of 64.  Bit for bit against the oracle in flavours 0 and 1 and on the exact step
(IEEE divisions everywhere).  The generator is seeded: a failure names its case."""
import functools
import types

import numpy as np
import pytest

from test_gpu_free_rays import assert_same, make_rays, new_ctx, oracle_extend, trace_free
from test_gpu_fuzz import random_scene

pytestmark = pytest.mark.gpu

CASES = list(range(16))
LDS_STACK_ROWS = 8          # PS6 of csrc/uvrt_traverse.h: a deeper stack uses the overflow rows of the general step


@functools.lru_cache(maxsize=None)
def case_inputs(orc, case):
    """scene, rays and the oracle's answer in flavours 0 and 1: made once per case"""
    rng = np.random.default_rng(7000 + case)
    tris, _extent = random_scene(rng)
    nodes, idx = orc.build_bvh(tris)
    scene = types.SimpleNamespace(tris=tris, nodes=nodes, triIdx=idx, T=tris.shape[0])
    n = int(rng.choice([1, 63, 65, 1000, 20001]))
    v = tris[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]].reshape(-1, 3)
    origins = rng.uniform(v.min(0), v.max(0), (n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3))
    dirs = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    rays = make_rays(orc, dirs, origins)
    want = {fl: oracle_extend(orc, scene, rays, fl) for fl in (0, 1)}
    return scene, rays, want


@pytest.mark.parametrize("case", CASES)
def test_free_rays_on_a_random_scene(pkg, orc, case):
    scene, rays, want = case_inputs(orc, case)
    for fl in (0, 1):
        o_rays, o_counts, st = want[fl]
        print("case %d flavour %d: %d triangles, %d rays, %d hits, deepest stack %d"
              % (case, fl, scene.T, rays.size, st["hits"], st["max_stack"]))
        c = new_ctx(pkg, scene, rays.size)
        try:
            c.set_flavour(fl)
            got, counts = trace_free(c, rays)
        finally:
            c.close()
        assert_same(got, counts, o_rays, o_counts, "case %d flavour %d" % (case, fl))
    # every ray on the exact step (variant 500 of the developer library): the IEEE-division form of the same step
    o_rays, o_counts, _ = want[0]
    c = new_ctx(pkg, scene, rays.size, dev=True)
    try:
        c.set_variant(500)
        got, counts = trace_free(c, rays)
    finally:
        c.close()
    assert_same(got, counts, o_rays, o_counts, "case %d variant 500" % case)


def test_the_cases_reach_overflow_rows_and_multi_triangle_leaves(orc):
    """What the set is for: stacks beyond the LDS rows in at least 4 of the 16 cases, a leaf with several triangles in at
    least one scene."""
    deep = [case for case in CASES if case_inputs(orc, case)[2][0][2]["max_stack"] > LDS_STACK_ROWS]
    multi = [case for case in CASES if (case_inputs(orc, case)[0].nodes["triCount"] > 1).any()]
    print("stack deeper than %d rows in cases %s; a leaf with several triangles in cases %s" % (LDS_STACK_ROWS, deep, multi))
    assert len(deep) >= 4
    assert len(multi) >= 1
