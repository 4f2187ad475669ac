#!/usr/bin/env python3
"""Developer tool (no GPU): the dedupe groups of tests/test_dedupe_periodic_cpu.py as text, one per line, for
tests/tools/dedupe_periodic_check.cpp:  name lx ly lz seed_mode first_gid n K prev[K] next[K]  (floats as hex bit patterns).

    python tests/tools/dedupe_periodic_cases.py > cases.txt"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as g  # noqa: E402

capi = g.load_package().capi
orc = g.load_oracle()
import dedupe_strip_cases as strips  # noqa: E402
import dedupe_tiled_cases as cases  # noqa: E402
from test_dedupe_cpu import seed_chain  # noqa: E402
from test_dedupe_periodic_cpu import WEIGHT  # noqa: E402

scene = orc.Scene(os.path.join(ROOT, "tests", "golden", "testroomopt.glb"))
route = orc.load_route(os.path.join(ROOT, "tests", "golden", "lange_route.xml"))
lamp0, length = cases.lamp0_of(orc, scene, route)
groups = cases.groups(capi, lamp0, length) + strips.groups(capi, lamp0, length)
prev, nxt = seed_chain(capi, lamp0, length, 8, 0, 0)
groups += [cases.Group(name, lamp0, prev, nxt, 0, first, n) for name, (first, n, _) in WEIGHT.items()]
for gr in groups:
    lamp = " ".join("%08x" % int(np.float32(x).view(np.uint32)) for x in gr.lamp)
    print(gr.name, lamp, gr.mode, gr.first, gr.n, gr.K, " ".join(str(int(s)) for s in gr.prev), " ".join(str(int(s)) for s in gr.nxt))
