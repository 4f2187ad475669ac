"""CPU: the two facts k_extend6's sign-ordered near / far block stands on (uvrt_extend6.hip R7_ENTER_BOX_SIGN, R7_NEARFAR_SIGN).

1. With the numerators of a slab pair in ascending order (prepare_record6 writes them so), the nearer and the farther of the
   two slab distances follow from the sign of the direction component alone: (t1, t2) for d > 0, (t2, t1) for d < 0 equal
   (min, max) of the two quotients AS VALUES, because correctly rounded division is monotone.  The division is the IEEE
   binary32 one of the oracle (uvrt_oracle.c writes `/` on floats; numpy's float32 division is the same operation), which
   the kernel's packed three-instruction form equals for the operands the stream admits (test_recip_division.py).
   Signed zeros count as equal: every later use is a comparison (extend.cl:37, 63-75), and -0 == +0 there.
2. The static tally of the new stream: 50 VALU instructions per inner-node trip and 170 + 6 x (the calibrated class of the
   exchange) issue cycles, while R7_BODY -- the min/max stream that the committed issue models price -- stays at 56 / 218
   (flavours 0, 1) and 44 / 170 (flavour 2)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))

f32 = np.float32


def assert_sign_selects_min_max(a1, a2, d):
    """a1 <= a2 elementwise, d a direction component the stream admits (2^-60 <= |d| <= 1)"""
    a1, a2, d = np.broadcast_arrays(np.asarray(a1, f32), np.asarray(a2, f32), np.asarray(d, f32))
    assert np.all(a1 <= a2) and np.all((np.abs(d) >= f32(2.0 ** -60)) & (np.abs(d) <= 1))
    with np.errstate(over="ignore"):
        t1, t2 = a1 / d, a2 / d
    assert t1.dtype == np.float32
    neg = d < 0
    near, far = np.where(neg, t2, t1), np.where(neg, t1, t2)
    with np.errstate(invalid="ignore"):
        bad = np.flatnonzero((near != np.minimum(t1, t2)) | (far != np.maximum(t1, t2)) | np.isnan(t1) | np.isnan(t2))
    assert bad.size == 0, (a1[bad[:5]], a2[bad[:5]], d[bad[:5]], t1[bad[:5]], t2[bad[:5]])
    return t1, t2


def directions(rng, n):
    """components of unit vectors, plus every binade down to 2^-60, both signs"""
    d = rng.uniform(-1, 1, n).astype(f32)
    tiny = rng.random(n) < 0.3
    d = np.where(tiny, (d * np.exp2(-rng.integers(0, 60, n))).astype(f32), d)
    d = np.where(np.abs(d) >= f32(2.0 ** -60), d, f32(0.37))
    return d


def test_seeded_operand_pairs():
    rng = np.random.default_rng(20)
    for _ in range(4):
        n = 1_000_000
        lo = (rng.normal(size=n) * 10.0 ** rng.uniform(-4, 3, n)).astype(f32)
        hi = (lo + np.abs(rng.normal(size=n) * 10.0 ** rng.uniform(-6, 2, n)).astype(f32)).astype(f32)     # f32 add: hi >= lo
        assert_sign_selects_min_max(lo, hi, directions(rng, n))
    # any finite bit patterns, ordered
    n = 2_000_000
    x = rng.integers(0, 2 ** 32, (2, n), dtype=np.uint64).astype(np.uint32).view(f32)
    x = np.where(np.isfinite(x), x, f32(1.5))
    assert_sign_selects_min_max(np.minimum(x[0], x[1]), np.maximum(x[0], x[1]), directions(rng, n))


def test_adversarial_operand_pairs():
    rng = np.random.default_rng(21)
    n = 500_000
    d = directions(rng, n)
    a = (rng.normal(size=n) * 10.0 ** rng.uniform(-4, 3, n)).astype(f32)
    # a flat box: a1 == a2
    assert_sign_selects_min_max(a, a, d)
    # zeros of either sign as one or both numerators (a bound in the plane of the origin)
    for z1, z2 in ((-0.0, 0.0), (0.0, 0.0), (-0.0, -0.0), (0.0, -0.0)):
        t1, t2 = assert_sign_selects_min_max(np.full(n, z1, f32), np.full(n, z2, f32), d)
        assert not t1.any() and not t2.any()
    assert_sign_selects_min_max(-np.abs(a), f32(0.0), d)
    assert_sign_selects_min_max(-np.abs(a), f32(-0.0), d)
    assert_sign_selects_min_max(f32(0.0), np.abs(a), d)
    assert_sign_selects_min_max(f32(-0.0), np.abs(a), d)
    # bounds on either side of the origin
    assert_sign_selects_min_max(-np.abs(a), np.abs(rng.permutation(a)), d)
    # numerators one or two ulps apart: the quotients often round to the same value
    same = 0
    for ulps in (1, 2):
        hi = a
        for _ in range(ulps):
            hi = np.nextafter(hi, f32(np.inf))
        t1, t2 = assert_sign_selects_min_max(a, hi, d)
        same += int((t1 == t2).sum())
    assert same > 1000
    # quotients beyond the largest float: both infinite, equal
    big = rng.uniform(1e36, 3e38, n).astype(f32)
    small_d = np.where(np.abs(d) < 1e-3, d, f32(-1e-7))
    for lo, hi in ((big, np.nextafter(big, f32(np.inf))), (-np.nextafter(big, f32(np.inf)), -big)):
        t1, t2 = assert_sign_selects_min_max(lo, hi, small_d)
        assert np.isinf(t1).all() and (t1 == t2).all()


def test_static_tally_of_the_sign_ordered_stream():
    import stream_census as sc
    import stream_census_nearfar as nf
    classes = nf.calibrated_classes()
    assert classes["v_fma_f32"] == 2 and classes["v_min_f32"] == 4             # the anchors of the calibration run
    cls = classes["v_pk_mov_b32"]
    assert cls in (2, 4)                                                       # otherwise the exchange buys nothing
    for fl in (0, 1):
        kinds = nf.per_trip_kind(fl)
        assert kinds["stream_in"]["valu"] == 50 and kinds["stream_in"]["exchanges"] == 6
        assert kinds["stream_in"]["valu_cycles"] == 170 + 6 * cls
        text = nf.stream_text(fl)
        assert not [s for s in text if s.split()[0] in ("v_min_f32", "v_max_f32")]
        assert sum(s.startswith(("v_max3_f32", "v_min3_f32")) for s in text) == 4
        # the other trip kinds: the triangle block and the fetch are the min/max stream's
        old = {k: sc.tally(v) for k, v in sc.segments(sc.stream_text(fl)).items()}
        new = {k: nf.tally(v, cls) for k, v in sc.segments(text).items()}
        for seg in "ABCDEG":
            assert {f: new[seg][f] for f in old[seg]} == old[seg], seg
    # the min/max stream keeps its text: what the committed issue models and kept lines were priced with
    for fl, (valu, cyc) in {0: (56, 218), 1: (56, 218), 2: (44, 170)}.items():
        seg = {k: sc.tally(v) for k, v in sc.segments(sc.stream_text(fl)).items()}
        assert [sum(seg[s][f] for s in "ACEF") for f in ("valu", "valu_cycles")] == [valu, cyc], fl


def test_restated_model_is_the_committed_one_with_the_new_stream():
    import json
    import stream_census_nearfar as nf
    with open(os.path.join(ROOT, "profiles", "r07", "extend_issue_model_batched_nearfar.json")) as f:
        kept = json.load(f)
    m = json.loads(json.dumps(nf.restated_model(0)))
    assert kept == m
    inner = m["trips_per_ray"]["stream_in"] + m["trips_per_ray"]["stream_both"]
    saved = m["per_ray"]["valu_issue_cycles_min_max_stream"] - m["per_ray"]["valu_issue_cycles"]
    assert abs(saved - (inner * (218 - 170 - 6 * m["exchange_class"]) - 12.0 * m["trips_per_ray"]["exit"])) < 1e-9
