#!/usr/bin/env python3
"""Developer tool: the static tally of k_extend6's sign-ordered stream (uvrt_extend6.hip R7_BODY_SIGN, flavours 0 / 1) through
tests/tools/stream_census.py, and the per-ray issue model that follows from it.

stream_census.py prices R7_BODY, the stream with the min/max near / far block (flavour 2 today, every flavour when the
committed issue models and kept lines were made), and stays as it is.  This wrapper hands it the other body, names the sign
masks as scalar operands, and prices the six exchanges (v_pk_mov_b32 ... op_sel:[1,0]) with the class the calibration measured
(profiles/r07/r07_swap_calibration.txt, tests/tools/swap_calib.hip) instead of a class taken from the mnemonic.

    python tests/tools/stream_census_nearfar.py                    # the tally per trip kind
    python tests/tools/stream_census_nearfar.py --out profiles/r07/extend_issue_model_batched_nearfar.json

--out restates the committed model of the batched headline (profiles/extend_issue_model_batched.json: its trip census and PMC
summary are of the min/max stream) for the new stream: the same trips per ray, the new cycles per trip kind, and three more
compiler-written v_cmp per stream entry (the sign-mask ballots).  It is a model, not a measurement."""
import argparse
import json
import os
import re
import sys
from unittest import mock

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import stream_census as sc  # noqa: E402

CALIBRATION = os.path.join(ROOT, "profiles", "r07", "r07_swap_calibration.txt")
BODY_SIGN = {fl: body.replace("R7_BODY(", "R7_BODY_SIGN(", 1) for fl, body in sc.FLAVOUR_BODY.items() if fl in (0, 1)}
SIGN_MASKS = ("nx", "ny", "nz")
EXCHANGE = re.compile(r"^v_pk_mov_b32 (v\[\d+:\d+\]), \1, \1 op_sel:\[1,0\]$")
CLASSES = (2, 4, 8)


def calibrated_classes(path=CALIBRATION):
    """-> {instruction: issue class}: the wall-based cycles per instruction with all lanes active, to the nearest class"""
    out = {}
    for l in open(path):
        m = re.match(r"^(v_\w+)(?: op_sel:\[1,0\])?\s+8\s+all\s+[0-9.]+\s+([0-9.]+)", l)
        if m:
            cyc = float(m.group(2))
            cls = min(CLASSES, key=lambda c: abs(cyc - c))
            assert abs(cyc - cls) < 0.2 * cls, (m.group(1), cyc)
            out[m.group(1)] = cls
    return out


def stream_text(flavour):
    with mock.patch.dict(sc.FLAVOUR_BODY, {flavour: BODY_SIGN[flavour]}):
        return sc.stream_text(flavour)


def tally(seg, exchange_class):
    """stream_census.tally with the sign masks as scalar registers and the exchanges at their calibrated class"""
    t = {"valu": 0, "valu_cycles": 0, "salu": 0, "lds": 0, "vmem": 0, "by_cost": {2: 0, 4: 0, 8: 0}, "exchanges": 0}
    for s in seg:
        s = re.sub(r"%%\[(%s)\]" % "|".join(SIGN_MASKS), "s[90:91]", s)
        u, c = sc.classify(s)
        if EXCHANGE.match(s):
            assert u == "valu"
            c = exchange_class
            t["exchanges"] += 1
        if u == "valu":
            t["valu"] += 1
            t["valu_cycles"] += c
            t["by_cost"][c] += 1
        elif u in ("salu", "lds", "vmem"):
            t[u] += 1
    return t


KINDS = {"stream_in": "ACEF", "stream_leaf": "ABCDEG", "stream_both": "ABCDEF", "exit": "A"}


def per_trip_kind(flavour, exchange_class=None):
    if exchange_class is None:
        exchange_class = calibrated_classes()["v_pk_mov_b32"]
    seg = {k: tally(v, exchange_class) for k, v in sc.segments(stream_text(flavour)).items()}
    out = {}
    for k, letters in KINDS.items():
        out[k] = {f: sum(seg[s][f] for s in letters) for f in ("valu", "valu_cycles", "salu", "lds", "vmem", "exchanges")}
        out[k]["by_cost"] = {c: sum(seg[s]["by_cost"][c] for s in letters) for c in CLASSES}
    return out


def restated_model(flavour=0):
    """the committed batched model with the new stream in place of the old"""
    name = "extend_issue_model_batched.json" if flavour == 0 else "extend_issue_model_batched_flavour1.json"
    with open(os.path.join(ROOT, "profiles", name)) as f:
        old = json.load(f)
    kinds = per_trip_kind(flavour)
    trips = old["trips_per_ray"]
    stream = {f: sum(trips[k] * kinds[k][f] for k in trips) for f in ("valu", "valu_cycles", "salu", "lds", "vmem")}
    cw = dict(old["compiler_written"])
    ballots = 3.0 * trips["exit"]                       # three v_cmp (class 4) before every entry of the stream
    rest_old = cw["valu_insts_per_ray"] * cw["static_mean_cycles"]
    rest_new = rest_old + 4.0 * ballots
    est_old = old["per_ray"]["valu_issue_cycles"]
    est = stream["valu_cycles"] + rest_new
    return {
        "restates": "profiles/" + name, "flavour": flavour, "calibration": os.path.relpath(CALIBRATION, ROOT),
        "method": "the committed model's trips per ray (census of the min/max stream: the trips do not change) x the static cycles "
                  "per trip kind of R7_BODY_SIGN, the exchanges at their calibrated class; the compiler-written rest as committed "
                  "plus three v_cmp per stream entry.  A model: no census or PMC run of the new stream is behind it",
        "exchange_class": calibrated_classes()["v_pk_mov_b32"], "trips_per_ray": trips, "per_trip_kind": kinds,
        "stream_per_ray": stream, "sign_mask_ballots_per_ray": ballots,
        "compiler_written_cycles_per_ray": rest_new,
        "per_ray": {"valu_issue_cycles": est, "valu_issue_cycles_min_max_stream": est_old,
                    "valu_insts": old["per_ray"]["valu_insts"] - old["stream_per_ray"]["valu"] + stream["valu"] + ballots,
                    "valu_insts_min_max_stream": old["per_ray"]["valu_insts"],
                    "salu_insts": old["per_ray"]["salu_insts"] - old["stream_per_ray"]["salu"] + stream["salu"],
                    "salu_insts_min_max_stream": old["per_ray"]["salu_insts"]},
        "predicted_change_of_valu_issue_cycles": est / est_old - 1.0,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--flavour", type=int, default=0, choices=(0, 1))
    ap.add_argument("--out")
    args = ap.parse_args()
    print("calibrated classes:", calibrated_classes())
    for k, v in per_trip_kind(args.flavour).items():
        print("trip kind %-12s VALU %3d instructions = %3d issue cycles  SALU %2d  LDS %d  VMEM %d  exchanges %d"
              % (k, v["valu"], v["valu_cycles"], v["salu"], v["lds"], v["vmem"], v["exchanges"]))
    m = restated_model(args.flavour)
    print(json.dumps({"per_ray": m["per_ray"], "predicted_change_of_valu_issue_cycles": m["predicted_change_of_valu_issue_cycles"]}, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(m, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
