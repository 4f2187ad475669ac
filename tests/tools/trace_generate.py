#!/usr/bin/env python3
"""Developer tool: tests/tools/trace_chain.py's report of a rocprofv3 --kernel-trace CSV of `bench.py` (batched mode), and
behind it what that report has for the mark pass only: EACH dedupe generate kernel (mark, scan, write) beside a traversal
(more than half of its interval inside some k_extend6 interval) against the same kernel alone, and the generate chain of a
chunk (the sum of their averages).

    python tests/tools/trace_generate.py <kernel_trace.csv> <steps> <warmup> [out.txt]"""
import csv
import sys

import trace_chain
from trace_chain import short, union_ns

GENERATE = ["k_dedupe_mark", "k_dedupe_scan", "k_dedupe_write"]


def main():
    trace_chain.main()
    path, steps, warmup = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
    out = open(sys.argv[4], "a") if len(sys.argv) > 4 else sys.stdout
    rows = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(path)))
    resets = [i for i, r in enumerate(rows) if short(r[2]) == "k_reset"]
    if len(resets) < warmup + steps + 1:
        return
    per = {}
    for s, e, k in rows[resets[warmup]:resets[warmup + steps]]:
        per.setdefault(short(k), []).append((s, e))
    ext = per.get("k_extend6", [])
    chain = 0.0
    for k in GENERATE:
        beside, alone = [], []
        for s, e in per.get(k, []):
            inside = union_ns([(max(s, a), min(e, b)) for a, b in ext if a < e and b > s])
            (beside if 2 * inside > e - s else alone).append((e - s) / 1e3)
        for name, d in (("beside a traversal", beside), ("alone", alone)):
            if d:
                print("%-14s %-18s calls %4d  average %8.1f us  min %8.1f  max %8.1f" % (k, name, len(d), sum(d) / len(d), min(d), max(d)), file=out)
        if beside or alone:
            chain += sum(beside + alone) / len(beside + alone)
    print("generate chain of a chunk (sum of the averages of %s): %.1f us" % (" + ".join(k for k in GENERATE if per.get(k)), chain), file=out)


if __name__ == "__main__":
    main()
