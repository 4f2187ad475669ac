#!/usr/bin/env python3
"""Developer tool: from a rocprofv3 --kernel-trace CSV of `bench.py` (batched mode), what a launch lane's chain costs.

    python tests/tools/trace_chain.py <kernel_trace.csv> <steps> <warmup> [out.txt]

The timed region is the `steps` computations after the first `warmup` ones, a computation being delimited by its k_reset
launch (tests/tools/trace_union.py).  Printed: every kernel above 0.1 % of the kernel time of the whole trace; over the
timed steps only the generate kernels (mark / scan / write or k_generate_batch), k_extend6 and k_replay_batch with their
average, minimum and maximum; the union of the generate + extend intervals per step; the lane chain (the sum of the
averages of a chunk's kernels); the traversals in flight (sum of k_extend6 kernel time over that union); and the mark
pass beside a traversal (more than half of its interval inside some k_extend6 interval) against the mark pass alone."""
import csv
import sys

CHAIN = ["k_dedupe_mark", "k_dedupe_scan", "k_dedupe_write", "k_generate_batch", "k_extend6"]


def short(name):
    n = name.split("(")[0]
    n = n.split("<")[0]
    return n.split("::")[-1].split(" ")[-1]


def union_ns(iv):
    iv = sorted(iv)
    if not iv:
        return 0
    total, cs, ce = 0, iv[0][0], iv[0][1]
    for s, e in iv[1:]:
        if s > ce:
            total += ce - cs
            cs, ce = s, e
        else:
            ce = max(ce, e)
    return total + ce - cs


def main():
    path, steps, warmup = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
    out = open(sys.argv[4], "w") if len(sys.argv) > 4 else sys.stdout
    rows = []
    for r in csv.DictReader(open(path)):
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    whole = {}
    for s, e, k in rows:
        a = whole.setdefault(k.split("(")[0], [0, 0])
        a[0] += 1
        a[1] += e - s
    ktime = sum(v[1] for v in whole.values())
    for k, (n, d) in sorted(whole.items(), key=lambda kv: -kv[1][1]):
        if d >= 0.001 * ktime:
            print("%-72s calls %4d  average %8.1f us  total %8.2f ms  %5.2f %% of kernel time"
                  % (k[:72], n, d / n / 1e3, d / 1e6, 100.0 * d / ktime), file=out)
    resets = [i for i, r in enumerate(rows) if short(r[2]) == "k_reset"]
    if len(resets) < warmup + steps + 1:
        print("only %d k_reset launches in the trace" % len(resets), file=out)
        return
    timed = rows[resets[warmup]:resets[warmup + steps]]
    per = {}
    for s, e, k in timed:
        per.setdefault(short(k), []).append((s, e))
    gen_ext = [iv for k in CHAIN for iv in per.get(k, [])]
    uni = union_ns(gen_ext)
    print("union of the generate + extend intervals: %.2f ms over %d steps = %.4f ms per step" % (uni / 1e6, steps, uni / steps / 1e6), file=out)
    t0, t1 = timed[0][0], max(e for _, e, _ in timed)
    print("timed region (k_reset to k_reset): %.4f ms per step first kernel start to last kernel end" % ((t1 - t0) / steps / 1e6), file=out)
    chain = 0.0
    for k in CHAIN + ["k_replay_batch"]:
        iv = per.get(k)
        if not iv:
            continue
        d = [(e - s) / 1e3 for s, e in iv]
        print("timed steps only: %-18s calls %4d  average %8.1f us  min %8.1f  max %8.1f" % (k, len(d), sum(d) / len(d), min(d), max(d)), file=out)
        if k in CHAIN:
            chain += sum(d) / len(d)
    ext = per.get("k_extend6", [])
    ext_sum = sum(e - s for s, e in ext)
    print("lane chain (sum of the averages of a chunk's generate kernels and its k_extend6): %.1f us" % chain, file=out)
    if uni:
        print("traversals in flight: %.3f ms of k_extend6 kernel time per step over the %.4f ms union = %.2f"
              % (ext_sum / steps / 1e6, uni / steps / 1e6, ext_sum / uni), file=out)
    beside, alone = [], []
    for s, e in per.get("k_dedupe_mark", []):
        inside = union_ns([(max(s, a), min(e, b)) for a, b in ext if a < e and b > s])
        (beside if 2 * inside > e - s else alone).append((e - s) / 1e3)
    for name, d in (("beside a traversal", beside), ("alone", alone)):
        if d:
            print("k_dedupe_mark %-18s calls %4d  average %8.1f us  min %8.1f  max %8.1f" % (name, len(d), sum(d) / len(d), min(d), max(d)), file=out)


if __name__ == "__main__":
    main()
