#!/usr/bin/env python3
"""Where the autograd pair's extra time per step goes, from a rocprofv3 kernel trace of scripts/time_train_pair.py:

    rocprofv3 --kernel-trace --output-format csv -d DIR -o pair -- python scripts/time_train_pair.py --steps 40
    python scripts/pair_trace_gaps.py DIR/pair_kernel_trace.csv

A step ends with the two Adam launches (one per network); a step holding lr_loss_kernel is the fused step, any other the pair.
Per step: wall time (Adam end to Adam end), time with a kernel running, idle time, and in the pair the idle time in front of
the backward's first kernel (composite_bwd_kernel) -- the wait of nsr_train_backward for the saved header.  Medians over the
steps; the first step of every timed block is dropped (the script synchronises between blocks).  Prints one JSON object."""
import csv
import json
import statistics
import sys


def main(path):
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    steps, cur, adam = [], [], 0
    for k in rows:
        cur.append(k)
        if "adam_kernel" in k[2]:
            adam += 1
            if adam == 2:
                steps.append(cur)
                cur, adam = [], 0
    out = {"fused": [], "pair": []}
    prev_end = None
    for s in steps:
        kind = "fused" if any("lr_loss_kernel" in k[2] for k in s) else "pair"
        start = prev_end if prev_end is not None else s[0][0]
        end = s[-1][1]
        prev_end = end
        busy, lo, hi = 0, None, None                       # union of the kernel intervals inside [start, end]
        for a, b, _ in s:
            a = max(a, start)
            if hi is None or a > hi:
                busy += (hi - lo) if hi is not None else 0
                lo, hi = a, b
            else:
                hi = max(hi, b)
        busy += hi - lo
        wait = None
        if kind == "pair":
            for i, k in enumerate(s):
                if "composite_bwd_kernel" in k[2]:
                    before = s[i - 1][1] if i > 0 else start
                    wait = k[0] - before
                    break
        gap_in = s[0][0] - start
        out[kind].append({"wall": end - start, "busy": busy, "idle": end - start - busy, "gap_in": gap_in,
                          "bwd_wait": wait, "kernels": len(s)})
    res = {}
    for kind, v in out.items():
        v = [x for x in v if x["gap_in"] < 200_000]        # drop the steps behind a block's synchronisation (ns)
        med = lambda key: statistics.median(x[key] for x in v) / 1e3 if v else None
        res[kind] = {"steps": len(v), "wall_us": med("wall"), "busy_us": med("busy"), "idle_us": med("idle"),
                     "kernels": statistics.median(x["kernels"] for x in v) if v else None}
        if kind == "pair" and v:
            res[kind]["idle_before_backward_us"] = med("bwd_wait")
    print(json.dumps(res))


if __name__ == "__main__":
    main(sys.argv[1])
