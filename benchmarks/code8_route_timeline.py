#!/usr/bin/env python3
"""Per-launch durations and the gaps between launches of the single-query int8 route, from a rocprofv3 kernel trace
(`--kernel-trace --output-format csv`, the directory or the *_kernel_trace.csv itself) of `code8_route_probe.py --timers 0`
or of `bench.py`.  A step is the run of dispatches from one floor launch (`code8_seed_kernel`; in traces of builds that
still had the one-block prologue, `code8_query_kernel`) to the next; only steps with the most
common number of launches are averaged (the first ones build the code).  Prints one JSON object:
launches in order with their mean / median duration, the mean gap before each, their sums, the mean step span, and the
mean duration of the exact scan's launches (steps with `code8_single_query = 0`) where the trace has them.

With the corpus' shape the prefilter launch (`code8_scan_kernel`) is also rated on its own streamed bytes: N (3 d / 4 + 8) — the
high plane of the code and (a, r) — for a build with the two planes (`planes` = 1, the default), N (d + 8) for a build from
before them (`planes` = 0).  The low plane of the refined rows (d / 4 bytes each, a few thousand rows) is not in the figure.
`planes` = 2: the front form (the traced kernel then names five template arguments) — N (5 d / 8 + 8) for the front plane and
(a, r), plus 3 d / 4 + 8 for each of the `survivors` rows per launch its stage 0 kept (code8_route_probe.py reports them).
`prefilter_form` says which form the trace holds, by the kernel's name.

usage: code8_route_timeline.py <trace dir or csv> [git-head [rows dim [planes [survivors]]]]"""
import collections
import csv
import glob
import json
import os
import statistics
import sys


def main():
    src = sys.argv[1]
    head = sys.argv[2] if len(sys.argv) > 2 else None
    if os.path.isdir(src):
        src = glob.glob(os.path.join(src, "**", "*_kernel_trace.csv"), recursive=True)[0]
    rows = []
    for r in csv.DictReader(open(src)):
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    first = "code8_query_kernel" if any("code8_query_kernel" in r[2] for r in rows) else "code8_seed_kernel"
    steps, cur = [], None
    for r in rows:
        if first in r[2]:
            cur = []
            steps.append(cur)
        elif cur is not None and "flat_scan_kernel<64, 2, 2, 0, 0, true, 0, false, false>" in r[2]:
            cur = None   # the exact scans behind the route steps
        if cur is not None:
            cur.append(r)
    common = collections.Counter(len(s) for s in steps).most_common(1)[0][0]
    steps = [s for s in steps if len(s) == common][5:]
    launches = []
    for j in range(common):
        dur = [s[j][1] - s[j][0] for s in steps]
        gap = [s[j][0] - s[j - 1][1] for s in steps] if j else [0]
        launches.append({"kernel": steps[0][j][2].split("(")[0], "mean_us": round(statistics.mean(dur) / 1e3, 3),
                         "median_us": round(statistics.median(dur) / 1e3, 3), "gap_before_mean_us": round(statistics.mean(gap) / 1e3, 3)})
    exact = [r[1] - r[0] for r in rows if "flat_scan_kernel<64, 2, 2, 0, 0, true, 0, false, false>" in r[2]]
    out = {"git_head": head, "steps_averaged": len(steps), "launches_per_step": common, "launches": launches,
           "sum_of_launches_us": round(sum(l["mean_us"] for l in launches), 3),
           "sum_of_gaps_us": round(sum(l["gap_before_mean_us"] for l in launches), 3),
           "step_span_mean_us": round(statistics.mean(s[-1][1] - s[0][0] for s in steps) / 1e3, 3),
           "exact_scan_launches": len(exact),
           "exact_scan_mean_us": round(statistics.mean(exact) / 1e3, 3) if exact else None,
           "exact_scan_median_us": round(statistics.median(exact) / 1e3, 3) if exact else None}
    if len(sys.argv) > 4:
        n, d = int(sys.argv[3]), int(sys.argv[4])
        planes = int(sys.argv[5]) if len(sys.argv) > 5 else 1
        nbytes = n * (d // 4 * 3 + 8) if planes else n * (d + 8)
        if planes == 2:
            nbytes = n * (d // 8 * 5 + 8) + int(float(sys.argv[6]) if len(sys.argv) > 6 else 0) * (d // 4 * 3 + 8)
        pre = [l for l in launches if "code8_scan_kernel" in l["kernel"]]
        if pre:
            out.update(prefilter_form="front" if pre[0]["kernel"].count(",") == 4 else "6-bit plane streamed")
            out.update(prefilter_streamed_bytes=nbytes, prefilter_mean_us=pre[0]["mean_us"],
                       prefilter_tb_per_s=round(nbytes / (pre[0]["mean_us"] * 1e-6) / 1e12, 4))
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
