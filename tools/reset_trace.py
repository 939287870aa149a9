#!/usr/bin/env python3
"""Split the step kernel's launches of one `rocprofv3 --kernel-trace` run of a
synchronized bench.py into the whole-batch reset launches (every env truncates in
the same step: one launch per max_steps) and all the others.

  python tools/reset_trace.py run_kernel_trace.csv [substring]

A launch counts as a reset launch when it takes more than four times the median
(a stray slow ordinary launch reaches about twice the median).
Prints one JSON line: the reset launches' durations (ns) and the median / p10 /
p90 of the ordinary ones.
"""
import csv
import json
import sys

import numpy as np


def main():
    path = sys.argv[1]
    sub = sys.argv[2] if len(sys.argv) > 2 else "pe_step"
    d = np.array([int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in csv.DictReader(open(path))
                  if sub in r["Kernel_Name"]], dtype=np.int64)
    if d.size == 0:
        raise SystemExit(f"no kernel matching {sub!r} in {path}")
    med = float(np.median(d))
    reset = d[d > 4 * med]
    rest = d[d <= 4 * med]
    print(json.dumps({"launches": int(d.size), "reset_launch_ns": [int(v) for v in reset],
                      "reset_launch_max_ns": int(reset.max()) if reset.size else None,
                      "ordinary_median_ns": float(np.median(rest)), "ordinary_p10_ns": float(np.percentile(rest, 10)),
                      "ordinary_p90_ns": float(np.percentile(rest, 90)), "ordinary_mean_ns": float(rest.mean())}))


if __name__ == "__main__":
    main()
