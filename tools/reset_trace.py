#!/usr/bin/env python3
"""Split the step kernel's launches of one `rocprofv3 --kernel-trace` run of a
synchronized bench.py into the whole-batch reset launches (every env truncates in
the same step: one launch per max_steps) and all the others.

  python tools/reset_trace.py run_kernel_trace.csv [substring]

A launch counts as a reset launch when it takes more than four times the median
(a stray slow ordinary launch reaches about twice the median).
Prints one JSON line: the reset launches' durations (ns), the median / p10 /
p90 of the ordinary ones, and the ordinary launches' median per episode phase --
the launch's step within its episode (launches since the last reset launch, mod
1000) in four bins of 250: a cost that grows with the visit counts of an episode
(the moves into cells past 15, tools/visit_overflow_rate.py) shows as later bins
slower than the first.
"""
import csv
import json
import sys

import numpy as np

EPISODE, BINS = 1000, 4


def main():
    path = sys.argv[1]
    sub = sys.argv[2] if len(sys.argv) > 2 else "pe_step"
    rows = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in csv.DictReader(open(path))
                   if sub in r["Kernel_Name"]))
    d = np.array([e - s for s, e in rows], dtype=np.int64)
    if d.size == 0:
        raise SystemExit(f"no kernel matching {sub!r} in {path}")
    med = float(np.median(d))
    is_reset = d > 4 * med
    reset = d[is_reset]
    rest = d[~is_reset]
    # episode phase: the launch after a reset launch is step 0 of its episode (no reset launch
    # in the trace: the first launch is)
    ridx = np.nonzero(is_reset)[0]
    anchor = int(ridx[0]) + 1 if ridx.size else 0
    phase = (np.arange(d.size) - anchor) % EPISODE
    width = EPISODE // BINS
    phases = []
    for k in range(BINS):
        sel = ~is_reset & (phase >= k * width) & (phase < (k + 1) * width)
        phases.append({"steps": [k * width, (k + 1) * width], "launches": int(sel.sum()),
                       "median_ns": float(np.median(d[sel])) if sel.any() else None,
                       "mean_ns": float(d[sel].mean()) if sel.any() else None})
    print(json.dumps({"launches": int(d.size), "reset_launch_ns": [int(v) for v in reset],
                      "reset_launch_max_ns": int(reset.max()) if reset.size else None,
                      "ordinary_median_ns": float(np.median(rest)), "ordinary_p10_ns": float(np.percentile(rest, 10)),
                      "ordinary_p90_ns": float(np.percentile(rest, 90)), "ordinary_mean_ns": float(rest.mean()),
                      "ordinary_by_episode_phase": phases}))


if __name__ == "__main__":
    main()
