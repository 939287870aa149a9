#!/usr/bin/env python3
"""How often the flagship workload's moves need a visit count past the nibble
(pe_device.hpp vx / vxb), from the CPU oracle on bench.py's own action stream.

  python tools/visit_overflow_rate.py [--envs 2048] [--steps 999] [--seed 0]

bench.py replays 64 pre-generated action rows (synth_action(seed, env, t % 64)), so every
env repeats a 64-action cycle and ends up pacing the same few cells.  An overflow event
is a successful move into a cell whose count is already >= 14 (the 15th visit sets the
exact count, later ones bump it).  Prints one JSON line: the share of env-steps with a
move and with an event, the events per env-episode (mean, p99, max), the rate per
episode phase, the cells at >= 15 at the end of the episode and the largest count.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import oracle as O  # noqa: E402

PHASES = [(0, 100), (100, 250), (250, 500), (500, 750), (750, 999)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=999)  # one episode, the truncating step excluded
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--action-steps", type=int, default=64)
    args = ap.parse_args()
    n, T = args.envs, args.action_steps
    cfg = O.config(20, 10, 12, 6, 16)
    b = O.Batch(cfg, n)
    for e in range(n):
        b.reset_philox(e, args.seed, e, 0)
    acts = np.array([[O.synth_action(args.seed, e, t) for e in range(n)] for t in range(T)], np.int64)
    moves = np.zeros(args.steps, np.int64)
    events = np.zeros((args.steps, n), bool)
    for t in range(args.steps):
        before = b.visits.copy()
        _, _, te, tr = b.step(acts[t % T])
        assert not (te | tr).any(), "the window must stay inside one episode"
        grew = b.visits > before  # the cell moved into (none: a collision or a watering)
        moves[t] = int(grew.any(axis=(1, 2)).sum())
        events[t] = (grew & (before >= 14)).any(axis=(1, 2))
    per_env = events.sum(axis=0)
    out = {
        "envs": n, "steps": args.steps, "seed": args.seed, "action_steps": T,
        "move_share": float(moves.sum() / (n * args.steps)),
        "event_share": float(events.mean()),
        "events_per_env": {"mean": float(per_env.mean()), "p99": float(np.percentile(per_env, 99)),
                           "max": int(per_env.max())},
        "phases": [{"steps": [lo, hi], "events_per_env": float(events[lo:hi].sum() / n),
                    "rate": float(events[lo:hi].mean())} for lo, hi in PHASES if lo < args.steps],
        "cells_at_15_or_more": {"mean": float((b.visits >= 15).sum(axis=(1, 2)).mean()),
                                "max": int((b.visits >= 15).sum(axis=(1, 2)).max())},
        "largest_count": int(b.visits.max()),
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
