#!/usr/bin/env python3
"""Time of on-policy rollout collection on the GPU (plantos_amd.RolloutCollector), against the
plain act / step loop it wraps.

Headline geometry (20x20, 16 rays, range 6, D = 107) with obs_codes, 65536 envs, A2C's
separate pi / vf towers [256, 256] with Tanh, n_steps T = 5 (A2C) and T = 128.  Per T, each
path on a batch and policy of its own, captured once with torch.cuda.graph and replayed:
  collect_bootstrap     one collect() with bootstrap_timeouts=True
  collect_no_bootstrap  one collect() with bootstrap_timeouts=False
  baseline_loop         T x { policy.act(); batch.step() } -- the loop a user had before
each as microseconds per env step (replay time / T); and alone, K launches back to back in a
graph (so a time includes one dependent-launch boundary):
  forward               one policy.act() (the collector adds one per collect, for last_values,
                        and one per step with the bootstrap)
  record                pe_rollout_record on one step's outputs
  gae                   pe_rollout_gae over [T, n]; its 17 T n bytes (reward, value, advantage,
                        return f32 and the start flag u8) over the time, against the HBM peak.
                        The launches rotate over several sets of arrays; `gae.set_bytes` x
                        `gae.sets` says whether they exceed the 256 MiB Infinity Cache.

Method: every path is warmed up (and replayed) before timing; then `rounds` rounds, each timing
one window of replays per path with device events, the order of the paths rotating from round
to round; median, min and max over the rounds.  The batches run with prefetch_every=0: a
captured step cannot carry the host-side schedule of the prefetch launches.  No GPU: the tool
fails.

  python tools/rollout_rate.py [--out profiles/rollout_rate.json] [--rounds 9]
"""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(REPO, "rl-env_amd"))

HBM_PEAK_SPEC = 8.0e12      # B/s
HBM_PEAK_MEASURED = 6.29e12  # B/s, float4 copy
GEOMETRY = dict(grid_size=20, num_plants=10, num_obstacles=12, lidar_range=6, lidar_channels=16)
TOWERS = [[256, 256, 5], [256, 256, 1]]


def window(torch, fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / iters


def capture(torch, fn):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    g.replay()
    torch.cuda.synchronize()
    return g


def stats(xs, scale):
    return {"us_median": round(statistics.median(xs) * scale * 1e6, 3), "us_min": round(min(xs) * scale * 1e6, 3),
            "us_max": round(max(xs) * scale * 1e6, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, nargs="*", default=[5, 128])
    ap.add_argument("--window-ms", type=float, default=120.0, help="target length of one timed window")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("rollout_rate: no GPU (a time cannot be measured on a CPU)")
    from plantos_amd import PlantOSBatch, Policy, RolloutCollector
    from plantos_amd.rollout import gae_device, record_device
    dev, n = "cuda:0", args.envs
    res = {"tool": "rollout_rate", "device": torch.cuda.get_device_name(0), "geometry": GEOMETRY, "envs": n,
           "towers": TOWERS, "obs_codes": True, "prefetch_every": 0, "rounds": args.rounds,
           "window_ms_target": args.window_ms, "hbm_peak_spec_TBs": HBM_PEAK_SPEC / 1e12,
           "hbm_peak_measured_TBs": HBM_PEAK_MEASURED / 1e12, "cases": []}
    torch.manual_seed(1)
    tensors, k = [], None
    for t in TOWERS:
        k, tw = 5 * GEOMETRY["lidar_channels"] + 27, []
        for w in t:
            lin = torch.nn.Linear(k, w)
            tw.append((lin.weight.detach(), lin.bias.detach()))
            k = w
        tensors.append(tw)

    def fresh():
        b = PlantOSBatch(n, seed=7, device=dev, obs_codes=True, prefetch_every=0, **GEOMETRY)
        pol = Policy(b, TOWERS, "tanh", seed=3).load(tensors)
        act = torch.empty(n, dtype=torch.int32, device=dev)
        for t in range(8):  # the io buffer holds codes; the envs have left their reset state
            b.synth_actions(7, t, out=act)
            b.step(act)
        return b, pol

    for T in args.steps:
        keep, graphs, per_step = [], {}, {}
        for name, boot in (("collect_bootstrap", True), ("collect_no_bootstrap", False)):
            b, pol = fresh()
            col = RolloutCollector(b, pol, T, gamma=0.99, gae_lambda=0.95, bootstrap_timeouts=boot)
            graphs[name] = capture(torch, col.collect)
            per_step[name] = T
            keep.append((b, pol, col))
        b, pol = fresh()

        def loop(b=b, pol=pol):
            for _ in range(T):
                a, _, _ = pol.act(deterministic=False)
                b.step(a)

        graphs["baseline_loop"] = capture(torch, loop)
        per_step["baseline_loop"] = T
        keep.append((b, pol))

        # the kernels alone, K launches per graph
        col = keep[0][2]
        K_fwd, K_rec = 8, 64

        def forwards(pol=pol):
            for _ in range(K_fwd):
                pol.act(deterministic=False)

        graphs["forward"] = capture(torch, forwards)
        per_step["forward"] = K_fwd
        _, rew, te, tr = col._row_views[1]

        def records(col=col, b=keep[0][0]):
            for _ in range(K_rec):
                record_device(col._logits, col.actions[0], rew, te, tr, 0.99, col.log_probs[0], rew, col._start[1],
                              terminal_value=col.terminal_values, episode_return=b.episode_return,
                              episode_length=b.episode_length, ep_count=col.ep_count,
                              ep_return_sum=col.ep_return_sum, ep_length_sum=col.ep_length_sum)

        graphs["record"] = capture(torch, records)
        per_step["record"] = K_rec
        set_bytes = 17 * T * n
        n_sets = max(1, min(8, -(-600 * 2 ** 20 // set_bytes)))
        sets = [(torch.rand((T, n), device=dev) * 60 - 10, torch.rand((T, n), device=dev) * 200 - 50,
                 (torch.rand((T + 1, n), device=dev) < 0.02).to(torch.uint8), torch.rand(n, device=dev),
                 torch.empty((T, n), device=dev), torch.empty((T, n), device=dev)) for _ in range(n_sets)]
        K_gae = n_sets * max(1, 16 // n_sets)

        def gaes():
            for i in range(K_gae):
                r, v, s, lv, adv, ret = sets[i % n_sets]
                gae_device(r, v, s, lv, 0.99, 0.95, adv, ret)

        graphs["gae"] = capture(torch, gaes)
        per_step["gae"] = K_gae

        names = list(graphs)
        iters = {}
        for k_ in names:  # replays per window, from one probe window
            one = window(torch, graphs[k_].replay, 3)
            iters[k_] = max(3, int(args.window_ms * 1e-3 / one))
        per = {k_: [] for k_ in names}
        for r in range(args.rounds):
            s = r % len(names)
            for k_ in names[s:] + names[:s]:
                per[k_].append(window(torch, graphs[k_].replay, iters[k_]))
        case = {"n_steps": T, "replays_per_window": iters}
        for k_ in names:
            case[k_] = stats(per[k_], 1.0 / per_step[k_])
        for k_ in ("collect_bootstrap", "collect_no_bootstrap", "baseline_loop"):
            case[k_]["per"] = "env step (one replay = n_steps steps)"
        for k_ in ("forward", "record", "gae"):
            case[k_]["per"] = "launch"
        gae_s = statistics.median(per["gae"]) / K_gae
        case["gae"].update(bytes=set_bytes, set_bytes=set_bytes, sets=n_sets, launches_per_graph=K_gae,
                           TBs=round(set_bytes / gae_s / 1e12, 3),
                           fraction_of_hbm_spec=round(set_bytes / gae_s / HBM_PEAK_SPEC, 4),
                           fraction_of_hbm_measured=round(set_bytes / gae_s / HBM_PEAK_MEASURED, 4))
        # logits, action, reward, two flags, terminal value in; log-prob, reward, start flag out
        case["record"]["bytes"] = n * (4 * TOWERS[0][-1] + 4 + 4 + 2 + 4 + 4 + 4 + 1)
        med = {k_: case[k_]["us_median"] for k_ in names}
        case["per_step_us"] = {
            "collect_no_bootstrap_minus_baseline": round(med["collect_no_bootstrap"] - med["baseline_loop"], 3),
            "record": med["record"],
            "gae_over_T": round(med["gae"] / T, 3),
            "last_values_forward_over_T": round(med["forward"] / T, 3),
            "unexplained": round(med["collect_no_bootstrap"] - med["baseline_loop"] - med["record"] - med["gae"] / T
                                 - med["forward"] / T, 3),
            "bootstrap_cost": round(med["collect_bootstrap"] - med["collect_no_bootstrap"], 3),
        }
        res["cases"].append(case)
        del graphs
        for item in keep:
            item[1].close()
            item[0].close()
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
