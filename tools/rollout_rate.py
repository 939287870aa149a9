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

With a package that has the value-only forward (Policy.value), further paths:
  value / value_flags / value_none
                        K x policy.value(): every env, the real (truncated, terminated) flags of
                        one step of the batch, and an all-zero want (every tile skipped); beside
                        `forward` of the same policy, and the same four for the LSTM policy
                        (H = 256, towers [128, 128]) under "lstm" (forward advances the state)
  recurrent_collect_first / recurrent_collect_all / recurrent_baseline_loop
                        RecurrentRolloutCollector.collect() with state_snapshots "first" / "all"
                        and T x { act(episode_start=flags); step() }, per env step.
--desync starts every env at a random step count in [0, 1000) (bench.py's desynchronize), so a
step cuts about n / 1000 envs by the time limit instead of all of them every 1000 steps.
--pkg names another checkout's package directory (a same-box A/B against the parent commit: the
paths that package lacks are left out).

Method: every path is warmed up (and replayed) before timing; then `rounds` rounds, each timing
one window of replays per path with device events, the order of the paths rotating from round
to round; median, min and max over the rounds.  The batches run with prefetch_every=0: a
captured step cannot carry the host-side schedule of the prefetch launches.  No GPU: the tool
fails.

  python tools/rollout_rate.py [--out profiles/rollout_rate.json] [--rounds 9] [--desync] [--pkg DIR]
"""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


HBM_PEAK_SPEC = 8.0e12      # B/s
HBM_PEAK_MEASURED = 6.29e12  # B/s, float4 copy
GEOMETRY = dict(grid_size=20, num_plants=10, num_obstacles=12, lidar_range=6, lidar_channels=16)
TOWERS = [[256, 256, 5], [256, 256, 1]]
LSTM_HIDDEN, LSTM_TOWERS = 256, [[128, 128, 5], [128, 128, 1]]


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
    ap.add_argument("--desync", action="store_true", help="every env at its own step count")
    ap.add_argument("--pkg", default=os.path.join(REPO, "rl-env_amd"), help="directory that holds plantos_amd")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.pkg))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("rollout_rate: no GPU (a time cannot be measured on a CPU)")
    import plantos_amd
    from plantos_amd import PlantOSBatch, Policy, RecurrentPolicy, RolloutCollector
    from plantos_amd.rollout import gae_device, record_device
    has_value = hasattr(Policy, "value")
    if has_value:
        from plantos_amd import RecurrentRolloutCollector
    dev, n = "cuda:0", args.envs
    res = {"tool": "rollout_rate", "device": torch.cuda.get_device_name(0), "geometry": GEOMETRY, "envs": n,
           "towers": TOWERS, "obs_codes": True, "prefetch_every": 0, "rounds": args.rounds, "desync": args.desync,
           "package": os.path.relpath(os.path.dirname(plantos_amd.__file__), REPO), "lstm_hidden": LSTM_HIDDEN,
           "lstm_towers": LSTM_TOWERS,
           "window_ms_target": args.window_ms, "hbm_peak_spec_TBs": HBM_PEAK_SPEC / 1e12,
           "hbm_peak_measured_TBs": HBM_PEAK_MEASURED / 1e12, "cases": []}
    torch.manual_seed(1)
    tensors, k0 = [], 5 * GEOMETRY["lidar_channels"] + 27
    for t in TOWERS:
        k, tw = k0, []
        for w in t:
            lin = torch.nn.Linear(k, w)
            tw.append((lin.weight.detach(), lin.bias.detach()))
            k = w
        tensors.append(tw)

    lstm_mod = [torch.nn.LSTM(k0, LSTM_HIDDEN) for _ in LSTM_TOWERS]
    lstm_tensors = [tuple(getattr(m, k_).detach() for k_ in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"))
                    for m in lstm_mod]
    lstm_mlp = []
    for t in LSTM_TOWERS:
        k, tw = LSTM_HIDDEN, []
        for w in t:
            lin = torch.nn.Linear(k, w)
            tw.append((lin.weight.detach(), lin.bias.detach()))
            k = w
        lstm_mlp.append(tw)

    def fresh(recurrent=False):
        b = PlantOSBatch(n, seed=7, device=dev, obs_codes=True, prefetch_every=0, **GEOMETRY)
        if recurrent:
            pol = RecurrentPolicy(b, LSTM_HIDDEN, LSTM_TOWERS, "tanh", seed=3).load((lstm_tensors, lstm_mlp))
        else:
            pol = Policy(b, TOWERS, "tanh", seed=3).load(tensors)
        if args.desync:  # every env at its own step count (bench.py's desynchronize)
            from plantos_amd import _capi as CA
            sc = b.get_state()["scalars"]
            g = torch.Generator(device="cpu").manual_seed(1)
            sc[:, CA.PE_S_STEP] = torch.randint(0, 1000, (n,), generator=g, dtype=torch.int32).to(sc.device)
            b.set_state(scalars=sc)
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

        step_paths = ["collect_bootstrap", "collect_no_bootstrap", "baseline_loop"]
        launch_paths = ["forward", "record", "gae"]
        flag_counts = {}
        if has_value:
            K_sel = 64
            for prefix, recurrent, K_full in (("", False, K_fwd), ("lstm_", True, 4)):
                vb, vpol = fresh(recurrent)
                # the flags of one real step of this batch, kept apart from the io buffer
                te, tr = vb.terminated.clone(), vb.truncated.clone()
                zero = torch.zeros(n, dtype=torch.uint8, device=dev)
                vout = torch.zeros(n, dtype=torch.float32, device=dev)
                sel, et = (tr != 0) & (te == 0), vpol.env_tile
                tiles = -(-n // et)
                flag_counts[prefix + "value_flags"] = {
                    "selected_envs": int(sel.sum()), "tiles": tiles, "env_tile": et,
                    "selected_tiles": int(torch.nn.functional.pad(sel, (0, tiles * et - n)).view(tiles, et).any(1).sum())}

                def reps(fn, K):
                    def run():
                        for _ in range(K):
                            fn()
                    return run

                if recurrent:
                    graphs["lstm_forward"] = capture(torch, reps(lambda p=vpol: p.act(deterministic=False), K_full))
                    per_step["lstm_forward"] = K_full
                    launch_paths.append("lstm_forward")
                for name, K, kw in (("value", K_full, {}), ("value_flags", K_sel, dict(select=(tr, te))),
                                    ("value_none", K_sel, dict(select=zero))):
                    graphs[prefix + name] = capture(torch, reps(lambda p=vpol, kw=kw: p.value(out=vout, **kw), K))
                    per_step[prefix + name] = K
                    launch_paths.append(prefix + name)
                keep.append((vb, vpol, te, tr, zero, vout))
            for name, mode in (("recurrent_collect_first", "first"), ("recurrent_collect_all", "all")):
                rb, rpol = fresh(True)
                rcol = RecurrentRolloutCollector(rb, rpol, T, gamma=0.99, gae_lambda=0.95, state_snapshots=mode)
                graphs[name] = capture(torch, rcol.collect)
                per_step[name] = T
                step_paths.append(name)
                keep.append((rb, rpol, rcol))
            rb, rpol = fresh(True)

            def rloop(b=rb, pol=rpol):
                for _ in range(T):
                    a, _, _ = pol.act(episode_start=(b.terminated, b.truncated), deterministic=False)
                    b.step(a)

            graphs["recurrent_baseline_loop"] = capture(torch, rloop)
            per_step["recurrent_baseline_loop"] = T
            step_paths.append("recurrent_baseline_loop")
            keep.append((rb, rpol))

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
        for k_ in step_paths:
            case[k_]["per"] = "env step (one replay = n_steps steps)"
        for k_ in launch_paths:
            case[k_]["per"] = "launch"
        for k_, v in flag_counts.items():
            case[k_].update(v)
        gae_s = statistics.median(per["gae"]) / K_gae
        case["gae"].update(bytes=set_bytes, set_bytes=set_bytes, sets=n_sets, launches_per_graph=K_gae,
                           TBs=round(set_bytes / gae_s / 1e12, 3),
                           fraction_of_hbm_spec=round(set_bytes / gae_s / HBM_PEAK_SPEC, 4),
                           fraction_of_hbm_measured=round(set_bytes / gae_s / HBM_PEAK_MEASURED, 4))
        # logits, action, reward, two flags, terminal value in; log-prob, reward, start flag out
        case["record"]["bytes"] = n * (4 * TOWERS[0][-1] + 4 + 4 + 2 + 4 + 4 + 4 + 1)
        med = {k_: case[k_]["us_median"] for k_ in names}
        lv = med["value"] if has_value else med["forward"]  # what collect() launches once for last_values
        case["per_step_us"] = {
            "collect_no_bootstrap_minus_baseline": round(med["collect_no_bootstrap"] - med["baseline_loop"], 3),
            "record": med["record"],
            "gae_over_T": round(med["gae"] / T, 3),
            "last_values_forward_over_T": round(lv / T, 3),
            "unexplained": round(med["collect_no_bootstrap"] - med["baseline_loop"] - med["record"] - med["gae"] / T
                                 - lv / T, 3),
            "bootstrap_cost": round(med["collect_bootstrap"] - med["collect_no_bootstrap"], 3),
        }
        res["cases"].append(case)
        if has_value:
            case["per_step_us"].update(
                bootstrap_cost_minus_value_flags=round(med["collect_bootstrap"] - med["collect_no_bootstrap"]
                                                       - med["value_flags"], 3),
                recurrent_collect_first_minus_baseline=round(med["recurrent_collect_first"]
                                                             - med["recurrent_baseline_loop"], 3),
                recurrent_collect_all_minus_first=round(med["recurrent_collect_all"] - med["recurrent_collect_first"], 3))
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
