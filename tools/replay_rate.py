#!/usr/bin/env python3
"""Time of DQN replay collection on the GPU (plantos_amd.ReplayCollector), against the plain
act / step loop it wraps.

Headline geometry (20x20, 16 rays, range 6, D = 107) with obs_codes, 65536 envs, DQN's
Q-network [512, 512, 256] with ReLU, buffer_size 2,000,000 (K = 30 slots), eps = 0.5, every
env at its own step count (bench.py's desynchronize; --sync leaves them together).  Each path on
a batch and policies of its own, captured once with torch.cuda.graph and replayed:
  baseline_loop   2 x { policy.act(); batch.step() } -- the loop a user had before
  collect         collect(2): act -> select -> step -> store, twice (an even k: no row copy)
each as microseconds per env step (replay time / 2); and alone, several launches back to back
in a graph (so a time includes one dependent-launch boundary, and for store and sample the
one-thread launch that advances the counter):
  select          pe_replay_select over n envs
  store           pe_replay_store of one step (the slots rotate: the counter advances)
  sample_B        pe_replay_sample for B = 64, 4096, 65536 from the full ring; its bytes (2 B D
                  read, 2 B D + 17 B written, 9 B of scalars read) over the time, against the
                  float4-copy rate DESIGN.md cites
  target          pe_replay_target over B = 65536
  targets_B       ReplayCollector.targets end to end (target net forward over B rows + target)
`expectation` compares collect with baseline_loop + select + store.

Method: every path is warmed up (and replayed) before timing; then `rounds` rounds, each timing
one window of replays per path with device events, the order of the paths rotating from round
to round; median, min and max over the rounds.  The batches run with prefetch_every=0: a
captured step cannot carry the host-side schedule of the prefetch launches.  No GPU: the tool
fails.

  python tools/replay_rate.py [--out profiles/replay_rate.json] [--rounds 9] [--sync]
"""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)

HBM_PEAK_MEASURED = 6.29e12  # B/s, float4 copy
GEOMETRY = dict(grid_size=20, num_plants=10, num_obstacles=12, lidar_range=6, lidar_channels=16)
QNET = [[512, 512, 256, 5]]
SAMPLE_B = (64, 4096, 65536)


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


def reps(fn, K):
    def run():
        for _ in range(K):
            fn()
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--buffer-size", type=int, default=2_000_000)
    ap.add_argument("--window-ms", type=float, default=120.0, help="target length of one timed window")
    ap.add_argument("--sync", action="store_true", help="leave every env at the same step count")
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(REPO, "rl-env_amd"))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("replay_rate: no GPU (a time cannot be measured on a CPU)")
    from plantos_amd import PlantOSBatch, Policy, ReplayCollector
    from plantos_amd import _capi as CA
    from plantos_amd.replay import select_device, store_device, target_device
    dev, n = "cuda:0", args.envs
    D = 5 * GEOMETRY["lidar_channels"] + 27
    res = {"tool": "replay_rate", "device": torch.cuda.get_device_name(0), "geometry": GEOMETRY, "envs": n,
           "towers": QNET, "obs_codes": True, "prefetch_every": 0, "rounds": args.rounds, "desync": not args.sync,
           "buffer_size": args.buffer_size, "eps": 0.5, "window_ms_target": args.window_ms,
           "hbm_float4_copy_TBs": HBM_PEAK_MEASURED / 1e12}
    torch.manual_seed(1)
    tensors, k = [[]], D
    for w in QNET[0]:
        lin = torch.nn.Linear(k, w)
        tensors[0].append((lin.weight.detach(), lin.bias.detach()))
        k = w

    def fresh():
        b = PlantOSBatch(n, seed=7, device=dev, obs_codes=True, prefetch_every=0, **GEOMETRY)
        pol = Policy(b, QNET, "relu").load(tensors)
        if not args.sync:  # every env at its own step count (bench.py's desynchronize)
            sc = b.get_state()["scalars"]
            g = torch.Generator(device="cpu").manual_seed(1)
            sc[:, CA.PE_S_STEP] = torch.randint(0, 1000, (n,), generator=g, dtype=torch.int32).to(sc.device)
            b.set_state(scalars=sc)
        act = torch.empty(n, dtype=torch.int32, device=dev)
        for t in range(8):  # the io buffer holds codes; the envs have left their reset state
            b.synth_actions(7, t, out=act)
            b.step(act)
        return b, pol

    keep, graphs, per = [], {}, {}
    b0, pol0 = fresh()

    def loop():
        for _ in range(2):
            a, _, _ = pol0.act(deterministic=True)
            b0.step(a)

    graphs["baseline_loop"], per["baseline_loop"] = capture(torch, loop), 2
    keep.append((b0, pol0))

    b, pol = fresh()
    rc = ReplayCollector(b, pol, buffer_size=args.buffer_size, seed=3)
    rc.set_eps(0.5)
    graphs["collect"], per["collect"] = capture(torch, lambda: rc.collect(2)), 2
    for _ in range(rc.K // 2 + 1):  # fill the ring
        graphs["collect"].replay()
    torch.cuda.synchronize()
    keep.append((b, pol))
    res.update(K=rc.K, ring_bytes=2 * rc.K * n * D + 9 * rc.K * n, env_tile=pol.env_tile)

    # the kernels alone, on a collector of their own (its counters move, the timed collect's do not)
    b2, pol2 = fresh()
    rs = ReplayCollector(b2, pol2, buffer_size=args.buffer_size, seed=3)
    rs.set_eps(0.5)
    for _ in range(rs.K + 1):
        rs.collect(2)
    torch.cuda.synchronize()
    tgt = Policy(b2, QNET, "relu").load(tensors)
    keep.append((b2, pol2, tgt))
    A = QNET[0][-1]
    K_small, K_big = 64, 16
    graphs["select"] = capture(torch, reps(lambda: select_device(rs.greedy, A, rs._eps, rs.ctrl, rs.seed, 0, rs.actions),
                                           K_small))
    per["select"] = K_small
    obs, rew, te, tr = rs._views[0]
    nxt = rs._views[1][0]

    def one_store():
        store_device(rs.ring, rs.geometry, obs, rs.actions, nxt, rew, te, tr, b2.terminal_obs, rs.ctrl,
                     episode_return=b2.episode_return, episode_length=b2.episode_length, ep_count=rs.ep_count,
                     ep_return_sum=rs.ep_return_sum, ep_length_sum=rs.ep_length_sum)

    graphs["store"], per["store"] = capture(torch, reps(one_store, K_big)), K_big
    for B in SAMPLE_B:
        K_s = K_small if B <= 4096 else K_big
        graphs[f"sample_{B}"], per[f"sample_{B}"] = capture(torch, reps(lambda B=B: rs.sample(B), K_s)), K_s
        mb = rs.sample(B)
        graphs[f"targets_{B}"] = capture(torch, reps(lambda mb=mb: rs.targets(mb, tgt), 4))
        per[f"targets_{B}"] = 4
    mb = rs.sample(65536)
    graphs["target"] = capture(torch, reps(lambda: target_device(mb._next_q, mb.rewards, mb.dones, 0.99, mb.targets),
                                           K_small))
    per["target"] = K_small

    names = list(graphs)
    iters = {}
    for k_ in names:  # replays per window, from one probe window
        one = window(torch, graphs[k_].replay, 3)
        iters[k_] = max(3, int(args.window_ms * 1e-3 / one))
    times = {k_: [] for k_ in names}
    for r in range(args.rounds):
        s = r % len(names)
        for k_ in names[s:] + names[:s]:
            times[k_].append(window(torch, graphs[k_].replay, iters[k_]))
    res["replays_per_window"] = iters
    for k_ in names:
        res[k_] = stats(times[k_], 1.0 / per[k_])
        res[k_]["per"] = "env step (one replay = 2 steps)" if k_ in ("baseline_loop", "collect") else "launch"
    # obs + next obs in and out, action / reward / flags in, ring scalars out
    res["store"]["bytes"] = n * (4 * D + 4 + 4 + 2 + 9)
    for B in SAMPLE_B:
        by = B * (4 * D + 9 + 9 + 8)
        s_ = res[f"sample_{B}"]["us_median"] * 1e-6
        res[f"sample_{B}"].update(bytes=by, TBs=round(by / s_ / 1e12, 4),
                                  fraction_of_float4_copy=round(by / s_ / HBM_PEAK_MEASURED, 4))
    by = res["store"]["bytes"]
    s_ = res["store"]["us_median"] * 1e-6
    res["store"].update(TBs=round(by / s_ / 1e12, 4), fraction_of_float4_copy=round(by / s_ / HBM_PEAK_MEASURED, 4))
    med = {k_: res[k_]["us_median"] for k_ in names}
    spread = {k_: res[k_]["us_max"] - res[k_]["us_min"] for k_ in names}
    res["expectation"] = {
        "collect": med["collect"],
        "baseline_plus_select_plus_store": round(med["baseline_loop"] + med["select"] + med["store"], 3),
        "unexplained": round(med["collect"] - med["baseline_loop"] - med["select"] - med["store"], 3),
        "spread_of_the_four": round(sum(spread[k_] for k_ in ("collect", "baseline_loop", "select", "store")), 3),
    }
    del graphs
    for item in keep:
        for x in item[1:]:
            x.close()
        item[0].close()
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
