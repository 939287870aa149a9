#!/usr/bin/env python3
"""Time of rollout minibatches on the GPU (Rollout.minibatches / env_minibatches), against the
route a learner had before them.

Headline geometry (20x20, 16 rays, range 6, D = 107) with obs_codes, 65536 envs, one real
collect() of n_steps T = 5 (A2C) and T = 128 under a small policy.  Per T and batch size
B in {128, 4096, 65536, T n} (row minibatches) and Be in {128, 4096} (env minibatches), two paths:
  device    K consecutive minibatches of one epoch with normalize_advantage=True: per minibatch
            one gather kernel (permutation, six fields, obs decoded from the codes) and the
            normalisation (one kernel up to 4096 elements, three above); device_gather_only: the
            same without the normalisation
  yardstick what the parent commit offers: ro.obs_f32() once per collect, torch.randperm once per
            epoch (both timed on their own, eagerly), then per minibatch six index_select and
            torch's (a - a.mean()) / (a.std() + 1e-8); env mode: the same along the env axis
each captured once with torch.cuda.graph (K minibatches per graph, the k and the index slices
baked in) and replayed, so neither side pays Python per minibatch.  Reported: microseconds per
minibatch (median [min, max] over the rounds), microseconds per epoch = minibatches per epoch x
that (+ randperm for the yardstick; derived, not run: an epoch of B = 128 at T = 128 is 65536
minibatches), the peak extra device memory of each path from torch's allocator (device: the
cached outputs; yardstick: the expanded obs, the permutation and one minibatch's outputs), and
the f32 obs bytes written per second beside the expansion kernel's own rate.

Method: every graph is replayed once before timing; then `rounds` rounds, each timing one window
of replays per path with device events, the order rotating from round to round.  No GPU: the tool
fails.

  python tools/minibatch_rate.py [--out profiles/minibatch_rate.json] [--rounds 9]
"""
import argparse
import itertools
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)

EXPAND_TBS = 5.84  # pe_expand_obs_codes, f32 bytes written per second (README)
GEOMETRY = dict(grid_size=20, num_plants=10, num_obstacles=12, lidar_range=6, lidar_channels=16)
TOWERS = [[64, 5], [64, 1]]
FIELDS = ("actions", "values", "log_probs", "advantages", "returns")


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


def peak_of(torch, fn):
    """(result, peak device bytes above what was allocated before) of one eager fn()."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    return out, torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, nargs="*", default=[5, 128])
    ap.add_argument("--window-ms", type=float, default=60.0, help="target length of one timed window")
    ap.add_argument("--max-k", type=int, default=16, help="minibatches per captured graph, at most")
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(REPO, "rl-env_amd"))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("minibatch_rate: no GPU (a time cannot be measured on a CPU)")
    from plantos_amd import PlantOSBatch, Policy, RolloutCollector
    dev, n = "cuda:0", args.envs
    D = 5 * GEOMETRY["lidar_channels"] + 27
    res = {"tool": "minibatch_rate", "device": torch.cuda.get_device_name(0), "geometry": GEOMETRY, "envs": n,
           "obs_dim": D, "obs_codes": True, "towers": TOWERS, "rounds": args.rounds, "window_ms_target": args.window_ms,
           "normalize_advantage": True, "expand_kernel_TBs_written": EXPAND_TBS,
           "epoch_us": "derived: minibatches per epoch x us per minibatch (+ randperm for the yardstick)", "cases": []}
    torch.manual_seed(1)
    tensors = []
    for t in TOWERS:
        k, tw = D, []
        for w in t:
            lin = torch.nn.Linear(k, w)
            tw.append((lin.weight.detach(), lin.bias.detach()))
            k = w
        tensors.append(tw)
    for T in args.steps:
        b = PlantOSBatch(n, seed=7, device=dev, obs_codes=True, prefetch_every=0, **GEOMETRY)
        pol = Policy(b, TOWERS, "tanh", seed=3).load(tensors)
        col = RolloutCollector(b, pol, T)
        ro = col.collect()
        M = T * n
        case = {"n_steps": T, "rows": M, "paths": []}
        # the yardstick's per-collect and per-epoch stages, eagerly
        obs32, peak_obs = peak_of(torch, ro.obs_f32)
        perm, peak_perm = peak_of(torch, lambda: torch.randperm(M, device=dev))
        eperm = torch.randperm(n, device=dev)
        flat = [getattr(ro, f).reshape(M) for f in FIELDS]
        obs3 = obs32.view(T, n, D)
        starts = ro.episode_starts.contiguous()
        case["yardstick_obs_f32"] = dict(stats([window(torch, ro.obs_f32, 3) for _ in range(args.rounds)], 1.0),
                                         bytes=obs32.numel() * 4, per="collect")
        case["yardstick_randperm"] = dict(
            stats([window(torch, lambda: torch.randperm(M, device=dev), 3) for _ in range(args.rounds)], 1.0), per="epoch")

        def yard_rows(idx):
            out = [obs32.index_select(0, idx)] + [x.index_select(0, idx) for x in flat]
            a = out[4]
            out[4] = (a - a.mean()) / (a.std() + 1e-8)
            return out

        def yard_envs(idx):
            out = [obs3.index_select(1, idx), starts.index_select(1, idx)] + [getattr(ro, f).index_select(1, idx) for f in FIELDS]
            a = out[5]
            out[5] = (a - a.mean()) / (a.std() + 1e-8)
            return out

        graphs, meta = {}, {}
        sizes = [("rows", B) for B in sorted({128, 4096, 65536, M})] + [("envs", Be) for Be in (128, 4096)]
        for mode, B in sizes:
            total = M if mode == "rows" else n
            nmb = -(-total // B)
            K = min(nmb, args.max_k)
            rows_out = B if mode == "rows" else T * B
            gen = ro.minibatches if mode == "rows" else ro.env_minibatches
            order, yard = (perm, yard_rows) if mode == "rows" else (eperm, yard_envs)

            def device_path(gen=gen, B=B, K=K, norm=True):
                for _ in itertools.islice(gen(B, epoch=1, seed=0, normalize_advantage=norm), K):
                    pass

            def yard_path(yard=yard, order=order, B=B, K=K):
                for k in range(K):
                    yard(order[k * B:(k + 1) * B])

            _, peak_dev = peak_of(torch, device_path)
            _, peak_yard = peak_of(torch, lambda: yard(order[:B]))
            for name, fn, peak in ((f"device_{mode}_{B}", device_path, peak_dev),
                                   (f"device_gather_only_{mode}_{B}", lambda f=device_path: f(norm=False), peak_dev),
                                   (f"yardstick_{mode}_{B}", yard_path, peak_yard + peak_obs + (peak_perm if mode == "rows" else 0))):
                graphs[name] = capture(torch, fn)
                meta[name] = dict(mode=mode, batch=B, rows_out=rows_out, minibatches_per_epoch=nmb, per_graph=K,
                                  peak_extra_bytes=int(peak))
        names = list(graphs)
        iters = {k_: max(2, int(args.window_ms * 1e-3 / window(torch, graphs[k_].replay, 2))) for k_ in names}
        per = {k_: [] for k_ in names}
        for r in range(args.rounds):
            s = r % len(names)
            for k_ in names[s:] + names[:s]:
                per[k_].append(window(torch, graphs[k_].replay, iters[k_]))
        rp = case["yardstick_randperm"]["us_median"]
        for k_ in names:
            m = meta[k_]
            st = stats(per[k_], 1.0 / m["per_graph"])
            epoch = st["us_median"] * m["minibatches_per_epoch"] + (rp if k_.startswith("yardstick_rows") else 0.0)
            sec = st["us_median"] * 1e-6
            case["paths"].append(dict(name=k_, **m, **st, per="minibatch", epoch_us=round(epoch, 1),
                                      obs_f32_bytes=m["rows_out"] * D * 4,
                                      obs_TBs_written=round(m["rows_out"] * D * 4 / sec / 1e12, 3),
                                      replays_per_window=iters[k_]))
        res["cases"].append(case)
        del graphs
        pol.close()
        b.close()
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
