#!/usr/bin/env python3
"""Rate of pe_render (PlantOSBatch.render) on the GPU: frames/s and bytes written per
second, as a fraction of the plain-store rate of the MI355X (6.0-6.3 TB/s measured,
MI355X_MICROARCH.md section HBM / the plain-store row of its atomics table).

Headline geometry (20x20, 16 rays, range 6), two shapes:
  k = 1024 frames at cell_size 8   (160 x 160 x 3 =  76.8 kB per frame, 78.6 MB per launch)
  k = 64   frames at cell_size 30  (600 x 600 x 3 = 1.08 MB per frame, 69.1 MB per launch)

Method: the envs are stepped with random actions first (a realistic mix of explored
cells and rays); each shape is warmed up, then timed with device events around `iters`
back-to-back launches, `rounds` times; the launches rotate over enough output buffers to
exceed the 256 MiB Infinity Cache, so the stores go to HBM.  A `fill_` of the same
buffers (a device memset) is timed the same way in the same run as a plain-store
comparator.  No GPU: the tool fails (there is nothing to measure on a CPU).

  python tools/render_rate.py [--out profiles/render_rate.json] [--iters 300] [--rounds 8]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(REPO, "rl-env_amd"))

STORE_RATE = (6.0e12, 6.3e12)  # measured plain-store / achievable HBM rate, bytes/s
SHAPES = [(1024, 8), (64, 30)]
GEOMETRY = dict(grid_size=20, num_plants=10, num_obstacles=12, lidar_range=6, lidar_channels=16)


def timed(torch, fn, nbuf, iters, rounds):
    """seconds per call of fn(i % nbuf): [median, min] over `rounds` windows of `iters` calls"""
    for i in range(2 * nbuf):
        fn(i % nbuf)
    torch.cuda.synchronize()
    per = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(iters):
            fn(i % nbuf)
        b.record()
        b.synchronize()
        per.append(a.elapsed_time(b) * 1e-3 / iters)
    return statistics.median(per), min(per)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--steps", type=int, default=200)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("render_rate: no GPU (a rate cannot be measured on a CPU)")
    from plantos_amd import PlantOSBatch
    from plantos_amd import _capi as C
    L = C.lib()
    dev = "cuda:0"
    n = max(k for k, _ in SHAPES)
    b = PlantOSBatch(n, seed=7, device=dev, **GEOMETRY)
    act = torch.empty(n, dtype=torch.int32, device=dev)
    for t in range(args.steps):
        b.synth_actions(7, t, out=act)
        b.step(act)
    explored = float((b.get_state(("explored",))["explored"] > 0).float().mean())
    res = {"tool": "render_rate", "device": torch.cuda.get_device_name(0), "geometry": GEOMETRY,
           "steps_before": args.steps, "explored_fraction": round(explored, 4), "iters": args.iters,
           "rounds": args.rounds, "store_rate_reference_TBps": [r / 1e12 for r in STORE_RATE], "shapes": []}
    for k, s in SHAPES:
        W = GEOMETRY["grid_size"] * s
        nbytes = k * W * W * 3
        nbuf = -(-(300 << 20) // nbytes)  # > 256 MiB in rotation
        bufs = [torch.empty((k, W, W, 3), dtype=torch.uint8, device=dev) for _ in range(nbuf)]
        idx = torch.arange(k, dtype=torch.int32, device=dev)
        # the C entry point itself (PlantOSBatch.render's argument checks would make short
        # launches host-bound); the first call builds the cell_size table and checks the result
        ptrs = [ctypes.c_void_p(t.data_ptr()) for t in bufs]
        ip, stream = ctypes.c_void_p(idx.data_ptr()), b._stream()
        C.check(L.pe_render(b.handle, k, ip, s, ptrs[0], 3 * W * W, 3 * W, stream), "pe_render")
        assert torch.equal(bufs[0], b.render(idx, cell_size=s))
        med, best = timed(torch, lambda i: L.pe_render(b.handle, k, ip, s, ptrs[i], 3 * W * W, 3 * W, stream),
                          nbuf, args.iters, args.rounds)
        fmed, fbest = timed(torch, lambda i: bufs[i].fill_(0xAB), nbuf, args.iters, args.rounds)
        res["shapes"].append({
            "k": k, "cell_size": s, "frame": [W, W, 3], "bytes_per_launch": nbytes, "buffers": nbuf,
            "us_per_launch_median": round(med * 1e6, 2), "us_per_launch_min": round(best * 1e6, 2),
            "frames_per_s": round(k / med), "TBps": round(nbytes / med / 1e12, 3),
            "fraction_of_store_rate": [round(nbytes / med / r, 3) for r in STORE_RATE],
            "fill_us_median": round(fmed * 1e6, 2), "fill_TBps": round(nbytes / fmed / 1e12, 3),
            "fraction_of_fill_rate": round(fmed / med, 3)})
        del bufs
    b.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
