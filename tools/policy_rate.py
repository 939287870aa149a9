#!/usr/bin/env python3
"""Time of one policy forward on the GPU (pe_policy_forward; plantos_amd.Policy), against the
path a user had without it.

Headline geometry (20x20, 16 rays, range 6, D = 107) with obs_codes, 65536 and 4096 envs,
the two reference nets: A2C's separate pi / vf towers [256, 256] with Tanh and DQN's
Q-network [512, 512, 256] with ReLU.  Per case, HIP-event times of
  (a) pe_policy_forward from the step's byte codes,
  (b) pe_policy_forward from f32 obs,
  (c) pe_expand_obs_codes + the same net as torch modules on the device + argmax
      (both towers for A2C, as model.predict evaluates them),
each as microseconds per call and as a fraction of the f32 matrix peak (157.3 TFLOP/s;
2 * multiply-adds * envs over the time).

Method: the envs are stepped with synthetic actions first; every path is warmed up; then
`rounds` rounds, each timing one window of `iters` back-to-back calls per path with device
events, the order of the paths rotating from round to round; median, min and max over the
rounds are reported (the spread).  No GPU: the tool fails.

  python tools/policy_rate.py [--out profiles/policy_rate.json] [--iters 50] [--rounds 9]
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

F32_MATRIX_PEAK = 157.3e12  # FLOP/s, v_mfma_f32_32x32x2_f32 on every CU at the peak clock
GEOMETRY = dict(grid_size=20, num_plants=10, num_obstacles=12, lidar_range=6, lidar_channels=16)
NETS = {"a2c": ([[256, 256, 5], [256, 256, 1]], "tanh"), "dqn": ([[512, 512, 256, 5]], "relu")}


def window(torch, fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--envs", type=int, nargs="*", default=[65536, 4096])
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("policy_rate: no GPU (a time cannot be measured on a CPU)")
    from plantos_amd import PlantOSBatch, Policy
    from plantos_amd import _capi as C
    L = C.lib()
    dev = "cuda:0"
    res = {"tool": "policy_rate", "device": torch.cuda.get_device_name(0), "geometry": GEOMETRY,
           "steps_before": args.steps, "iters": args.iters, "rounds": args.rounds,
           "f32_matrix_peak_TFLOPs": F32_MATRIX_PEAK / 1e12, "cases": []}
    P = ctypes.c_void_p
    for n in args.envs:
        b = PlantOSBatch(n, seed=7, device=dev, obs_codes=True, **GEOMETRY)
        D = b.obs_dim
        act = torch.empty(n, dtype=torch.int32, device=dev)
        for t in range(args.steps):
            b.synth_actions(7, t, out=act)
            b.step(act)
        codes = b.obs
        f32 = b.expand_codes(b.io)[0]
        scratch = torch.empty_like(f32)
        for name, (towers, actv) in NETS.items():
            torch.manual_seed(1)
            mods = []
            for t in towers:
                k, layers = D, []
                for i, w in enumerate(t):
                    layers.append(torch.nn.Linear(k, w))
                    if i < len(t) - 1:
                        layers.append(torch.nn.Tanh() if actv == "tanh" else torch.nn.ReLU())
                    k = w
                mods.append(torch.nn.Sequential(*layers).to(dev))
            tensors = [[(m.weight, m.bias) for m in seq if isinstance(m, torch.nn.Linear)] for seq in mods]
            pol = Policy(b, towers, actv).load(tensors)
            a_out, lg, v = pol.actions, pol.logits, pol.values
            stream = b._stream()
            fwd = L.pe_policy_forward
            args_common = (0, 0, 0, P(a_out.data_ptr()), P(lg.data_ptr()), P(v.data_ptr()) if v is not None else None,
                           stream)
            cp, fp, sp, io = P(codes.data_ptr()), P(f32.data_ptr()), P(scratch.data_ptr()), P(b.io.data_ptr())

            def path_a():
                fwd(pol._p, cp, 1, *args_common)

            def path_b():
                fwd(pol._p, fp, 0, *args_common)

            @torch.no_grad()
            def path_c():
                L.pe_expand_obs_codes(b.handle, 1, n, io, b.io_bytes(), sp, None, None, None, stream)
                out = [m(scratch) for m in mods]
                return out[0].argmax(dim=1)

            paths = {"a_codes": path_a, "b_f32": path_b, "c_torch": path_c}
            for fn in paths.values():  # warm-up: code objects, GEMM algorithm choice
                for _ in range(5):
                    fn()
            torch.cuda.synchronize()
            C.check(fwd(pol._p, cp, 1, *args_common), "pe_policy_forward")
            agree = float((path_c().to(torch.int32) == a_out).float().mean())
            per = {k: [] for k in paths}
            order = list(paths)
            for r in range(args.rounds):
                for k in order[r % 3:] + order[:r % 3]:
                    per[k].append(window(torch, paths[k], args.iters))
            macs = sum(kk * w for t in towers for kk, w in zip([D] + t[:-1], t))
            case = {"envs": n, "net": name, "towers": towers, "activation": actv, "env_tile": pol.env_tile,
                    "macs_per_env": macs, "flop_per_call": 2 * macs * n,
                    "argmax_agreement_with_torch": round(agree, 5)}
            for k, v_ in per.items():
                med = statistics.median(v_)
                case[k] = {"us_median": round(med * 1e6, 2), "us_min": round(min(v_) * 1e6, 2),
                           "us_max": round(max(v_) * 1e6, 2),
                           "fraction_of_f32_matrix_peak": round(2 * macs * n / med / F32_MATRIX_PEAK, 4)}
            case["c_over_a"] = round(case["c_torch"]["us_median"] / case["a_codes"]["us_median"], 3)
            res["cases"].append(case)
            pol.close()
        b.close()
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
