#!/usr/bin/env python3
"""Time of one recurrent policy forward on the GPU (pe_policy_forward_lstm;
plantos_amd.RecurrentPolicy), against the path a user had without it.

Headline geometry (20x20, 16 rays, range 6, D = 107) with obs_codes, 65536 and 4096 envs,
the reference's family: RecurrentPPO("MlpLstmPolicy") with H = 256, net_arch [128, 128],
actor and critic each with its own LSTM.  Per case, HIP-event times of
  (a) pe_policy_forward_lstm from the step's byte codes with the step's terminated /
      truncated buffers as the start flags (state in HBM, updated in place),
  (a1) the same with the actor tower only (what predict() evaluates): where (a)'s time goes,
  (b) pe_expand_obs_codes + torch.nn.LSTM and Linear modules on the device, the state masked
      by the flags as SB3 does ((1 - episode_start) * state), + argmax,
each as microseconds per call and as a fraction of the f32 matrix peak (157.3 TFLOP/s;
2 * multiply-adds * envs over the time).

Method: the envs are stepped with synthetic actions first; every path is warmed up; then
`rounds` rounds, each timing one window of `iters` back-to-back calls per path with device
events, the order of the paths rotating from round to round; median, min and max over the
rounds are reported (the spread).  No GPU: the tool fails.

  python tools/lstm_policy_rate.py [--out profiles/lstm_policy_rate.json] [--iters 30] [--rounds 9]
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
HIDDEN = 256
TOWERS = [[128, 128, 5], [128, 128, 1]]


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
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--envs", type=int, nargs="*", default=[65536, 4096])
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("lstm_policy_rate: no GPU (a time cannot be measured on a CPU)")
    from plantos_amd import PlantOSBatch, RecurrentPolicy
    from plantos_amd import _capi as C
    L = C.lib()
    dev = "cuda:0"
    H = HIDDEN
    res = {"tool": "lstm_policy_rate", "device": torch.cuda.get_device_name(0), "geometry": GEOMETRY,
           "hidden": H, "towers": TOWERS, "steps_before": args.steps, "iters": args.iters, "rounds": args.rounds,
           "f32_matrix_peak_TFLOPs": F32_MATRIX_PEAK / 1e12, "cases": []}
    P = ctypes.c_void_p
    for n in args.envs:
        b = PlantOSBatch(n, seed=7, device=dev, obs_codes=True, max_steps=25, **GEOMETRY)
        D = b.obs_dim
        act = torch.empty(n, dtype=torch.int32, device=dev)
        for t in range(args.steps):   # max_steps=25: the last step's flags are set for some envs
            b.synth_actions(7, t, out=act)
            b.step(act)
        b.truncated[::5] = 1
        codes = b.obs
        scratch = torch.empty((n, D), dtype=torch.float32, device=dev)
        torch.manual_seed(1)
        lstms, mlps = [], []
        for t in TOWERS:
            lstms.append(torch.nn.LSTM(D, H).to(dev))
            k, layers = H, []
            for i, w in enumerate(t):
                layers.append(torch.nn.Linear(k, w))
                if i < len(t) - 1:
                    layers.append(torch.nn.Tanh())
                k = w
            mlps.append(torch.nn.Sequential(*layers).to(dev))
        lt = [tuple(getattr(m, k) for k in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")) for m in lstms]
        mt = [[(m.weight, m.bias) for m in seq if isinstance(m, torch.nn.Linear)] for seq in mlps]
        pol = RecurrentPolicy(b, H, TOWERS).load((lt, mt))
        pol1 = RecurrentPolicy(b, H, TOWERS[:1], env_tile=pol.env_tile).load((lt[:1], mt[:1]))
        stream = b._stream()
        fwd = L.pe_policy_forward_lstm
        cp, sp, io = P(codes.data_ptr()), P(scratch.data_ptr()), P(b.io.data_ptr())
        te, tr = P(b.terminated.data_ptr()), P(b.truncated.data_ptr())
        args_a = (pol._p, cp, 1, te, tr, 0, 0, 0, P(pol.actions.data_ptr()), P(pol.logits.data_ptr()),
                  P(pol.values.data_ptr()), stream)
        args_a1 = (pol1._p, cp, 1, te, tr, 0, 0, 0, P(pol1.actions.data_ptr()), P(pol1.logits.data_ptr()), None, stream)
        state = [(torch.zeros(1, n, H, device=dev), torch.zeros(1, n, H, device=dev)) for _ in TOWERS]

        def path_a():
            fwd(*args_a)

        def path_a1():
            fwd(*args_a1)

        @torch.no_grad()
        def path_b():
            L.pe_expand_obs_codes(b.handle, 1, n, io, b.io_bytes(), sp, None, None, None, stream)
            keep = (1.0 - (b.terminated | b.truncated).to(torch.float32)).view(1, n, 1)
            x = scratch.unsqueeze(0)
            out = []
            for i in range(len(TOWERS)):
                h, c = state[i]
                y, state[i] = lstms[i](x, (h * keep, c * keep))
                out.append(mlps[i](y[0]))
            return out[0].argmax(dim=1)

        paths = {"a_kernel": path_a, "a1_actor_only": path_a1, "b_torch": path_b}
        for fn in paths.values():  # warm-up: code objects, GEMM algorithm choice
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        # one step of both from the same zero state: how often the two argmaxes agree
        pol.reset_states()
        state[:] = [(torch.zeros_like(h), torch.zeros_like(c)) for h, c in state]
        C.check(fwd(*args_a), "pe_policy_forward_lstm")
        agree = float((path_b().to(torch.int32) == pol.actions).float().mean())
        per = {k: [] for k in paths}
        order = list(paths)
        for r in range(args.rounds):
            for k in order[r % 3:] + order[:r % 3]:
                per[k].append(window(torch, paths[k], args.iters))
        macs_lstm = 4 * H * (D + H)
        macs_mlp = [sum(kk * w for kk, w in zip([H] + t[:-1], t)) for t in TOWERS]
        macs = {"a_kernel": 2 * macs_lstm + sum(macs_mlp), "a1_actor_only": macs_lstm + macs_mlp[0],
                "b_torch": 2 * macs_lstm + sum(macs_mlp)}
        case = {"envs": n, "env_tile": pol.env_tile, "macs_per_env": macs["a_kernel"],
                "lstm_share_of_macs": round(2 * macs_lstm / macs["a_kernel"], 4),
                "flop_per_call": 2 * macs["a_kernel"] * n, "argmax_agreement_with_torch": round(agree, 5)}
        for k, v_ in per.items():
            med = statistics.median(v_)
            case[k] = {"us_median": round(med * 1e6, 2), "us_min": round(min(v_) * 1e6, 2),
                       "us_max": round(max(v_) * 1e6, 2),
                       "fraction_of_f32_matrix_peak": round(2 * macs[k] * n / med / F32_MATRIX_PEAK, 4)}
        case["b_over_a"] = round(case["b_torch"]["us_median"] / case["a_kernel"]["us_median"], 3)
        res["cases"].append(case)
        pol.close()
        pol1.close()
        b.close()
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
