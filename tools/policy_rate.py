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

--host-cost measures the host side of a call instead: 64 envs, the net [[32, 5], [32, 1]] (LSTM
hidden 32), K back-to-back calls and one synchronize at the end, wall time / K, for Policy.act(),
Policy.value(), RecurrentPolicy.act() and the bare ctypes pe_policy_forward (and, as *_issue, the
time of the K calls alone: where the kernel takes longer than the host, the wall time is the kernel's).  One process is one
round; --label names the side and --package-root the checkout whose plantos_amd is imported, so a
driver alternates two checkouts on one machine.  --out then collects the rounds per label, with
their medians and spread (max - min).

  python tools/policy_rate.py --host-cost --label new --out profiles/policy_host_cost.json
  python tools/policy_rate.py --host-cost --label parent --package-root <parent>/rl-env_amd --out ...

--precision bf16 measures Policy(precision="bf16") against the f32 policy: the same run and the same
method (warm-up, `rounds` windows of `iters` calls, device events, median / min / max), the headline
geometry with codes, both nets, 65536 and 4096 envs, the f32 kernel and the bf16 kernel alternating
-- the order swaps from round to round --, and the worst difference of the two kernels' heads.  Then
one RolloutCollector step (collect() of 5 steps / 5, A2C's net) with each precision, alternating the
same way.

  python tools/policy_rate.py --precision bf16 --out profiles/policy_rate_bf16.json
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)

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


HOST_COST_PATHS = ("policy_act", "policy_value", "recurrent_act", "ctypes_forward")


def host_cost(args):
    """one round: {path: microseconds per call}"""
    import torch
    from plantos_amd import PlantOSBatch, Policy, RecurrentPolicy
    from plantos_amd import _capi as C
    dev, towers, K = "cuda:0", [[32, 5], [32, 1]], args.calls
    b = PlantOSBatch(64, seed=7, device=dev, obs_codes=True, **GEOMETRY)
    b.reset()
    act = torch.empty(64, dtype=torch.int32, device=dev)
    for t in range(4):
        b.synth_actions(7, t, out=act)
        b.step(act)
    pol, rec = Policy(b, towers), RecurrentPolicy(b, 32, towers)
    P = ctypes.c_void_p
    fwd, obs = C.lib().pe_policy_forward, P(b.obs.data_ptr())
    outs = (P(pol.actions.data_ptr()), P(pol.logits.data_ptr()), P(pol.values.data_ptr()), b._stream())
    paths = {"policy_act": pol.act, "policy_value": pol.value, "recurrent_act": rec.act,
             "ctypes_forward": lambda: fwd(pol._p, obs, 1, 0, 0, 0, *outs)}
    row = {}
    for name in HOST_COST_PATHS:
        fn = paths[name]
        for _ in range(200):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(K):
            fn()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        row[name] = round((time.perf_counter() - t0) / K * 1e6, 3)
        row[name + "_issue"] = round((t1 - t0) / K * 1e6, 3)  # the host's share: the calls alone, before the synchronize
    pol.close()
    rec.close()
    b.close()
    return row


def host_cost_main(args):
    row = host_cost(args)
    print(json.dumps({"label": args.label, **row}))
    if not args.out:
        return
    doc = {"tool": "policy_rate --host-cost", "envs": 64, "towers": [[32, 5], [32, 1]], "lstm_hidden": 32,
           "calls_per_round": args.calls, "unit": "us per call (wall time / calls, one synchronize at the end)",
           "rounds": {}}
    if os.path.exists(args.out):
        with open(args.out) as f:
            doc = json.load(f)
    doc["rounds"].setdefault(args.label, []).append(row)
    doc["summary"] = {lab: {k: {"median": statistics.median(r[k] for r in rs),
                                "spread": round(max(r[k] for r in rs) - min(r[k] for r in rs), 3)}
                            for k in rs[0]} for lab, rs in doc["rounds"].items()}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(doc, indent=1) + "\n")


def spread(v):
    med = statistics.median(v)
    return {"us_median": round(med * 1e6, 2), "us_min": round(min(v) * 1e6, 2), "us_max": round(max(v) * 1e6, 2)}


def outside_both_spreads(lo, hi):
    """whether every window of `lo` is below every window of `hi`"""
    return lo["us_max"] < hi["us_min"]


def bf16_main(args):
    import torch
    from plantos_amd import PlantOSBatch, Policy, RolloutCollector
    from plantos_amd import _capi as C
    L, dev, P = C.lib(), "cuda:0", ctypes.c_void_p
    res = {"tool": "policy_rate --precision bf16", "device": torch.cuda.get_device_name(0), "geometry": GEOMETRY,
           "steps_before": args.steps, "iters": args.iters, "rounds": args.rounds, "cases": [], "rollout": []}
    precisions = ("f32", "bf16")
    for n in args.envs:
        b = PlantOSBatch(n, seed=7, device=dev, obs_codes=True, **GEOMETRY)
        D = b.obs_dim
        act = torch.empty(n, dtype=torch.int32, device=dev)
        for t in range(args.steps):
            b.synth_actions(7, t, out=act)
            b.step(act)
        codes = b.obs.clone()
        for name, (towers, actv) in NETS.items():
            torch.manual_seed(1)
            tensors = []
            for t in towers:
                k, tw = D, []
                for w in t:
                    lin = torch.nn.Linear(k, w).to(dev)
                    tw.append((lin.weight.detach(), lin.bias.detach()))
                    k = w
                tensors.append(tw)
            pols = {pr: Policy(b, towers, actv, precision=pr).load(tensors) for pr in precisions}
            stream, fwd, cp = b._stream(), L.pe_policy_forward, P(codes.data_ptr())

            def path(pol):
                tail = (0, 0, 0, P(pol.actions.data_ptr()), P(pol.logits.data_ptr()),
                        P(pol.values.data_ptr()) if pol.values is not None else None, stream)
                return lambda: fwd(pol._p, cp, 1, *tail)

            paths = {pr: path(pols[pr]) for pr in precisions}
            for fn in paths.values():
                for _ in range(5):
                    C.check(fn(), "pe_policy_forward")
            torch.cuda.synchronize()
            diff = float((pols["f32"].logits - pols["bf16"].logits).abs().max())
            agree = float((pols["f32"].actions == pols["bf16"].actions).float().mean())
            per = {pr: [] for pr in precisions}
            for r in range(args.rounds):
                for pr in (precisions if r % 2 == 0 else precisions[::-1]):
                    per[pr].append(window(torch, paths[pr], args.iters))
            macs = sum(kk * w for t in towers for kk, w in zip([D] + t[:-1], t))
            case = {"envs": n, "net": name, "towers": towers, "activation": actv, "macs_per_env": macs,
                    "env_tile": {pr: pols[pr].env_tile for pr in precisions},
                    "worst_logit_difference": diff, "argmax_agreement": round(agree, 5)}
            for pr in precisions:
                case[pr] = spread(per[pr])
                case[pr]["TFLOPs"] = round(2 * macs * n / statistics.median(per[pr]) / 1e12, 2)
            case["f32_over_bf16"] = round(case["f32"]["us_median"] / case["bf16"]["us_median"], 3)
            case["bf16_below_f32_outside_both_spreads"] = outside_both_spreads(case["bf16"], case["f32"])
            res["cases"].append(case)
            if name == "a2c":  # one collected step: collect() of 5 steps / 5
                T = 5
                cols = {pr: RolloutCollector(b, pols[pr], T) for pr in precisions}
                for col in cols.values():
                    for _ in range(3):
                        col.collect()
                torch.cuda.synchronize()
                per = {pr: [] for pr in precisions}
                for r in range(args.rounds):
                    for pr in (precisions if r % 2 == 0 else precisions[::-1]):
                        per[pr].append(window(torch, cols[pr].collect, max(args.iters // T, 1)) / T)
                row = {"envs": n, "n_steps": T, "unit": "us per collected step"}
                for pr in precisions:
                    row[pr] = spread(per[pr])
                row["f32_over_bf16"] = round(row["f32"]["us_median"] / row["bf16"]["us_median"], 3)
                res["rollout"].append(row)
            for pol in pols.values():
                pol.close()
        b.close()
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", choices=("f32", "bf16"), default="f32")
    ap.add_argument("--host-cost", action="store_true")
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--label", default="new")
    ap.add_argument("--package-root", default=os.path.join(REPO, "rl-env_amd"))
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--envs", type=int, nargs="*", default=[65536, 4096])
    args = ap.parse_args()
    sys.path.insert(0, args.package_root)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("policy_rate: no GPU (a time cannot be measured on a CPU)")
    if args.host_cost:
        return host_cost_main(args)
    if args.precision == "bf16":
        return bf16_main(args)
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
