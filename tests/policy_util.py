"""Shared inputs of the policy tests (test infra): seeded weights, obs rows, and state dicts
with Stable-Baselines3's key names built from plain torch.nn.Linear modules."""
import os

import numpy as np
import torch

from plantos_amd.codes import CODE_POS, CODE_VIS, code_table

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def make_tensors(towers, D, seed, scale="std"):
    """numpy f32 [(W, b), ..] per tower: weights 2 N(0, sigma), biases 0.1 N(0, 1).
    scale="std": sigma = 1 / fan_in -- the reading of "N(0, 1/fan_in) * 2" under which the
    argmax test's 1 % cap on undecided rows can be met at all: the bound's sum |w| e term
    grows by sum_k |w_jk| per layer, about 1.6 here.  scale="var": sigma = 1 / sqrt(fan_in),
    where that factor is 1.6 sqrt(K) (36 for K = 512), the bound of the 512-wide net
    reaches 2.5 and 68 of its 74 rows stay undecided whatever the seed; the bound test
    runs on both scales."""
    rng = np.random.default_rng(seed)
    out = []
    for t in towers:
        k, tw = D, []
        for w in t:
            tw.append(((rng.standard_normal((w, k)) * (2.0 / (k if scale == "std" else np.sqrt(k)))).astype(np.float32),
                       (rng.standard_normal(w) * 0.1).astype(np.float32)))
            k = w
        out.append(tw)
    return out


def geometry_codes(rng, rows, G, R, D):
    """u8 [rows, D] of obs codes a (grid G, range R) geometry of D = 5C + 27 values can write, every
    column from its own range: distances 0..R, one-hots 0 / R + 1, positions 96.., visits 80..90."""
    C = (D - 27) // 5
    assert D == 5 * C + 27 and C >= 1, D
    out = np.zeros((rows, D), np.uint8)
    lid = out[:, :5 * C].reshape(rows, C, 5)
    lid[..., 0] = rng.integers(0, R + 1, (rows, C))
    lid[..., 1:] = rng.integers(0, 2, (rows, C, 4)) * (R + 1)
    out[:, 5 * C:5 * C + 2] = CODE_POS + rng.integers(0, G, (rows, 2))
    out[:, 5 * C + 2:] = CODE_VIS + rng.integers(0, 11, (rows, 25))
    return out


def obs_rows(D, n=37, seed=7, geometry=None):
    """n obs rows: real env rows from the golden trajectories (spread over the rollout), then
    uniform [0, 1) rows for the last third.  geometry = (G, R): the real rows are expanded from
    that geometry's own code table instead (geometry_codes), for lengths without a trajectory."""
    rng = np.random.default_rng(seed)
    n_uni = n // 3
    n_real = n - n_uni
    if geometry is not None:
        G, R = geometry
        real = code_table(G, R)[geometry_codes(rng, n_real, G, R, D)]
        return np.ascontiguousarray(np.concatenate([real, rng.random((n_uni, D), np.float32)]).astype(np.float32))
    name = {107: "traj_g20_random.npz", 77: "traj_g21_explore.npz"}.get(D)
    path = os.path.join(GOLDEN, name) if name else None
    if path and os.path.exists(path):
        o = np.load(path)["obs"].reshape(-1, D)
        real = o[np.linspace(0, len(o) - 1, n_real).astype(int)]
    else:
        G, R = (20, 6) if D == 107 else (21, 2)
        real = code_table(G, R)[rng.integers(0, R + 2, (n_real, D))]
    return np.ascontiguousarray(np.concatenate([real, rng.random((n_uni, D), np.float32)]).astype(np.float32))


def a2c_state_dict(D, hidden=(64, 64), A=5, seed=0):
    torch.manual_seed(seed)
    sd = {}
    for net, head, out in (("policy_net", "action_net", A), ("value_net", "value_net", 1)):
        k = D
        for i, w in enumerate(hidden):
            lin = torch.nn.Linear(k, w)
            sd[f"mlp_extractor.{net}.{2 * i}.weight"], sd[f"mlp_extractor.{net}.{2 * i}.bias"] = lin.weight, lin.bias
            k = w
        lin = torch.nn.Linear(k, out)
        sd[f"{head}.weight"], sd[f"{head}.bias"] = lin.weight, lin.bias
    return sd


def dqn_state_dict(D, hidden=(64, 32), A=5, seed=0):
    torch.manual_seed(seed)
    sd, k = {}, D
    for i, w in enumerate(tuple(hidden) + (A,)):
        lin = torch.nn.Linear(k, w)
        for pre in ("q_net.q_net", "q_net_target.q_net"):
            sd[f"{pre}.{2 * i}.weight"], sd[f"{pre}.{2 * i}.bias"] = lin.weight, lin.bias
        k = w
    return sd
