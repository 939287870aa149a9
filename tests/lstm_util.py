"""Shared inputs of the recurrent policy tests (test infra): state dicts with sb3_contrib's
key names built from plain torch.nn.LSTM / nn.Linear modules, seeded weights, and torch
references (f32 and f64) of the forward pass with SB3's state masking."""
import numpy as np
import torch


def lstm_state_dict(D, H, hidden=(64, 64), A=5, critic=True, seed=0, scale=1.0):
    """RecurrentActorCriticPolicy's keys (n_lstm_layers=1, enable_critic_lstm=`critic`), torch's
    default init times `scale`."""
    torch.manual_seed(seed)
    sd = {}
    nets = [("lstm_actor", "policy_net", "action_net", A)]
    if critic:
        nets.append(("lstm_critic", "value_net", "value_net", 1))
    for lstm_name, net, head, out in nets:
        lstm = torch.nn.LSTM(D, H)
        for k in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"):
            sd[f"{lstm_name}.{k}"] = getattr(lstm, k)
        k = H
        for i, w in enumerate(hidden):
            lin = torch.nn.Linear(k, w)
            sd[f"mlp_extractor.{net}.{2 * i}.weight"], sd[f"mlp_extractor.{net}.{2 * i}.bias"] = lin.weight, lin.bias
            k = w
        lin = torch.nn.Linear(k, out)
        sd[f"{head}.weight"], sd[f"{head}.bias"] = lin.weight, lin.bias
    return {k: (v.detach() * scale).contiguous() for k, v in sd.items()}


def make_lstm_tensors(D, H, towers, seed):
    """numpy f32 (lstm_tensors, mlp_tensors) for `towers`: LSTM weights U(-a, a), a = 2 / sqrt(H)
    (twice torch's default, so the gates leave their linear range), biases 0.1 N(0, 1); MLP
    weights 2 N(0, 1 / sqrt(fan_in)), biases 0.1 N(0, 1)."""
    rng = np.random.default_rng(seed)
    a = 2.0 / np.sqrt(H)
    lstm, mlp = [], []
    for t in towers:
        lstm.append(((rng.uniform(-a, a, (4 * H, D))).astype(np.float32), (rng.uniform(-a, a, (4 * H, H))).astype(np.float32),
                     (rng.standard_normal(4 * H) * 0.1).astype(np.float32),
                     (rng.standard_normal(4 * H) * 0.1).astype(np.float32)))
        k, tw = H, []
        for w in t:
            tw.append(((rng.standard_normal((w, k)) * (2.0 / np.sqrt(k))).astype(np.float32),
                       (rng.standard_normal(w) * 0.1).astype(np.float32)))
            k = w
        mlp.append(tw)
    return lstm, mlp


class TorchRecurrent:
    """The policy in torch modules of `dtype`, loaded with the f32 weights of
    parse_lstm_state_dict's tensors; step() masks the state as SB3 does."""

    def __init__(self, D, H, lstm, mlp, dtype, n):
        self.dtype = dtype
        self.towers = []
        for (w_ih, w_hh, b_ih, b_hh), tw in zip(lstm, mlp):
            m = torch.nn.LSTM(D, H).to(dtype)
            with torch.no_grad():
                for name, x in (("weight_ih_l0", w_ih), ("weight_hh_l0", w_hh), ("bias_ih_l0", b_ih), ("bias_hh_l0", b_hh)):
                    getattr(m, name).copy_(torch.as_tensor(x).to(dtype))
            lins = [(torch.as_tensor(w).detach().to(dtype), torch.as_tensor(b).detach().to(dtype)) for w, b in tw]
            self.towers.append((m, lins))
        self.state = [(torch.zeros(1, n, H, dtype=dtype), torch.zeros(1, n, H, dtype=dtype)) for _ in self.towers]

    def step(self, x, start):
        """x f32 [n, D], start bool [n] -> per tower (head [n, out], h [n, H], c [n, H]) as f64 numpy"""
        out = []
        keep = torch.as_tensor(~np.asarray(start, bool)).to(self.dtype).view(1, -1, 1)
        xt = torch.as_tensor(x).to(self.dtype).unsqueeze(0)
        with torch.no_grad():
            for i, (m, lins) in enumerate(self.towers):
                h, c = self.state[i]
                y, (h, c) = m(xt, (h * keep, c * keep))
                self.state[i] = (h, c)
                z = y[0]
                for l, (w, b) in enumerate(lins):
                    z = torch.nn.functional.linear(z, w, b)
                    if l < len(lins) - 1:
                        z = torch.tanh(z)
                out.append(tuple(v.double().numpy() for v in (z, h[0], c[0])))
        return out
