"""The host twin of the policy kernel (pe_policy_forward_host) against an f64 reference with
a derived error bound, its argmax, its sampler, and the SB3 state-dict reader.  No GPU.

The bound is the standard running error bound of an fma chain, u = 2^-24,
gamma_m = m u / (1 - m u):
    pre-activation:  gamma_{K+1} (sum_k |w_jk| |x_k| + |b_j|) + sum_k |w_jk| e_k
    through tanh:    e' = e + TAU u |tanh z|     (tanh is 1-Lipschitz; TAU below)
    through relu:    e' = e
TAU is the worst error of pe_tanhf against tanh over ALL finite f32 inputs in units of
u |tanh x|, measured by tools/tanh_ulp.cpp: 3.1567 at x = 0.554013729
(1.5895 ulp of the result), rounded up here.  test_tanh_tau re-checks it on a fixed subsample.
"""

import numpy as np
import pytest
import torch

from oracle import oracle as O
from plantos_amd import policy as P
from policy_util import a2c_state_dict, dqn_state_dict, make_tensors, obs_rows

U = 2.0 ** -24
TAU = 3.16
N = 37
WEIGHT_SEED = 20251
DOMAIN_POLICY = 0x594C4F50

SHAPES = [
    ([[32, 5]], "tanh"),
    ([[64, 64, 5], [64, 64, 1]], "tanh"),
    ([[256, 256, 5], [256, 256, 1]], "tanh"),
    ([[512, 512, 256, 5]], "relu"),
]


def gamma(m):
    return m * U / (1.0 - m * U)


def reference(towers, tensors, activation, x):
    """f64 forward of the same f32 weights with the running bound; returns per tower
    (head f64 [n, out], bound f64 [n, out])."""
    out = []
    for tw in tensors:
        h = x.astype(np.float64)
        e = np.zeros_like(h)
        for l, (w, b) in enumerate(tw):
            w64, b64 = w.astype(np.float64), b.astype(np.float64)
            K = w.shape[1]
            z = h @ w64.T + b64
            ez = gamma(K + 1) * (np.abs(h) @ np.abs(w64).T + np.abs(b64)) + e @ np.abs(w64).T
            if l == len(tw) - 1:
                out.append((z, ez))
            elif activation == "tanh":
                h = np.tanh(z)
                e = ez + TAU * U * np.abs(h)
            else:
                h = np.maximum(z, 0.0)
                e = ez
    return out


@pytest.fixture(scope="module")
def cases():
    """Every (D, shape): twin outputs and the f64 reference, computed once."""
    res = []
    for scale in ("std", "var"):
        for D in (77, 107):
            x = obs_rows(D)
            for towers, act in SHAPES:
                tensors = make_tensors(towers, D, WEIGHT_SEED, scale)
                a, lg, v = P.host_forward(towers, tensors, act, x)
                res.append(dict(scale=scale, D=D, towers=towers, act=act, x=x, tensors=tensors, actions=a, logits=lg,
                                values=v, ref=reference(towers, tensors, act, x)))
    return res


def test_twin_within_bound_of_f64_reference(cases):
    for c in cases:
        z, ez = c["ref"][0]
        err = np.abs(c["logits"].astype(np.float64) - z)
        print(f"{c['scale']} D={c['D']} {c['towers']} {c['act']}: max |twin-ref| {err.max():.3e}, min bound {ez.min():.3e}, "
              f"max err/bound {(err / ez).max():.3f}")
        assert c["logits"].shape == (N, c["towers"][0][-1])
        assert (err <= ez).all()
        if len(c["towers"]) == 2:
            zv, ev = c["ref"][1]
            errv = np.abs(c["values"].astype(np.float64) - zv[:, 0])
            assert (errv <= ev[:, 0]).all()
        else:
            assert c["values"] is None


def test_argmax_matches_f64_reference(cases):
    """Rows whose f64 top-two gap exceeds twice the row's bound must agree; the excluded
    rows are at most 1 % of all rows (with WEIGHT_SEED: 0 of 296; seed 20250 gives 1)."""
    rows = excluded = 0
    for c in cases:
        if c["scale"] != "std":
            continue
        z, ez = c["ref"][0]
        srt = np.sort(z, axis=1)
        gap = srt[:, -1] - srt[:, -2]
        decided = gap > 2.0 * ez.max(axis=1)
        rows += len(z)
        excluded += int((~decided).sum())
        assert np.array_equal(c["actions"][decided], np.argmax(z, axis=1)[decided].astype(np.int32))
        # argmax is the first index of the twin's own maximum
        assert np.array_equal(c["actions"], np.argmax(c["logits"], axis=1).astype(np.int32))
    print(f"excluded {excluded} of {rows} rows")
    assert excluded <= 0.01 * rows
    assert excluded == 0


def uniforms(n, seed, off, t):
    key = [seed & 0xFFFFFFFF, seed >> 32]
    x = np.array([O.philox4x32([t, (off + e) & 0xFFFFFFFF, 0, DOMAIN_POLICY], key)[0] for e in range(n)], np.uint32)
    return (x >> 8).astype(np.float32) * np.float32(2.0 ** -24)


def test_sampler_uniform_logits_exact():
    """All-zero weights and biases: every p_a is 1, so the action is the first a with
    u * 5 < a + 1 in f32, exactly."""
    n, D = 4096, 77
    towers = [[32, 5]]
    tensors = [[(np.zeros((32, D), np.float32), np.zeros(32, np.float32)),
                (np.zeros((5, 32), np.float32), np.zeros(5, np.float32))]]
    x = np.random.default_rng(3).random((n, D), np.float32)
    seen = set()
    for seed, off, t in ((2025, 1000, 0), (0xDEADBEEF12345678, 77, 5), (1, 4000000000, 4294967295)):
        a, lg, _ = P.host_forward(towers, tensors, "tanh", x, deterministic=False, seed=seed, env_id_offset=off, t=t)
        assert not lg.any()
        us = uniforms(n, seed, off, t) * np.float32(5.0)
        assert us.dtype == np.float32
        want = np.minimum((us[:, None] >= np.arange(1, 6, dtype=np.float32)[None, :]).sum(axis=1), 4).astype(np.int32)
        assert np.array_equal(a, want)
        seen.add(a.tobytes())
        assert set(np.unique(a)) == {0, 1, 2, 3, 4}
    assert len(seen) == 3  # seed / offset / t all reach the counter


def test_sampler_matches_f64_recomputation():
    """Random weights: the sample recomputed in f64 from the twin's own logits and the same u.
    A mismatch is allowed only where u S lies within 1e-5 S of a cumulative boundary, on at
    most 0.5 % of rows (expected < 1 row of 4096; with these seeds: 0)."""
    n, D = 4096, 107
    towers = [[32, 5]]
    tensors = make_tensors(towers, D, WEIGHT_SEED + 1)
    x = obs_rows(D, n=n, seed=11)
    seed, off, t = 99, 12345, 17
    a, lg, _ = P.host_forward(towers, tensors, "tanh", x, deterministic=False, seed=seed, env_id_offset=off, t=t)
    l = lg.astype(np.float64)
    p = np.exp(l - l.max(axis=1, keepdims=True))
    cum = np.cumsum(p, axis=1)
    S = cum[:, -1]
    us = uniforms(n, seed, off, t).astype(np.float64) * S
    want = np.minimum((us[:, None] >= cum).sum(axis=1), 4)
    bad = np.nonzero(a != want)[0]
    print(f"sampler mismatches: {len(bad)} of {n}")
    for e in bad:
        assert np.abs(cum[e] - us[e]).min() <= 1e-5 * S[e]
    assert len(bad) <= 0.005 * n
    assert len(np.unique(a)) > 1


def test_tanh_tau():
    """pe_tanhf against f64 tanh on a fixed subsample (> 1e6 inputs): every 2039th f32 bit
    pattern of both signs, +-0, the subnormals' ends, the neighbourhoods of the branch
    points 0.55 and 9.1, +-large, +-inf."""
    pos = np.arange(0, 0x7F800000, 2039, dtype=np.uint64).astype(np.uint32)
    special = np.array([0.0, 1e-45, 1.1754942e-38, 1.17549435e-38, 0.55, 9.1, 9.02, 88.0, 1e30, 3.4028235e38, np.inf],
                       np.float32).view(np.uint32)
    near = np.concatenate([np.arange(-2000, 2001, dtype=np.int64) + int(np.array(v, np.float32).view(np.uint32))
                           for v in (0.55, 9.1, 9.02, 1.0)]).astype(np.uint32)
    bits = np.concatenate([pos, special, near])
    bits = np.concatenate([bits, bits | np.uint32(0x80000000)])
    x = bits.view(np.float32)
    assert x.size >= 1_000_000
    y = P.math_host("tanh", x)
    exact = np.tanh(x.astype(np.float64))
    zero = exact == 0.0
    assert not y[zero].any() and np.array_equal(np.signbit(y), np.signbit(x))
    rel = np.abs(y[~zero].astype(np.float64) - exact[~zero]) / (U * np.abs(exact[~zero]))
    print(f"worst {rel.max():.4f} u at x = {x[~zero][rel.argmax()]!r}")
    assert rel.max() <= TAU
    assert np.array_equal(P.math_host("tanh", np.array([np.inf, -np.inf, 100.0], np.float32)),
                          np.array([1.0, -1.0, 1.0], np.float32))
    assert np.isnan(P.math_host("tanh", np.array([np.nan], np.float32))[0])


def test_from_state_dict_layouts():
    D = 77
    x = obs_rows(D)
    sd = a2c_state_dict(D)
    towers, act, tensors = P.parse_state_dict(sd)
    assert towers == [[64, 64, 5], [64, 64, 1]] and act == "tanh"
    assert tensors[0][2][0] is sd["action_net.weight"] and tensors[1][0][1] is sd["mlp_extractor.value_net.0.bias"]
    a, lg, v = P.host_forward(towers, tensors, act, x)
    with torch.no_grad():
        xt = torch.as_tensor(x)
        h = xt
        for i in (0, 2):
            h = torch.tanh(torch.nn.functional.linear(h, sd[f"mlp_extractor.policy_net.{i}.weight"],
                                                      sd[f"mlp_extractor.policy_net.{i}.bias"]))
        want = torch.nn.functional.linear(h, sd["action_net.weight"], sd["action_net.bias"]).numpy()
    assert np.allclose(lg, want, rtol=0, atol=1e-5) and v.shape == (N,)
    assert P.parse_state_dict(sd, activation="relu")[1] == "relu"

    sd = dqn_state_dict(D)
    towers, act, tensors = P.parse_state_dict(sd)
    assert towers == [[64, 32, 5]] and act == "relu" and len(tensors) == 1
    a, lg, v = P.host_forward(towers, tensors, act, x)
    with torch.no_grad():
        h = torch.as_tensor(x)
        for i in (0, 2):
            h = torch.relu(torch.nn.functional.linear(h, sd[f"q_net.q_net.{i}.weight"], sd[f"q_net.q_net.{i}.bias"]))
        want = torch.nn.functional.linear(h, sd["q_net.q_net.4.weight"], sd["q_net.q_net.4.bias"]).numpy()
    assert np.allclose(lg, want, rtol=0, atol=1e-5) and v is None

    shared = dict(a2c_state_dict(D))
    lin = torch.nn.Linear(D, 64)
    shared["mlp_extractor.shared_net.0.weight"], shared["mlp_extractor.shared_net.0.bias"] = lin.weight, lin.bias
    for bad in (shared, a2c_state_dict(D, hidden=(48, 64)), dqn_state_dict(D, hidden=(48,)), {"foo.weight": lin.weight}):
        with pytest.raises(ValueError):
            P.parse_state_dict(bad)
        with pytest.raises(ValueError):
            P.Policy.from_state_dict(None, bad)
