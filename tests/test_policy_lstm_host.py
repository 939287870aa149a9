"""The host twin of the recurrent policy kernel (pe_policy_lstm_forward_host) against torch's
own LSTM in f64, with torch's f32 LSTM as the yardstick; the episode-start rule; pe_sigmoidf;
the sb3_contrib state-dict reader.  No GPU.

SIG_ABS is the worst absolute error of pe_sigmoidf against 1 / (1 + exp(-x)) in f64 over ALL
finite f32 inputs, measured by tools/tanh_ulp.cpp: 6.1626e-08 (1.0339
u, u = 2^-24) at x = 1.1118592, rounded up here.  test_sigmoid re-checks it on the subsample
test_policy_host.test_tanh_tau uses.
"""
import numpy as np
import pytest
import torch

from lstm_util import TorchRecurrent, lstm_state_dict
from plantos_amd import policy as P
from policy_util import obs_rows

SIG_ABS = 6.2e-8
N, T = 37, 12
MARGIN = 8.0  # the twin's deviation from f64 <= MARGIN x torch-f32's (test_twin_against_f64)


def sequence(D, seed=5, geometry=None):
    """xs f32 [T, N, D] (obs_rows' real and uniform rows, shuffled over the steps) and starts
    bool [T, N]: all set at t = 0, then random with p = 0.15."""
    rng = np.random.default_rng(seed)
    x = obs_rows(D, n=N * T, geometry=geometry)
    xs = np.ascontiguousarray(x[rng.permutation(N * T)].reshape(T, N, D))
    starts = rng.random((T, N)) < 0.15
    starts[0] = True
    return xs, starts


CASES = [(H, D, 1.0) for H in (32, 96, 256) for D in (77, 107)] + [(96, 107, 3.0)]


@pytest.mark.parametrize("H,D,scale", CASES)
def test_twin_against_f64(H, D, scale):
    """Twelve steps with carried state: the twin's worst |h|, |c|, |logit| and |value| deviation
    from torch.nn.LSTM(...).double() + f64 Linear layers (the same f32 weights) is at most 8x
    the deviation of torch's own f32 modules.  The margin: the sequential chain over K = D + H
    accumulates about sqrt(K) roundings where torch's blocked sums do not, and pe_tanhf is
    3.16 u against libm's < 1 u."""
    check_twin_against_f64(H, D, scale)


def check_twin_against_f64(H, D, scale, geometry=None):
    """test_twin_against_f64's scheme; geometry = (G, R): obs rows of that geometry (obs_rows)."""
    sd = lstm_state_dict(D, H, seed=H + D, scale=scale)
    Hp, towers, act, lstm, mlp = P.parse_lstm_state_dict(sd)
    assert Hp == H and act == "tanh"
    xs, starts = sequence(D, geometry=geometry)
    ref64 = TorchRecurrent(D, H, lstm, mlp, torch.float64, N)
    ref32 = TorchRecurrent(D, H, lstm, mlp, torch.float32, N)
    states = None
    dev_twin = dict(h=0.0, c=0.0, head=0.0)
    dev_f32 = dict(h=0.0, c=0.0, head=0.0)
    for t in range(T):
        (a, lg, v), states = P.lstm_host_forward(H, towers, lstm, mlp, act, xs[t], states, starts[t])
        r64, r32 = ref64.step(xs[t], starts[t]), ref32.step(xs[t], starts[t])
        heads = (lg, v[:, None])
        for ti in range(2):
            z64, h64, c64 = r64[ti]
            z32, h32, c32 = r32[ti]
            for key, got, y32, y64 in (("head", heads[ti], z32, z64), ("h", states[ti][0], h32, h64),
                                       ("c", states[ti][1], c32, c64)):
                dev_twin[key] = max(dev_twin[key], float(np.abs(got.astype(np.float64) - y64).max()))
                dev_f32[key] = max(dev_f32[key], float(np.abs(y32 - y64).max()))
        assert np.array_equal(a, np.argmax(lg, axis=1).astype(np.int32))
    for key in ("h", "c", "head"):
        print(f"H={H} D={D} x{scale}: {key}: twin {dev_twin[key]:.3e}, torch f32 {dev_f32[key]:.3e}, "
              f"ratio {dev_twin[key] / dev_f32[key]:.2f}")
    for key in ("h", "c", "head"):
        assert dev_twin[key] <= MARGIN * dev_f32[key], key


def test_episode_start():
    D, H = 77, 64
    sd = lstm_state_dict(D, H, seed=1)
    _, towers, act, lstm, mlp = P.parse_lstm_state_dict(sd)
    rng = np.random.default_rng(2)
    x = obs_rows(D)
    states = [(rng.uniform(-1, 1, (N, H)).astype(np.float32), rng.uniform(-2, 2, (N, H)).astype(np.float32))
              for _ in towers]
    before = [(h.copy(), c.copy()) for h, c in states]
    start = np.zeros(N, bool)
    start[::3] = True
    out_s, new_s = P.lstm_host_forward(H, towers, lstm, mlp, act, x, states, start)
    out_z, new_z = P.lstm_host_forward(H, towers, lstm, mlp, act, x, None, None)                # explicit zero state
    out_k, new_k = P.lstm_host_forward(H, towers, lstm, mlp, act, x, states, np.zeros(N, np.uint8))
    out_n, new_n = P.lstm_host_forward(H, towers, lstm, mlp, act, x, states, None)
    for (h, c), (h0, c0) in zip(states, before):  # the inputs are left alone
        assert np.array_equal(h, h0) and np.array_equal(c, c0)
    for u, v in zip(out_k, out_n):  # all-zero flags = no flags
        assert u.tobytes() == v.tobytes()
    s, k = start, ~start
    for got, zero, kept in zip(out_s[1:], out_z[1:], out_k[1:]):
        assert got[s].tobytes() == zero[s].tobytes()     # a started row = the row from a zero state, bitwise
        assert got[k].tobytes() == kept[k].tobytes()
        assert (got[k] != zero[k]).reshape(k.sum(), -1).any(axis=1).all()   # a kept row depends on its state
    for ti in range(2):
        for q in range(2):
            got, zero, kept = new_s[ti][q], new_z[ti][q], new_k[ti][q]
            assert got[s].tobytes() == zero[s].tobytes() and got[k].tobytes() == kept[k].tobytes()
            assert (got[k] != zero[k]).any(axis=1).all()
    # u8 flags with values other than 1 count as set
    out_b, _ = P.lstm_host_forward(H, towers, lstm, mlp, act, x, states, start.astype(np.uint8) * 200)
    assert out_b[1].tobytes() == out_s[1].tobytes()


def test_sigmoid():
    """pe_sigmoidf against f64 on test_tanh_tau's subsample; exact ends; NaN."""
    pos = np.arange(0, 0x7F800000, 2039, dtype=np.uint64).astype(np.uint32)
    special = np.array([0.0, 1e-45, 1.1754942e-38, 1.17549435e-38, 0.55, 9.1, 9.02, 88.0, 1e30, 3.4028235e38, np.inf],
                       np.float32).view(np.uint32)
    near = np.concatenate([np.arange(-2000, 2001, dtype=np.int64) + int(np.array(v, np.float32).view(np.uint32))
                           for v in (0.55, 9.1, 9.02, 1.0, 1.1, 18.2, 1.1118592)]).astype(np.uint32)
    bits = np.concatenate([pos, special, near])
    bits = np.concatenate([bits, bits | np.uint32(0x80000000)])
    x = bits.view(np.float32)
    assert x.size >= 1_000_000
    y = P.math_host("sigmoid", x)
    with np.errstate(over="ignore"):
        exact = 1.0 / (1.0 + np.exp(-x.astype(np.float64)))
    err = np.abs(y.astype(np.float64) - exact)
    print(f"worst {err.max():.4e} at x = {x[err.argmax()]!r}")
    assert err.max() <= SIG_ABS
    assert ((y == 0.0) | (y >= np.float32(2.0 ** -25))).all() and (y <= 1.0).all()   # no subnormal results
    edge = np.array([0.0, -0.0, np.inf, -np.inf, 100.0, -100.0, 3e38, -3e38], np.float32)
    assert np.array_equal(P.math_host("sigmoid", edge), np.array([0.5, 0.5, 1, 0, 1, 0, 1, 0], np.float32))
    assert not np.signbit(P.math_host("sigmoid", np.array([-np.inf, -100.0], np.float32))).any()
    assert np.isnan(P.math_host("sigmoid", np.array([np.nan], np.float32))[0])
    assert P.C.lib().pe_policy_math_host(3, 0, None, None) == P.C.PE_ERR_ARG


def test_parse_lstm_state_dict():
    D, H = 77, 64
    x = obs_rows(D)
    sd = lstm_state_dict(D, H, hidden=(128, 64), seed=3)
    Hp, towers, act, lstm, mlp = P.parse_lstm_state_dict(sd)
    assert Hp == H and towers == [[128, 64, 5], [128, 64, 1]] and act == "tanh"
    assert lstm[0][0] is sd["lstm_actor.weight_ih_l0"] and lstm[1][3] is sd["lstm_critic.bias_hh_l0"]
    assert mlp[0][2][0] is sd["action_net.weight"] and mlp[1][0][1] is sd["mlp_extractor.value_net.0.bias"]
    assert [tuple(t.shape) for t in lstm[0]] == [(4 * H, D), (4 * H, H), (4 * H,), (4 * H,)]
    assert P.parse_lstm_state_dict(sd, activation="relu")[2] == "relu"
    ref = TorchRecurrent(D, H, lstm, mlp, torch.float32, N)
    states = None
    for t in range(3):
        start = np.zeros(N, bool) if t else np.ones(N, bool)
        (a, lg, v), states = P.lstm_host_forward(H, towers, lstm, mlp, act, x, states, start)
        r = ref.step(x, start)
        assert np.allclose(lg, r[0][0], rtol=0, atol=1e-5) and np.allclose(v, r[1][0][:, 0], rtol=0, atol=1e-5)
        assert np.allclose(states[0][0], r[0][1], rtol=0, atol=1e-5) and np.allclose(states[1][1], r[1][2], rtol=0, atol=1e-5)

    actor = lstm_state_dict(D, H, critic=False, seed=3)
    Hp, towers, act, lstm, mlp = P.parse_lstm_state_dict(actor)
    assert towers == [[64, 64, 5]] and len(lstm) == 1 and len(mlp) == 1
    (a, lg, v), st = P.lstm_host_forward(H, towers, lstm, mlp, act, x)
    assert v is None and lg.shape == (N, 5) and len(st) == 1

    lin = torch.nn.Linear(D, H)
    linear_critic = dict(lstm_state_dict(D, H, critic=False))
    linear_critic["critic.weight"], linear_critic["critic.bias"] = lin.weight, lin.bias      # enable_critic_lstm=False
    two_layers = dict(sd)
    for k in P.LSTM_KEYS:
        two_layers["lstm_actor." + k.replace("_l0", "_l1")] = sd["lstm_actor.weight_hh_l0" if "weight" in k else "lstm_actor." + k]
    shared = dict(sd)
    shared["mlp_extractor.shared_net.0.weight"], shared["mlp_extractor.shared_net.0.bias"] = lin.weight, lin.bias
    no_chain = dict(sd)
    no_chain["lstm_critic.weight_hh_l0"] = torch.zeros(4 * 32, 32)
    no_head = {k: v for k, v in sd.items() if not k.startswith("value_net.")}
    bad = [linear_critic, two_layers, shared, no_chain, no_head,
           lstm_state_dict(D, 48), lstm_state_dict(D, 544), lstm_state_dict(D, H, hidden=(48,)),
           lstm_state_dict(D, H, hidden=()), {"foo.weight": lin.weight}]
    for b in bad:
        with pytest.raises(ValueError):
            P.parse_lstm_state_dict(b)
        with pytest.raises(ValueError):
            P.RecurrentPolicy.from_state_dict(None, b)
    with pytest.raises(ValueError, match="K-streamed"):
        P.check_lstm_hidden(2562)
