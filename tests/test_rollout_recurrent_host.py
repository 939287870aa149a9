"""The host twin of recurrent rollout collection (RecurrentRolloutCollector.host_rollout), no GPU:
its terminal values and last_values are the policy twin's values on COPIES of the carried states,
which those calls leave alone; and its semantics against torch -- SB3's state masking, the
bootstrap value from the state after the step's forward on the terminal obs with no start flag,
last_values with the last done flags -- restated with torch modules in f64, torch's own f32
modules as the yardstick (the rule of test_policy_lstm_host.py).
"""
import numpy as np
import pytest
import torch

from lstm_util import TorchRecurrent, lstm_state_dict
from plantos_amd import RecurrentRolloutCollector
from plantos_amd import policy as P
from policy_util import obs_rows

N, T = 37, 12
MARGIN = 8.0  # the twin's deviation from f64 <= MARGIN x torch-f32's, as test_policy_lstm_host.py holds it


def inputs(D, seed=9):
    """A recorded rollout without a device: obs f32 [T + 1, N, D], terminal obs [T, N, D], actions,
    rewards, flags (all four (terminated, truncated) pairs, about one env in five done per step),
    episode statistics."""
    rng = np.random.default_rng(seed)
    rows = obs_rows(D, n=N * (2 * T + 1))
    rows = rows[rng.permutation(len(rows))]
    obs = np.ascontiguousarray(rows[:N * (T + 1)].reshape(T + 1, N, D))
    tobs = np.ascontiguousarray(rows[N * (T + 1):].reshape(T, N, D))
    te = (rng.random((T, N)) < 0.12).astype(np.uint8)
    tr = (rng.random((T, N)) < 0.12).astype(np.uint8)
    assert {(int(x), int(y)) for x, y in zip(te.ravel(), tr.ravel())} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    return dict(obs=obs, tobs=tobs, actions=rng.integers(0, 5, (T, N)).astype(np.int32),
                rewards=rng.uniform(-10, 50, (T, N)).astype(np.float32), te=te, tr=tr,
                er=rng.uniform(-200, 400, (T, N)), el=rng.integers(1, 1000, (T, N)).astype(np.int32))


def run(weights, x, start0, states0, **kw):
    Hh, towers, act, lstm, mlp = weights
    return RecurrentRolloutCollector.host_rollout(
        Hh, towers, lstm, mlp, act, x["obs"][:T], x["obs"][T], x["tobs"], x["actions"], x["rewards"], x["te"], x["tr"],
        start0, states0, 0.99, 0.95, episode_return=x["er"], episode_length=x["el"], **kw)


@pytest.mark.parametrize("H,D", [(32, 77), (96, 107)])
def test_values_come_from_copies_of_the_carried_states(H, D):
    weights = P.parse_lstm_state_dict(lstm_state_dict(D, H, seed=H))
    Hh, towers, act, lstm, mlp = weights
    x = inputs(D)
    rng = np.random.default_rng(3)
    states0 = [(rng.uniform(-1, 1, (N, H)).astype(np.float32), rng.uniform(-2, 2, (N, H)).astype(np.float32))
               for _ in towers]
    kept0 = [(h.copy(), c.copy()) for h, c in states0]
    start0 = (np.arange(N) % 3 == 0).astype(np.uint8)
    acc = (np.zeros(N, np.int32), np.zeros(N, np.float64), np.zeros(N, np.int32))
    out = run(weights, x, start0, states0, state_snapshots="all", ep_count=acc[0], ep_return_sum=acc[1],
              ep_length_sum=acc[2])
    for (h, c), (h0, c0) in zip(states0, kept0):   # the inputs are left alone
        assert np.array_equal(h, h0) and np.array_equal(c, c0)
    fwd = lambda o, st, s: P.lstm_host_forward(H, towers, lstm, mlp, act, o, st, s)  # noqa: E731
    st, start = kept0, start0
    logits = []
    for t in range(T):   # the carried states of a loop that never computes a terminal value
        for ti in range(2):
            assert out["lstm_states"][ti][0][t].tobytes() == st[ti][0].tobytes(), f"snapshot h, step {t}"
            assert out["lstm_states"][ti][1][t].tobytes() == st[ti][1].tobytes(), f"snapshot c, step {t}"
        (_, lg, v), st = fwd(x["obs"][t], st, start)
        logits.append(lg)
        assert out["values"][t].tobytes() == v.tobytes(), f"values, step {t}"
        copies = [(h.copy(), c.copy()) for h, c in st]
        tv = fwd(x["tobs"][t], copies, None)[0][2]
        assert out["terminal_values"][t].tobytes() == tv.tobytes(), f"terminal values, step {t}"
        for (h, c), (h1, c1) in zip(copies, st):
            assert np.array_equal(h, h1) and np.array_equal(c, c1)
        start = x["te"][t] | x["tr"][t]
    assert out["last_values"].tobytes() == fwd(x["obs"][T], st, start)[0][2].tobytes()
    for ti in range(2):   # the value calls advanced nothing
        assert out["final_states"][ti][0].tobytes() == st[ti][0].tobytes()
        assert out["final_states"][ti][1].tobytes() == st[ti][1].tobytes()
    # the rest is the feed-forward twin over the same steps
    from plantos_amd import RolloutCollector
    acc2 = (np.zeros(N, np.int32), np.zeros(N, np.float64), np.zeros(N, np.int32))
    ff = RolloutCollector.host_rollout(np.stack(logits), x["actions"], x["rewards"], x["te"], x["tr"], out["values"],
                                       out["last_values"], start0, 0.99, 0.95, terminal_values=out["terminal_values"],
                                       episode_return=x["er"], episode_length=x["el"], ep_count=acc2[0],
                                       ep_return_sum=acc2[1], ep_length_sum=acc2[2])
    for k, v in ff.items():
        assert out[k].tobytes() == v.tobytes(), k
    for u, v in zip(acc, acc2):
        assert u.tobytes() == v.tobytes()
    only = (x["tr"] != 0) & (x["te"] == 0)
    assert only.any() and np.array_equal(out["rewards"] != x["rewards"], only)
    # "first": one snapshot, the state before step 0; no bootstrap: no terminal values, rewards as given
    first = run(weights, x, start0, states0, state_snapshots="first", bootstrap_timeouts=False)
    for ti in range(2):
        assert first["lstm_states"][ti][0].shape == (1, N, H)
        assert first["lstm_states"][ti][0][0].tobytes() == kept0[ti][0].tobytes()
        assert first["lstm_states"][ti][1][0].tobytes() == kept0[ti][1].tobytes()
    assert first["terminal_values"] is None and first["rewards"].tobytes() == x["rewards"].tobytes()
    assert first["values"].tobytes() == out["values"].tobytes()
    with pytest.raises(ValueError):
        run(weights, x, start0, states0, state_snapshots="last")


@pytest.mark.parametrize("H,D", [(32, 77), (96, 107), (256, 107)])
def test_semantics_against_torch_f64(H, D):
    """The same loop in torch: step() masks the state with the start flags as SB3 does and carries
    it; the terminal value is a forward from the state after that step on the terminal obs with
    no flag, undone afterwards; last_values a forward on the last obs with the last done flags.
    Worst deviation of the twin's values / terminal values / last_values from the f64 modules <=
    8x that of torch's f32 modules."""
    weights = P.parse_lstm_state_dict(lstm_state_dict(D, H, seed=H + D))
    Hh, towers, act, lstm, mlp = weights
    assert act == "tanh"
    x = inputs(D, seed=H)
    start0 = np.ones(N, np.uint8)
    out = run(weights, x, start0, None)
    none = np.zeros(N, bool)

    def torch_loop(dtype):
        ref = TorchRecurrent(D, H, lstm, mlp, dtype, N)
        res = dict(values=[], terminal_values=[])
        start = start0 != 0
        for t in range(T):
            res["values"].append(ref.step(x["obs"][t], start)[1][0][:, 0])
            carried = list(ref.state)
            res["terminal_values"].append(ref.step(x["tobs"][t], none)[1][0][:, 0])
            ref.state = carried   # predict_values does not advance the collector's state
            start = (x["te"][t] | x["tr"][t]) != 0
        res["last_values"] = ref.step(x["obs"][T], start)[1][0][:, 0]
        return {k: np.asarray(v) for k, v in res.items()}

    r64, r32 = torch_loop(torch.float64), torch_loop(torch.float32)
    for key in ("values", "terminal_values", "last_values"):
        twin = float(np.abs(out[key].astype(np.float64) - r64[key]).max())
        f32 = float(np.abs(r32[key] - r64[key]).max())
        print(f"H={H} D={D}: {key}: twin {twin:.3e}, torch f32 {f32:.3e}, ratio {twin / f32:.2f}")
        assert twin <= MARGIN * f32, key
