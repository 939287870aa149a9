"""CPU checks of the rollout definition (no GPU): pe_logf, policy_logprob and the host twins of
pe_rollout_record / pe_rollout_gae (include/plantos_batch.h, "Rollout collection").

- pe_logf against np.log in f64 on EVERY f32 in [1, 8] (where the sampler's S lies): worst
  error measured 0.835 ulp (at x = 1.4054595), asserted < 1 ulp; a coarse sweep over all
  positive normal exponents (measured 0.76 ulp, same bound); the documented special values;
- policy_logprob against an f64 log_softmax: worst absolute error measured on LOGIT_SETS
  1.444e-05 (the rows spread over +-80: a result near -160, where one f32 ulp is 1.5e-05,
  carries the rounding of l_k - max l and its own), asserted < 2x that;
- the record twin and the GAE twin against numpy restatements in explicit float32
  operations, bit for bit.
"""
import numpy as np
import pytest

from plantos_amd.policy import math_host
from plantos_amd.rollout import RolloutCollector, host_gae, host_record
from rollout_util import gae_inputs, record_inputs

F32 = np.float32
LOGF_ULP_BOUND = 1.0        # measured 0.835, rounded up to the next whole ulp
LOGPROB_MEASURED = 1.444e-05 # worst |error| on LOGIT_SETS (CPU); the assertion allows 2x


def ulp_error(x):
    """|pe_logf(x) - log(x)| in ulps of the f32 nearest to the true value."""
    y = math_host("log", x).astype(np.float64)
    ref = np.log(x.astype(np.float64))
    ulp = np.spacing(np.abs(ref.astype(F32))).astype(np.float64)
    return np.abs(y - ref) / ulp


def test_logf_every_float_in_1_8():
    lo, hi = int(F32(1).view(np.uint32)), int(F32(8).view(np.uint32))
    assert hi - lo == 3 << 23
    assert math_host("log", np.array([1.0], F32))[0] == 0.0  # (its ulp error below is 0 / ulp(0))
    worst, at = 0.0, None
    for a in range(lo + 1, hi + 1, 1 << 22):
        x = np.arange(a, min(a + (1 << 22), hi + 1), dtype=np.uint32).view(F32)
        e = ulp_error(x)
        i = int(e.argmax())
        if e[i] > worst:
            worst, at = float(e[i]), float(x[i])
    print(f"pe_logf on [1, 8]: worst {worst:.4f} ulp at {at!r}")
    assert worst < LOGF_ULP_BOUND


def test_logf_all_normal_exponents():
    rng = np.random.default_rng(0)
    man = np.concatenate([rng.integers(0, 1 << 23, 4093, dtype=np.uint32),
                          np.array([0, 1, (1 << 23) - 1], np.uint32)])
    worst = 0.0
    for ex in range(1, 255):
        x = ((np.uint32(ex) << np.uint32(23)) + man).astype(np.uint32).view(F32)
        x = x[x != 1.0]
        worst = max(worst, float(ulp_error(x).max()))
    print(f"pe_logf over all normal exponents: worst {worst:.4f} ulp")
    assert worst < LOGF_ULP_BOUND


def test_logf_special_values():
    x = np.array([np.nan, 0.0, -0.0, -1.0, -np.inf, np.inf, 1.0], F32)
    y = math_host("log", x)
    assert np.isnan(y[0]) and y[1] == -np.inf and y[2] == -np.inf
    assert y[3:5].view(np.uint32).tolist() == [0x7FC00000, 0x7FC00000]
    assert y[5] == np.inf and y[6] == 0.0 and not np.signbit(y[6])
    sub = np.array([1e-45, 1e-40, 1.1754942e-38], F32)  # subnormals get their own logarithm
    assert np.all(sub < np.finfo(F32).tiny)
    assert np.all(ulp_error(sub) < LOGF_ULP_BOUND)


# ---------------------------------------------------------------- policy_logprob
def logit_sets():
    rng = np.random.default_rng(11)
    sets = [(rng.standard_normal((2048, A)) * 3.0).astype(F32) for A in (2, 5, 8)]
    for A in (2, 5, 8):
        sets.append(np.full((4, A), [[0.0], [1.5], [-40.0], [77.0]], F32))        # all equal
        dom = (rng.standard_normal((64, A)) * 3.0).astype(F32)                    # one dominant by 100
        dom[np.arange(64), rng.integers(0, A, 64)] = dom.max(axis=1) + F32(100.0)
        sets.append(dom)
        sets.append(rng.uniform(-80.0, 80.0, (256, A)).astype(F32))               # extreme spread
        ext = rng.uniform(-80.0, 80.0, (64, A)).astype(F32)
        ext[:, 0], ext[:, -1] = -80.0, 80.0
        sets.append(ext)
    return sets


def logprob(logits, a):
    n = logits.shape[0]
    z = np.zeros(n, np.uint8)
    return host_record(logits, np.full(n, a, np.int32), np.zeros(n, F32), z, z, 0.99)[0]


def test_logprob_accuracy():
    worst = 0.0
    for l in logit_sets():
        x = l.astype(np.float64)
        x = x - x.max(axis=1, keepdims=True)
        ref = x - np.log(np.exp(x).sum(axis=1, keepdims=True))
        for a in range(l.shape[1]):
            worst = max(worst, float(np.abs(logprob(l, a).astype(np.float64) - ref[:, a]).max()))
    print(f"policy_logprob: worst |error| {worst:.3e}")
    assert worst < 2 * LOGPROB_MEASURED


# ---------------------------------------------------------------- record
def np_logprob(l, a):
    """policy_logprob restated: f32 operations one by one (exp and log are the project's)."""
    n, A = l.shape
    m = l[:, 0].copy()
    for k in range(1, A):
        m = np.where(l[:, k] > m, l[:, k], m)
    S = np.zeros(n, F32)
    za = np.zeros(n, F32)
    for k in range(A):
        z = (l[:, k] - m).astype(F32)
        S = (S + math_host("exp", z)).astype(F32)
        za = np.where(a == k, z, za)
    return (za - math_host("log", S)).astype(F32)


def np_record(l, a, r, te, tr, gamma, tv):
    g = F32(gamma)
    out = r.copy()
    if tv is not None:
        boot = (tr != 0) & (te == 0)
        prod = (g * tv).astype(F32)
        out = np.where(boot, (r + prod).astype(F32), r)
    return np_logprob(l, a), out, ((te | tr) != 0).astype(np.uint8)


@pytest.mark.parametrize("A", [2, 5, 8])
def test_record_twin_equals_numpy(A):
    n, gamma = 33, 0.99
    cnt, rs, ls = np.zeros(n, np.int32), np.zeros(n, np.float64), np.zeros(n, np.int32)
    w_cnt, w_rs, w_ls = cnt.copy(), rs.copy(), ls.copy()
    for call in range(3):
        l, a, r, te, tr, tv, er, el = record_inputs(n, A, 100 * A + call)
        assert {(int(x), int(y)) for x, y in zip(te, tr)} == {(0, 0), (0, 1), (1, 0), (1, 1)}
        for boot in (True, False):
            acc = dict(ep_count=cnt, ep_return_sum=rs, ep_length_sum=ls) if boot else {}
            got = host_record(l, a, r, te, tr, gamma, terminal_value=tv if boot else None, episode_return=er,
                              episode_length=el, **acc)
            want = np_record(l, a, r, te, tr, gamma, tv if boot else None)
            for g_, w_, what in zip(got, want, ("log_prob", "reward", "start_next")):
                assert g_.tobytes() == w_.tobytes(), f"call {call} bootstrap {boot}: {what}"
            only = (tr != 0) & (te == 0)
            assert np.array_equal(got[1] != r, only & boot)
        done = (te | tr) != 0
        w_cnt += done
        w_rs += np.where(done, er, 0.0)
        w_ls += np.where(done, el, 0).astype(np.int32)
        assert np.array_equal(cnt, w_cnt) and rs.tobytes() == w_rs.tobytes() and np.array_equal(ls, w_ls)
    assert cnt.sum() > 0


def test_record_and_gae_argument_checks():
    l, a, r, te, tr, tv, er, el = record_inputs(4, 5, 0)
    with pytest.raises(ValueError):
        host_record(np.zeros((4, 1), F32), a, r, te, tr, 0.99)
    with pytest.raises(ValueError):
        host_record(np.zeros((4, 9), F32), a, r, te, tr, 0.99)
    with pytest.raises(ValueError):
        host_record(np.zeros((0, 5), F32), a[:0], r[:0], te[:0], tr[:0], 0.99)
    with pytest.raises(ValueError):
        host_gae(np.zeros((0, 4), F32), np.zeros((0, 4), F32), np.zeros((1, 4), np.uint8), np.zeros(4, F32), 0.99, 0.95)
    with pytest.raises(ValueError):
        host_gae(np.zeros((2, 4), F32), np.zeros((2, 4), F32), np.zeros((2, 4), np.uint8), np.zeros(4, F32), 0.99, 0.95)


# ---------------------------------------------------------------- GAE
def np_gae(rewards, values, starts, last_values, gamma, gae_lambda):
    """SB3 2.2.1's RolloutBuffer.compute_returns_and_advantage in float32, one rounded
    operation per line."""
    T, n = rewards.shape
    g, gl = F32(gamma), F32(gamma * gae_lambda)
    adv = np.zeros((T, n), F32)
    last = np.zeros(n, F32)
    for t in range(T - 1, -1, -1):
        nnt = (F32(1.0) - (starts[t + 1] != 0).astype(F32)).astype(F32)
        nv = last_values if t == T - 1 else values[t + 1]
        gv = (g * nv).astype(F32)
        gvn = (gv * nnt).astype(F32)
        rg = (rewards[t] + gvn).astype(F32)
        delta = (rg - values[t]).astype(F32)
        gn = (gl * nnt).astype(F32)
        c = (gn * last).astype(F32)
        last = (delta + c).astype(F32)
        adv[t] = last
    return adv, (adv + values).astype(F32)


@pytest.mark.parametrize("T", [1, 2, 9, 33])
@pytest.mark.parametrize("density", [0.2, 0.0, 1.0])
def test_gae_twin_equals_numpy(T, density):
    r, v, s, lv = gae_inputs(T, 33, density, 7 * T + int(10 * density))
    assert density not in (0.0, 1.0) or s.min() == s.max() == int(density)
    for gamma, lam in ((0.99, 0.95), (0.99, 1.0), (1.0, 1.0), (0.9, 0.0)):
        adv, ret = host_gae(r, v, s, lv, gamma, lam)
        w_adv, w_ret = np_gae(r, v, s, lv, gamma, lam)
        assert adv.tobytes() == w_adv.tobytes(), f"advantages, gamma {gamma} lambda {lam}"
        assert ret.tobytes() == w_ret.tobytes(), f"returns, gamma {gamma} lambda {lam}"


def test_host_rollout_chains_record_and_gae():
    T, n, A = 9, 33, 5
    rng = np.random.default_rng(3)
    steps = [record_inputs(n, A, 50 + t) for t in range(T)]
    logits, actions, rewards, te, tr, tv, er, el = (np.stack(x) for x in zip(*steps))
    values = rng.uniform(-50.0, 150.0, (T, n)).astype(F32)
    lv = rng.uniform(-50.0, 150.0, n).astype(F32)
    cnt = np.zeros(n, np.int32)
    out = RolloutCollector.host_rollout(logits, actions, rewards, te, tr, values, lv, np.ones(n, np.uint8), 0.99, 0.95,
                                        terminal_values=tv, episode_return=er, episode_length=el, ep_count=cnt)
    st = np.concatenate([np.ones((1, n), np.uint8), ((te | tr) != 0).astype(np.uint8)])
    rw = np.stack([np_record(logits[t], actions[t], rewards[t], te[t], tr[t], 0.99, tv[t])[1] for t in range(T)])
    w_adv, w_ret = np_gae(rw, values, st, lv, 0.99, 0.95)
    assert out["rewards"].tobytes() == rw.tobytes()
    assert np.array_equal(out["episode_starts"], st[:T]) and np.array_equal(out["last_dones"], st[T])
    assert out["advantages"].tobytes() == w_adv.tobytes() and out["returns"].tobytes() == w_ret.tobytes()
    assert np.array_equal(cnt, st[1:].sum(axis=0))
