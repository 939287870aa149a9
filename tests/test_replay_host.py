"""Host checks of replay collection (no GPU): the twins pe_replay_select_host,
pe_replay_sample_indices_host and pe_replay_target_host against independent numpy restatements
of their definitions (include/plantos_batch.h, "Replay collection"), the numpy ring, the
epsilon schedule and every ValueError that needs no device.
"""
import types

import numpy as np
import pytest

from replay_util import DOMAIN_EPS, DOMAIN_SAMPLE, mulhi32, philox4x32, store_inputs

F32 = np.float32


def np_select(greedy, A, eps, steps, seed, off):
    n = len(greedy)
    x, y, _, _ = philox4x32(steps & 0xFFFFFFFF, off + np.arange(n), steps >> 32, DOMAIN_EPS, seed)
    u = (x >> 8).astype(F32) * F32(2.0 ** -24)
    explore = u < F32(eps)
    return np.where(explore, mulhi32(y, A), greedy).astype(np.int32), explore.astype(np.uint8)


def np_indices(B, n, K, steps, draws, seed):
    filled = min(steps, K)
    if filled == 0:
        return np.full((B, 2), -1, np.int32)
    x, y, _, _ = philox4x32(draws & 0xFFFFFFFF, np.arange(B), draws >> 32, DOMAIN_SAMPLE, seed)
    return np.stack([mulhi32(x, filled), mulhi32(y, n)], axis=1).astype(np.int32)


def test_philox_known_answer():
    """The restatement itself: Random123's known-answer vectors of philox4x32-10."""
    assert [int(v) for v in philox4x32(0, 0, 0, 0, 0)] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    key = (0x299F31D0 << 32) | 0xA4093822  # k0 = a4093822, k1 = 299f31d0
    got = philox4x32(0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, key)
    assert [int(v) for v in got] == [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]


@pytest.mark.parametrize("A", [2, 5, 8])
@pytest.mark.parametrize("eps", [0.0, 0.3, 1.0])
def test_select_twin_equals_numpy(A, eps):
    from plantos_amd.replay import host_select
    rng = np.random.default_rng(10 * A)
    for n, steps, seed, off in ((1, 0, 0, 0), (257, 3, 77, 0), (130, 12345, 2 ** 63 + 5, 65), (65, 2 ** 32 + 1, 9, 4000)):
        greedy = rng.integers(0, A, n).astype(np.int32)
        got, ex = host_select(greedy, A, eps, steps, seed, off, return_explored=True)
        want, wex = np_select(greedy, A, eps, steps, seed, off)
        assert got.dtype == np.int32 and np.array_equal(got, want), (n, steps)
        assert np.array_equal(ex, wex)
        assert got.min() >= 0 and got.max() < A
        if eps == 0.0:
            assert got.tobytes() == greedy.tobytes() and not ex.any()
        if eps == 1.0:
            assert ex.all()
    # an explored action is uniform over ALL actions, the greedy one included
    greedy = np.zeros(4096, np.int32)
    got = host_select(greedy, A, 1.0, 5, 1)
    assert set(got.tolist()) == set(range(A))
    # steps moves the draw; the env id offset shifts it
    a = host_select(np.zeros(130, np.int32), A, 1.0, 7, 3, 0)
    assert not np.array_equal(a, host_select(np.zeros(130, np.int32), A, 1.0, 8, 3, 0))
    assert np.array_equal(a[65:], host_select(np.zeros(65, np.int32), A, 1.0, 7, 3, 65))


def test_explored_share():
    """n = 4096, eps = 0.25: the explored share within 4 binomial sigma of 0.25 (a condition
    on fixed seeds, checked here for the seeds the GPU tests use)."""
    from plantos_amd.replay import host_select
    n, eps = 4096, 0.25
    sigma = np.sqrt(eps * (1 - eps) / n)
    for seed, steps in ((0, 0), (7, 1), (77, 1000)):
        _, ex = host_select(np.zeros(n, np.int32), 5, eps, steps, seed, return_explored=True)
        assert abs(ex.mean() - eps) <= 4 * sigma, (seed, steps, ex.mean())


@pytest.mark.parametrize("n", [1, 65])
@pytest.mark.parametrize("filled", [1, 2, 5])
def test_sample_indices_twin(n, filled):
    from plantos_amd.replay import host_sample_indices
    for K, steps in ((filled, filled), (filled, 3 * filled + 1), (filled + 3, filled)):
        for B, draws, seed in ((1, 0, 0), (63, 1, 5), (4096, 2 ** 32 + 2, 11)):
            idx = host_sample_indices(B, n, K, steps, draws, seed)
            assert idx.shape == (B, 2) and idx.dtype == np.int32
            assert np.array_equal(idx, np_indices(B, n, K, steps, draws, seed))
            assert idx[:, 0].min() >= 0 and idx[:, 0].max() < filled
            assert idx[:, 1].min() >= 0 and idx[:, 1].max() < n
    a = host_sample_indices(64, n, filled, filled, 0, 3)
    if filled * n > 1:
        assert not np.array_equal(a, host_sample_indices(64, n, filled, filled, 1, 3))  # draws moves the draw


def test_sample_covers_the_ring():
    """filled = 5, n = 65, B = 4096: every slot and every env is drawn at least once."""
    from plantos_amd.replay import host_sample_indices
    for seed, draws in ((0, 0), (77, 3)):
        idx = host_sample_indices(4096, 65, 5, 5, draws, seed)
        assert set(idx[:, 0].tolist()) == set(range(5)) and set(idx[:, 1].tolist()) == set(range(65))


def test_sample_empty_ring():
    from plantos_amd.replay import host_sample_indices
    assert np.array_equal(host_sample_indices(7, 65, 4, 0, 0, 0), np.full((7, 2), -1, np.int32))


@pytest.mark.parametrize("A", [2, 5, 8])
def test_target_twin(A):
    """Against f64: each of the product g * m and the final sum is rounded once (half an ulp,
    2^-24 relative, each), so |target - exact| <= 2^-24 (|g m| + |exact|) (1 + 2^-20); exact
    where done (the target is the reward's bits) and the first maximum is what is taken."""
    from plantos_amd.replay import host_target
    rng = np.random.default_rng(A)
    B, gamma = 257, 0.99
    q = (rng.standard_normal((B, A)) * 30.0).astype(F32)
    q[5] = q[5, 0]                       # ties: every entry the maximum
    r = rng.uniform(-10.0, 50.0, B).astype(F32)
    d = (rng.random(B) < 0.3).astype(np.uint8)
    d[:4] = (0, 1, 0, 1)
    got = host_target(q, r, d, gamma)
    assert got.dtype == F32 and got.shape == (B,)
    g = np.float64(F32(gamma))
    gm = g * q.max(axis=1).astype(np.float64)
    exact = r.astype(np.float64) + gm * (1.0 - d)
    bound = 2.0 ** -24 * (np.abs(gm) + np.abs(exact)) * (1 + 2.0 ** -20)
    assert np.all(np.abs(got.astype(np.float64) - exact) <= bound)
    assert got[d != 0].tobytes() == r[d != 0].tobytes()
    # the definition's own rounding order, restated in numpy f32
    want = r + (F32(gamma) * q.max(axis=1)) * (F32(1.0) - d.astype(F32))
    assert got.tobytes() == want.astype(F32).tobytes()
    for bad_A in (1, 9):
        with pytest.raises(ValueError):
            host_target(np.zeros((3, bad_A), F32), np.zeros(3, F32), np.zeros(3, np.uint8), 0.99)
    with pytest.raises(ValueError):
        host_target(q, r[:-1], d, 0.99)


def test_linear_eps_is_sb3s_linear_fn():
    from plantos_amd.replay import linear_eps

    def get_linear_fn(start, end, end_fraction):  # stable_baselines3/common/utils.py, 2.2.1
        def func(progress_remaining):
            if (1 - progress_remaining) > end_fraction:
                return end
            return start + (1 - progress_remaining) * (end - start) / end_fraction
        return func

    for start, end, frac in ((1.0, 0.05, 0.7), (1.0, 0.05, 0.1), (0.5, 0.5, 1.0), (0.9, 0.0, 0.33)):
        f = get_linear_fn(start, end, frac)
        for rem in np.linspace(1.0, 0.0, 41):
            assert linear_eps(1 - rem, start, end, frac) == f(rem)
    assert linear_eps(0.0) == 1.0 and linear_eps(1.0) == 0.05
    with pytest.raises(ValueError):
        linear_eps(0.5, fraction=0.0)


def test_host_ring_rules():
    """The numpy ring: slots wrap, a done env's next_obs is the codes of its terminal obs,
    done = terminated only, rows of terminal_obs of envs that are not done are never read."""
    from plantos_amd.codes import code_table
    from plantos_amd.replay import HostRing
    n, K, (G, P, Ob, R, Cn) = 65, 2, (20, 10, 12, 6, 16)
    ring = HostRing(n, K, G, Cn, R)
    tab = code_table(G, R)
    combos = set()
    for call in range(2 * K + 1):
        s = store_inputs(n, (G, R, Cn), 100 + call)
        combos |= {(int(a), int(b)) for a, b in zip(s["terminated"], s["truncated"])}
        slot = ring.add(s["obs"], s["actions"], s["next_obs"], s["reward"], s["terminated"], s["truncated"],
                        s["terminal_obs"], s["episode_return"], s["episode_length"])
        assert slot == call % K and ring.steps == call + 1 and ring.filled == min(call + 1, K)
        done = (s["terminated"] | s["truncated"]) != 0
        assert np.isnan(s["terminal_obs"][~done]).all() and not np.isnan(s["terminal_obs"][done]).any()
        assert np.array_equal(ring.next_obs[slot][~done], s["next_obs"][~done])
        assert tab[ring.next_obs[slot][done]].tobytes() == s["terminal_obs"][done].tobytes()
        assert np.array_equal(ring.dones[slot], s["terminated"])
        assert np.array_equal(ring.obs[slot], s["obs"]) and np.array_equal(ring.actions[slot], s["actions"])
        assert ring.rewards[slot].tobytes() == s["reward"].tobytes()
    assert combos == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert ring.ep_count.sum() > 0 and ring.ep_length_sum.sum() > 0


@pytest.mark.parametrize("G, Cn, R", [(20, 16, 6), (21, 10, 2), (32, 24, 9), (64, 64, 32)])
def test_encode_obs_returns_the_codes(G, Cn, R):
    """codes.encode_obs, the one Python statement of pe_replay_math.hpp's replay_encode: code rows
    that hold every distance code 0..R, both one-hot codes, every position code and the visit
    codes 80..90, expanded with code_table, come back exactly -- from the numpy form and from the
    torch form on CPU tensors.  Codes 91..95 expand to the same float as 90 (a visit count past 10
    reads as 1.0), so the encoder cannot give them back and they are left out."""
    import torch
    from plantos_amd.codes import CODE_POS, CODE_VIS, code_table, encode_obs
    rows, D = max(G, R + 1, 11), 5 * Cn + 27
    i, c = np.arange(rows)[:, None], np.arange(D)[None, :]
    codes = np.where(c % 5 == 0, (i + c // 5) % (R + 1), ((i + c) % 2) * (R + 1))      # lidar: distance, one-hot
    codes = np.where(c >= 5 * Cn, CODE_POS + (i + c) % G, codes)                       # the two position columns
    codes = np.where(c >= 5 * Cn + 2, CODE_VIS + (i + c) % 11, codes).astype(np.uint8)  # the 25 visit columns
    assert set(codes[:, 0:5 * Cn:5].ravel()) == set(range(R + 1))
    assert set(codes[:, 1:5 * Cn:5].ravel()) == {0, R + 1}
    assert set(codes[:, 5 * Cn:5 * Cn + 2].ravel()) == set(range(CODE_POS, CODE_POS + G))
    assert set(codes[:, 5 * Cn + 2:].ravel()) == set(range(CODE_VIS, CODE_VIS + 11))
    obs = code_table(G, R)[codes]
    assert obs.dtype == np.float32 and obs.shape == (rows, D)
    got = encode_obs(obs, G, Cn, R)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and np.array_equal(got, codes)
    got = encode_obs(torch.from_numpy(obs), G, Cn, R)
    assert type(got) is torch.Tensor and got.dtype is torch.uint8 and np.array_equal(got.numpy(), codes)


def _stub_policy(cls, towers, batch):
    p = object.__new__(cls)
    p.towers, p.batch = towers, batch
    return p


def test_value_errors_without_a_device():
    from plantos_amd import Policy, RecurrentPolicy
    from plantos_amd.replay import HostRing, check_batch_size, check_replay_args, host_sample_indices, host_select

    def batch(**kw):
        d = dict(num_envs=64, obs_codes=True, cfg=types.SimpleNamespace(autoreset=1))
        d.update(kw)
        return types.SimpleNamespace(**d)

    b = batch()
    q = _stub_policy(Policy, [[64, 5]], b)
    assert check_replay_args(b, q, 2_000_000) == 2_000_000 // 64
    assert check_replay_args(b, q, 64) == 1 and check_replay_args(b, q, 200) == 3
    cases = [
        (b, _stub_policy(Policy, [[64, 5], [64, 1]], b), 1000),        # two towers
        (b, _stub_policy(RecurrentPolicy, [[64, 5]], b), 1000),         # recurrent
        (b, "policy", 1000),                                            # no Policy at all
        (batch(), q, 1000),                                             # a policy of another batch
        (b, q, 63),                                                     # buffer_size < n
    ]
    f32 = batch(obs_codes=False)
    cases.append((f32, _stub_policy(Policy, [[64, 5]], f32), 1000))     # an f32 batch
    fixed = batch(cfg=types.SimpleNamespace(autoreset=0))
    cases.append((fixed, _stub_policy(Policy, [[64, 5]], fixed), 1000))  # no autoreset
    for args in cases:
        with pytest.raises(ValueError):
            check_replay_args(*args)
    for B in (0, -3, 1.5):
        with pytest.raises(ValueError):
            check_batch_size(B)
    assert check_batch_size(64) == 64
    with pytest.raises(ValueError):
        host_sample_indices(0, 65, 4, 1, 0)
    with pytest.raises(ValueError):
        host_sample_indices(8, 0, 4, 1, 0)
    for A in (1, 9):
        with pytest.raises(ValueError):
            host_select(np.zeros(4, np.int32), A, 0.5, 0)
    with pytest.raises(ValueError):
        host_select(np.zeros((2, 2), np.int32), 5, 0.5, 0)
    with pytest.raises(ValueError):
        HostRing(0, 4, 20, 16, 6)
