"""GPU checks of the replay ring, sampler and encoder and of the three collectors at the obs
lengths of tests/policy_geometries.py:

- pe_replay_store at D % 4 = 0 (e52, e72: every ring row dword-aligned), 1 (p57) and 3 (far347),
  with (G, R, C) = (8, 4, 5), (10, 5, 9), (9, 3, 6) and (33, 32, 64) in the terminal-obs encoder:
  R = 32 and G = 33 for the first time.  The inputs are a real batch's: envs cut by max_steps = 3
  and envs made to finish their map (rules_util.inject_last_cell on the batch's own state; a
  random walk never finishes one), so terminated-only, truncated-only, both and neither occur;
- pe_replay_sample at D = 52, 72, 57, 347 over planes of n K D = 0, 1 and 2 (mod 4) bytes;
- ReplayCollector, RolloutCollector and RecurrentRolloutCollector against the manual loops of
  test_gpu_replay / test_gpu_rollout / test_gpu_rollout_recurrent, reused as they are.

Everything is bit for bit.  The step kernels are asserted by policy_geometries.make.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import policy_geometries as PG
import test_gpu_rollout_recurrent as RR
from policy_util import make_tensors
from replay_util import random_codes
from rules_util import inject_last_cell
from test_gpu_replay import QNET, check_ring, dev, device_ring, host_replay, new_ctrl, np_, pads_untouched
from test_gpu_rollout import check_rollout, expected, manual_loop, new_acc

pytestmark = pytest.mark.gpu

DEV = PG.DEV


def finish_maps(b, envs):
    """Leave the listed envs of batch b one move away from a fully explored map (inject_last_cell
    on the batch's own state); returns the action per env that ends its episode."""
    st = {k: np_(v).copy() for k, v in b.get_state().items()}
    shim = SimpleNamespace(b=SimpleNamespace(cfg=SimpleNamespace(grid_size=b.grid_size), scal=st["scalars"],
                                             cells=st["cells"], visits=st["visits"], explored=st["explored"]))
    acts = inject_last_cell(shim, envs)
    b.set_state(st["cells"], st["visits"], st["explored"], st["scalars"])
    return acts


# ---------------------------------------------------------------- store
@pytest.mark.parametrize("K", [2, 5])
@pytest.mark.parametrize("n", [1, 63, 65])
@pytest.mark.parametrize("name", ["e52", "e72", "p57", "far347"])
def test_store_kernel_on_a_real_batch(name, n, K):
    """2 K + 1 steps of a max_steps = 3 batch into a ring of K slots (it wraps twice); before
    step c the envs e = c (mod 4) are made to finish their map.  After every store: the ring
    equals HostRing's, and -- with no encoder in between -- code_table[stored next obs] of every
    done env is its terminal obs, bit for bit."""
    from plantos_amd.codes import code_table
    from plantos_amd.replay import HostRing, store_device
    geo = G, R, Cn = PG.replay_geometry(name)
    b = PG.make(name, n, True, seed=11 + n + K, max_steps=3)
    D = b.obs_dim
    tab = code_table(G, R)
    assert tab.tobytes() == b.code_table().tobytes()
    host = HostRing(n, K, G, Cn, R)
    ring, flats = device_ring(n, K, D)
    ctrl = new_ctrl()
    acc = (torch.zeros(n, dtype=torch.int32, device=DEV), torch.zeros(n, dtype=torch.float64, device=DEV),
           torch.zeros(n, dtype=torch.int32, device=DEV))
    act = torch.empty(n, dtype=torch.int32, device=DEV)
    b.step(b.synth_actions(3, 1000))   # the io buffer now holds codes
    combos = set()
    for call in range(2 * K + 1):
        obs = b.obs.clone()
        T = np.arange(call % 4, n, 4)
        b.synth_actions(3, call, out=act)
        if len(T):
            act[torch.as_tensor(T, device=DEV)] = torch.as_tensor(finish_maps(b, T), device=DEV)
        nxt, rew, te, tr = (x.clone() for x in b.step(act))
        s = dict(obs=obs, actions=act, next_obs=nxt, reward=rew, terminated=te, truncated=tr, terminal_obs=b.terminal_obs,
                 episode_return=b.episode_return, episode_length=b.episode_length)
        h = {k: np_(v).copy() for k, v in s.items()}
        assert h["terminated"][T].all()
        combos |= {(int(x), int(y)) for x, y in zip(h["terminated"], h["truncated"])}
        done = (h["terminated"] | h["truncated"]) != 0
        slot = host.add(h["obs"], h["actions"], h["next_obs"], h["reward"], h["terminated"], h["truncated"],
                        h["terminal_obs"], h["episode_return"], h["episode_length"])
        store_device(ring, geo, s["obs"], s["actions"], s["next_obs"], s["reward"], s["terminated"], s["truncated"],
                     s["terminal_obs"], ctrl, episode_return=s["episode_return"], episode_length=s["episode_length"],
                     ep_count=acc[0], ep_return_sum=acc[1], ep_length_sum=acc[2])
        what = f"{name} n={n} K={K} call {call}"
        if call >= K - 1:  # every slot written at least once: the whole ring, byte for byte
            for plane, g_, w_ in zip(("obs", "next_obs", "actions", "rewards", "dones"), ring,
                                     (host.obs, host.next_obs, host.actions, host.rewards, host.dones)):
                assert np_(g_).tobytes() == w_.tobytes(), f"{plane} {what}"
        stored = np_(ring[1][slot])
        assert np.array_equal(stored[~done], h["next_obs"][~done]), f"next obs of running envs {what}"
        assert tab[stored[done]].tobytes() == h["terminal_obs"][done].tobytes(), f"terminal obs of done envs {what}"
        assert np.array_equal(np_(ring[4][slot]), h["terminated"]), f"done = terminated {what}"
        assert np.array_equal(np_(ctrl), [call + 1, 0, 0, 0])
    # both kinds of ending were seen, alone -- and with n > 1 on one env at once
    assert {(1, 0), (0, 1), (0, 0)} <= combos, combos
    assert n == 1 or (1, 1) in combos
    assert np.array_equal(np_(acc[0]), host.ep_count) and np_(acc[1]).tobytes() == host.ep_return_sum.tobytes()
    assert np.array_equal(np_(acc[2]), host.ep_length_sum) and host.ep_count.sum() > 0
    assert pads_untouched(flats)
    b.close()


# ---------------------------------------------------------------- sample
@pytest.mark.parametrize("B", [1, 17, 64, 65])
@pytest.mark.parametrize("name", ["e52", "e72", "p57", "far347"])
def test_sample_kernel(name, B):
    """Gathers from rings of random codes of the geometry: the outputs equal a numpy gather at the
    host twin's indices, the row behind the outputs is untouched.  Planes of (n, K) = (65, 2) and
    (63, 3): n K D = 2 and an odd number (mod 4) at the odd lengths (the last row's second dword
    would leave the plane), 0 at the even ones (every row dword-aligned at D = 52 and 72)."""
    from plantos_amd.replay import host_sample_indices, sample_device
    geo = PG.replay_geometry(name)
    D, seed = PG.obs_dim(name), 37
    residues = set()
    for n, K in ((65, 2), (63, 3)):
        residues.add(n * K * D % 4)
        rng = np.random.default_rng(B + n)
        planes = (random_codes(rng, K * n, geo).reshape(K, n, D), random_codes(rng, K * n, geo).reshape(K, n, D),
                  rng.integers(0, 5, (K, n)).astype(np.int32), rng.uniform(-10, 50, (K, n)).astype(np.float32),
                  rng.integers(0, 2, (K, n)).astype(np.uint8))
        ring = tuple(dev(p) for p in planes)
        for steps in (1, K, 2 * K + 1):  # filled < K, == K, wrapped
            ctrl = new_ctrl(steps, 4)
            obs = torch.full((B + 1, D), 0xEE, dtype=torch.uint8, device=DEV)
            nxt = torch.full((B + 1, D), 0xEE, dtype=torch.uint8, device=DEV)
            act = torch.full((B + 1,), -7, dtype=torch.int32, device=DEV)
            rew = torch.full((B + 1,), -7.0, device=DEV)
            dn = torch.full((B + 1,), 0xEE, dtype=torch.uint8, device=DEV)
            idx = torch.full((B + 1, 2), -7, dtype=torch.int32, device=DEV)
            sample_device(ring, ctrl, seed, obs[:B], nxt[:B], act[:B], rew[:B], dn[:B], idx[:B])
            what = f"{name} B={B} n={n} K={K} steps={steps}"
            want = host_sample_indices(B, n, K, steps, 4, seed)
            got = np_(idx[:B])
            assert np.array_equal(got, want), f"indices {what}"
            assert got[:, 0].max() < min(steps, K) and got[:, 1].max() < n
            s_, e_ = got[:, 0], got[:, 1]
            for plane, t, p in zip(("obs", "next_obs", "actions", "rewards", "dones"), (obs, nxt, act, rew, dn), planes):
                assert np_(t[:B]).tobytes() == p[s_, e_].tobytes(), f"{plane} {what}"
            for t, s in ((obs, 0xEE), (nxt, 0xEE), (act, -7), (rew, -7.0), (dn, 0xEE), (idx, -7)):
                assert bool((t[B:] == s).all()), f"padding {what}"
            assert np.array_equal(np_(ctrl), [steps, 5, 0, 0])
    assert residues == {0} if D % 4 == 0 else (2 in residues and len(residues) == 2), residues


# ---------------------------------------------------------------- ReplayCollector
@pytest.mark.parametrize("name", ["e52", "w347"])
def test_replay_collect_equals_manual_loop(name):
    """Six steps (collects of 1, 2, 1, 2) into a ring of 4 slots against host_replay on a twin
    batch; max_steps = 3: every env is cut at steps 3 and 6, so terminal obs go through the
    encoder and time-limit rows are stored as not done."""
    from plantos_amd import Policy, ReplayCollector
    n, K, eps = 65, 4, 0.5
    tensors = make_tensors(QNET, PG.obs_dim(name), 8, "var")
    b, b2 = (PG.make(name, n, True, seed=21, max_steps=3) for _ in range(2))
    pol, pol2 = (Policy(x, QNET, "relu").load(tensors) for x in (b, b2))
    rc = ReplayCollector(b, pol, buffer_size=K * n + 7, seed=123)
    assert rc.K == K and rc.geometry == PG.replay_geometry(name)
    rc.set_eps(eps)
    for k in (1, 2, 1, 2):
        rc.collect(k)
    twin = ReplayCollector(b2, pol2, buffer_size=K * n, seed=123)
    ring = twin.host_ring()
    codes, after, actions = host_replay(b2, pol2, twin, 6, eps, ring)
    check_ring(rc, ring, f"{name}: 6 steps")
    assert np.array_equal(np_(rc.ctrl), [6, 0, 0, 0])
    assert np.array_equal(np_(rc.current_obs), codes) and np.array_equal(np_(rc.actions), actions[-1])
    assert ring.ep_count.sum() >= 2 * n and len({a.tobytes() for a in actions}) > 1
    differs = limit_rows = 0
    for t in range(6 - K, 6):
        slot = t % K
        ended = (np_(rc.next_obs[slot]) != after[t]).any(axis=1)
        differs += int(ended.sum())
        if (t + 1) % 3 == 0:
            limit = np_(rc.dones[slot]) == 0
            limit_rows += int(limit.sum())
            assert (ended & limit).any(), f"step {t}: the time-limit rows hold the post-reset obs"
    assert differs > 0 and limit_rows > 0
    for x in (pol, pol2, b, b2):
        x.close()


# ---------------------------------------------------------------- RolloutCollector
@pytest.mark.parametrize("name,form", [("e72", "codes"), ("p87", "f32")])
def test_rollout_collect_equals_manual_loop(name, form):
    """collect() of 5 steps against test_gpu_rollout's manual loop and host twins, sampled and
    argmax; max_steps = 3: the time-limit bootstrap evaluates terminal obs of the new length."""
    from plantos_amd import Policy, RolloutCollector
    n, T, gamma, lam = 65, 5, 0.99, 0.95
    towers = [[64, 64, 5], [64, 64, 1]]
    tensors = make_tensors(towers, PG.obs_dim(name), 77, "var")
    for det in (False, True):
        what = f"{name} {form} det={det}"
        b, b2 = (PG.make(name, n, form == "codes", seed=21, max_steps=3) for _ in range(2))
        pol, pol2 = (Policy(x, towers, "tanh", seed=99).load(tensors) for x in (b, b2))
        col = RolloutCollector(b, pol, T, gamma=gamma, gae_lambda=lam, deterministic=det)
        ro = col.collect()
        log = manual_loop(b2, pol2, T, det)
        want = expected(log, 0, T, np.ones(n, np.uint8), log["next_values"], gamma, lam, True, new_acc(n))
        check_rollout(ro, want, what)
        obs = np_(ro.obs)
        assert obs.shape == (T, n, b.obs_dim) and obs.dtype == (np.uint8 if b.obs_codes else np.float32)
        if b.obs_codes:
            assert np.array_equal(b.code_table()[obs], log["obs"]), f"{what}: obs codes"
        assert np_(ro.obs_f32()).tobytes() == log["obs"].tobytes(), f"{what}: obs_f32"
        only = (log["truncated"] != 0) & (log["terminated"] == 0)
        assert only.any() and np.array_equal(np_(ro.rewards) != log["rewards"], only), f"{what}: bootstrapped rows"
        pol.close(), pol2.close(), b.close(), b2.close()


# ---------------------------------------------------------------- RecurrentRolloutCollector
def test_recurrent_rollout_collect_equals_manual_loop(monkeypatch):
    """test_gpu_rollout_recurrent's run_collects (H = 32, two collects of 4 steps, every state
    snapshot) on e52: that module's geometry table gets the entry for the length of this call."""
    monkeypatch.setitem(RR.GEO, "e52", dict(cfg=PG.GEO["e52"]["cfg"], codes=True))
    assert RR.H == 32
    log = RR.run_collects("e52", 65, 4, False, True, "all", collects=2)
    assert log["obs"].shape == (9, 65, PG.obs_dim("e52"))
    assert ((log["truncated"] != 0) & (log["terminated"] == 0)).any()
