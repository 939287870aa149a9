"""GPU checks of replay collection (pe_policy_forward_rows, pe_replay_select / _store /
_sample / _target; plantos_amd.ReplayCollector): every kernel equals its host twin bit for
bit, collect() equals a manual act / select / step / store loop on a twin batch replayed on the
host (truncations every third step, so terminal obs and time-limit rows occur), and captured
graphs advance the device counters from replay to replay.
"""
import ctypes

import numpy as np
import pytest
import torch

from policy_util import make_tensors
from replay_util import random_codes, store_inputs

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
G20 = (20, 10, 12, 6, 16)            # grid, plants, obstacles, range, channels: D = 107
GEOMETRIES = {107: (20, 6, 16), 77: (21, 2, 10)}   # (grid_size, lidar_range, lidar_channels) by D
QNET = [[64, 32, 5]]


def np_(t):
    return t.detach().cpu().numpy()


def dev(x):
    return torch.as_tensor(x, device=DEV)


def make(n, **kw):
    from plantos_amd import PlantOSBatch
    G, P, Ob, R, C = G20
    return PlantOSBatch(n, grid_size=G, num_plants=P, num_obstacles=Ob, lidar_range=R, lidar_channels=C,
                        device=DEV, obs_codes=True, **kw)


def new_ctrl(steps=0, draws=0):
    return dev(np.array([steps, draws, 0, 0], np.int64))


def device_ring(n, K, D, pad=8):
    """(ring planes, their padded flat buffers): every plane ends in `pad` sentinel elements."""
    flats = [torch.full((K * n * D + pad,), 0xEE, dtype=torch.uint8, device=DEV) for _ in range(2)]
    flats.append(torch.full((K * n + pad,), -7, dtype=torch.int32, device=DEV))
    flats.append(torch.full((K * n + pad,), -7.0, dtype=torch.float32, device=DEV))
    flats.append(torch.full((K * n + pad,), 0xEE, dtype=torch.uint8, device=DEV))
    ring = (flats[0][:K * n * D].view(K, n, D), flats[1][:K * n * D].view(K, n, D), flats[2][:K * n].view(K, n),
            flats[3][:K * n].view(K, n), flats[4][:K * n].view(K, n))
    return ring, flats


def pads_untouched(flats, pad=8):
    return all(bool((f[-pad:] == s).all()) for f, s in zip(flats, (0xEE, 0xEE, -7, -7.0, 0xEE)))


# ---------------------------------------------------------------- act_rows
@pytest.mark.parametrize("towers,act,tile", [(QNET, "relu", None), (QNET, "relu", 64),
                                             ([[32, 5], [32, 1]], "tanh", None), ([[32, 5], [32, 1]], "tanh", 64)])
def test_act_rows_equals_host_forward(towers, act, tile):
    from plantos_amd import Policy
    b = make(64, seed=3)
    D = b.obs_dim
    pol = Policy(b, towers, act, env_tile=tile).load(make_tensors(towers, D, 5, "var"))
    tab = b.code_table()
    rng = np.random.default_rng(1)
    A = towers[0][-1]
    for rows in (1, 31, 32, 33, 100, 200):
        codes = random_codes(rng, rows, GEOMETRIES[107])
        x32 = tab[codes]
        want = pol.host_forward(x32)
        for obs in (dev(codes), dev(x32)):
            a = torch.full((rows + 3,), -7, dtype=torch.int32, device=DEV)
            lg = torch.full((rows + 3, A), -7.0, device=DEV)
            v = torch.full((rows + 3,), -7.0, device=DEV) if len(towers) == 2 else None
            out = pol.act_rows(obs, out=(a[:rows], lg[:rows], v[:rows] if v is not None else None))
            what = f"{towers} tile {tile} rows {rows} {obs.dtype}"
            assert np_(out[0]).tobytes() == want[0].tobytes(), f"actions {what}"
            assert np_(out[1]).tobytes() == want[1].tobytes(), f"q-values {what}"
            assert bool((a[rows:] == -7).all()) and bool((lg[rows:] == -7.0).all()), f"padding {what}"
            if v is not None:
                assert np_(out[2]).tobytes() == want[2].tobytes() and bool((v[rows:] == -7.0).all()), f"values {what}"
        fresh = pol.act_rows(dev(codes))  # allocating form
        assert np_(fresh[0]).tobytes() == want[0].tobytes() and np_(fresh[1]).tobytes() == want[1].tobytes()
    # Policy.act is what it was: the handle's n envs
    codes = random_codes(rng, 64, GEOMETRIES[107])
    a, lg, _ = pol.act(dev(codes))
    want = pol.host_forward(tab[codes])
    assert np_(a).tobytes() == want[0].tobytes() and np_(lg).tobytes() == want[1].tobytes()
    for bad in (dev(codes)[:0], dev(codes)[:, :50], dev(codes).to(torch.int32), codes):
        with pytest.raises(ValueError):
            pol.act_rows(bad)
    pol.close()
    b.close()


def test_forward_rows_argument_errors():
    from plantos_amd import Policy, RecurrentPolicy, _capi as C
    b = make(64, seed=3)
    pol = Policy(b, QNET, "relu")
    rec = RecurrentPolicy(b, 32, [[32, 5]])
    x = torch.zeros((8, b.obs_dim), dtype=torch.uint8, device=DEV)
    a = torch.full((8,), -7, dtype=torch.int32, device=DEV)
    L, P = C.lib(), ctypes.c_void_p
    ok = [pol._p, 8, P(x.data_ptr()), 1, P(a.data_ptr()), None, None, None]
    for pos, bad in ((0, rec._p), (1, 0), (1, -1), (2, None), (4, None), (3, 2), (6, P(a.data_ptr()))):
        args = list(ok)
        args[pos] = bad
        assert L.pe_policy_forward_rows(*args) == C.PE_ERR_ARG, pos
    torch.cuda.synchronize()
    assert bool((a == -7).all())
    pol.close(), rec.close(), b.close()


# ---------------------------------------------------------------- select
@pytest.mark.parametrize("n", [1, 63, 64, 65, 200])
def test_select_kernel_equals_twin(n):
    from plantos_amd.replay import host_select, select_device
    rng = np.random.default_rng(n)
    for A in (2, 5, 8):
        greedy = rng.integers(0, A, n).astype(np.int32)
        for eps in (0.0, 0.3, 1.0):
            steps, seed, off = 3 + A, 77, 1000
            out = torch.full((n,), -7, dtype=torch.int32, device=DEV)
            ex = torch.full((n,), 9, dtype=torch.uint8, device=DEV)
            ctrl = new_ctrl(steps)
            select_device(dev(greedy), A, dev(np.float32([eps])), ctrl, seed, off, out, ex)
            want, wex = host_select(greedy, A, eps, steps, seed, off, return_explored=True)
            assert np_(out).tobytes() == want.tobytes(), f"n={n} A={A} eps={eps}"
            assert np_(ex).tobytes() == wex.tobytes()
            if eps == 0.0:
                assert np_(out).tobytes() == greedy.tobytes()
            assert np.array_equal(np_(ctrl), [steps, 0, 0, 0])  # select reads the counter, nothing else


def test_select_offsets_and_steps():
    from plantos_amd.replay import host_select, select_device, store_device
    A, seed, eps = 5, 9, dev(np.float32([0.5]))
    greedy = np.arange(130, dtype=np.int32) % A
    ctrl = new_ctrl(4)
    whole = torch.zeros(130, dtype=torch.int32, device=DEV)
    halves = torch.zeros(130, dtype=torch.int32, device=DEV)
    select_device(dev(greedy), A, eps, ctrl, seed, 0, whole)
    select_device(dev(greedy[:65]), A, eps, ctrl, seed, 0, halves[:65])
    select_device(dev(greedy[65:]), A, eps, ctrl, seed, 65, halves[65:])
    assert np_(whole).tobytes() == np_(halves).tobytes() == host_select(greedy, A, 0.5, 4, seed).tobytes()
    # in place, and again once a store has advanced `steps`
    s = store_inputs(1, GEOMETRIES[107], 0)
    ring, _ = device_ring(1, 1, 107)
    d = {k: dev(v) for k, v in s.items()}
    store_device(ring, GEOMETRIES[107], d["obs"], d["actions"], d["next_obs"], d["reward"], d["terminated"],
                 d["truncated"], d["terminal_obs"], ctrl)
    again = dev(greedy.copy())
    select_device(again, A, eps, ctrl, seed, 0, again)
    assert np_(again).tobytes() == host_select(greedy, A, 0.5, 5, seed).tobytes()
    assert np_(again).tobytes() != np_(whole).tobytes()
    assert np.array_equal(np_(ctrl), [5, 0, 0, 0])


# ---------------------------------------------------------------- store
@pytest.mark.parametrize("K", [1, 2, 5])
@pytest.mark.parametrize("n", [1, 63, 65, 200])
def test_store_kernel_equals_numpy_ring(n, K):
    from plantos_amd.codes import code_table
    from plantos_amd.replay import HostRing, store_device
    for D, geo in GEOMETRIES.items():
        G, R, Cn = geo
        host = HostRing(n, K, G, Cn, R)
        ring, flats = device_ring(n, K, D)
        ctrl = new_ctrl()
        acc = (torch.zeros(n, dtype=torch.int32, device=DEV), torch.zeros(n, dtype=torch.float64, device=DEV),
               torch.zeros(n, dtype=torch.int32, device=DEV))
        combos = set()
        tab = code_table(G, R)
        for call in range(max(2 * K + 1, 4 if n < 4 else 0)):  # the ring wraps twice; n < 4: a combination per call
            s = store_inputs(n, geo, 1000 * n + 10 * K + call)
            combos |= {(int(a), int(b)) for a, b in zip(s["terminated"], s["truncated"])}
            done = (s["terminated"] | s["truncated"]) != 0
            assert np.isnan(s["terminal_obs"][~done]).all()  # rows that must never be read
            slot = host.add(s["obs"], s["actions"], s["next_obs"], s["reward"], s["terminated"], s["truncated"],
                            s["terminal_obs"], s["episode_return"], s["episode_length"])
            d = {k: dev(v) for k, v in s.items()}
            store_device(ring, geo, d["obs"], d["actions"], d["next_obs"], d["reward"], d["terminated"], d["truncated"],
                         d["terminal_obs"], ctrl, episode_return=d["episode_return"], episode_length=d["episode_length"],
                         ep_count=acc[0], ep_return_sum=acc[1], ep_length_sum=acc[2])
            what = f"n={n} K={K} D={D} call {call}"
            if call >= K - 1:  # every slot written at least once: the whole ring, byte for byte
                for name, g_, w_ in zip(("obs", "next_obs", "actions", "rewards", "dones"), ring,
                                        (host.obs, host.next_obs, host.actions, host.rewards, host.dones)):
                    assert np_(g_).tobytes() == w_.tobytes(), f"{name} {what}"
            nxt = np_(ring[1][slot])
            assert np.array_equal(nxt[~done], s["next_obs"][~done]), f"next obs of running envs {what}"
            assert tab[nxt[done]].tobytes() == s["terminal_obs"][done].tobytes(), f"terminal obs of done envs {what}"
            assert np.array_equal(np_(ring[4][slot]), s["terminated"]), f"done = terminated {what}"
            assert np.array_equal(np_(ctrl), [call + 1, 0, 0, 0])
        assert combos == {(0, 0), (0, 1), (1, 0), (1, 1)}
        assert np.array_equal(np_(acc[0]), host.ep_count) and np_(acc[1]).tobytes() == host.ep_return_sum.tobytes()
        assert np.array_equal(np_(acc[2]), host.ep_length_sum)
        assert pads_untouched(flats)


# ---------------------------------------------------------------- sample
@pytest.mark.parametrize("B", [1, 63, 64, 65, 257])
def test_sample_kernel(B):
    from plantos_amd.replay import host_sample_indices, sample_device
    n, K, D, seed = 65, 5, 107, 31
    rng = np.random.default_rng(B)
    planes = (rng.integers(0, 256, (K, n, D)).astype(np.uint8), rng.integers(0, 256, (K, n, D)).astype(np.uint8),
              rng.integers(0, 5, (K, n)).astype(np.int32), rng.uniform(-10, 50, (K, n)).astype(np.float32),
              rng.integers(0, 2, (K, n)).astype(np.uint8))
    ring = tuple(dev(p) for p in planes)
    for steps in (2, 5, 13, 0):  # filled < K, == K, wrapped, nothing stored
        ctrl = new_ctrl(steps, 6)
        prev = None
        for draw in (6, 7):
            obs = torch.full((B + 1, D), 0xEE, dtype=torch.uint8, device=DEV)
            nxt = torch.full((B + 1, D), 0xEE, dtype=torch.uint8, device=DEV)
            act = torch.full((B + 1,), -7, dtype=torch.int32, device=DEV)
            rew = torch.full((B + 1,), -7.0, device=DEV)
            dn = torch.full((B + 1,), 0xEE, dtype=torch.uint8, device=DEV)
            idx = torch.full((B + 1, 2), -7, dtype=torch.int32, device=DEV)
            sample_device(ring, ctrl, seed, obs[:B], nxt[:B], act[:B], rew[:B], dn[:B], idx[:B])
            what = f"B={B} steps={steps} draw {draw}"
            want = host_sample_indices(B, n, K, steps, draw, seed)
            got = np_(idx[:B])
            assert np.array_equal(got, want), f"indices {what}"
            if steps == 0:
                assert (got == -1).all()
                for t in (obs, nxt, act, rew, dn):
                    assert not np_(t[:B]).any(), f"zeros {what}"
            else:
                assert got[:, 0].max() < min(steps, K)
                s_, e_ = got[:, 0], got[:, 1]
                for name, t, p in zip(("obs", "next_obs", "actions", "rewards", "dones"), (obs, nxt, act, rew, dn), planes):
                    assert np_(t[:B]).tobytes() == p[s_, e_].tobytes(), f"{name} {what}"
                if prev is not None and B > 1:
                    assert not np.array_equal(prev, got), f"consecutive draws {what}"
            prev = got
            for t, s in ((obs, 0xEE), (nxt, 0xEE), (act, -7), (rew, -7.0), (dn, 0xEE), (idx, -7)):
                assert bool((t[B:] == s).all()), f"padding {what}"
            assert np.array_equal(np_(ctrl), [steps, draw + 1, 0, 0])


# ---------------------------------------------------------------- target
@pytest.mark.parametrize("B", [1, 65, 257])
def test_target_kernel_equals_twin(B):
    from plantos_amd.replay import host_target, target_device
    rng = np.random.default_rng(B)
    for A in (2, 5, 8):
        q = (rng.standard_normal((B, A)) * 30.0).astype(np.float32)
        q[0] = q[0, 0]
        r = rng.uniform(-10.0, 50.0, B).astype(np.float32)
        d = (np.arange(B) % 3 == 1).astype(np.uint8)
        out = torch.full((B + 1,), -7.0, device=DEV)
        target_device(dev(q), dev(r), dev(d), 0.99, out[:B])
        assert np_(out[:B]).tobytes() == host_target(q, r, d, 0.99).tobytes(), f"B={B} A={A}"
        assert float(out[B]) == -7.0


# ---------------------------------------------------------------- collect() vs a manual loop
def host_replay(b, pol, rc_like, steps, eps, ring, t0=0, codes=None):
    """`steps` steps of act / host_select / step on batch b, every transition added to the numpy
    `ring`; returns (the current obs codes, the post-step obs codes of every step, the actions)."""
    from plantos_amd.codes import encode_obs
    n = b.num_envs
    G, R, Cn = rc_like.geometry
    if codes is None:
        x = b.reset(mask=torch.zeros(n, dtype=torch.uint8, device=DEV))
        codes = encode_obs(np_(x), G, Cn, R)
    after, actions = [], []
    for t in range(t0, t0 + steps):
        greedy = np_(pol.act(dev(codes))[0]).copy()
        a = rc_like.host_select(greedy, eps, t)
        nxt, rew, te, tr = (np_(v).copy() for v in b.step(dev(a)))
        ring.add(codes, a, nxt, rew, te, tr, np_(b.terminal_obs), np_(b.episode_return), np_(b.episode_length))
        after.append(nxt)
        actions.append(a)
        codes = nxt
    return codes, np.stack(after), np.stack(actions)


def check_ring(rc, ring, what):
    for name, g_, w_ in zip(("obs", "next_obs", "actions", "rewards", "dones"), rc.ring,
                            (ring.obs, ring.next_obs, ring.actions, ring.rewards, ring.dones)):
        assert np_(g_).tobytes() == w_.tobytes(), f"{what}: {name}"
    assert np.array_equal(np_(rc.ep_count), ring.ep_count), what
    assert np_(rc.ep_return_sum).tobytes() == ring.ep_return_sum.tobytes(), what
    assert np.array_equal(np_(rc.ep_length_sum), ring.ep_length_sum), what


def test_collect_equals_manual_loop():
    from plantos_amd import Policy, ReplayCollector
    n, K, eps = 65, 4, 0.5
    tensors = make_tensors(QNET, 107, 8, "var")
    b, b2 = make(n, seed=21, max_steps=3), make(n, seed=21, max_steps=3)
    pol, pol2 = (Policy(x, QNET, "relu").load(tensors) for x in (b, b2))
    rc = ReplayCollector(b, pol, buffer_size=K * n + 7, seed=123)
    assert rc.K == K
    rc.set_eps(eps)
    for k in (1, 1, 1, 2, 2, 2, 2):  # 11 steps: odd and even k
        rc.collect(k)
    twin = ReplayCollector(b2, pol2, buffer_size=K * n, seed=123)
    ring = twin.host_ring()
    codes, after, actions = host_replay(b2, pol2, twin, 11, eps, ring)
    check_ring(rc, ring, "11 steps")
    assert np.array_equal(np_(rc.ctrl), [11, 0, 0, 0]) and rc.steps == 11 and rc.draws == 0
    assert np.array_equal(np_(rc.current_obs), codes) and np.array_equal(np_(rc.actions), actions[-1])
    assert ring.ep_count.sum() >= 3 * n
    # the last K steps are in the ring: the stored next_obs of a done env is its terminal obs, not
    # the post-reset obs the step returned, and a time-limit row is not done
    differs = limit_rows = 0
    for t in range(11 - K, 11):
        slot = t % K
        stored = np_(rc.next_obs[slot])
        ended = (stored != after[t]).any(axis=1)
        differs += int(ended.sum())
        if (t + 1) % 3 == 0:  # max_steps = 3: every env is cut here
            limit = np_(rc.dones[slot]) == 0
            limit_rows += int(limit.sum())
            assert (ended & limit).any(), f"step {t}: the time-limit rows hold the post-reset obs"
    assert differs > 0 and limit_rows > 0
    for x in (pol, pol2, b, b2):
        x.close()


def test_collect_and_sample_in_graphs():
    """collect(2) captured once and replayed three times equals six manual steps (the ring wraps,
    every replay draws its own exploration); a captured sample(64) replayed twice gives the draws
    d and d + 1."""
    from plantos_amd import Policy, ReplayCollector
    n, K, eps = 200, 4, 0.5
    tensors = make_tensors(QNET, 107, 8, "var")
    b, b2 = make(n, seed=12, max_steps=3, prefetch_every=0), make(n, seed=12, max_steps=3, prefetch_every=0)
    pol, pol2 = (Policy(x, QNET, "relu").load(tensors) for x in (b, b2))
    rc = ReplayCollector(b, pol, buffer_size=K * n, seed=5)
    rc.set_eps(eps)
    rc.collect(2)  # primed, and every kernel of the chain has run before the capture
    rc.sample(64)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        rc.collect(2)
    gs = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gs):
        mb = rc.sample(64)
    twin = ReplayCollector(b2, pol2, buffer_size=K * n, seed=5)
    ring = twin.host_ring()
    codes, _, acts = host_replay(b2, pol2, twin, 2, eps, ring)
    seen = [acts[-1]]
    for it in range(3):
        gr.replay()
        torch.cuda.synchronize()
        codes, _, acts = host_replay(b2, pol2, twin, 2, eps, ring, t0=2 + 2 * it, codes=codes)
        check_ring(rc, ring, f"replay {it}")
        assert np.array_equal(np_(rc.actions), acts[-1]) and np.array_equal(np_(rc.current_obs), codes)
        seen.append(acts[-1])
    assert np.array_equal(np_(rc.ctrl), [8, 1, 0, 0])
    assert all(not np.array_equal(seen[i], seen[i + 1]) for i in range(3))
    for d in (1, 2):
        gs.replay()
        torch.cuda.synchronize()
        want = twin.host_sample_indices(64, 8, d)
        got = np_(mb.indices)
        assert np.array_equal(got, want), f"draw {d}"
        assert np_(mb.next_obs).tobytes() == ring.next_obs[got[:, 0], got[:, 1]].tobytes()
        assert np_(mb.rewards).tobytes() == ring.rewards[got[:, 0], got[:, 1]].tobytes()
    assert np.array_equal(np_(rc.ctrl), [8, 3, 0, 0])
    del gr, gs
    for x in (pol, pol2, b, b2):
        x.close()


def test_targets_end_to_end():
    from plantos_amd import Policy, ReplayBatch, ReplayCollector
    n = 64
    b = make(n, seed=2, max_steps=3)
    pol = Policy(b, QNET, "relu").load(make_tensors(QNET, 107, 8, "var"))
    tgt = Policy(b, [[32, 5]], "relu").load(make_tensors([[32, 5]], 107, 9, "var"))
    rc = ReplayCollector(b, pol, buffer_size=3 * n, seed=1)
    rc.set_eps(0.3)
    rc.collect(4)
    tab = b.code_table()
    for B in (65, 1):
        mb = rc.sample(B)
        assert isinstance(mb, ReplayBatch) and rc.sample(B) is mb
        y = rc.targets(mb, tgt, gamma=0.99)
        assert y is mb.targets
        nxt, rew, dn = np_(mb.next_obs), np_(mb.rewards), np_(mb.dones)
        _, q, _ = tgt.host_forward(tab[nxt])
        want = rc.host_target(q, rew, dn, 0.99)
        assert np_(y).tobytes() == want.tobytes(), f"B={B}"
        out = torch.zeros(B, device=DEV)
        assert rc.targets(mb, tgt, gamma=0.9, out=out) is out
        assert np_(out).tobytes() == rc.host_target(q, rew, dn, 0.9).tobytes()
        assert np_(mb.obs_f32()).tobytes() == tab[np_(mb.obs)].tobytes()
        assert np_(mb.next_obs_f32()).tobytes() == tab[nxt].tobytes()
    assert dn.dtype == np.uint8 and rc.draws == 4
    two = Policy(b, [[32, 5], [32, 1]], "tanh")
    other_A = Policy(b, [[32, 4]], "relu")
    for bad in (two, other_A, "policy"):
        with pytest.raises(ValueError):
            rc.targets(mb, bad)
    with pytest.raises(ValueError):
        rc.targets("batch", tgt)
    for B in (0, -1):
        with pytest.raises(ValueError):
            rc.sample(B)
    with pytest.raises(ValueError):
        rc.collect(0)
    for x in (pol, tgt, two, other_A):
        x.close()
    b.close()
    with pytest.raises(ValueError):
        ReplayCollector(b, pol)  # a closed batch


def test_replay_c_argument_errors():
    """The C boundary: nothing is launched for a bad argument."""
    from plantos_amd import _capi as C
    L, P = C.lib(), ctypes.c_void_p
    n, A, D = 8, 5, 107
    i = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    f = torch.full((n,), -7.0, device=DEV)
    u = torch.zeros(n, dtype=torch.uint8, device=DEV)
    q = torch.zeros((n, A), device=DEV)
    ctrl = new_ctrl(1, 1)
    p = lambda t: P(t.data_ptr())  # noqa: E731
    ok = [n, A, p(i), p(f), p(ctrl), 0, 0, p(i), None, None]
    for pos, bad in ((0, 0), (1, 1), (1, 9), (2, None), (3, None), (4, None), (7, None)):
        args = list(ok)
        args[pos] = bad
        assert L.pe_replay_select(*args) == C.PE_ERR_ARG, ("select", pos)
    ok = [n, A, p(q), p(f), p(u), 0.99, p(f), None]
    for pos, bad in ((0, 0), (1, 1), (1, 9), (2, None), (3, None), (4, None), (6, None)):
        args = list(ok)
        args[pos] = bad
        assert L.pe_replay_target(*args) == C.PE_ERR_ARG, ("target", pos)
    ring, flats = device_ring(n, 2, D)
    o = torch.full((n, D), 0xEE, dtype=torch.uint8, device=DEV)
    t32 = torch.zeros((n, D), device=DEV)
    idx = torch.full((n, 2), -7, dtype=torch.int32, device=DEV)
    ok = [n, 2, 20, 6, 16, p(o), p(i), p(o), p(f), p(u), p(u), p(t32), None, None] + [p(r) for r in ring] + \
         [None, None, None, p(ctrl), None]
    for pos, bad in ((0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (5, None), (11, None), (14, None), (18, None), (22, None),
                     (5, P(o.data_ptr() + 1)), (14, P(ring[0].data_ptr() + 2))):
        args = list(ok)
        args[pos] = bad
        assert L.pe_replay_store(*args) == C.PE_ERR_ARG, ("store", pos)
    ok = [n, n, 2, D] + [p(r) for r in ring] + [0, p(ctrl), p(o), p(o), p(i), p(f), p(u), p(idx), None]
    for pos, bad in ((0, 0), (1, 0), (2, 0), (3, 0), (4, None), (10, None), (11, None), (16, None),
                     (11, P(o.data_ptr() + 1)), (4, P(ring[0].data_ptr() + 2))):
        args = list(ok)
        args[pos] = bad
        assert L.pe_replay_sample(*args) == C.PE_ERR_ARG, ("sample", pos)
    torch.cuda.synchronize()
    assert np.array_equal(np_(ctrl), [1, 1, 0, 0]) and bool((i == -7).all()) and bool((f == -7.0).all())
    assert bool((o == 0xEE).all()) and pads_untouched(flats) and bool((ring[0] == 0xEE).all())
