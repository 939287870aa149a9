"""GPU checks of rollout collection (pe_rollout_record / pe_rollout_gae;
plantos_amd.RolloutCollector): the two kernels equal their host twins bit for bit, and
collect() equals a manual act / step loop on a twin batch whose recorded steps go through the
host twins -- byte codes and f32 obs, truncations every third step with the time-limit
bootstrap, sampling and argmax actions; continuity across collects, graph capture, argument
checks.
"""
import ctypes

import numpy as np
import pytest
import torch

from policy_util import make_tensors
from rollout_util import gae_inputs, record_inputs

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GEO = {"g20": dict(cfg=(20, 10, 12, 6, 16), codes=True), "g21": dict(cfg=(21, 8, 50, 2, 10), codes=False)}
TOWERS = ([[32, 5], [32, 1]], [[64, 64, 5], [64, 64, 1]])
SEED = 77
FIELDS = ("actions", "values", "log_probs", "rewards", "episode_starts", "last_dones", "advantages", "returns",
          "last_values", "ep_count", "ep_return_sum", "ep_length_sum")


def np_(t):
    return t.detach().cpu().numpy()


def dev(x):
    return torch.as_tensor(x, device=DEV)


def make(name, n, **kw):
    from plantos_amd import PlantOSBatch
    G, P, Ob, R, C = GEO[name]["cfg"]
    return PlantOSBatch(n, grid_size=G, num_plants=P, num_obstacles=Ob, lidar_range=R, lidar_channels=C,
                        device=DEV, obs_codes=GEO[name]["codes"], max_steps=3, **kw)


# ---------------------------------------------------------------- standalone kernels
@pytest.mark.parametrize("n", [1, 63, 64, 65, 200])
def test_record_kernel_equals_twin(n):
    from plantos_amd.rollout import host_record, record_device
    for A in (2, 5, 8):
        cnt, rs, ls = np.zeros(n, np.int32), np.zeros(n, np.float64), np.zeros(n, np.int32)
        d_cnt, d_rs, d_ls = dev(cnt.copy()), dev(rs.copy()), dev(ls.copy())
        for call in range(3):
            l, a, r, te, tr, tv, er, el = record_inputs(n, A, 1000 * n + 10 * A + call)
            if n >= 4:
                assert {(int(x), int(y)) for x, y in zip(te, tr)} == {(0, 0), (0, 1), (1, 0), (1, 1)}
            for boot in (True, False):
                acc = (cnt, rs, ls) if boot else (None, None, None)
                d_acc = (d_cnt, d_rs, d_ls) if boot else (None, None, None)
                want = host_record(l, a, r, te, tr, 0.99, terminal_value=tv if boot else None, episode_return=er,
                                   episode_length=el, ep_count=acc[0], ep_return_sum=acc[1], ep_length_sum=acc[2])
                lp = torch.full((n,), 7.0, device=DEV)
                ro = dev(r.copy())  # in place, as the collector runs it
                st = torch.full((n,), 9, dtype=torch.uint8, device=DEV)
                record_device(dev(l), dev(a), ro, dev(te), dev(tr), 0.99, lp, ro, st,
                              terminal_value=dev(tv) if boot else None, episode_return=dev(er), episode_length=dev(el),
                              ep_count=d_acc[0], ep_return_sum=d_acc[1], ep_length_sum=d_acc[2])
                for g_, w_, what in zip((lp, ro, st), want, ("log_prob", "reward", "start_next")):
                    assert np_(g_).tobytes() == w_.tobytes(), f"n={n} A={A} call {call} bootstrap {boot}: {what}"
            assert np.array_equal(np_(d_cnt), cnt) and np_(d_rs).tobytes() == rs.tobytes()
            assert np.array_equal(np_(d_ls), ls)


def run_gae(T, n, density, seed, pad=0):
    """(device advantages, returns) and the twin's, for every (gamma, lambda); pad > 0: every
    array lives in wider rows (row stride > n)."""
    from plantos_amd.rollout import gae_device, host_gae
    r, v, s, lv = gae_inputs(T, n, density, seed)

    def wide(x, extra, fill):
        if not pad:
            return dev(x)
        w = torch.full((x.shape[0], n + extra), fill, dtype=dev(x[:1]).dtype, device=DEV)
        w[:, :n] = dev(x)
        return w[:, :n]

    d_r, d_v, d_s = wide(r, pad, 1e9), wide(v, pad + 3, 1e9), wide(s, pad + 9, 1)
    for gamma, lam in ((0.99, 0.95), (0.99, 1.0), (1.0, 1.0), (0.9, 0.0)):
        out = torch.full((2, T, n + pad), -7.0, device=DEV)
        adv, ret = out[0, :, :n], out[1, :, :n]
        gae_device(d_r, d_v, d_s, dev(lv), gamma, lam, adv, ret)
        w_adv, w_ret = host_gae(r, v, s, lv, gamma, lam)
        what = f"T={T} n={n} density={density} gamma={gamma} lambda={lam} pad={pad}"
        assert np_(adv).tobytes() == w_adv.tobytes(), f"advantages {what}"
        assert np_(ret).tobytes() == w_ret.tobytes(), f"returns {what}"
        if pad:
            assert bool((out[:, :, n:] == -7.0).all()), f"padding written {what}"


@pytest.mark.parametrize("T", [1, 2, 9, 33])
@pytest.mark.parametrize("n", [1, 63, 65, 200])
def test_gae_kernel_equals_twin(T, n):
    for density in (0.2, 0.0, 1.0):
        run_gae(T, n, density, 31 * T + n)


def test_gae_kernel_large_and_padded():
    run_gae(33, 4096, 0.2, 5)
    run_gae(9, 65, 0.2, 6, pad=7)   # row strides > n, every array a different one
    run_gae(17, 200, 0.2, 7, pad=56)


# ---------------------------------------------------------------- collect() vs a manual loop
def manual_loop(b, pol, steps, det):
    """`steps` steps of act / step on batch b, everything a rollout needs recorded as numpy
    [steps, ..]; the obs as f32.  The first obs is the batch's current one."""
    n, D = b.num_envs, b.obs_dim
    x = b.reset(mask=torch.zeros(n, dtype=torch.uint8, device=DEV),
                obs=torch.empty((n, D), dtype=torch.float32, device=DEV))
    x32 = x
    keys = ("obs", "actions", "logits", "values", "rewards", "terminated", "truncated", "tv", "er", "el")
    log = {k: [] for k in keys}
    for _ in range(steps):
        a, lg, v = pol.act(x, deterministic=det)
        log["obs"].append(np_(x32).copy())
        log["actions"].append(np_(a).copy())
        log["logits"].append(np_(lg).copy())
        log["values"].append(np_(v).copy())
        x, rew, te, tr = b.step(a)
        x32 = b.expand_codes(b.io)[0] if b.obs_codes else x
        log["rewards"].append(np_(rew).copy())
        log["terminated"].append(np_(te).copy())
        log["truncated"].append(np_(tr).copy())
        log["tv"].append(np_(pol.act(b.terminal_obs, deterministic=True)[2]).copy())
        log["er"].append(np_(b.episode_return).copy())
        log["el"].append(np_(b.episode_length).copy())
    out = {k: np.stack(v) for k, v in log.items()}
    out["next_values"] = np_(pol.act(x, deterministic=True)[2]).copy()
    return out


def expected(log, lo, hi, start0, last_values, gamma, lam, boot, acc):
    from plantos_amd import RolloutCollector
    sl = slice(lo, hi)
    out = RolloutCollector.host_rollout(
        log["logits"][sl], log["actions"][sl], log["rewards"][sl], log["terminated"][sl], log["truncated"][sl],
        log["values"][sl], last_values, start0, gamma, lam, terminal_values=log["tv"][sl] if boot else None,
        episode_return=log["er"][sl], episode_length=log["el"][sl], ep_count=acc[0], ep_return_sum=acc[1],
        ep_length_sum=acc[2])
    out.update(actions=log["actions"][sl], values=log["values"][sl], last_values=last_values,
               ep_count=acc[0].copy(), ep_return_sum=acc[1].copy(), ep_length_sum=acc[2].copy())
    return out


def check_rollout(ro, want, what):
    for k in FIELDS:
        g, w = np_(getattr(ro, k)), want[k]
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what}: {k} {g.dtype}{g.shape} vs {w.dtype}{w.shape}"
        assert np.ascontiguousarray(g).tobytes() == np.ascontiguousarray(w).tobytes(), f"{what}: {k} differs"


def new_acc(n):
    return np.zeros(n, np.int32), np.zeros(n, np.float64), np.zeros(n, np.int32)


@pytest.mark.parametrize("name,n", [(g, n) for g in GEO for n in (1, 65, 200)])
def test_collect_equals_manual_loop(name, n):
    from plantos_amd import Policy, RolloutCollector
    gamma, lam = 0.99, 0.95
    truncated_rows = 0
    combos = [(T, tw, det, True) for T in (1, 5, 12) for tw in TOWERS for det in (False, True)]
    combos.append((5, TOWERS[0], False, False))  # no bootstrap
    for T, towers, det, boot in combos:
        what = f"{name} n={n} T={T} {towers} det={det} bootstrap={boot}"
        tensors = make_tensors(towers, 5 * GEO[name]["cfg"][4] + 27, SEED, "var")
        b, b2 = make(name, n, seed=21), make(name, n, seed=21)
        pol, pol2 = (Policy(x, towers, "tanh", seed=99).load(tensors) for x in (b, b2))
        col = RolloutCollector(b, pol, T, gamma=gamma, gae_lambda=lam, bootstrap_timeouts=boot, deterministic=det)
        ro = col.collect()
        log = manual_loop(b2, pol2, T, det)
        want = expected(log, 0, T, np.ones(n, np.uint8), log["next_values"], gamma, lam, boot, new_acc(n))
        check_rollout(ro, want, what)
        assert pol.t == pol2.t == (0 if det else T)
        # obs: the buffer's own form, and expanded
        obs = np_(ro.obs)
        assert obs.shape == (T, n, b.obs_dim) and obs.dtype == (np.uint8 if b.obs_codes else np.float32)
        if b.obs_codes:
            assert np.array_equal(b.code_table()[obs], log["obs"]), f"{what}: obs codes"
        f32 = ro.obs_f32()
        assert f32.shape == (T * n, b.obs_dim)
        assert np_(f32).tobytes() == log["obs"].tobytes(), f"{what}: obs_f32"
        into = torch.empty((T * n, b.obs_dim), dtype=torch.float32, device=DEV)
        assert ro.obs_f32(out=into) is into and np_(into).tobytes() == log["obs"].tobytes()
        # the bootstrap changed exactly the rewards of rows cut by the time limit only
        only = (log["truncated"] != 0) & (log["terminated"] == 0)
        assert np.array_equal(np_(ro.rewards) != log["rewards"], only & boot), f"{what}: bootstrapped rows"
        truncated_rows += int(only.sum()) if boot else 0
        assert T < 3 or only.any(), f"{what}: no truncation in {T} steps of max_steps=3"
        pol.close(), pol2.close(), b.close(), b2.close()
    assert truncated_rows > 0


def test_two_collects_continue():
    """Two collect() calls of T = 5 equal one manual 10-step loop cut in two."""
    from plantos_amd import Policy, RolloutCollector
    n, T, gamma, lam = 65, 5, 0.99, 1.0
    for name in GEO:
        towers = TOWERS[1]
        tensors = make_tensors(towers, 5 * GEO[name]["cfg"][4] + 27, SEED, "var")
        b, b2 = make(name, n, seed=4), make(name, n, seed=4)
        pol, pol2 = (Policy(x, towers, "tanh", seed=5).load(tensors) for x in (b, b2))
        col = RolloutCollector(b, pol, T, gamma=gamma, gae_lambda=lam)
        log = manual_loop(b2, pol2, 2 * T, False)
        acc = new_acc(n)
        ro = col.collect()
        first = {k: np_(getattr(ro, k)).copy() for k in FIELDS}
        want = expected(log, 0, T, np.ones(n, np.uint8), log["values"][T], gamma, lam, True, acc)
        for k in FIELDS:
            assert first[k].tobytes() == np.ascontiguousarray(want[k]).tobytes(), f"{name} first collect: {k}"
        ro = col.collect()
        assert np.array_equal(np_(ro.episode_starts[0]), first["last_dones"])
        want = expected(log, T, 2 * T, first["last_dones"], log["next_values"], gamma, lam, True, acc)
        check_rollout(ro, want, f"{name} second collect")
        assert np_(ro.obs_f32()).tobytes() == log["obs"][T:].tobytes()
        assert pol.t == 2 * T
        pol.close(), pol2.close(), b.close(), b2.close()


def test_collect_in_a_graph():
    """One collect() captured on a side stream (a linear chain) and replayed twice against two
    eager collects on a twin batch (argmax actions: nothing in the graph depends on t)."""
    from plantos_amd import Policy, RolloutCollector
    towers, T = TOWERS[1], 5
    res = []
    for graphed in (True, False):
        b = make("g20", 200, seed=12, prefetch_every=0)
        pol = Policy(b, towers, "tanh").load(make_tensors(towers, b.obs_dim, SEED, "var"))
        col = RolloutCollector(b, pol, T, deterministic=True)
        col.collect()  # row 0 is primed and every kernel of the chain has run before the capture
        torch.cuda.synchronize()
        if graphed:
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                col.collect()
        log = []
        for _ in range(2):
            ro = gr.replay() if graphed else col.collect()
            torch.cuda.synchronize()
            ro = col._rollout
            log.append([np_(getattr(ro, k)).copy() for k in FIELDS] + [np_(ro.obs).copy()])
        res.append(log)
        if graphed:
            del gr
        pol.close()
        b.close()
    for it, (u, v) in enumerate(zip(*res)):
        for k, p, q in zip(FIELDS + ("obs",), u, v):
            assert p.tobytes() == q.tobytes(), f"replay {it}: {k}"
    assert res[0][0][0].tobytes() != res[0][1][0].tobytes()  # the loop moved


def test_argument_checks():
    from plantos_amd import Policy, RecurrentPolicy, RolloutCollector, _capi as C
    b = make("g21", 64, seed=1)
    pol = Policy(b, TOWERS[0], "tanh")
    one = Policy(b, [[32, 5]], "tanh")
    rec = RecurrentPolicy(b, 32, [[32, 5], [32, 1]])
    other = make("g21", 64, seed=1)
    fixed = make("g21", 64, seed=1, autoreset=False)
    pol_fixed = Policy(fixed, TOWERS[0], "tanh")
    for args in ((b, one, 5), (b, rec, 5), (b, pol, 0), (other, pol, 5), (fixed, pol_fixed, 5), (b, "policy", 5)):
        with pytest.raises(ValueError):
            RolloutCollector(*args)
    RolloutCollector(b, pol, 1)
    # the C boundary: nothing is launched for a bad argument
    L, P = C.lib(), ctypes.c_void_p
    n, A = 64, 5
    lg = torch.zeros((n, A), device=DEV)
    f = torch.full((n,), -7.0, device=DEV)
    i = torch.zeros(n, dtype=torch.int32, device=DEV)
    u = torch.zeros(n, dtype=torch.uint8, device=DEV)
    p = lambda t: P(t.data_ptr())  # noqa: E731
    ok = [n, A, p(lg), p(i), p(f), p(u), p(u), None, None, None, 0.99, p(f), p(f), p(u), None, None, None, None]
    for pos, bad in ((0, 0), (1, 1), (1, 9), (2, None), (3, None), (11, None), (13, None)):
        args = list(ok)
        args[pos] = bad
        assert L.pe_rollout_record(*args) == C.PE_ERR_ARG
    m = torch.full((3, n), -7.0, device=DEV)
    s = torch.zeros((3, n), dtype=torch.uint8, device=DEV)
    ok = [2, n, n, n, n, n, p(m), p(m), p(s), p(f), 0.99, 0.95, p(m), p(m), None]
    for pos, bad in ((0, 0), (1, 0), (2, n - 1), (5, 1), (6, None), (8, None), (9, None), (12, None)):
        args = list(ok)
        args[pos] = bad
        assert L.pe_rollout_gae(*args) == C.PE_ERR_ARG
    torch.cuda.synchronize()
    assert bool((f == -7.0).all()) and bool((m == -7.0).all())
    for x in (pol, one, rec, pol_fixed):
        x.close()
    b.close()
    with pytest.raises(ValueError):
        RolloutCollector(b, pol, 5)  # a closed batch
    other.close(), fixed.close()
