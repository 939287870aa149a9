"""GPU checks of recurrent rollout collection (plantos_amd.RecurrentRolloutCollector): collect()
equals a manual act / step loop on a twin batch whose recorded steps go through the host twin
(RecurrentRolloutCollector.host_rollout) -- every Rollout field, the state snapshots of both
modes and the policy's final state, over three consecutive collects; byte codes and f32 obs,
truncations every third step with the bootstrap from the value-only forward, sampling and
argmax; desynchronized episodes, where the bootstrap skips tiles; graph capture; argument checks.
"""
import numpy as np
import pytest
import torch

from lstm_util import make_lstm_tensors
from policy_util import make_tensors
from test_gpu_rollout import FIELDS

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GEO = {"g20": dict(cfg=(20, 10, 12, 6, 16), codes=True), "g21": dict(cfg=(21, 8, 50, 2, 10), codes=False)}
H, TOWERS = 32, [[32, 5], [32, 1]]
SEED = 80
GAMMA, LAM = 0.99, 0.95


def np_(t):
    return t.detach().cpu().numpy()


def make(name, n, **kw):
    from plantos_amd import PlantOSBatch
    G, P, Ob, R, C = GEO[name]["cfg"]
    return PlantOSBatch(n, grid_size=G, num_plants=P, num_obstacles=Ob, lidar_range=R, lidar_channels=C,
                        device=DEV, obs_codes=GEO[name]["codes"], max_steps=3, **kw)


def states_np(pol):
    return [(np_(h).copy(), np_(c).copy()) for h, c in pol.get_states()]


def manual_loop(b, pol, steps, det):
    """`steps` steps of act / step on batch b with the step's own flags as episode starts (all
    set at the first step): what a rollout needs, as numpy [steps, ..]; obs f32 has steps + 1
    rows (the last: the obs after the last step)."""
    n, D = b.num_envs, b.obs_dim
    x = b.reset(mask=torch.zeros(n, dtype=torch.uint8, device=DEV),
                obs=torch.empty((n, D), dtype=torch.float32, device=DEV))
    x32 = x
    start = torch.ones(n, dtype=torch.uint8, device=DEV)
    log = {k: [] for k in ("obs", "actions", "rewards", "terminated", "truncated", "tobs", "er", "el")}
    for _ in range(steps):
        a, _, _ = pol.act(x, episode_start=start, deterministic=det)
        log["obs"].append(np_(x32).copy())
        log["actions"].append(np_(a).copy())
        x, rew, te, tr = b.step(a)
        start = (te, tr)
        x32 = b.expand_codes(b.io)[0] if b.obs_codes else x
        for k, v in (("rewards", rew), ("terminated", te), ("truncated", tr), ("tobs", b.terminal_obs),
                     ("er", b.episode_return), ("el", b.episode_length)):
            log[k].append(np_(v).copy())
    log["obs"].append(np_(x32).copy())
    return {k: np.stack(v) for k, v in log.items()}


def expected(tensors, log, lo, hi, start0, states0, boot, mode, acc):
    from plantos_amd import RecurrentRolloutCollector
    sl = slice(lo, hi)
    out = RecurrentRolloutCollector.host_rollout(
        H, TOWERS, tensors[0], tensors[1], "tanh", log["obs"][sl], log["obs"][hi], log["tobs"][sl], log["actions"][sl],
        log["rewards"][sl], log["terminated"][sl], log["truncated"][sl], start0, states0, GAMMA, LAM,
        bootstrap_timeouts=boot, state_snapshots=mode, episode_return=log["er"][sl], episode_length=log["el"][sl],
        ep_count=acc[0], ep_return_sum=acc[1], ep_length_sum=acc[2])
    out.update(actions=log["actions"][sl], ep_count=acc[0].copy(), ep_return_sum=acc[1].copy(),
               ep_length_sum=acc[2].copy())
    return out


def check_rollout(ro, pol, want, what):
    for k in FIELDS:
        g, w = np_(getattr(ro, k)), want[k]
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what}: {k} {g.dtype}{g.shape} vs {w.dtype}{w.shape}"
        assert np.ascontiguousarray(g).tobytes() == np.ascontiguousarray(w).tobytes(), f"{what}: {k} differs"
    assert len(ro.lstm_states) == len(want["lstm_states"]) == 2
    for ti, (got, exp) in enumerate(zip(ro.lstm_states, want["lstm_states"])):
        for q, g, w in zip("hc", got, exp):
            assert tuple(g.shape) == w.shape, f"{what}: snapshot shape {tuple(g.shape)} vs {w.shape}"
            assert np_(g).tobytes() == w.tobytes(), f"{what}: snapshot of tower {ti} {q} differs"
    for ti, (got, exp) in enumerate(zip(states_np(pol), want["final_states"])):
        for q, g, w in zip("hc", got, exp):
            assert g.tobytes() == w.tobytes(), f"{what}: the policy's final state, tower {ti} {q}"


def new_acc(n):
    return np.zeros(n, np.int32), np.zeros(n, np.float64), np.zeros(n, np.int32)


def run_collects(name, n, T, det, boot, mode, collects=3, desync=False):
    """`collects` consecutive collect() calls against one manual loop cut into pieces; returns the
    manual loop's log"""
    from plantos_amd import RecurrentPolicy, RecurrentRolloutCollector
    what = f"{name} n={n} T={T} det={det} bootstrap={boot} snapshots={mode}"
    tensors = make_lstm_tensors(5 * GEO[name]["cfg"][4] + 27, H, TOWERS, SEED)
    b, b2 = make(name, n, seed=21), make(name, n, seed=21)
    pol, pol2 = (RecurrentPolicy(x, H, TOWERS, "tanh", seed=99).load(tensors) for x in (b, b2))
    rng = np.random.default_rng(n + T)
    held = [(rng.uniform(-1, 1, (n, H)).astype(np.float32), rng.uniform(-2, 2, (n, H)).astype(np.float32)) for _ in TOWERS]
    for x, p in ((b, pol), (b2, pol2)):
        p.set_states(held)   # row 0 flags every env: the first forward reads zeros whatever the policy held
        if desync:   # envs 64.. one step behind, env 5 two: their time limits fall on different steps
            for lo, hi in ((64, n), (5, 6)):
                x.step(x.synth_actions(3, lo))
                mask = torch.zeros(n, dtype=torch.uint8, device=DEV)
                mask[lo:hi] = 1
                x.reset(mask=mask)
    col = RecurrentRolloutCollector(b, pol, T, gamma=GAMMA, gae_lambda=LAM, bootstrap_timeouts=boot,
                                    deterministic=det, state_snapshots=mode)
    log = manual_loop(b2, pol2, collects * T, det)
    acc, start0, states0 = new_acc(n), np.ones(n, np.uint8), held
    for k in range(collects):
        ro = col.collect()
        want = expected(tensors, log, k * T, (k + 1) * T, start0, states0, boot, mode, acc)
        check_rollout(ro, pol, want, f"{what} collect {k}")
        assert tuple(ro.lstm_states[0][0].shape) == (T if mode == "all" else 1, n, H)
        f32 = ro.obs_f32()
        assert np_(f32).tobytes() == log["obs"][k * T:(k + 1) * T].tobytes(), f"{what} collect {k}: obs_f32"
        only = (log["truncated"][k * T:(k + 1) * T] != 0) & (log["terminated"][k * T:(k + 1) * T] == 0)
        assert np.array_equal(np_(ro.rewards) != log["rewards"][k * T:(k + 1) * T], only & boot), f"{what}: bootstrapped rows"
        start0, states0 = want["last_dones"], want["final_states"]
    assert pol.t == pol2.t == (0 if det else collects * T)
    for (h, c), (h2, c2) in zip(states_np(pol), states_np(pol2)):
        assert h.tobytes() == h2.tobytes() and c.tobytes() == c2.tobytes(), f"{what}: the twin policy's state"
    pol.close(), pol2.close(), b.close(), b2.close()
    return log


@pytest.mark.parametrize("name,n", [(g, n) for g in GEO for n in (63, 130)])
def test_collect_equals_manual_loop(name, n):
    truncated = 0
    for i, (T, det, boot) in enumerate((T, det, boot) for T in (1, 4) for det in (False, True) for boot in (True, False)):
        for mode in (("first", "all") if (T == 4 and boot and not det) else (("all", "first")[i % 2],)):
            log = run_collects(name, n, T, det, boot, mode)
            truncated += int(((log["truncated"] != 0) & (log["terminated"] == 0)).sum()) if boot else 0
    assert truncated > 0


def test_desynchronized_time_limits():
    """Time limits that fall on different steps in different tiles: at every step the bootstrap
    evaluates some tiles and skips others, and at one step a single env of the whole batch."""
    for name in GEO:
        log = run_collects(name, 130, 4, False, True, "all", collects=2, desync=True)
        tr = log["truncated"][:3] != 0
        assert all(m.any() and not m.all() for m in tr), "the truncation masks must be neither empty nor full"
        assert [int(m.sum()) for m in tr][2] == 1 and tr[2][5]
        assert tr[0][:64].sum() == 63 and not tr[0][64:].any() and tr[1][64:].all() and not tr[1][:64].any()


def test_collect_in_a_graph():
    """One collect() captured and replayed twice against two eager collects on a twin batch
    (argmax actions: nothing in the graph depends on t)."""
    from plantos_amd import RecurrentPolicy, RecurrentRolloutCollector
    T, n = 4, 130
    res = []
    for graphed in (True, False):
        b = make("g20", n, seed=12, prefetch_every=0)
        pol = RecurrentPolicy(b, H, TOWERS).load(make_lstm_tensors(b.obs_dim, H, TOWERS, SEED))
        col = RecurrentRolloutCollector(b, pol, T, deterministic=True, state_snapshots="all")
        col.collect()   # row 0 is primed and every kernel of the chain has run before the capture
        torch.cuda.synchronize()
        if graphed:
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                col.collect()
        log = []
        for _ in range(2):
            gr.replay() if graphed else col.collect()
            torch.cuda.synchronize()
            ro = col._rollout
            log.append([np_(getattr(ro, k)).copy() for k in FIELDS] + [np_(ro.obs).copy()]
                       + [np_(x).copy() for hc in ro.lstm_states for x in hc] + [x for hc in states_np(pol) for x in hc])
        res.append(log)
        if graphed:
            del gr
        pol.close()
        b.close()
    for it, (u, v) in enumerate(zip(*res)):
        for i, (p, q) in enumerate(zip(u, v)):
            assert p.tobytes() == q.tobytes(), f"replay {it}: item {i}"
    assert res[0][0][0].tobytes() != res[0][1][0].tobytes()   # the loop moved
    assert np.any(res[0][0][FIELDS.index("rewards")] != 0)


def test_argument_checks():
    from plantos_amd import Policy, RecurrentPolicy, RecurrentRolloutCollector, RolloutCollector
    b = make("g21", 64, seed=1)
    rec = RecurrentPolicy(b, H, TOWERS)
    actor = RecurrentPolicy(b, H, TOWERS[:1])
    ff = Policy(b, TOWERS, "tanh").load(make_tensors(TOWERS, b.obs_dim, SEED, "var"))
    other = make("g21", 64, seed=1)
    fixed = make("g21", 64, seed=1, autoreset=False)
    rec_fixed = RecurrentPolicy(fixed, H, TOWERS)
    for args, kw in (((b, ff, 4), {}), ((b, actor, 4), {}), ((b, rec, 4), dict(state_snapshots="last")),
                     ((b, rec, 4), dict(state_snapshots=None)), ((b, rec, 0), {}), ((other, rec, 4), {}),
                     ((fixed, rec_fixed, 4), {}), ((b, "policy", 4), {})):
        with pytest.raises(ValueError):
            RecurrentRolloutCollector(*args, **kw)
    with pytest.raises(ValueError, match="RecurrentRolloutCollector"):
        RolloutCollector(b, rec, 4)
    col = RecurrentRolloutCollector(b, rec, 1)
    assert col.state_snapshots == "first"
    for x in (rec, actor, ff, rec_fixed):
        x.close()
    b.close(), other.close(), fixed.close()
