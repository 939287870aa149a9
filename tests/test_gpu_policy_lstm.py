"""GPU checks of the recurrent policy kernel (pe_policy_*_lstm; plantos_amd.RecurrentPolicy):
actions, logits, values and every tower's (h, c) equal the host twin's bit for bit after every
step of a sequence with episode starts, at sizes around the env tiles and with every legal
tile; state set / get / reset; padding; graph capture of act -> step with the step's own flags;
a policy-driven loop against the oracle across auto-resets; argument checks.
"""
import ctypes

import numpy as np
import pytest
import torch

from lstm_util import lstm_state_dict, make_lstm_tensors
from oracle_rollout import OracleVec

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GEO = {"g20": dict(cfg=(20, 10, 12, 6, 16), codes=True), "g21": dict(cfg=(21, 8, 50, 2, 10), codes=False)}
SHAPES = [
    (32, [[32, 5]]),                           # one unit tile for 8 waves
    (96, [[64, 64, 5], [64, 64, 1]]),          # 3 unit tiles: no divisor of 8
    (256, [[128, 128, 5], [128, 128, 1]]),     # the reference's family
    (512, [[256, 5]]),                         # fits 32 envs per workgroup only
]
SEED = 78


def np_(t):
    return None if t is None else t.detach().cpu().numpy()


def make(name, n, **kw):
    from plantos_amd import PlantOSBatch
    G, P, Ob, R, C = GEO[name]["cfg"]
    return PlantOSBatch(n, grid_size=G, num_plants=P, num_obstacles=Ob, lidar_range=R, lidar_channels=C,
                        device=DEV, obs_codes=GEO[name]["codes"], **kw)


def tiles(H):
    return (32,) if H > 256 else (32, 64)


def u8(x):
    return torch.as_tensor(np.asarray(x, np.uint8), device=DEV)


def states_np(pol):
    return [(np_(h), np_(c)) for h, c in pol.get_states()]


def check_equal(got, want, what):
    a, lg, v = (np_(x) for x in got)
    wa, wl, wv = want
    assert np.array_equal(lg, wl), f"{what}: logits differ ({(lg != wl).sum()} of {lg.size})"
    if wv is None:
        assert v is None
    else:
        assert np.array_equal(v, wv), f"{what}: values differ"
    assert np.array_equal(a, wa), f"{what}: actions differ"


def check_states(pol, want, what):
    for ti, ((h, c), (wh, wc)) in enumerate(zip(states_np(pol), want)):
        assert np.array_equal(h, wh), f"{what}: tower {ti} h differs ({(h != wh).sum()} of {h.size})"
        assert np.array_equal(c, wc), f"{what}: tower {ti} c differs ({(c != wc).sum()} of {c.size})"


def record(b, steps=6):
    """[(obs as the batch holds it, obs f32)] of `steps` steps: the reset, then synthetic steps."""
    n = b.num_envs
    first = b.reset(mask=torch.zeros(n, dtype=torch.uint8, device=DEV),
                    obs=torch.empty((n, b.obs_dim), dtype=torch.float32, device=DEV)).clone()
    seq = [(first, np_(first))]
    act = torch.empty(n, dtype=torch.int32, device=DEV)
    for t in range(steps - 1):
        b.synth_actions(5, t, out=act)
        b.step(act)
        x = b.obs.clone()
        f32 = b.expand_codes(b.io)[0] if b.obs_codes else x
        seq.append((x, np_(f32).copy()))
    return seq


def start_plan(n, rng):
    """per step (start_a, start_b) as numpy u8 or None: none, none, a third as a, a disjoint few
    as b, both, two all-zero flags"""
    a = (rng.random(n) < 1 / 3).astype(np.uint8) * 3   # any non-zero value counts
    rest = np.nonzero(a == 0)[0]
    b = np.zeros(n, np.uint8)
    b[rest[::4]] = 1
    if n == 1:
        a[:] = 1
    z = np.zeros(n, np.uint8)
    return [(None, None), (None, None), (a, None), (None, b), (a, b), (z, z)]


@pytest.mark.parametrize("name,n", [(g, n) for g in GEO for n in (1, 31, 33, 64, 65, 200)])
def test_kernel_equals_twin_over_a_sequence(name, n):
    from plantos_amd import RecurrentPolicy
    b = make(name, n, seed=3, env_id_offset=1000)
    D = b.obs_dim
    seq = record(b)
    plan = start_plan(n, np.random.default_rng(n))
    for H, towers in SHAPES:
        tensors = make_lstm_tensors(D, H, towers, SEED)
        want = None
        for et in tiles(H):
            pols = {det: RecurrentPolicy(b, H, towers, "tanh", seed=99, env_tile=et).load(tensors) for det in (True, False)}
            assert pols[True].env_tile == et
            if want is None:   # the twin's sequence, once per shape
                want, st = [], None
                for t, ((_, x32), (sa, sb)) in enumerate(zip(seq, plan)):
                    start = None if sa is None and sb is None else ((sa if sa is not None else 0) | (sb if sb is not None else 0))
                    outs = {}
                    for det in (True, False):
                        outs[det], new = pols[det].host_forward(x32, st, start, tensors, deterministic=det, t=7 + t)
                    st = new
                    want.append((outs, st))
            for t, ((x, _), (sa, sb)) in enumerate(zip(seq, plan)):
                flags = (None if sa is None else u8(sa), None if sb is None else u8(sb))
                for det in (True, False):
                    what = f"{name} n={n} H={H} {towers} tile {et} step {t + 1} det={det}"
                    got = pols[det].act(x, episode_start=flags, deterministic=det, t=7 + t)
                    check_equal(got, want[t][0][det], what)
                    check_states(pols[det], want[t][1], what)
            for p in pols.values():
                p.close()
    b.close()


def test_state_set_get_reset_roundtrip():
    from plantos_amd import RecurrentPolicy
    n = 65
    b = make("g21", n, seed=5)
    x = b.reset()
    H, towers = SHAPES[1]
    tensors = make_lstm_tensors(b.obs_dim, H, towers, SEED)
    rng = np.random.default_rng(4)
    for et in (32, 64):
        pol = RecurrentPolicy(b, H, towers, env_tile=et).load(tensors)
        fresh, fresh_st = pol.host_forward(np_(x))
        check_states(pol, [(np.zeros((n, H), np.float32),) * 2] * 2, "fresh")
        st = [(rng.uniform(-1, 1, (n, H)).astype(np.float32), rng.uniform(-3, 3, (n, H)).astype(np.float32)) for _ in towers]
        pol.set_states(st)
        check_states(pol, st, "set -> get")
        want, want_st = pol.host_forward(np_(x), st)
        check_equal(pol.act(x), want, f"tile {et} from a set state")
        check_states(pol, want_st, f"tile {et} from a set state")
        assert not np.array_equal(want[1], fresh[1])
        pol.set_states([(torch.as_tensor(h, device=DEV), torch.as_tensor(c, device=DEV)) for h, c in st])   # device tensors
        check_states(pol, st, "set (device) -> get")
        pol.reset_states()
        check_states(pol, [(np.zeros((n, H), np.float32),) * 2] * 2, "reset")
        check_equal(pol.act(x), fresh, f"tile {et} after reset_states")
        check_states(pol, fresh_st, f"tile {et} after reset_states")
        with pytest.raises(ValueError):
            pol.set_states(st[:1])
        with pytest.raises(ValueError):
            pol.set_states([(h[:-1], c[:-1]) for h, c in st])
        pol.close()
    b.close()


def guarded(shape, dtype, fill, pad):
    """a contiguous tensor of `shape` inside a larger one filled with `fill`: (view, whole)"""
    size = int(np.prod(shape))
    whole = torch.full((pad + size + pad,), fill, dtype=dtype, device=DEV)
    return whole[pad:pad + size].view(shape), whole


def test_padding_reads_and_writes_nothing_outside():
    from plantos_amd import RecurrentPolicy
    n = 65
    b = make("g20", n, seed=9)
    D = b.obs_dim
    seq = record(b, steps=4)
    codes, f32 = seq[-1]
    nan = float("nan")
    H, towers = SHAPES[1]
    lstm, mlp = make_lstm_tensors(D, H, towers, SEED)
    wholes = []

    def guard(arr, pad):
        view, whole = guarded(arr.shape, torch.float32, nan, pad)
        view.copy_(torch.as_tensor(arr))
        wholes.append((whole, whole.clone()))
        return view

    dl = [tuple(guard(x, 3 if x.ndim == 2 else 1) for x in tw) for tw in lstm]
    dm = [[(guard(w, 3), guard(bias, 1)) for w, bias in tw] for tw in mlp]
    x32, x32_whole = guarded((n, D), torch.float32, nan, 3)
    x32.copy_(torch.as_tensor(f32))
    x8, x8_whole = guarded((n, D), torch.uint8, 255, 5)
    x8.copy_(codes)
    start = (np.arange(n) % 3 == 0).astype(np.uint8)
    fa, fa_whole = guarded((n,), torch.uint8, 255, 5)
    fa.copy_(u8(start))
    fb, fb_whole = guarded((n,), torch.uint8, 255, 5)
    fb.zero_()
    wholes += [(w, w.clone()) for w in (x32_whole, x8_whole, fa_whole, fb_whole)]
    rng = np.random.default_rng(6)
    st = [(rng.uniform(-1, 1, (n, H)).astype(np.float32), rng.uniform(-2, 2, (n, H)).astype(np.float32)) for _ in towers]
    for et in (32, 64):
        pol = RecurrentPolicy(b, H, towers, seed=2, env_tile=et).load((dl, dm))
        other = RecurrentPolicy(b, H, towers, seed=2, env_tile=et).load((dl, dm))   # its own state
        other_st = [(h[::-1].copy(), c[::-1].copy()) for h, c in st]
        other.set_states(other_st)
        for x in (x32, x8):
            pol.set_states(st)
            a, a_whole = guarded((n,), torch.int32, -7, 5)
            lg, lg_whole = guarded((n, 5), torch.float32, nan, 3)
            v, v_whole = guarded((n,), torch.float32, nan, 3)
            got = pol.act(x, episode_start=(fa, fb), deterministic=False, t=1, out=(a, lg, v))
            want, want_st = pol.host_forward(f32, st, start, (lstm, mlp), deterministic=False, t=1)
            check_equal(got, want, f"tile {et}")
            check_states(pol, want_st, f"tile {et}")
            assert (np_(a_whole)[:5] == -7).all() and (np_(a_whole)[-5:] == -7).all()
            for whole in (lg_whole, v_whole):
                assert np.isnan(np_(whole)[:3]).all() and np.isnan(np_(whole)[-3:]).all()
        check_states(other, other_st, "the second policy's state")
        pol.close()
        other.close()
    for whole, before in wholes:  # inputs untouched, surroundings included
        assert np_(whole).tobytes() == np_(before).tobytes()
    b.close()


def test_recurrent_act_and_step_in_a_graph():
    """act(episode_start=(terminated, truncated)) then step captured as one chain; ten replays
    against ten eager iterations on a twin batch.  max_steps=6: every window crosses auto-resets."""
    from plantos_amd import RecurrentPolicy
    H, towers = SHAPES[1]
    res, flagged = [], 0
    for graphed in (True, False):
        b = make("g20", 200, seed=12, prefetch_every=0, max_steps=6)
        pol = RecurrentPolicy(b, H, towers).load(make_lstm_tensors(b.obs_dim, H, towers, SEED))
        b.step(b.synth_actions(1, 0))  # the io buffer now holds codes
        pol.act(episode_start=(b.terminated, b.truncated))   # (every kernel of the chain has run once before the capture)
        torch.cuda.synchronize()
        log = []

        def one():
            a, _, _ = pol.act(episode_start=(b.terminated, b.truncated))
            b.step(a)

        if graphed:
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                one()
        for _ in range(10):
            gr.replay() if graphed else one()
            torch.cuda.synchronize()
            flagged += int((np_(b.terminated) | np_(b.truncated)).any())
            log.append([np_(pol.actions).copy(), np_(pol.logits).copy(), np_(b.io).copy()]
                       + [x for hc in states_np(pol) for x in hc])
        res.append(log)
        if graphed:
            del gr
        pol.close()
        b.close()
    for it, (u, v) in enumerate(zip(*res)):
        for p, q in zip(u, v):
            assert p.tobytes() == q.tobytes(), f"iteration {it}"
    assert flagged >= 2  # the flags were set (in both runs)
    assert len({l[0].tobytes() for l in res[0]}) > 1  # the loop moved


def test_recurrent_loop_equals_oracle():
    """64 envs, max_steps=40, 100 steps: the GPU loop act -> step against the oracle driven by the
    twin's actions from the oracle's obs and the oracle's own done flags."""
    from plantos_amd import PlantOSBatch, RecurrentPolicy
    cfg, n, seed = (20, 10, 12, 6, 16), 64, 2025
    b = PlantOSBatch(n, grid_size=20, num_plants=10, num_obstacles=12, lidar_range=6, lidar_channels=16,
                     seed=seed, device=DEV, max_steps=40)
    H, towers = 64, [[64, 5], [64, 1]]
    tensors = make_lstm_tensors(b.obs_dim, H, towers, SEED)
    pol = RecurrentPolicy(b, H, towers).load(tensors)
    ov = OracleVec(cfg, np.arange(n), seed, max_steps=40)
    obs = b.reset(mask=torch.zeros(n, dtype=torch.uint8, device=DEV))
    o_obs = ov.obs()
    assert np.array_equal(np_(obs), o_obs)
    moved, dones = set(), 0
    flags, o_start, o_st = None, None, None
    for t in range(100):
        a, _, _ = pol.act(episode_start=flags)
        a_np = np_(a).copy()
        check = states_np(pol)
        obs, rew, te, tr = b.step(a)
        flags = (te, tr)
        (o_a, _, _), o_st = pol.host_forward(o_obs, o_st, o_start, tensors)
        o_obs, o_rew, o_te, o_tr, *_ = ov.step(o_a)
        o_start = o_te | o_tr
        dones += int(o_start.sum())
        assert np.array_equal(a_np, o_a), f"step {t}: actions"
        for (h, c), (wh, wc) in zip(check, o_st):
            assert np.array_equal(h, wh) and np.array_equal(c, wc), f"step {t}: states"
        if not (np.array_equal(np_(obs), o_obs) and np.array_equal(np_(rew), o_rew.astype(np.float32))
                and np.array_equal(np_(te).astype(bool), o_te) and np.array_equal(np_(tr).astype(bool), o_tr)):
            raise AssertionError(f"GPU step {t} differs from the oracle")
        moved.update(o_a.tolist())
    assert len(moved) > 1 and dones >= n
    pol.close()
    b.close()


def test_argument_checks_launch_nothing():
    from plantos_amd import Policy, RecurrentPolicy, _capi as C
    from plantos_amd.policy import _lstm_structs, _tower_structs
    from policy_util import make_tensors
    L = C.lib()
    b = make("g21", 64, seed=1)  # no obs_codes
    for H in (48, 544, 2562):
        with pytest.raises(ValueError):
            RecurrentPolicy(b, H, [[32, 5]])
        p = ctypes.c_void_p()
        assert L.pe_policy_create_lstm(b.handle, 1, _lstm_structs(H, 1), _tower_structs([[32, 5]]), C.PE_ACT_TANH, 0,
                                       ctypes.byref(p)) == C.PE_ERR_ARG
        assert not p.value
    assert b"K-streamed" in L.pe_last_error()
    with pytest.raises(ValueError):
        RecurrentPolicy(b, 32, [[32, 5]] * 3)
    p = ctypes.c_void_p()
    assert L.pe_policy_create_lstm(b.handle, 3, _lstm_structs(32, 3), _tower_structs([[32, 5]] * 3), C.PE_ACT_TANH, 0,
                                   ctypes.byref(p)) == C.PE_ERR_ARG
    with pytest.raises(ValueError):
        RecurrentPolicy(b, 512, [[32, 5]], env_tile=64)   # H = 512 does not fit 64 envs per workgroup
    assert b"LDS" in L.pe_last_error()
    assert L.pe_policy_create_lstm(b.handle, 1, _lstm_structs(32, 1), _tower_structs([[32, 5]]), C.PE_ACT_TANH, 48,
                                   ctypes.byref(p)) == C.PE_ERR_ARG
    assert not p.value

    H, towers = 32, [[32, 5]]
    tensors = make_lstm_tensors(b.obs_dim, H, towers, SEED)
    pol = RecurrentPolicy(b, H, towers).load(tensors)
    ff = Policy(b, towers, "tanh").load(make_tensors(towers, b.obs_dim, SEED, "var"))
    n = b.num_envs
    x = b.reset()
    rng = np.random.default_rng(8)
    st = [(rng.uniform(-1, 1, (n, H)).astype(np.float32), rng.uniform(-1, 1, (n, H)).astype(np.float32))]
    pol.set_states(st)
    a = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    lg = torch.full((n, 5), -7.0, dtype=torch.float32, device=DEV)
    v = torch.full((n,), -7.0, dtype=torch.float32, device=DEV)
    flag = torch.zeros(n, dtype=torch.uint8, device=DEV)
    s = b._stream()
    P = ctypes.c_void_p
    X, A_, LG, F = P(x.data_ptr()), P(a.data_ptr()), P(lg.data_ptr()), P(flag.data_ptr())
    calls = [
        (ff._p, X, 0, F, None, 0, 0, 0, A_, LG, None, s),               # a feed-forward policy
        (pol._p, None, 0, F, None, 0, 0, 0, A_, LG, None, s),           # null obs
        (pol._p, X, 0, F, None, 0, 0, 0, None, LG, None, s),            # null actions
        (pol._p, X, 1, F, None, 0, 0, 0, A_, LG, None, s),              # codes, no obs_codes
        (pol._p, X, 0, F, None, 5, 0, 0, A_, LG, None, s),              # bad mode
        (pol._p, X, 0, F, None, 0, 0, 0, A_, LG, P(v.data_ptr()), s),   # no value tower
        (None, X, 0, F, None, 0, 0, 0, A_, LG, None, s),                # null policy
    ]
    for args in calls:
        assert L.pe_policy_forward_lstm(*args) == C.PE_ERR_ARG
    assert L.pe_policy_forward(pol._p, X, 0, 0, 0, 0, A_, LG, None, s) == C.PE_ERR_ARG   # the feed-forward forward
    assert L.pe_policy_load(pol._p, _tower_structs(towers), s) == C.PE_ERR_ARG
    assert L.pe_policy_lstm_reset_state(ff._p, s) == C.PE_ERR_ARG
    assert L.pe_policy_lstm_get_state(ff._p, 0, LG, None, s) == C.PE_ERR_ARG
    assert L.pe_policy_lstm_get_state(pol._p, 1, LG, None, s) == C.PE_ERR_ARG            # no such tower
    assert L.pe_policy_lstm_set_state(pol._p, -1, LG, None, s) == C.PE_ERR_ARG
    with pytest.raises(ValueError):
        pol.act(x[:-1])
    bad_flags = [flag.to(torch.int32), flag.to(torch.float32), flag[:-1], torch.zeros((n, 1), dtype=torch.uint8, device=DEV),
                 flag.cpu(), np.zeros(n, np.uint8), (flag, flag, flag), (flag, flag.to(torch.int64))]
    for f in bad_flags:
        with pytest.raises(ValueError):
            pol.act(x, episode_start=f, out=(a, lg, None))
    with pytest.raises(ValueError):
        pol.act(torch.zeros((n, b.obs_dim), dtype=torch.uint8, device=DEV), out=(a, lg, None))
    with pytest.raises(ValueError):
        pol.act(x, out=(a, lg, v))
    with pytest.raises(ValueError):
        pol.load(make_lstm_tensors(b.obs_dim, 64, towers, SEED))
    torch.cuda.synchronize()
    assert (np_(a) == -7).all() and (np_(lg) == -7.0).all() and (np_(v) == -7.0).all()
    check_states(pol, st, "the state after the refusals")
    pol.act(x, episode_start=flag.bool(), out=(a, lg, None))
    want, want_st = pol.host_forward(np_(x), st, None)
    check_equal((a, lg, None), want, "after the refusals")
    check_states(pol, want_st, "after the refusals")
    ff.close()
    pol.close()
    b.close()


def test_from_state_dict_on_device():
    from plantos_amd import RecurrentPolicy
    b = make("g21", 63, seed=4)
    x = b.reset()
    for critic in (True, False):
        pol = RecurrentPolicy.from_state_dict(b, lstm_state_dict(b.obs_dim, 64, critic=critic))
        assert pol.hidden == 64 and len(pol.towers) == 1 + critic
        want, st = pol.host_forward(np_(x))
        check_equal(pol.act(x), want, f"critic={critic}")
        want, st = pol.host_forward(np_(x), st)
        check_equal(pol.act(x), want, f"critic={critic} step 2")
        check_states(pol, st, f"critic={critic}")
        pol.close()
    b.close()
