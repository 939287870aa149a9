"""GPU checks of the policy kernel (pe_policy_*; plantos_amd.Policy): logits, values and
actions equal the host twin's bit for bit on obs of real batches (byte codes and f32), at
sizes around the env tiles and with both tiles; padding, stream order of load, graph
capture, a 1010-step policy-driven loop against the oracle, argument checks.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle_rollout import OracleVec
from policy_util import a2c_state_dict, dqn_state_dict, make_tensors, obs_rows

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GEO = {"g20": dict(cfg=(20, 10, 12, 6, 16), codes=True), "g21": dict(cfg=(21, 8, 50, 2, 10), codes=False)}
A2C = ([[256, 256, 5], [256, 256, 1]], "tanh")
SHAPES = [
    ([[32, 5]], "tanh"),
    ([[64, 64, 5], [64, 64, 1]], "tanh"),
    A2C,
    ([[512, 512, 256, 5]], "relu"),
    ([[32, 96, 5], [32, 96, 1]], "tanh"),
]
SEED = 77


def np_(t):
    return None if t is None else t.detach().cpu().numpy()


def make(name, n, **kw):
    from plantos_amd import PlantOSBatch
    G, P, Ob, R, C = GEO[name]["cfg"]
    return PlantOSBatch(n, grid_size=G, num_plants=P, num_obstacles=Ob, lidar_range=R, lidar_channels=C,
                        device=DEV, obs_codes=GEO[name]["codes"], **kw)


def tiles(towers):
    """env tiles to run: 512-wide layers only fit 32 envs per workgroup"""
    return (32,) if max(max(t[:-1]) for t in towers) > 256 else (32, 64)


def dev_tensors(tensors):
    return [[(torch.as_tensor(w, device=DEV), torch.as_tensor(b, device=DEV)) for w, b in tw] for tw in tensors]


def check_equal(got, want, what):
    a, lg, v = (np_(x) for x in got)
    wa, wl, wv = want
    assert np.array_equal(lg, wl), f"{what}: logits differ ({(lg != wl).sum()} of {lg.size})"
    if wv is None:
        assert v is None
    else:
        assert np.array_equal(v, wv), f"{what}: values differ"
    assert np.array_equal(a, wa), f"{what}: actions differ"


def rollout_obs(b, steps=30):
    """f32 obs after reset, and after `steps` synthetic steps: (reset_f32, stepped, stepped_f32);
    `stepped` is the batch's own io view (codes on an obs_codes batch)."""
    n = b.num_envs
    first = b.reset(mask=torch.zeros(n, dtype=torch.uint8, device=DEV),
                    obs=torch.empty((n, b.obs_dim), dtype=torch.float32, device=DEV)).clone()
    act = torch.empty(n, dtype=torch.int32, device=DEV)
    for t in range(steps):
        b.synth_actions(5, t, out=act)
        b.step(act)
    stepped = b.obs
    f32 = b.expand_codes(b.io)[0] if b.obs_codes else stepped
    return first, stepped, f32


@pytest.mark.parametrize("name,n", [(g, n) for g in GEO for n in (1, 63, 64, 65, 200)] + [("g20", 4096)])
def test_kernel_equals_twin(name, n):
    from plantos_amd import Policy
    b = make(name, n, seed=3, env_id_offset=1000)
    D = b.obs_dim
    first, stepped, stepped_f32 = rollout_obs(b)
    uni = torch.as_tensor(obs_rows(D, n=max(n, 3), seed=n)[-n:], device=DEV).contiguous()  # (uniform rows last)
    if n == 4096:
        shapes, inputs = [A2C], [("stepped", stepped, stepped_f32)]
    else:
        shapes = SHAPES
        inputs = [("reset", first, first), ("stepped", stepped, stepped_f32), ("uniform", uni, uni)]
        if b.obs_codes:
            inputs.append(("stepped f32", stepped_f32, stepped_f32))
    for towers, act in shapes:
        tensors = make_tensors(towers, D, SEED, "var")
        want = {}
        for et in tiles(towers):
            pol = Policy(b, towers, act, seed=99, env_tile=et).load(tensors)
            assert pol.env_tile == et
            for what, x, x32 in inputs:
                for det in (True, False):
                    key = (what, det)
                    if key not in want:
                        want[key] = pol.host_forward(np_(x32), tensors, deterministic=det, t=7)
                    got = pol.act(x, deterministic=det, t=7)
                    check_equal(got, want[key], f"{name} n={n} {towers} tile {et} {what} det={det}")
            pol.close()
    b.close()


def test_library_tile_choice_and_counter():
    """env_tile=None picks a tile itself; sampling without t walks the policy's counter."""
    from plantos_amd import Policy
    b = make("g21", 65, seed=3)
    towers, act = SHAPES[1]
    tensors = make_tensors(towers, b.obs_dim, SEED, "var")
    pol = Policy(b, towers, act, seed=5).load(tensors)
    assert pol.env_tile in (32, 64)
    x = b.reset()
    for t in range(3):
        got = pol.act(x, deterministic=False)
        check_equal(got, pol.host_forward(np_(x), deterministic=False, t=t), f"t={t}")
    assert pol.t == 3
    pol.close()
    b.close()


def test_from_state_dict_on_device():
    from plantos_amd import Policy
    b = make("g21", 63, seed=4)
    x = b.reset()
    for sd, act in ((a2c_state_dict(b.obs_dim), "tanh"), (dqn_state_dict(b.obs_dim), "relu")):
        pol = Policy.from_state_dict(b, sd)
        assert pol.activation == act
        check_equal(pol.act(x), pol.host_forward(np_(x)), act)
        pol.close()
    b.close()


def test_codes_path_equals_f32_path():
    from plantos_amd import Policy
    b = make("g20", 200, seed=8)
    _, codes, f32 = rollout_obs(b, steps=12)
    assert codes.dtype is torch.uint8
    for towers, act in (SHAPES[1], SHAPES[3]):
        pol = Policy(b, towers, act, seed=1).load(make_tensors(towers, b.obs_dim, SEED, "var"))
        for det in (True, False):
            r1 = [np_(x).copy() if x is not None else None for x in pol.act(codes, deterministic=det, t=3)]
            r2 = [np_(x).copy() if x is not None else None for x in pol.act(f32, deterministic=det, t=3)]
            for u, v in zip(r1, r2):
                assert (u is None and v is None) or (u.tobytes() == v.tobytes())
        pol.close()
    b.close()


def guarded(shape, dtype, fill, pad):
    """a contiguous tensor of `shape` inside a larger one filled with `fill`: (view, whole)"""
    size = int(np.prod(shape))
    whole = torch.full((pad + size + pad,), fill, dtype=dtype, device=DEV)
    return whole[pad:pad + size].view(shape), whole


def test_padding_reads_and_writes_nothing_outside():
    from plantos_amd import Policy
    n = 65
    b = make("g20", n, seed=9)
    D = b.obs_dim
    _, codes, f32 = rollout_obs(b, steps=9)
    nan = float("nan")
    for towers, act in (SHAPES[1], SHAPES[4]):
        tensors = make_tensors(towers, D, SEED, "var")
        wholes, dev = [], []
        for tw in tensors:
            row = []
            for w, bias in tw:
                pair = []
                for arr, pad in ((w, 3), (bias, 1)):
                    view, whole = guarded(arr.shape, torch.float32, nan, pad)
                    view.copy_(torch.as_tensor(arr))
                    wholes.append((whole, whole.clone()))
                    pair.append(view)
                row.append(tuple(pair))
            dev.append(row)
        x32, x32_whole = guarded((n, D), torch.float32, nan, 3)
        x32.copy_(f32)
        x8, x8_whole = guarded((n, D), torch.uint8, 255, 5)
        x8.copy_(codes)
        wholes += [(x32_whole, x32_whole.clone()), (x8_whole, x8_whole.clone())]
        for et in (32, 64):
            pol = Policy(b, towers, act, seed=2, env_tile=et).load(dev)
            for x in (x32, x8):
                a, a_whole = guarded((n,), torch.int32, -7, 5)
                lg, lg_whole = guarded((n, 5), torch.float32, nan, 3)
                v, v_whole = guarded((n,), torch.float32, nan, 3)
                got = pol.act(x, deterministic=False, t=1, out=(a, lg, v))
                check_equal(got, pol.host_forward(np_(f32), tensors, deterministic=False, t=1), f"{towers} tile {et}")
                assert (np_(a_whole)[:5] == -7).all() and (np_(a_whole)[-5:] == -7).all()
                for whole in (lg_whole, v_whole):
                    assert np.isnan(np_(whole)[:3]).all() and np.isnan(np_(whole)[-3:]).all()
            pol.close()
        for whole, before in wholes:  # inputs untouched, surroundings included
            assert np_(whole).tobytes() == np_(before).tobytes()
    b.close()


def test_load_is_ordered_on_the_stream():
    from plantos_amd import Policy
    b = make("g21", 200, seed=10)
    x = b.reset()
    towers, act = SHAPES[2]
    ta, tb = make_tensors(towers, b.obs_dim, 1, "var"), make_tensors(towers, b.obs_dim, 2, "var")
    da, db = dev_tensors(ta), dev_tensors(tb)
    pol = Policy(b, towers, act)
    n = b.num_envs
    outs = [(torch.zeros(n, dtype=torch.int32, device=DEV), torch.zeros((n, 5), dtype=torch.float32, device=DEV),
             torch.zeros(n, dtype=torch.float32, device=DEV)) for _ in range(2)]
    torch.cuda.synchronize()
    pol.load(da)
    pol.act(x, out=outs[0])
    pol.load(db)
    pol.act(x, out=outs[1])
    torch.cuda.synchronize()
    check_equal(outs[0], pol.host_forward(np_(x), ta), "weights A")
    check_equal(outs[1], pol.host_forward(np_(x), tb), "weights B")
    assert not np.array_equal(np_(outs[0][1]), np_(outs[1][1]))
    pol.close()
    b.close()


def test_act_and_step_in_a_graph():
    """policy.act() then batch.step() captured as one chain; eight replays against eight
    eager iterations on a twin batch (argmax mode: nothing in the graph depends on t)."""
    from plantos_amd import Policy
    towers, act = SHAPES[1]
    res = []
    for graphed in (True, False):
        b = make("g20", 200, seed=12, prefetch_every=0)
        pol = Policy(b, towers, act).load(make_tensors(towers, b.obs_dim, SEED, "var"))
        a0 = b.synth_actions(1, 0)
        b.step(a0)  # the io buffer now holds codes
        pol.act()   # (every kernel of the chain has run once before the capture)
        torch.cuda.synchronize()
        log = []

        def one():
            a, _, _ = pol.act()
            b.step(a)

        if graphed:
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                one()
        for _ in range(8):
            gr.replay() if graphed else one()
            torch.cuda.synchronize()
            log.append([np_(pol.actions).copy(), np_(pol.logits).copy(), np_(b.io).copy()])
        res.append(log)
        if graphed:
            del gr
        pol.close()
        b.close()
    for it, (u, v) in enumerate(zip(*res)):
        for p, q in zip(u, v):
            assert p.tobytes() == q.tobytes(), f"iteration {it}"
    assert len({l[0].tobytes() for l in res[0]}) > 1  # the loop moved


def test_policy_loop_equals_oracle():
    """64 envs, 1010 steps across the 1000-step truncation and auto-reset: the GPU loop
    act -> step against the oracle driven by the twin's actions from the oracle's obs."""
    from plantos_amd import PlantOSBatch, Policy
    cfg, n, seed = (20, 10, 12, 6, 16), 64, 2025
    b = PlantOSBatch(n, grid_size=20, num_plants=10, num_obstacles=12, lidar_range=6, lidar_channels=16,
                     seed=seed, device=DEV)
    towers, act = SHAPES[1]
    tensors = make_tensors(towers, b.obs_dim, SEED, "var")
    pol = Policy(b, towers, act).load(tensors)
    ov = OracleVec(cfg, np.arange(n), seed)
    obs = b.reset(mask=torch.zeros(n, dtype=torch.uint8, device=DEV))
    o_obs = ov.obs()
    assert np.array_equal(np_(obs), o_obs)
    moved = set()
    for t in range(1010):
        a, _, _ = pol.act()
        obs, rew, te, tr = b.step(a)
        o_a, _, _ = pol.host_forward(o_obs, tensors)
        o_obs, o_rew, o_te, o_tr, *_ = ov.step(o_a)
        assert np.array_equal(np_(a), o_a), f"step {t}: actions"
        if not (np.array_equal(np_(obs), o_obs) and np.array_equal(np_(rew), o_rew.astype(np.float32))
                and np.array_equal(np_(te).astype(bool), o_te) and np.array_equal(np_(tr).astype(bool), o_tr)):
            raise AssertionError(f"GPU step {t} differs from the oracle")
        moved.update(o_a.tolist())
    assert len(moved) > 1
    pol.close()
    b.close()


def test_argument_checks_launch_nothing():
    from plantos_amd import Policy, _capi as C
    from plantos_amd.policy import _tower_structs
    L = C.lib()
    b = make("g21", 64, seed=1)  # no obs_codes
    for bad in ([[48, 5]], [[32, 5], [32, 2]], [[32, 1]], [[32, 32, 32, 32, 5]], [[544, 5]], [[32, 5]] * 3):
        with pytest.raises(ValueError):
            Policy(b, bad)
    p = ctypes.c_void_p()
    shapes = _tower_structs([[48, 5]])
    assert L.pe_policy_create(b.handle, 1, shapes, C.PE_ACT_TANH, 0, ctypes.byref(p)) == C.PE_ERR_ARG
    shapes = _tower_structs([[32, 5]])
    assert L.pe_policy_create(b.handle, 1, shapes, 7, 0, ctypes.byref(p)) == C.PE_ERR_ARG
    assert L.pe_policy_create(b.handle, 1, shapes, C.PE_ACT_TANH, 48, ctypes.byref(p)) == C.PE_ERR_ARG
    assert not p.value
    with pytest.raises(ValueError):
        Policy(b, [[512, 5]], env_tile=64)  # a 512-wide layer does not fit 64 envs per workgroup

    towers = [[32, 5]]
    pol = Policy(b, towers, "tanh").load(make_tensors(towers, b.obs_dim, SEED, "var"))
    n = b.num_envs
    x = b.reset()
    a = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    lg = torch.full((n, 5), -7.0, dtype=torch.float32, device=DEV)
    v = torch.full((n,), -7.0, dtype=torch.float32, device=DEV)
    s = b._stream()
    P = ctypes.c_void_p
    calls = [
        (pol._p, P(x.data_ptr()), 1, 0, 0, 0, P(a.data_ptr()), P(lg.data_ptr()), None, s),   # codes, no obs_codes
        (pol._p, P(x.data_ptr()), 0, 0, 0, 0, None, P(lg.data_ptr()), None, s),              # null actions
        (pol._p, None, 0, 0, 0, 0, P(a.data_ptr()), P(lg.data_ptr()), None, s),              # null obs
        (pol._p, P(x.data_ptr()), 0, 5, 0, 0, P(a.data_ptr()), P(lg.data_ptr()), None, s),   # bad mode
        (pol._p, P(x.data_ptr()), 0, 0, 0, 0, P(a.data_ptr()), P(lg.data_ptr()), P(v.data_ptr()), s),  # no value tower
        (None, P(x.data_ptr()), 0, 0, 0, 0, P(a.data_ptr()), P(lg.data_ptr()), None, s),     # null policy
    ]
    for args in calls:
        assert L.pe_policy_forward(*args) == C.PE_ERR_ARG
    with pytest.raises(ValueError):
        pol.act(torch.zeros((n, b.obs_dim), dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        pol.act(x[:-1])
    with pytest.raises(ValueError):
        pol.act(x, out=(a, lg, v))
    with pytest.raises(ValueError):
        pol.load(make_tensors([[64, 5]], b.obs_dim, SEED))
    torch.cuda.synchronize()
    assert (np_(a) == -7).all() and (np_(lg) == -7.0).all() and (np_(v) == -7.0).all()
    pol.act(x, out=(a, lg, None))
    check_equal((a, lg, None), pol.host_forward(np_(x)), "after the refusals")
    pol.close()
    b.close()
