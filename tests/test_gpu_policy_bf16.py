"""GPU checks of bf16 policy inference (Policy(precision="bf16"); include/plantos_batch.h,
"Reduced-precision policy inference"; csrc/pe_policy_bf16.hip) at obs lengths of every residue
mod 16 that matters to a k step of 16 (policy_bf16_util.GEO), one env past each tile (n = 33,
70), both env tiles wherever the plan accepts them:

1. the exact cases: lattice weights and obs (policy_bf16_util; proven exact on the host by
   test_policy_bf16_host.py) -- logits, values and actions equal the host twin's bit for bit;
2. self-consistency on realistic weights: run to run, tile to tile, act_rows, value and its
   selection, argmax and sampler over the GPU's own logits, graph capture;
3. accuracy on realistic weights against f64, with torch's own bf16 modules as the yardstick;
4. RolloutCollector and ReplayCollector with a bf16 policy against their host twins fed with
   the GPU's own logits, values and Q rows;
5. argument checks that launch nothing.
"""
import ctypes

import numpy as np
import pytest
import torch

import policy_bf16_util as BU
from policy_util import a2c_state_dict, dqn_state_dict, make_tensors

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NS = (33, 70)
CASES = [(g, f) for g in BU.GEO for f in BU.GEO[g]["obs"]]
FILL = -7.0


def np_(t):
    return None if t is None else t.detach().cpu().numpy()


def dev(x):
    return torch.as_tensor(x, device=DEV)


def make(name, n, form, **kw):
    from plantos_amd import PlantOSBatch
    G, P, Ob, R, C = BU.GEO[name]["cfg"]
    b = PlantOSBatch(n, grid_size=G, num_plants=P, num_obstacles=Ob, lidar_range=R, lidar_channels=C, device=DEV,
                     obs_codes=form == "codes", **kw)
    assert b.obs_dim == BU.obs_dim(name)
    return b


def stepped_obs(b, steps=6):
    """(the batch's own obs after `steps` synthetic steps -- codes on an obs_codes batch --, as f32 numpy)"""
    act = torch.empty(b.num_envs, dtype=torch.int32, device=DEV)
    for t in range(steps):
        b.synth_actions(5, t, out=act)
        b.step(act)
    x = b.obs.clone()
    return x, np_(b.expand_codes(b.io)[0] if b.obs_codes else x).copy()


def bf16_tiles(D, n, towers, act):
    """the env tiles the bf16 plan accepts"""
    from plantos_amd import _capi as C
    from plantos_amd import policy as P
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    out = []
    for et in (32, 64):
        try:
            C.policy_plan(D, n, cus, None, P._tower_structs(towers), P.ACTIVATIONS[act], et, precision=C.PE_PREC_BF16)
            out.append(et)
        except ValueError:
            assert et == 64
    return out


def check_equal(got, want, what):
    a, lg, v = (np_(x) for x in got)
    wa, wl, wv = want
    assert np.array_equal(lg, wl), f"{what}: logits differ ({(lg != wl).sum()} of {lg.size})"
    assert (v is None) == (wv is None) and (v is None or np.array_equal(v, wv)), f"{what}: values differ"
    assert np.array_equal(a, wa), f"{what}: actions differ"


def bits(got):
    return [None if x is None else np_(x).tobytes() for x in got]


def host_actions(logits, deterministic, seed, env_id_offset, t):
    """The definition's argmax / sampler over given logits [n, A]: the f32 host twin on a net that
    passes its input through exactly -- units a and A + a hold relu(l_a) and relu(-l_a), the head
    subtracts them (one of the two is zero, every product is exact)."""
    from plantos_amd import policy as P
    A = logits.shape[1]
    W = np.zeros((32, A), np.float32)
    W[np.arange(A), np.arange(A)] = 1
    W[A + np.arange(A), np.arange(A)] = -1
    H = np.zeros((A, 32), np.float32)
    H[np.arange(A), np.arange(A)] = 1
    H[np.arange(A), A + np.arange(A)] = -1
    net = [[(W, np.zeros(32, np.float32)), (H, np.zeros(A, np.float32))]]
    a, lg, _ = P.host_forward([[32, A]], net, "relu", logits, deterministic=deterministic, seed=seed,
                              env_id_offset=env_id_offset, t=t)
    assert np.array_equal(lg, logits)
    return a


# ---------------------------------------------------------------- 1: exact cases
@pytest.mark.parametrize("net", range(len(BU.EXACT_NETS)))
@pytest.mark.parametrize("name,form", CASES)
def test_exact_cases_equal_the_twin(name, form, net):
    """Lattice weights: every partial sum of every hidden pre-activation is exact in f32 whatever
    the order (asserted here too, with the code table where the obs are codes), so the kernel
    must give the twin's bits.  f32 obs: lattice rows through act(obs=...); codes: the batch's
    own codes after a few steps."""
    from plantos_amd import Policy
    towers, act = BU.EXACT_NETS[net]
    D = BU.obs_dim(name)
    tensors = BU.lattice_tensors(towers, D, BU.LATTICE_SEED)
    BU.lattice_check(towers, tensors, act, BU.exact_x_values(name, form))
    ran = set()
    for n in NS:
        b = make(name, n, form, seed=3, env_id_offset=1000)
        if form == "codes":
            x, x32 = stepped_obs(b)
            assert x.dtype is torch.uint8 and np.array_equal(b.code_table()[np_(x)], x32)
        else:
            x32 = BU.lattice_obs(n, D, BU.LATTICE_SEED + n)
            x = dev(x32)
        want = None
        for et in bf16_tiles(D, n, towers, act):
            pol = Policy(b, towers, act, seed=99, env_tile=et, precision="bf16").load(tensors)
            assert pol.env_tile == et and pol.precision == "bf16"
            if want is None:
                want = pol.host_forward(x32, tensors)
                assert np.isfinite(want[1]).all() and len(np.unique(want[1])) > n  # the net says something
            check_equal(pol.act(x), want, f"{name} {form} n={n} {towers} {act} tile {et}")
            ran.add(et)
            pol.close()
        b.close()
    assert 32 in ran


# ---------------------------------------------------------------- 2: self-consistency
def realistic(kind, D):
    from plantos_amd import policy as P
    sd = a2c_state_dict(D, (256, 256), seed=D) if kind == "a2c" else dqn_state_dict(D, (512, 512, 256), seed=D)
    towers, act, tensors = P.parse_state_dict(sd)
    return towers, act, BU.np_tensors(tensors)


@pytest.mark.parametrize("kind", ["a2c", "dqn"])
@pytest.mark.parametrize("name,form", CASES)
def test_self_consistency(name, form, kind):
    from plantos_amd import Policy
    D = BU.obs_dim(name)
    towers, act, tensors = realistic(kind, D)
    two = len(towers) == 2
    for n in NS:
        b = make(name, n, form, seed=5, env_id_offset=40)
        x, _ = stepped_obs(b)
        first = None
        for et in bf16_tiles(D, n, towers, act):
            what = f"{name} {form} {kind} n={n} tile {et}"
            pol = Policy(b, towers, act, seed=17, env_tile=et, precision="bf16").load(tensors)
            got = bits(pol.act(x))
            assert got == bits(pol.act(x)), f"{what}: act() twice"
            if first is None:
                first = got
            assert got == first, f"{what}: against the other tile"
            logits, actions = np_(pol.logits).copy(), np_(pol.actions).copy()
            assert np.isfinite(logits).all() and len(np.unique(logits)) > n
            # rows: the same rows, one row, more rows than the batch has envs
            assert bits(pol.act_rows(x)) == got, f"{what}: act_rows"
            one = pol.act_rows(x[:1].contiguous())
            assert np_(one[1]).tobytes() == logits[:1].tobytes() and np_(one[0])[0] == actions[0], f"{what}: one row"
            many = pol.act_rows(torch.cat([x, x, x[:3]]).contiguous())
            assert np_(many[1]).tobytes() == np.concatenate([logits, logits, logits[:3]]).tobytes(), f"{what}: 2 n + 3 rows"
            assert np.array_equal(np_(many[0]), np.concatenate([actions, actions, actions[:3]]))
            # argmax and the sampler, over the GPU's own logits
            off = int(b.cfg.env_id_offset)
            assert np.array_equal(actions, host_actions(logits, True, pol.seed, off, 0)), f"{what}: argmax"
            a, lg, v = pol.act(x, deterministic=False, t=7)
            assert bits((lg, v)) == got[1:], f"{what}: the sampler changed a head"
            assert np.array_equal(np_(a), host_actions(logits, False, pol.seed, off, 7)), f"{what}: sampler"
            if two:
                values = np_(pol.values).copy()
                out = torch.full((n,), FILL, dtype=torch.float32, device=DEV)
                assert pol.value(x, out=out) is out and np_(out).tobytes() == values.tobytes(), f"{what}: value()"
                rng = np.random.default_rng(n + et)
                want_f, unless_f = rng.integers(0, 2, n).astype(np.uint8), rng.integers(0, 2, n).astype(np.uint8)
                want_f[32:64] = 0                          # a whole tile of 32 with nothing selected
                sel = (want_f != 0) & (unless_f == 0)
                assert sel.any() and not sel.all()
                out.fill_(FILL)
                pol.value(x, select=(dev(want_f), dev(unless_f)), out=out)
                assert np_(out).tobytes() == np.where(sel, values, np.float32(FILL)).tobytes(), f"{what}: select"
                out.fill_(FILL)
                pol.value(x, select=dev(np.zeros(n, np.uint8)), out=out)
                assert (np_(out) == FILL).all(), f"{what}: nothing selected"
            pol.close()
        b.close()


def test_act_and_step_in_a_graph():
    """act() then step() captured as one chain: six replays against six eager iterations on a twin batch."""
    from plantos_amd import Policy
    sd = a2c_state_dict(107, (256, 256), seed=107)
    res = []
    for graphed in (True, False):
        b = make("g20", 70, "codes", seed=12, prefetch_every=0)
        pol = Policy.from_state_dict(b, sd, precision="bf16")   # the keyword passes through
        assert pol.precision == "bf16" and pol.towers == [[256, 256, 5], [256, 256, 1]]
        b.step(b.synth_actions(1, 0))  # the io buffer now holds codes
        pol.act()                      # (every kernel of the chain has run once before the capture)
        torch.cuda.synchronize()
        log = []

        def one():
            a, _, _ = pol.act()
            b.step(a)

        if graphed:
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                one()
        for _ in range(6):
            gr.replay() if graphed else one()
            torch.cuda.synchronize()
            log.append([np_(pol.actions).copy(), np_(pol.logits).copy(), np_(pol.values).copy(), np_(b.io).copy()])
        res.append(log)
        if graphed:
            del gr
        pol.close()
        b.close()
    for it, (u, v) in enumerate(zip(*res)):
        for p, q in zip(u, v):
            assert p.tobytes() == q.tobytes(), f"iteration {it}"
    assert len({l[1].tobytes() for l in res[0]}) > 1  # the loop moved


# ---------------------------------------------------------------- 3: accuracy
@pytest.mark.parametrize("kind", ["a2c", "dqn"])
@pytest.mark.parametrize("name,form", CASES)
def test_accuracy_against_f64(name, form, kind):
    """Reference: f64 torch on the f32 weights; yardstick: torch's own bf16 modules on the CPU.  The
    GPU's worst head deviation is at most 1.25 x the yardstick's: the definition sits at 0.65 ..
    0.91 on the CPU, another f32 summation order moves a head by at most 0.17 of the quantization
    error, and a kernel bug shows as 10 or more.  Measured ratios: DESIGN.md section 4."""
    from plantos_amd import Policy
    D, n = BU.obs_dim(name), 70
    towers, act, tensors = realistic(kind, D)
    b = make(name, n, form, seed=9)
    x, x32 = stepped_obs(b)
    pol = Policy(b, towers, act, precision="bf16").load(tensors)
    _, lg, v = pol.act(x)
    gpu = BU.worst_deviation((np_(lg), np_(v)), BU.reference_heads(tensors, act, x32))
    yard = BU.torch_bf16_heads(tensors, act, x32)
    ref = BU.reference_heads(tensors, act, x32)
    yardstick = BU.worst_deviation((yard[0], yard[1][:, 0] if len(yard) == 2 else None), ref)
    twin = BU.worst_deviation(pol.host_forward(x32)[1:], ref)
    print(f"ACCURACY {name} {form} {kind}: gpu {gpu:.3e} twin {twin:.3e} torch-bf16 {yardstick:.3e} "
          f"ratio {gpu / yardstick:.3f} (twin {twin / yardstick:.3f})")
    pol.close()
    b.close()
    assert 0 < gpu <= 1.25 * yardstick


# ---------------------------------------------------------------- 4: collectors
def test_rollout_collector_with_a_bf16_policy():
    """RolloutCollector(n_steps=5) on g20 codes, 70 envs: every tensor of the Rollout equals
    host_rollout fed with the GPU's own per-step logits and values of a manual act / step loop."""
    from plantos_amd import Policy, RolloutCollector
    from test_gpu_rollout import check_rollout, expected, manual_loop, new_acc
    n, T, gamma, lam = 70, 5, 0.99, 0.95
    towers, act, tensors = realistic("a2c", 107)
    for det in (False, True):
        b, b2 = (make("g20", n, "codes", seed=21, max_steps=3) for _ in range(2))
        pol, pol2 = (Policy(x, towers, act, seed=99, precision="bf16").load(tensors) for x in (b, b2))
        ro = RolloutCollector(b, pol, T, gamma=gamma, gae_lambda=lam, deterministic=det).collect()
        log = manual_loop(b2, pol2, T, det)
        want = expected(log, 0, T, np.ones(n, np.uint8), log["next_values"], gamma, lam, True, new_acc(n))
        check_rollout(ro, want, f"bf16 det={det}")
        assert np.array_equal(b.code_table()[np_(ro.obs)], log["obs"])
        assert ((log["truncated"] != 0) & (log["terminated"] == 0)).any()   # the bootstrap's value() ran
        for z in (pol, pol2, b, b2):
            z.close()


def test_replay_collector_with_a_bf16_policy():
    """ReplayCollector: collect() against the host ring driven by the GPU's own greedy actions, then
    sample() and targets() against the host twins fed with the GPU's own Q rows."""
    from plantos_amd import Policy, ReplayCollector
    from test_gpu_replay import check_ring, host_replay
    n, K, eps = 70, 4, 0.5
    towers, act, tensors = realistic("dqn", 107)
    b, b2 = (make("g20", n, "codes", seed=21, max_steps=3) for _ in range(2))
    pol, pol2 = (Policy(x, towers, act, precision="bf16").load(tensors) for x in (b, b2))
    tgt = Policy(b, [[32, 5]], "relu", precision="bf16").load(make_tensors([[32, 5]], 107, 9, "var"))
    rc = ReplayCollector(b, pol, buffer_size=K * n, seed=123)
    rc.set_eps(eps)
    rc.collect(5)
    twin = ReplayCollector(b2, pol2, buffer_size=K * n, seed=123)
    ring = twin.host_ring()
    codes, _, actions = host_replay(b2, pol2, twin, 5, eps, ring)
    check_ring(rc, ring, "5 steps")
    assert np.array_equal(np_(rc.current_obs), codes) and np.array_equal(np_(rc.actions), actions[-1])
    mb = rc.sample(65)
    idx = np_(mb.indices)
    assert np.array_equal(idx, twin.host_sample_indices(65, 5, 0))
    assert np_(mb.next_obs).tobytes() == ring.next_obs[idx[:, 0], idx[:, 1]].tobytes()
    y = rc.targets(mb, tgt, gamma=0.99)
    q = np_(tgt.act_rows(mb.next_obs)[1])
    assert np_(y).tobytes() == rc.host_target(q, np_(mb.rewards), np_(mb.dones), 0.99).tobytes()
    assert np.abs(q - tgt.host_forward(b.code_table()[np_(mb.next_obs)])[1]).max() < 1e-2  # (and Q is the twin's net)
    for z in (pol, pol2, tgt, b, b2):
        z.close()


# ---------------------------------------------------------------- 5: argument checks
def test_argument_checks_launch_nothing():
    from plantos_amd import Policy, RecurrentPolicy, _capi as C
    from plantos_amd.policy import _tower_structs
    L = C.lib()
    b = make("g21", 33, "f32", seed=1)
    n, D = b.num_envs, b.obs_dim
    for bad in ("f16", "fp8", None, 1):
        with pytest.raises(ValueError, match="precision"):
            Policy(b, [[32, 5]], precision=bad)
    with pytest.raises(TypeError):
        RecurrentPolicy(b, 32, [[32, 5]], precision="bf16")
    p = ctypes.c_void_p()
    shapes = _tower_structs([[32, 5]])
    for bad in (-1, 2):
        assert L.pe_policy_create_prec(b.handle, 1, shapes, C.PE_ACT_TANH, 0, bad, ctypes.byref(p)) == C.PE_ERR_ARG
        assert not p.value and b"precision" in L.pe_last_error()
    # the f32 spelling gives an f32 policy, the old entry point too
    for create in (lambda: L.pe_policy_create_prec(b.handle, 1, shapes, C.PE_ACT_TANH, 0, C.PE_PREC_F32, ctypes.byref(p)),
                   lambda: L.pe_policy_create(b.handle, 1, shapes, C.PE_ACT_TANH, 0, ctypes.byref(p))):
        assert create() == C.PE_OK and L.pe_policy_precision(p) == C.PE_PREC_F32
        assert L.pe_policy_destroy(p) == C.PE_OK
    assert Policy(b, [[32, 5]]).precision == "f32"

    # a shape whose bf16 images do not fit LDS: the plan's message, from the constructor and from C
    big = make("max417", 33, "f32", seed=1)
    with pytest.raises(ValueError, match="bf16 obs and activation images do not fit 160 KiB of LDS"):
        Policy(big, [[512, 512, 5]], env_tile=64, precision="bf16")
    p = ctypes.c_void_p()
    assert L.pe_policy_create_prec(big.handle, 1, _tower_structs([[512, 512, 5]]), C.PE_ACT_RELU, 64, C.PE_PREC_BF16,
                                   ctypes.byref(p)) == C.PE_ERR_ARG
    assert not p.value and b"LDS" in L.pe_last_error()
    big.close()

    towers = [[32, 5], [32, 1]]
    pol = Policy(b, towers, "tanh", precision="bf16").load(make_tensors(towers, D, 3, "var"))
    assert L.pe_policy_precision(pol._p) == C.PE_PREC_BF16
    x = b.reset()
    a = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    lg = torch.full((n, 5), FILL, dtype=torch.float32, device=DEV)
    v = torch.full((n,), FILL, dtype=torch.float32, device=DEV)
    s, P = b._stream(), ctypes.c_void_p
    xa, aa, la, va = P(x.data_ptr()), P(a.data_ptr()), P(lg.data_ptr()), P(v.data_ptr())
    # the *_lstm calls refuse a bf16 policy as they refuse any feed-forward one
    assert L.pe_policy_forward_lstm(pol._p, xa, 0, None, None, 0, 0, 0, aa, la, va, s) == C.PE_ERR_ARG
    assert L.pe_policy_value_lstm(pol._p, xa, 0, None, None, None, None, va, s) == C.PE_ERR_ARG
    # check_forward's refusals hold for a bf16 policy
    for args in ((pol._p, xa, 1, 0, 0, 0, aa, la, None, s),      # codes, no obs_codes
                 (pol._p, xa, 0, 0, 0, 0, None, la, None, s),    # null actions
                 (pol._p, None, 0, 0, 0, 0, aa, la, None, s),    # null obs
                 (pol._p, xa, 0, 5, 0, 0, aa, la, None, s)):     # bad mode
        assert L.pe_policy_forward(*args) == C.PE_ERR_ARG
    assert L.pe_policy_forward_rows(pol._p, 0, xa, 0, aa, la, None, s) == C.PE_ERR_ARG
    assert L.pe_policy_value(pol._p, None, 0, None, None, va, s) == C.PE_ERR_ARG
    one = Policy(b, [[32, 5]], "tanh", precision="bf16")
    assert L.pe_policy_forward(one._p, xa, 0, 0, 0, 0, aa, la, va, s) == C.PE_ERR_ARG   # no value tower
    assert L.pe_policy_value(one._p, xa, 0, None, None, va, s) == C.PE_ERR_ARG
    torch.cuda.synchronize()
    assert (np_(a) == -7).all() and (np_(lg) == FILL).all() and (np_(v) == FILL).all()
    one.close()
    pol.close()
    b.close()
