"""GPU checks of the A2C learner (plantos_amd.A2CLearner; csrc/pe_learner.hip): gradients, loss
scalars, the gradient norm, parameters and square_avg equal the host twin bit for bit after each of
three updates, at the smallest shapes at which each path can go wrong -- below one tile, ragged
tiles, the edges of a gradient chunk (kGradChunk), more than two chunks; one, two and three hidden
layers (the third reads a layer's activations back from the workspace), the 512-wide net that only
fits 32-row tiles, 2 / 5 / 8 actions, both activations, obs as codes and as f32, a clip that binds
and one that does not, both env_tiles; the hand-off to the policy; the collect / train loop; graph
capture.

Obs lengths: 52, 72, 107, and the residues the learner's own D-dependent code meets (the row-major
copy of the staging image, layer 0's weight-gradient problem with pitch D and the bias as column K
of the last 32-wide tile): 57 (7 padded columns, D % 4 = 1), 87 (1 padded column), 127 (K + 1 = 128:
the bias is the last column of the last tile) and 347 (only 32-row tiles fit, HB is the staging
pitch, layer 0 takes three groups of input tiles with a ragged last one).  Row counts past
kNormChunk, where the row-term sums take more than one chunk and the sums grid comes from the rows.
One learner over many row counts below max_rows with every scratch buffer poisoned before each
update.  Hyper-parameters other than the loop's, a per-call learning rate, a loaded optimizer
state.  Saturated heads (subnormal gradients), huge returns, the exact zero gradient, a dead relu
layer.  train() on a batch without obs codes.
"""
import numpy as np
import pytest
import torch

import plantos_amd.learner as L
from learner_util import HYPER_SETS, NETS, flat, scale_pi_head
from plantos_amd.rollout import NORM_CHUNK as NC
from policy_util import geometry_codes, make_tensors

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CH = L.GRAD_CHUNK
# D -> (G, plants, obstacles, R, C): policy_geometries' e52, e72; g20; then one per residue of the docstring
GEO = {52: (8, 3, 3, 4, 5), 72: (10, 4, 4, 5, 9), 107: (20, 10, 12, 6, 16),
       57: (9, 3, 3, 3, 6), 87: (12, 4, 6, 7, 12), 127: (12, 4, 6, 5, 20), 347: (24, 10, 12, 6, 64)}
HYPER = dict(learning_rate=7e-4, ent_coef=0.01, vf_coef=0.5)


def np_(t):
    return t.detach().cpu().numpy()


def dev(x):
    return torch.as_tensor(x, device=DEV)


def make_batch(D, n=64, **kw):
    from plantos_amd import PlantOSBatch
    G, P, Ob, R, C = GEO[D]
    kw.setdefault("obs_codes", True)
    b = PlantOSBatch(n, grid_size=G, num_plants=P, num_obstacles=Ob, lidar_range=R, lidar_channels=C, device=DEV, **kw)
    assert b.obs_dim == D
    return b


def make_rows(b, towers, rows, seed):
    """(codes u8 [rows, D], obs f32 = table[codes], actions, advantages, returns), numpy."""
    rng = np.random.default_rng(seed)
    G, _, _, R, _ = GEO[b.obs_dim]
    codes = geometry_codes(rng, rows, G, R, b.obs_dim)
    obs = np.ascontiguousarray(b.code_table()[codes])
    return (codes, obs, rng.integers(0, towers[0][-1], rows).astype(np.int32),
            rng.standard_normal(rows).astype(np.float32), (2.0 * rng.standard_normal(rows)).astype(np.float32))


def read(tensors):
    return [[(np_(w).copy(), np_(b).copy()) for w, b in tw] for tw in tensors]


def check_against_twin(learner, stats, twin, what):
    torch.cuda.synchronize()
    assert np.array_equal(flat(read(learner.gradients)), twin["flat_gradients"]), f"{what}: gradients"
    for k in L.STATS:
        assert np.array_equal(np_(stats[k]), twin[k]), f"{what}: {k} {np_(stats[k])} != {twin[k]}"
    assert np.array_equal(flat(read(learner.parameters)), flat(twin["tensors"])), f"{what}: parameters"
    assert np.array_equal(flat(read(learner.square_avg)), flat(twin["square_avg"])), f"{what}: square_avg"


# (net, activation, D, rows, env_tile, obs form, max_grad_norm)
CASES = [
    ("n32", "tanh", 52, 1, 32, "codes", 0.5),
    ("n32", "relu", 52, 31, 64, "f32", 1e6),
    ("n64x32", "tanh", 72, 70, 64, "codes", 0.5),
    ("n64x32", "relu", 107, 210, 32, "f32", 1e6),
    ("n96_3x32", "tanh", 107, CH - 1, 64, "codes", 0.5),
    ("n96_3x32", "relu", 52, CH, 32, "codes", 1e6),
    ("n96_3x32", "tanh", 72, 2 * CH + 5, 32, "f32", 0.5),
    ("a2c", "tanh", 107, CH + 1, 64, "codes", 0.5),
    ("a2c", "relu", 72, 2 * CH + 5, 32, "f32", 0.5),
    ("w512", "tanh", 72, 70, 32, "codes", 0.5),
    ("w512", "relu", 107, 2 * CH + 5, 32, "f32", 1e6),
    ("n64x32", "tanh", 52, CH + 1, 32, "f32", 0.5),
    # obs lengths 57 / 87 / 127: both activations, both obs forms, both tiles, a binding and a loose clip
    ("n64x32", "relu", 57, 70, 64, "f32", 1e6),
    ("n96_3x32", "tanh", 87, CH + 1, 32, "codes", 0.5),
    ("n32", "relu", 127, CH + 1, 64, "codes", 0.5),
    # 347: tile 32 only, layer 0's weight gradient in three groups of input tiles
    ("n64x32", "tanh", 347, 70, 32, "codes", 0.5),
    ("n96_3x32", "relu", 347, 2 * CH + 5, 32, "f32", 1e6),
    # more rows than kNormChunk: rows > n_params (3590: the sums grid comes from the rows), then n_params
    # (11529) > rows > 2 kNormChunk
    ("n32", "tanh", 52, NC + 1, 64, "codes", 0.5),
    ("n64x32", "relu", 72, 2 * NC + 3, 32, "f32", 1e6),
]


@pytest.mark.parametrize("net,act,D,rows,tile,form,max_grad_norm", CASES)
def test_three_updates_equal_the_twin(net, act, D, rows, tile, form, max_grad_norm):
    from plantos_amd import A2CLearner, Policy
    towers = NETS[net]
    b = make_batch(D)
    tensors = make_tensors(towers, D, 31, "var")
    pol = Policy(b, towers, act, env_tile=tile).load(tensors)
    assert pol.env_tile == tile
    learner = A2CLearner(pol, max_grad_norm=max_grad_norm, max_rows=rows, **HYPER)
    codes, obs, a, adv, ret = make_rows(b, towers, rows, seed=rows)
    x = dev(codes) if form == "codes" else dev(obs)
    a_d, adv_d, ret_d = dev(a), dev(adv), dev(ret)
    sq, clipped = None, []
    for step in range(3):
        twin = L.host_update(towers, tensors, act, obs, a, adv, ret, square_avg=sq, max_grad_norm=max_grad_norm, **HYPER)
        stats = learner.update(obs=x, actions=a_d, advantages=adv_d, returns=ret_d)
        check_against_twin(learner, stats, twin, f"update {step}")
        assert int(np_(stats["n_updates"])[0]) == step + 1
        tensors, sq = twin["tensors"], twin["square_avg"]
        clipped.append(bool(twin["clip_coef"] < 1.0))
    assert clipped[0] == (max_grad_norm == 0.5) and (max_grad_norm == 0.5 or not any(clipped))
    with pytest.raises(ValueError, match="max_rows"):
        learner.update(obs=dev(np.zeros((rows + 1, D), np.float32)), actions=dev(np.zeros(rows + 1, np.int32)),
                       advantages=dev(np.zeros(rows + 1, np.float32)), returns=dev(np.zeros(rows + 1, np.float32)))
    if D == 347:  # the hand-off: the policy's own kernel (HB = the staging pitch here too) acts with the new weights
        from plantos_amd.policy import host_forward
        acts, logits, values = pol.act(obs=x[:b.num_envs])
        torch.cuda.synchronize()
        wa, wl, wv = host_forward(towers, tensors, act, obs[:b.num_envs])
        assert np.array_equal(np_(logits), wl) and np.array_equal(np_(values), wv) and np.array_equal(np_(acts), wa)
    learner.close(), pol.close(), b.close()


def test_no_learner_on_64_row_tiles_at_347():
    """At D = 347 the LDS holds 32-row tiles only: the plan refuses env_tile = 64 for the learner and
    for the policy it would be built on, so no learner of that tile can exist."""
    from plantos_amd import Policy
    towers = NETS["n64x32"]
    assert L.learner_plan(347, 70, 256, towers, env_tile=32).env_tile == 32
    with pytest.raises(ValueError, match="LDS"):
        L.learner_plan(347, 70, 256, towers, env_tile=64)
    b = make_batch(347)
    with pytest.raises(ValueError, match="LDS"):
        Policy(b, towers, "tanh", env_tile=64)
    b.close()


def test_tiles_and_obs_forms_give_the_same_bits():
    from plantos_amd import A2CLearner, Policy
    towers, D, rows = NETS["n64x32"], 107, 210
    got = []
    for tile, form in ((32, "codes"), (64, "f32"), (64, "codes")):
        b = make_batch(D)
        pol = Policy(b, towers, "tanh", env_tile=tile).load(make_tensors(towers, D, 5, "var"))
        learner = A2CLearner(pol, max_rows=rows + 40, **HYPER)
        codes, obs, a, adv, ret = make_rows(b, towers, rows, seed=8)
        stats = learner.update(obs=dev(codes if form == "codes" else obs), actions=dev(a), advantages=dev(adv),
                               returns=dev(ret))
        torch.cuda.synchronize()
        got.append(np.concatenate([flat(read(learner.gradients)), flat(read(learner.parameters)),
                                   flat(read(learner.square_avg)), np_(learner._out)]))
        learner.close(), pol.close(), b.close()
    assert got[0].tobytes() == got[1].tobytes() == got[2].tobytes()


def test_refusals_on_the_device():
    from plantos_amd import A2CLearner, Policy
    b = make_batch(52)
    one = Policy(b, [[32, 5]], "relu").load(make_tensors([[32, 5]], 52, 1))
    with pytest.raises(ValueError, match="two-tower"):
        A2CLearner(one, max_rows=8)
    bf = Policy(b, NETS["n32"], "tanh", precision="bf16").load(make_tensors(NETS["n32"], 52, 1))
    with pytest.raises(ValueError, match="bf16"):
        A2CLearner(bf, max_rows=8)
    empty = Policy(b, NETS["n32"], "tanh")
    with pytest.raises(ValueError, match="loaded"):
        A2CLearner(empty, max_rows=8)
    pol = Policy(b, NETS["n32"], "tanh").load(make_tensors(NETS["n32"], 52, 1))
    lazy = A2CLearner(pol)
    with pytest.raises(ValueError, match="max_rows"):
        lazy.update(obs=dev(np.zeros((4, 52), np.float32)), actions=dev(np.zeros(4, np.int32)),
                    advantages=dev(np.zeros(4, np.float32)), returns=dev(np.zeros(4, np.float32)))
    for p in (one, bf, empty, pol):
        p.close()
    b.close()


def test_the_policy_acts_with_the_new_weights():
    from plantos_amd import A2CLearner, Policy
    towers, D, n = NETS["n64x32"], 72, 70
    b = make_batch(D, n=n)
    tensors = make_tensors(towers, D, 12, "var")
    pol = Policy(b, towers, "tanh").load(tensors)
    learner = A2CLearner(pol, max_rows=n, **HYPER)
    codes, obs, a, adv, ret = make_rows(b, towers, n, seed=2)
    twin = L.host_update(towers, tensors, "tanh", obs, a, adv, ret, **HYPER)
    learner.update(obs=dev(codes), actions=dev(a), advantages=dev(adv), returns=dev(ret))
    acts, logits, values = pol.act(obs=dev(codes))
    torch.cuda.synchronize()
    from plantos_amd.policy import host_forward
    wa, wl, wv = host_forward(towers, twin["tensors"], "tanh", obs)
    assert np.array_equal(np_(logits), wl) and np.array_equal(np_(values), wv) and np.array_equal(np_(acts), wa)
    assert not np.array_equal(wl, host_forward(towers, tensors, "tanh", obs)[1])
    # the policy's own twin and the state dict read the master parameters
    assert np.array_equal(pol.host_forward(obs)[1], wl)
    sd = learner.state_dict()
    assert np.array_equal(np_(sd["action_net.weight"]), twin["tensors"][0][-1][0])
    assert np.array_equal(np_(sd["mlp_extractor.value_net.2.bias"]), twin["tensors"][1][1][1])
    learner.close(), pol.close(), b.close()


def test_collect_train_loop():
    from plantos_amd import A2CLearner, Policy, RolloutCollector, host_adv_norm
    from plantos_amd.policy import host_forward
    towers, D, n, T = NETS["n64x32"], 107, 70, 5
    b = make_batch(D, n=n, max_steps=7, seed=4)
    tensors = make_tensors(towers, D, 21, "var")
    pol = Policy(b, towers, "tanh", seed=3).load(tensors)
    col = RolloutCollector(b, pol, T, gamma=0.99, gae_lambda=1.0)
    learner = A2CLearner(pol, **HYPER)  # max_rows: the collector's n_steps * n, at the first train
    table, sq = b.code_table(), None
    for it in range(3):
        ro = col.collect()
        torch.cuda.synchronize()
        last_obs = table[np_(ro.obs[T - 1])]
        assert np.array_equal(np_(col._logits), host_forward(towers, tensors, "tanh", last_obs)[1]), f"collect {it}: logits"
        raw_adv = np_(ro.advantages).reshape(-1)
        stats = learner.train(ro, normalize_advantage=True)
        torch.cuda.synchronize()
        mb = learner.last_minibatch
        assert mb.count == T * n == learner.max_rows
        idx = np_(mb.indices)
        assert np.array_equal(np_(mb.advantages), host_adv_norm(raw_adv[idx]))
        twin = L.host_update(towers, tensors, "tanh", table[np_(mb.codes)], np_(mb.actions), np_(mb.advantages),
                             np_(mb.returns), square_avg=sq, **HYPER)
        check_against_twin(learner, stats, twin, f"iteration {it}")
        tensors, sq = twin["tensors"], twin["square_avg"]
    learner.close(), pol.close(), b.close()


def test_graph_capture_replays_the_next_update():
    from plantos_amd import A2CLearner, Policy
    towers, D, rows = NETS["n64x32"], 52, CH + 1
    b = make_batch(D)
    tensors = make_tensors(towers, D, 6, "var")
    pol = Policy(b, towers, "relu").load(tensors)
    learner = A2CLearner(pol, max_rows=rows, **HYPER)
    codes, obs, a, adv, ret = make_rows(b, towers, rows, seed=3)
    args = dict(obs=dev(codes), actions=dev(a), advantages=dev(adv), returns=dev(ret))
    for _ in range(3):
        learner.update(**args)
    torch.cuda.synchronize()
    want = np.concatenate([flat(read(learner.parameters)), flat(read(learner.square_avg)), np_(learner._out)])
    learner.load(tensors)  # every kernel has run before the capture; back to the start
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        learner.update(**args)
    learner.load(tensors)  # whatever the capture did
    for _ in range(3):
        gr.replay()
    torch.cuda.synchronize()
    got = np.concatenate([flat(read(learner.parameters)), flat(read(learner.square_avg)), np_(learner._out)])
    assert got.tobytes() == want.tobytes() and int(np_(learner.n_updates)[0]) == 3
    acts, logits, _ = pol.act(obs=dev(codes[:64]))
    from plantos_amd.policy import host_forward
    assert np.array_equal(np_(logits), host_forward(towers, read(learner.parameters), "relu", obs[:64])[1])
    del gr
    learner.close(), pol.close(), b.close()


def test_graph_capture_of_train_replays_the_next_update():
    """One train() -- the all-rows minibatch gather, the advantage normalisation and the update --
    captured after a warm-up call and replayed equals eager train() calls on the same rollout."""
    from plantos_amd import A2CLearner, Policy, RolloutCollector
    from plantos_amd.policy import host_forward
    towers, D, n, T = NETS["n64x32"], 107, 70, 5
    b = make_batch(D, n=n, max_steps=7, seed=11)
    tensors = make_tensors(towers, D, 17, "var")
    pol = Policy(b, towers, "tanh", seed=5).load(tensors)
    ro = RolloutCollector(b, pol, T, gamma=0.99, gae_lambda=1.0).collect()
    learner = A2CLearner(pol, **HYPER)  # max_rows None: built by the first train()

    def state():
        torch.cuda.synchronize()
        return np.concatenate([flat(read(learner.parameters)), flat(read(learner.square_avg)),
                               flat(read(learner.gradients)), np_(learner._out)])
    for _ in range(3):  # (also the warm-up: the lazy build and every allocation happen here)
        learner.train(ro, normalize_advantage=True)
    want = state()
    assert learner.max_rows == T * n
    learner.load(tensors)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        stats = learner.train(ro, normalize_advantage=True)
    learner.load(tensors)  # whatever the capture did
    gr.replay()
    first = state()
    for _ in range(2):
        gr.replay()
    assert state().tobytes() == want.tobytes() and int(np_(stats["n_updates"])[0]) == 3
    assert first.tobytes() != want.tobytes()  # a replay performed an update, each one the next
    # ... and equals the twin on the minibatch the captured gather wrote
    mb, table = learner.last_minibatch, b.code_table()
    twin = L.host_update(towers, tensors, "tanh", table[np_(mb.codes)], np_(mb.actions), np_(mb.advantages),
                         np_(mb.returns), **HYPER)
    assert np.array_equal(first[:flat(tensors).size], flat(twin["tensors"]))
    obs = table[np_(mb.codes)[:n]]
    assert np.array_equal(np_(pol.act(obs=dev(np_(mb.codes)[:n]))[1]),
                          host_forward(towers, read(learner.parameters), "tanh", obs)[1])
    del gr
    learner.close(), pol.close(), b.close()


def step_against_twin(learner, act, state, data, form, hyper, what, learning_rate=None):
    """One update of `learner` and of the twin from state = (tensors, square_avg) on data =
    make_rows' tuple, compared; returns the twin's result."""
    towers = learner.towers
    codes, obs, a, adv, ret = data
    h = dict(hyper) if learning_rate is None else dict(hyper, learning_rate=learning_rate)
    twin = L.host_update(towers, state[0], act, obs, a, adv, ret, square_avg=state[1], **h)
    stats = learner.update(obs=dev(codes if form == "codes" else obs), actions=dev(a), advantages=dev(adv),
                           returns=dev(ret), learning_rate=learning_rate)
    check_against_twin(learner, stats, twin, what)
    return twin


def test_many_row_counts_on_one_learner_with_poisoned_scratch():
    """Updates of 517, 70, 257, 1, 255 and 517 rows on one learner of max_rows = 517 -- a short last
    minibatch is ordinary use -- each against the twin carried forward.  Before every update the
    workspace, the chunk partials and the f64 sums are filled with NaN, so whatever an update reads
    without having written it (a stale partial of a longer update, a row term at a stride taken from
    rows instead of max_rows, a workspace row past rows) becomes a NaN in its outputs."""
    from plantos_amd import A2CLearner, Policy
    towers, D, act, max_rows = NETS["n96_3x32"], 72, "tanh", 2 * CH + 5
    b = make_batch(D)
    tensors = make_tensors(towers, D, 41, "var")
    pol = Policy(b, towers, act).load(tensors)
    learner = A2CLearner(pol, max_rows=max_rows, **HYPER)
    state = (tensors, None)
    for step, rows in enumerate((2 * CH + 5, 70, CH + 1, 1, CH - 1, 2 * CH + 5)):
        for scratch in learner._work[:3]:  # (the two packed weight buffers are state, not scratch)
            scratch.fill_(float("nan"))
        twin = step_against_twin(learner, act, state, make_rows(b, towers, rows, seed=100 + step),
                                 ("codes", "f32")[step % 2], HYPER, f"update {step} of {rows} rows")
        assert np.isfinite(twin["flat_gradients"]).all() and twin["flat_gradients"].any()
        state = (twin["tensors"], twin["square_avg"])
    learner.close(), pol.close(), b.close()


@pytest.mark.parametrize("tile,form", [(32, "f32"), (64, "codes")])
def test_fewer_rows_than_max_rows_equal_the_twin(tile, form):
    """test_tiles_and_obs_forms_give_the_same_bits' shape (max_rows = rows + 40), against the twin."""
    from plantos_amd import A2CLearner, Policy
    towers, D, rows = NETS["n64x32"], 107, 210
    b = make_batch(D)
    tensors = make_tensors(towers, D, 5, "var")
    pol = Policy(b, towers, "tanh", env_tile=tile).load(tensors)
    learner = A2CLearner(pol, max_rows=rows + 40, **HYPER)
    state, data = (tensors, None), make_rows(b, towers, rows, seed=8)
    for step in range(3):
        twin = step_against_twin(learner, "tanh", state, data, form, HYPER, f"update {step}")
        state = (twin["tensors"], twin["square_avg"])
    learner.close(), pol.close(), b.close()


@pytest.mark.parametrize("name", sorted(HYPER_SETS))
def test_hyper_parameters_equal_the_twin(name):
    from plantos_amd import A2CLearner, Policy
    hyper = HYPER_SETS[name]
    towers, D, rows = NETS["n64x32"], 72, 70
    b = make_batch(D)
    tensors = make_tensors(towers, D, 13, "var")
    pol = Policy(b, towers, "tanh").load(tensors)
    learner = A2CLearner(pol, max_rows=rows, **hyper)
    assert learner.hyper == dict(L.DEFAULTS, **hyper)
    state, data = (tensors, None), make_rows(b, towers, rows, seed=14)
    for step in range(3):
        twin = step_against_twin(learner, "tanh", state, data, "codes", hyper, f"{name}: update {step}")
        state = (twin["tensors"], twin["square_avg"])
        if name == "vf0":  # the value tower: no gradient, parameters bit-unchanged, square_avg = alpha^k
            assert not flat([read(learner.gradients)[1]]).any()
            assert np.array_equal(flat([read(learner.parameters)[1]]), flat([tensors[1]]))
            want = np.float32(1.0)
            for _ in range(step + 1):
                want = np.float32(np.float32(0.99) * want)
            assert np.array_equal(flat([read(learner.square_avg)[1]]), np.full_like(flat([tensors[1]]), want))
            assert not np.array_equal(flat([read(learner.parameters)[0]]), flat([tensors[0]]))
    learner.close(), pol.close(), b.close()


def test_learning_rate_per_call_and_a_loaded_optimizer_state():
    from plantos_amd import A2CLearner, Policy
    towers, D, rows = NETS["n64x32"], 72, 70
    b = make_batch(D)
    tensors = make_tensors(towers, D, 13, "var")
    pol = Policy(b, towers, "relu").load(tensors)
    learner = A2CLearner(pol, max_rows=rows, **HYPER)
    state, data = (tensors, None), make_rows(b, towers, rows, seed=15)
    twins = []
    for step, lr in enumerate((3e-3, 0.0, 1e-4)):
        before = flat(state[0]).copy()
        sq_before = np.ones_like(before) if state[1] is None else flat(state[1])
        twin = step_against_twin(learner, "relu", state, data, "f32", HYPER, f"lr {lr}", learning_rate=lr)
        # at 0.0 no parameter moves, and square_avg still does
        assert np.array_equal(flat(read(learner.parameters)), before) == (lr == 0.0)
        assert not np.array_equal(flat(read(learner.square_avg)), sq_before)
        state = (twin["tensors"], twin["square_avg"])
        twins.append(twin)
    # ... and the constructor's rate is back without the keyword
    twin = step_against_twin(learner, "relu", state, data, "f32", HYPER, "the constructor's rate again")
    assert not np.array_equal(flat(twin["tensors"]), flat(twins[2]["tensors"]))
    # load(tensors, square_avg=..) with the state after two updates: the third update is the twin's third
    learner.load(twins[1]["tensors"], square_avg=twins[1]["square_avg"])
    torch.cuda.synchronize()
    assert int(np_(learner.n_updates)[0]) == 0
    assert np.array_equal(flat(read(learner.square_avg)), flat(twins[1]["square_avg"]))
    stats = learner.update(obs=dev(data[1]), actions=dev(data[2]), advantages=dev(data[3]), returns=dev(data[4]),
                           learning_rate=1e-4)
    check_against_twin(learner, stats, twins[2], "after load with square_avg")
    assert int(np_(stats["n_updates"])[0]) == 1
    # ... and load without one is a fresh optimizer
    learner.load(tensors)
    torch.cuda.synchronize()
    assert np.array_equal(flat(read(learner.square_avg)), np.ones_like(flat(tensors)))
    learner.close(), pol.close(), b.close()


def is_subnormal(x):
    return (x != 0) & (np.abs(x) < np.finfo(np.float32).tiny)


@pytest.mark.parametrize("act", ["relu", "tanh"])
def test_saturated_pi_head_equals_the_twin(act):
    """The pi head's weights times 30: logit gaps of order 100, probabilities that underflow.  The
    relu case carries subnormal non-zero gradients (asserted on the twin, so that a change of seed
    cannot empty the case): they pass through the MFMA's operands, the f32 divides and the fmaf
    chains on the device, which must keep them as the host does."""
    from plantos_amd import A2CLearner, Policy
    towers, D, rows = NETS["n64x32"], 72, 70
    b = make_batch(D)
    tensors = scale_pi_head(make_tensors(towers, D, 31, "var"), 30.0)
    pol = Policy(b, towers, act).load(tensors)
    learner = A2CLearner(pol, max_rows=rows, **HYPER)
    state, data = (tensors, None), make_rows(b, towers, rows, seed=rows)
    for step in range(3):
        twin = step_against_twin(learner, act, state, data, "codes", HYPER, f"update {step}")
        g = twin["flat_gradients"]
        assert np.isfinite(g).all() and g.any()
        if step == 0 and act == "relu":
            n_sub = int(is_subnormal(g).sum())
            print(f"subnormal non-zero gradients: {n_sub} of {g.size}")
            assert n_sub >= 1
        state = (twin["tensors"], twin["square_avg"])
    learner.close(), pol.close(), b.close()


def test_huge_returns_equal_the_twin():
    """Returns times 1e3: a value gradient of order 1e3, a clip coefficient of order 1e-4."""
    from plantos_amd import A2CLearner, Policy
    towers, D, rows = NETS["n64x32"], 72, 70
    b = make_batch(D)
    tensors = make_tensors(towers, D, 31, "var")
    pol = Policy(b, towers, "tanh").load(tensors)
    learner = A2CLearner(pol, max_rows=rows, **HYPER)
    codes, obs, a, adv, ret = make_rows(b, towers, rows, seed=rows)
    state, data = (tensors, None), (codes, obs, a, adv, (ret * np.float32(1e3)).astype(np.float32))
    for step in range(3):
        twin = step_against_twin(learner, "tanh", state, data, "f32", HYPER, f"update {step}")
        assert 0.0 < twin["clip_coef"] < 1e-3 and np.isfinite(twin["flat_gradients"]).all()
        state = (twin["tensors"], twin["square_avg"])
    learner.close(), pol.close(), b.close()


def test_zero_gradient_moves_nothing():
    """test_learner_host's exact case on the device: no advantage, no entropy bonus, no value loss."""
    from plantos_amd import A2CLearner, Policy
    towers, D, rows = NETS["n32"], 52, 70
    hyper = dict(learning_rate=7e-4, ent_coef=0.0, vf_coef=0.0)
    b = make_batch(D)
    tensors = make_tensors(towers, D, 9, "var")
    pol = Policy(b, towers, "tanh").load(tensors)
    learner = A2CLearner(pol, max_rows=rows, **hyper)
    codes, obs, a, adv, ret = make_rows(b, towers, rows, seed=9)
    twin = step_against_twin(learner, "tanh", (tensors, None), (codes, obs, a, 0 * adv, ret), "codes", hyper, "zero")
    assert not flat(read(learner.gradients)).any() and float(np_(learner.stats["grad_norm"])) == 0.0
    assert float(np_(learner.stats["clip_coef"])) == 1.0 == float(twin["clip_coef"])
    assert np.array_equal(flat(read(learner.parameters)), flat(tensors))
    assert np.array_equal(flat(read(learner.square_avg)), np.full_like(flat(tensors), np.float32(0.99)))
    learner.close(), pol.close(), b.close()


def test_dead_relu_layer_has_zero_gradients_below():
    """The pi tower's second hidden layer with every bias at -50: no row activates it, so its own
    gradient tensors and the first layer's are zero, and the head keeps its bias gradient only."""
    from plantos_amd import A2CLearner, Policy
    towers, D, rows = NETS["n64x32"], 72, 70
    b = make_batch(D)
    tensors = make_tensors(towers, D, 31, "var")
    tensors[0][1] = (tensors[0][1][0], np.full_like(tensors[0][1][1], -50.0))
    pol = Policy(b, towers, "relu").load(tensors)
    learner = A2CLearner(pol, max_rows=rows, **HYPER)
    state, data = (tensors, None), make_rows(b, towers, rows, seed=rows)
    for step in range(3):
        twin = step_against_twin(learner, "relu", state, data, "codes", HYPER, f"update {step}")
        for g in (twin["gradients"], read(learner.gradients)):
            assert not flat([g[0][:2]]).any() and not g[0][2][0].any() and g[0][2][1].any() and flat([g[1]]).any()
        state = (twin["tensors"], twin["square_avg"])
    learner.close(), pol.close(), b.close()


def test_train_on_a_batch_without_obs_codes():
    """train() through the minibatch's f32 observations (a batch created with obs_codes=False has
    no codes to give), with GAE(0.95) advantages, raw and then normalised.  The learner is built
    for more rows than the rollout holds."""
    from plantos_amd import A2CLearner, Policy, RolloutCollector, host_adv_norm
    towers, D, n, T = NETS["n64x32"], 57, 70, 5
    b = make_batch(D, n=n, max_steps=7, seed=4, obs_codes=False)
    tensors = make_tensors(towers, D, 21, "var")
    pol = Policy(b, towers, "tanh", seed=3).load(tensors)
    col = RolloutCollector(b, pol, T, gamma=0.99, gae_lambda=0.95)
    learner = A2CLearner(pol, max_rows=T * n + 40, **HYPER)
    sq = None
    for it, normalize in enumerate((False, True)):
        ro = col.collect()
        torch.cuda.synchronize()
        raw_adv = np_(ro.advantages).reshape(-1)
        stats = learner.train(ro, normalize_advantage=normalize)
        torch.cuda.synchronize()
        mb = learner.last_minibatch
        assert mb.codes is None and mb.count == T * n
        idx = np_(mb.indices)
        assert np.array_equal(np_(mb.advantages), host_adv_norm(raw_adv[idx]) if normalize else raw_adv[idx])
        assert np.array_equal(np_(mb.observations), np_(ro.obs_f32())[idx])
        twin = L.host_update(towers, tensors, "tanh", np_(mb.observations), np_(mb.actions), np_(mb.advantages),
                             np_(mb.returns), square_avg=sq, **HYPER)
        check_against_twin(learner, stats, twin, f"iteration {it}")
        tensors, sq = twin["tensors"], twin["square_avg"]
    learner.close(), pol.close(), b.close()
