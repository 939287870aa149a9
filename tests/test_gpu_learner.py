"""GPU checks of the A2C learner (plantos_amd.A2CLearner; csrc/pe_learner.hip): gradients, loss
scalars, the gradient norm, parameters and square_avg equal the host twin bit for bit after each of
three updates, at the smallest shapes at which each path can go wrong -- below one tile, ragged
tiles, the edges of a gradient chunk (kGradChunk), more than two chunks; one, two and three hidden
layers (the third reads a layer's activations back from the workspace), the 512-wide net that only
fits 32-row tiles, 2 / 5 / 8 actions, both activations, three obs lengths, obs as codes and as f32,
a clip that binds and one that does not, both env_tiles; the hand-off to the policy; the collect /
train loop; graph capture.
"""
import numpy as np
import pytest
import torch

import plantos_amd.learner as L
from learner_util import NETS, flat
from policy_util import geometry_codes, make_tensors

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CH = L.GRAD_CHUNK
GEO = {52: (8, 3, 3, 4, 5), 72: (10, 4, 4, 5, 9), 107: (20, 10, 12, 6, 16)}  # policy_geometries' e52, e72; g20
HYPER = dict(learning_rate=7e-4, ent_coef=0.01, vf_coef=0.5)


def np_(t):
    return t.detach().cpu().numpy()


def dev(x):
    return torch.as_tensor(x, device=DEV)


def make_batch(D, n=64, **kw):
    from plantos_amd import PlantOSBatch
    G, P, Ob, R, C = GEO[D]
    b = PlantOSBatch(n, grid_size=G, num_plants=P, num_obstacles=Ob, lidar_range=R, lidar_channels=C, device=DEV,
                     obs_codes=True, **kw)
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
    learner.close(), pol.close(), b.close()


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
