"""Host checks of the A2C learner's definition (csrc/pe_learner_math.hpp) through its twin
(plantos_amd.learner.host_update), no device: the gradients and loss scalars against float64
autograd of A2C.train's loss restated in torch, measured beside torch's own float32 autograd; the
clip and the RMSpropTFLike step against a float64 numpy restatement over three updates; exact
special cases; the device-free plan against arithmetic restated here; the refusals; descent.

How the comparison is made (the figures are recorded in DESIGN section 4 "A2C learner").  Per
parameter tensor, the ratio (twin error) / (torch float32 error), both against float64 and
normalised by the tensor's max-abs gradient, with both errors floored at one float32 ulp of that
maximum, 2^-23 (below it an error is the rounding of the gradient itself).  The cases fall into two
classes with a bound each, twice the worst ratio measured in the class:

- MANY rows (70, 210, kGradChunk + 1): a tensor's error is a maximum over many draws, and this is
  the class that guards the chunk chains, the f64 combine and the bias sums.  Measured worst
  MANY_MEASURED.
- ONE row: every error is a single draw and the ratio of two single draws has a heavy tail; the
  value tower's relative gradient error is err(v) / |v - ret| of one forward chain over the last
  hidden layer (pe_policy_forward_host's, which the learner must reproduce), the same on every
  tensor of the tower.  Measured worst ONE_MEASURED, documented apart so that it does not widen
  the bound of the other class.

The loss scalars are means that can cancel (policy_loss = -mean(adv logp) reaches -0.028 from
terms of order 1), so their errors are floored at one ulp of the mean ABSOLUTE row term
(learner_util.torch_a2c's scales), not of the mean, and bounded in the same two classes: with 70
rows and more every error of the twin and of torch float32 lies within that floor
(LOSS_MANY_MEASURED = 1.0); at one row the mean is the single term, value_loss = (ret - v)^2
carries the single v draw above, and the worst is LOSS_ONE_MEASURED.
"""
import numpy as np
import pytest
import torch

import plantos_amd.learner as L
from learner_util import NETS, flat, minibatch, np_clip_rmsprop, torch_a2c

CHUNK = L.GRAD_CHUNK
ULP = 2.0 ** -23
MANY_MEASURED = 6.82       # gradients, 70 rows and more ([[96,2],[32,32,32,1]], relu, D = 107, 257 rows)
ONE_MEASURED = 18.4        # gradients, one row ([[256,256,5],[256,256,1]], tanh, D = 107)
LOSS_MANY_MEASURED = 1.0   # loss scalars, 70 rows and more: every error within the one-ulp floor
LOSS_ONE_MEASURED = 37.0   # loss scalars, one row (the same case as ONE_MEASURED: value_loss from one v)
OPT_MEASURED = 8.1e-8  # optimizer: worst |twin - float64| / max(|float64|, 1e-3) over three updates
OPT_BOUND = 2 * OPT_MEASURED

GRAD_NETS = ("n32", "n64x32", "n96_3x32", "a2c")
ENT, VF = 0.01, 0.5
_cache = {}


def case(net, act, D, rows):
    """The twin's and both autograd results of one case, computed once."""
    key = (net, act, D, rows)
    if key not in _cache:
        towers = NETS[net]
        tensors, obs, a, adv, ret = minibatch(towers, D, rows, seed=1 + sum(ord(c) for c in net + act) + 7 * D + rows)
        twin = L.host_update(towers, tensors, act, obs, a, adv, ret, apply=False, ent_coef=ENT, vf_coef=VF)
        s64, g64, scales = torch_a2c(tensors, act, obs, a, adv, ret, ENT, VF, torch.float64)
        s32, g32, _ = torch_a2c(tensors, act, obs, a, adv, ret, ENT, VF, torch.float32)
        _cache[key] = (twin, s64, g64, s32, g32, scales)
    return _cache[key]


CASES = [(net, act, D, rows) for net in GRAD_NETS for act in ("tanh", "relu") for D in (52, 107)
         for rows in (1, 70, 210, CHUNK + 1)]


@pytest.mark.parametrize("net,act,D,rows", CASES)
def test_twin_gradients_against_float64_autograd(net, act, D, rows):
    twin, _, g64, _, g32, _ = case(net, act, D, rows)
    worst = 0.0
    for i, tw in enumerate(g64):
        for l, pair in enumerate(tw):
            for q, ref in enumerate(pair):
                m = np.abs(ref).max()
                if m == 0.0:  # e.g. a relu layer dead on every row: both must be zero too
                    assert not twin["gradients"][i][l][q].any()
                    continue
                e_twin = np.abs(twin["gradients"][i][l][q] - ref).max() / m
                e_f32 = np.abs(g32[i][l][q] - ref).max() / m
                worst = max(worst, max(e_twin, ULP) / max(e_f32, ULP))
    print(f"gradient ratio {net} {act} D={D} rows={rows}: {worst:.3f}")
    assert worst <= 2 * (ONE_MEASURED if rows == 1 else MANY_MEASURED)


@pytest.mark.parametrize("net,act,D,rows", CASES)
def test_twin_losses_against_float64(net, act, D, rows):
    twin, s64, _, s32, _, scales = case(net, act, D, rows)
    worst = 0.0
    for name, ref, f32, scale in zip(("policy_loss", "value_loss", "entropy_loss", "loss"), s64, s32, scales):
        floor = ULP * scale
        worst = max(worst, max(abs(float(twin[name]) - ref), floor) / max(abs(f32 - ref), floor))
    print(f"loss ratio {net} {act} D={D} rows={rows}: {worst:.3f}")
    assert worst <= 2 * (LOSS_ONE_MEASURED if rows == 1 else LOSS_MANY_MEASURED)


def test_twin_norm_is_the_gradients_norm():
    twin = case("n64x32", "tanh", 52, 70)[0]
    g = twin["flat_gradients"].astype(np.float64)
    assert abs(float(twin["grad_norm"]) - np.sqrt(np.sum(g * g))) <= 2e-7 * float(twin["grad_norm"])


@pytest.mark.parametrize("max_grad_norm", [0.5, 1e6])
def test_optimizer_and_clip_against_float64(max_grad_norm):
    towers = NETS["n64x32"]
    tensors, obs, a, adv, ret = minibatch(towers, 52, 70, seed=5)
    hyper = dict(learning_rate=7e-4, ent_coef=ENT, vf_coef=VF, max_grad_norm=max_grad_norm, alpha=0.99, rms_prop_eps=1e-5)
    sq, worst = None, 0.0
    for step in range(3):
        r = L.host_update(towers, tensors, "tanh", obs, a, adv, ret, square_avg=sq, **hyper)
        p0 = flat(tensors)
        s0 = np.ones_like(p0) if sq is None else flat(sq)
        p64, s64, norm, coef = np_clip_rmsprop(p0, s0, r["flat_gradients"], 7e-4, max_grad_norm, 0.99, 1e-5)
        assert (coef < 1.0) == (max_grad_norm == 0.5)
        for got, ref in ((flat(r["tensors"]), p64), (flat(r["square_avg"]), s64),
                         (np.array([r["grad_norm"], r["clip_coef"]]), np.array([norm, coef]))):
            worst = max(worst, float((np.abs(got - ref) / np.maximum(np.abs(ref), 1e-3)).max()))
        tensors, sq = r["tensors"], r["square_avg"]
    print(f"optimizer error max_grad_norm={max_grad_norm}: {worst:.3e}")
    assert worst <= OPT_BOUND


def test_exact_cases():
    towers = NETS["n32"]
    tensors, obs, a, adv, ret = minibatch(towers, 52, 70, seed=9)
    # a zero gradient: no advantage, no entropy bonus, no value loss -> coef == 1, nothing moves
    r = L.host_update(towers, tensors, "tanh", obs, a, 0 * adv, ret, ent_coef=0.0, vf_coef=0.0)
    assert not r["flat_gradients"].any() and r["grad_norm"] == 0.0 and r["clip_coef"] == 1.0
    assert np.array_equal(flat(r["tensors"]), flat(tensors))
    assert np.array_equal(flat(r["square_avg"]), np.full_like(flat(tensors), np.float32(0.99) * np.float32(1.0)))
    # square_avg after one update from ones: fmaf(1 - alpha, (g coef)^2, alpha) in f32
    r = L.host_update(towers, tensors, "tanh", obs, a, adv, ret, ent_coef=ENT)
    gc = r["flat_gradients"] * r["clip_coef"]
    want = (np.float64(np.float32(1.0 - 0.99)) * (gc * gc).astype(np.float64) + np.float64(np.float32(0.99))).astype(np.float32)
    assert np.array_equal(flat(r["square_avg"]), want)
    # ent_coef = 0: the policy tower's gradient is the policy loss's alone, the loss has no entropy term
    r0 = L.host_update(towers, tensors, "tanh", obs, a, adv, ret, ent_coef=0.0, apply=False)
    assert r0["loss"] == np.float32(r0["policy_loss"] + np.float32(0.5) * r0["value_loss"])
    assert r0["entropy_loss"] == r["entropy_loss"]
    # vf_coef = 0: the value tower gets no gradient at all
    rv = L.host_update(towers, tensors, "tanh", obs, a, adv, ret, vf_coef=0.0, apply=False)
    assert not flat([rv["gradients"][1]]).any() and flat([rv["gradients"][0]]).any()
    assert np.array_equal(flat([rv["gradients"][0]]), flat([r0["gradients"][0]]))
    # all advantages zero: only the entropy gradient remains in the policy tower
    re_ = L.host_update(towers, tensors, "tanh", obs, a, 0 * adv, ret, ent_coef=ENT, vf_coef=0.0, apply=False)
    _, g64, _ = torch_a2c(tensors, "tanh", obs, a, 0 * adv, ret, ENT, 0.0, torch.float64)
    assert re_["policy_loss"] == 0.0 and flat([re_["gradients"][0]]).any()
    ref = flat([g64[0]])
    assert np.abs(flat([re_["gradients"][0]]) - ref).max() <= 1e-5 * np.abs(ref).max()


@pytest.mark.parametrize("net,D,rows,cus", [("a2c", 107, 327680, 256), ("n96_3x32", 52, 70, 256),
                                            ("w512", 72, 2 * CHUNK + 5, 64), ("n64x32", 107, 16384, 256)])
def test_plan_arithmetic(net, D, rows, cus):
    from plantos_amd import _capi as C
    from plantos_amd.policy import _tower_structs
    towers = NETS[net]
    info = L.learner_plan(D, rows, cus, towers)
    pol = C.policy_plan(D, rows, cus, None, _tower_structs(towers), C.PE_ACT_TANH)
    P = sum(w * k + w for t in towers for w, k in zip(t, [D] + t[:-1]))
    hidden = sum(w for t in towers for w in t[:-1])
    A = towers[0][-1]
    groups = sum(-(-(-(-w // 32)) // 2) * -(-(-(-(k + 1) // 32)) // 4) for t in towers for w, k in zip(t, [D] + t[:-1]))
    assert L.param_layout(towers, D)[1] == P == info.n_params
    assert info.env_tile == pol.env_tile and info.lds_bytes == pol.lds_bytes and info.packed_floats == pol.packed_floats
    assert info.grad_chunk == CHUNK <= 4096 and info.max_chunks == -(-rows // CHUNK)
    assert info.ws_floats == rows * (D + 2 * hidden + A + 1 + 3)
    assert info.partial_floats == info.max_chunks * P
    assert info.n_layers == sum(len(t) for t in towers) and info.wgrad_groups == groups
    assert info.sum_chunks == -(-max(rows, P) // 4096) and info.sums_doubles == 4 * info.sum_chunks
    assert info.packed_t_floats == max(4, sum(w * k for t in towers for w, k in list(zip(t, [D] + t[:-1]))[1:-1]))
    # the launch decisions change speed, never the definition: the chunk does not move with CUs or tiles
    assert L.learner_plan(D, rows, 8, towers, env_tile=32).grad_chunk == CHUNK


def test_refusals():
    with pytest.raises(ValueError, match="two-tower"):
        L.check_learner_policy([[64, 64, 5]])
    with pytest.raises(ValueError, match="two-tower"):
        L.learner_plan(107, 64, 256, [[64, 64, 5]])
    with pytest.raises(ValueError, match="bf16"):
        L.check_learner_policy(NETS["a2c"], precision="bf16")
    with pytest.raises(ValueError, match="RecurrentPolicy"):
        L.check_learner_policy(NETS["a2c"], recurrent=True)
    with pytest.raises(ValueError, match="max_rows"):
        L.check_rows(71, 70)
    with pytest.raises(ValueError, match="max_rows"):
        L.learner_plan(107, 0, 256, NETS["a2c"])
    assert L.learner_plan(107, 65535 * CHUNK, 256, NETS["n32"]).max_chunks == 65535
    with pytest.raises(ValueError, match="max_rows"):  # more chunks than a grid's y dimension holds
        L.learner_plan(107, 65535 * CHUNK + 1, 256, NETS["n32"])
    assert L.check_rows(70, 70) == 70
    with pytest.raises(ValueError, match="two-tower"):
        t, obs, a, adv, ret = minibatch(NETS["n32"], 52, 3, seed=1)
        L.host_update([[32, 5]], t[:1], "tanh", obs, a, adv, ret)
    with pytest.raises(ValueError, match="LDS"):
        L.learner_plan(107, 64, 256, NETS["w512"], env_tile=64)


def test_state_dict_names():
    t = minibatch(NETS["n64x32"], 52, 1, seed=1)[0]
    from plantos_amd.policy import parse_state_dict
    sd = {k: torch.as_tensor(v) for k, v in L.sb3_state_dict(t).items()}
    towers, act, back = parse_state_dict(sd)
    assert towers == NETS["n64x32"] and act == "tanh"
    assert np.array_equal(flat([[(w.numpy(), b.numpy()) for w, b in tw] for tw in back]), flat(t))


def test_ten_updates_descend():
    towers = NETS["n64x32"]
    tensors, obs, a, adv, ret = minibatch(towers, 107, 210, seed=3)
    sq, losses = None, []
    for _ in range(10):
        r = L.host_update(towers, tensors, "tanh", obs, a, adv, ret, square_avg=sq, ent_coef=ENT)
        losses.append(float(r["loss"]))
        tensors, sq = r["tensors"], r["square_avg"]
    losses.append(float(L.host_update(towers, tensors, "tanh", obs, a, adv, ret, apply=False, ent_coef=ENT)["loss"]))
    print("losses:", losses)
    assert losses[-1] < losses[0] and all(b < a_ for a_, b in zip(losses, losses[1:]))
