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

- SATURATED pi head (the head's weights times 10, 30, 100, 300; 70 to 257 rows; three draws of
  each of four nets and both activations): logit gaps of tens to thousands, probabilities down to
  the smallest the definition can produce.  Gradients: measured worst SAT_MEASURED, inside the MANY
  bound but kept apart.  policy_loss, value_loss and loss stay under the MANY bound (measured worst
  1.13).  entropy_loss has a bound of its own, twice SAT_ENTROPY_MEASURED: the head multiplies the
  rounding of the forward's f32 logits (one fmaf chain per neuron, the definition's; torch's f32
  forward sums in blocks and lands closer) by its scale, log p moves by that much, and H of a
  saturated row is a few p log p terms with no cancellation to hide it.  Read off by recomputing H
  in float64 from the twin's own f32 logits: that alone reproduces the twin's error to within one
  floor in every case looked at (94.6 of 93.6 floors at the worst ratio, 1145 of 1154 at the worst
  error), while rounding S = 1 + eps to f32 before its logarithm (pe_logf is accurate to an ulp of
  S, not of log S) accounts for under one floor at x10 .. x100 and 9 of 1154 floors at x300.
  In this class the entropy's floor has a second term: pe_expf clamps its argument at -87
  (pe_policy_math.hpp), so no p_k is below e^-87 = 1.6e-38 where float64 goes on to e^-190 and
  beyond, and a row's H keeps up to (A - 1) e^-87 times the largest logit gap of the case.  That
  share, about 1e-34, is added to the floor; without it the case whose float64 entropy is 4.8e-86
  (twin -1.2e-34, torch float32 -0) would measure 2.5e51 "floors" of nothing.
"""
import numpy as np
import pytest
import torch

import plantos_amd.learner as L
from learner_util import HYPER_SETS, NETS, flat, minibatch, np_clip_rmsprop, torch_a2c
from plantos_amd.policy import host_forward
from plantos_amd.rollout import NORM_CHUNK, host_record

CHUNK = L.GRAD_CHUNK
ULP = 2.0 ** -23
MANY_MEASURED = 6.82       # gradients, 70 rows and more ([[96,2],[32,32,32,1]], relu, D = 107, 257 rows)
ONE_MEASURED = 18.4        # gradients, one row ([[256,256,5],[256,256,1]], tanh, D = 107)
LOSS_MANY_MEASURED = 1.0   # loss scalars, 70 rows and more: every error within the one-ulp floor
LOSS_ONE_MEASURED = 37.0   # loss scalars, one row (the same case as ONE_MEASURED: value_loss from one v)
# optimizer: worst |twin - float64| / max(|float64|, 1e-3) over three updates (HYPER_SETS' "moved": lr 1e-2, alpha 0.9;
# 8.1e-8 under the loop's hyper-parameters)
OPT_MEASURED = 1.06e-7
OPT_BOUND = 2 * OPT_MEASURED
SAT_MEASURED = 5.59           # gradients, saturated pi head ([[256,256,5],[256,256,1]], relu, D = 107, 70 rows, x10, draw 1)
SAT_ENTROPY_MEASURED = 14.17  # entropy_loss, saturated pi head ([[64,32,8],[32,64,1]], tanh, D = 72, 70 rows, x100, draw 2)

GRAD_NETS = ("n32", "n64x32", "n96_3x32", "a2c")
ENT, VF = 0.01, 0.5
_cache = {}


def case(net, act, D, rows, head_scale=None, draw=0):
    """The twin's and both autograd results of one case, computed once.  head_scale: the pi head's
    weights times that (learner_util.scale_pi_head); draw: a further seeded draw of the same case."""
    key = (net, act, D, rows, head_scale, draw)
    if key not in _cache:
        towers = NETS[net]
        seed = 1 + sum(ord(c) for c in net + act) + 7 * D + rows + 1009 * draw
        tensors, obs, a, adv, ret = minibatch(towers, D, rows, seed=seed, head_scale=head_scale)
        twin = L.host_update(towers, tensors, act, obs, a, adv, ret, apply=False, ent_coef=ENT, vf_coef=VF)
        s64, g64, scales = torch_a2c(tensors, act, obs, a, adv, ret, ENT, VF, torch.float64)
        s32, g32, _ = torch_a2c(tensors, act, obs, a, adv, ret, ENT, VF, torch.float32)
        clamp = 0.0
        if head_scale is not None:  # see the SATURATED class in the module's docstring
            logits = host_forward(towers, tensors, act, obs)[1].astype(np.float64)
            clamp = (towers[0][-1] - 1) * np.exp(-87.0) * float((logits.max(axis=1) - logits.min(axis=1)).max())
        _cache[key] = (twin, s64, g64, s32, g32, scales, clamp)
    return _cache[key]


CASES = [(net, act, D, rows) for net in GRAD_NETS for act in ("tanh", "relu") for D in (52, 107)
         for rows in (1, 70, 210, CHUNK + 1)]
# More of the MANY class, under its bounds as they are: the obs lengths whose residues the device's
# layer-0 weight gradient meets (57, 87, 127, 347), more rows than kNormChunk (4097, 8195: the f64
# row-term sums and the parameter gradients over 17 and 33 chunks), and the 512-wide net.
CASES += [(net, act, D, 70) for D in (57, 87, 127, 347) for net in ("n32", "n64x32") for act in ("tanh", "relu")]
CASES += [(net, act, D, rows) for net, D, rows in (("n32", 52, NORM_CHUNK + 1), ("n64x32", 72, NORM_CHUNK + 1),
                                                   ("n64x32", 52, 2 * NORM_CHUNK + 3)) for act in ("tanh", "relu")]
CASES += [("w512", act, D, rows) for D, rows in ((72, 70), (107, CHUNK + 1)) for act in ("tanh", "relu")]


def gradient_ratio(c):
    """The worst (twin error) / (torch float32 error) over the parameter tensors of case() c."""
    twin, _, g64, _, g32, _, _ = c
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
    return worst


def loss_ratios(c):
    """{scalar: (twin error) / (torch float32 error)}, both floored at one ulp of the mean absolute
    row term (the saturated class: plus the exp clamp's share of the entropy), of case() c."""
    twin, s64, _, s32, _, scales, clamp = c
    out = {}
    for name, ref, f32, scale in zip(("policy_loss", "value_loss", "entropy_loss", "loss"), s64, s32, scales):
        floor = ULP * scale + {"entropy_loss": clamp, "loss": ENT * clamp}.get(name, 0.0)
        out[name] = max(abs(float(twin[name]) - ref), floor) / max(abs(f32 - ref), floor)
    return out


@pytest.mark.parametrize("net,act,D,rows", CASES)
def test_twin_gradients_against_float64_autograd(net, act, D, rows):
    worst = gradient_ratio(case(net, act, D, rows))
    print(f"gradient ratio {net} {act} D={D} rows={rows}: {worst:.3f}")
    assert worst <= 2 * (ONE_MEASURED if rows == 1 else MANY_MEASURED)


@pytest.mark.parametrize("net,act,D,rows", CASES)
def test_twin_losses_against_float64(net, act, D, rows):
    worst = max(loss_ratios(case(net, act, D, rows)).values())
    print(f"loss ratio {net} {act} D={D} rows={rows}: {worst:.3f}")
    assert worst <= 2 * (LOSS_ONE_MEASURED if rows == 1 else LOSS_MANY_MEASURED)


# the saturated class: (net, D, rows) of the sweep, the pi head's weights times each scale, three draws
SAT_SHAPES = (("n64x32", 72, 70), ("n32", 52, CHUNK + 1), ("n96_3x32", 107, 210), ("a2c", 107, 70))
SAT_CASES = [(net, act, D, rows, scale, draw) for net, D, rows in SAT_SHAPES for act in ("tanh", "relu")
             for scale in (10.0, 30.0, 100.0, 300.0) for draw in range(3)]


@pytest.mark.parametrize("net,act,D,rows,scale,draw", SAT_CASES)
def test_saturated_gradients_against_float64_autograd(net, act, D, rows, scale, draw):
    worst = gradient_ratio(case(net, act, D, rows, scale, draw))
    print(f"saturated gradient ratio {net} {act} D={D} rows={rows} x{scale:g} draw {draw}: {worst:.3f}")
    assert worst <= 2 * SAT_MEASURED


@pytest.mark.parametrize("net,act,D,rows,scale,draw", SAT_CASES)
def test_saturated_losses_against_float64(net, act, D, rows, scale, draw):
    r = loss_ratios(case(net, act, D, rows, scale, draw))
    print(f"saturated loss ratios {net} {act} D={D} rows={rows} x{scale:g} draw {draw}: "
          + " ".join(f"{k} {v:.3f}" for k, v in r.items()))
    assert r["entropy_loss"] <= 2 * SAT_ENTROPY_MEASURED
    assert max(r["policy_loss"], r["value_loss"], r["loss"]) <= 2 * LOSS_MANY_MEASURED


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


@pytest.mark.parametrize("name", sorted(HYPER_SETS))
def test_optimizer_and_clip_against_float64_other_hyper_parameters(name):
    """The same comparison under learner_util.HYPER_SETS (the sets the device runs in
    test_gpu_learner): the defaults without an entropy bonus, no value loss, and lr 1e-2 / clip at
    0.1 / alpha 0.9 / eps 1e-8."""
    towers = NETS["n64x32"]
    tensors, obs, a, adv, ret = minibatch(towers, 52, 70, seed=5)
    hyper = dict(L.DEFAULTS, **HYPER_SETS[name])
    sq, worst = None, 0.0
    for step in range(3):
        r = L.host_update(towers, tensors, "tanh", obs, a, adv, ret, square_avg=sq, **hyper)
        p0 = flat(tensors)
        s0 = np.ones_like(p0) if sq is None else flat(sq)
        p64, s64, norm, coef = np_clip_rmsprop(p0, s0, r["flat_gradients"], hyper["learning_rate"], hyper["max_grad_norm"],
                                               hyper["alpha"], hyper["rms_prop_eps"])
        assert coef < 1.0
        for got, ref in ((flat(r["tensors"]), p64), (flat(r["square_avg"]), s64),
                         (np.array([r["grad_norm"], r["clip_coef"]]), np.array([norm, coef]))):
            worst = max(worst, float((np.abs(got - ref) / np.maximum(np.abs(ref), 1e-3)).max()))
        tensors, sq = r["tensors"], r["square_avg"]
    print(f"optimizer error {name}: {worst:.3e}")
    assert worst <= OPT_BOUND


def np_chunk_sum(terms):
    """pe_learner_host.cpp's chunk_sum restated: per chunk of NORM_CHUNK elements, lane q % 256 adds
    its elements in ascending order in f64, the 256 lanes are folded as a tree (l += l + h, h = 128
    .. 1), and the chunk sums are added in ascending order."""
    t = np.asarray(terms, np.float64)
    total = np.float64(0.0)
    for base in range(0, len(t), NORM_CHUNK):
        s = np.zeros(256, np.float64)
        for q, v in enumerate(t[base:base + NORM_CHUNK]):
            s[q % 256] += v
        h = 128
        while h >= 1:
            for l in range(h):
                s[l] += s[l + h]
            h //= 2
        total += s[0]
    return total


def test_loss_sums_follow_the_chunk_order():
    """A case whose loss scalars depend on the association of the f64 row-term sums, so that the
    definition's order is guarded and not only its accuracy.  4097 rows (two chunks, the second of
    one row).  Rows 0 and 1 are the same obs and action with advantages +-2^62, so that t_pol[0] =
    -t_pol[1] exactly, of magnitude about 2^62: in the definition's order they sit in lanes 0 and 1,
    each lane absorbs what it adds later, lane 0 absorbs every lane the tree folds into it before it
    meets lane 1, and the chunk's sum keeps almost nothing of its 4094 other terms; a row-order sum
    or an exact sum keeps them all.  The returns span 2^-2 .. 2^30, t_val = (ret - v)^2 about 2^60:
    those terms are all positive, an association moves their f64 sum by at most 4097 * 2^-53 of it
    and the f32 cannot show that, so value_loss guards the restated sum and its accuracy only.  The
    row terms are restated from the forward's outputs: logp by the rollout's record step
    (policy_logprob, which learner_row's logp is), t_val = (ret - v)^2 in f32."""
    import math
    towers, D, B = NETS["n32"], 52, NORM_CHUNK + 1
    tensors, obs, a, adv, ret = minibatch(towers, D, B, seed=77)
    rng = np.random.default_rng(78)
    obs[1], a[1] = obs[0], a[0]
    adv[0], adv[1] = np.float32(2.0 ** 62), np.float32(-2.0 ** 62)
    ret = (np.sign(ret) * np.exp2(rng.uniform(-2.0, 30.0, B))).astype(np.float32)
    ret[5] = np.float32(2.0 ** 30)
    twin = L.host_update(towers, tensors, "tanh", obs, a, adv, ret, apply=False, ent_coef=ENT, vf_coef=VF)
    _, logits, values = host_forward(towers, tensors, "tanh", obs)
    zeros = np.zeros(B, np.float32)
    logp = host_record(logits, a, zeros, zeros, zeros, 0.99)[0]
    t_pol = adv * logp                                   # f32 products
    d = ret - values.reshape(-1).astype(np.float32)
    t_val = d * d
    assert t_pol.dtype == t_val.dtype == np.float32 and t_pol[0] == -t_pol[1] and abs(t_pol[0]) > 2.0 ** 60
    assert t_val.max() / t_val[t_val > 0].min() > 2.0 ** 55
    n = np.float64(B)
    want_pol, want_val = np.float32(-(np_chunk_sum(t_pol) / n)), np.float32(np_chunk_sum(t_val) / n)
    print(f"policy_loss {twin['policy_loss']!r} (chunk order {want_pol!r}, row order "
          f"{np.float32(-(sum(map(float, t_pol)) / n))!r}, exact {np.float32(-(math.fsum(map(float, t_pol)) / n))!r}); "
          f"value_loss {twin['value_loss']!r} ({want_val!r})")
    assert twin["policy_loss"] == want_pol and twin["value_loss"] == want_val
    e = np.float32(np.float32(ENT) * twin["entropy_loss"])
    assert twin["loss"] == np.float32(np.float32(want_pol + e) + np.float32(np.float32(VF) * want_val))
    # the case discriminates: other associations of the same terms give another f32
    row_order = np.float64(0.0)
    for v in t_pol:
        row_order += np.float64(v)
    lanes_of_64 = sum(np.float64(t_pol[l::64].astype(np.float64).sum()) for l in range(64))
    for other in (row_order, math.fsum(map(float, t_pol)), lanes_of_64, np_chunk_sum(t_pol[::-1])):
        assert np.float32(-(other / n)) != want_pol


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
