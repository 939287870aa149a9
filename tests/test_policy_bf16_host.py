"""bf16 policy inference without a GPU (include/plantos_batch.h, "Reduced-precision policy
inference"): the plan for a precision, the host twin's accuracy against torch's own bf16
modules, and the proof that the lattice generator of the GPU "exact" cases is exact.
"""
import json
import os

import numpy as np
import pytest

import policy_bf16_util as BU
from plantos_amd import _capi as C
from plantos_amd import policy as P
from policy_util import a2c_state_dict, dqn_state_dict, obs_rows

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(REPO, "tests", "golden", "policy_plan_parent.json")) as _f:
    GOLDEN = json.load(_f)   # the sweep of tools/gen_golden_policy_plan.py, with obs_dim and n per case
CUS = GOLDEN["cu_count"]
MAX_LDS = 160 * 1024


def structs(case):
    """(lstms, shapes) of a sweep case, without the Python-side checks: the library's own answer"""
    towers = [[int(v) for v in t] for t in case["towers"]]
    lstms = P._lstm_structs(case["hidden"], len(towers)) if case["hidden"] is not None else None
    return lstms, P._tower_structs(towers)


def outcome(fn):
    try:
        info = fn()
    except ValueError as e:
        return ("error", str(e).split(": ", 1)[1])
    return ("ok", info.env_tile, info.lds_bytes, info.packed_floats, info.state_floats)


def activation_id(case):
    return P.ACTIVATIONS.get(case["activation"], 7)


# ---------------------------------------------------------------- 1: symbols and plan
def test_new_symbols_are_bound():
    L = C.lib()
    for name in ("pe_policy_create_prec", "pe_policy_precision", "pe_policy_forward_host_bf16"):
        assert name in C.EXPORTS and hasattr(L, name)
    assert (C.PE_PREC_F32, C.PE_PREC_BF16) == (0, 1)
    assert L.pe_policy_precision(None) == -1


def test_f32_plan_for_a_precision_is_the_plan():
    for c in GOLDEN["cases"]:
        lstms, shapes = structs(c)
        args = (c["obs_dim"], c["n"], CUS, lstms, shapes, activation_id(c), c["env_tile"])
        assert outcome(lambda: C.policy_plan(*args, precision=C.PE_PREC_F32)) == outcome(lambda: C.policy_plan(*args)), c


def bf16_plan(D, n, cus, towers, env_tile):
    """The bf16 plan restated: ("ok", tile, lds bytes, packed floats) or ("error",)."""
    packed, hmax = 0, 0
    for t in towers:
        k = D
        for i, w in enumerate(t):
            if i == len(t) - 1:
                packed += (w * k + 3) // 4 * 4              # head weights f32
            else:
                packed += w * ((k + 15) // 16 * 16) // 2    # bf16, K padded to 16: two per float
                hmax = max(hmax, w)
            packed += (w + 3) // 4 * 4                      # bias f32
            k = w
    kp0 = (D + 15) // 16 * 16
    lds = lambda E: 4 * (256 + 9 * E) + 2 * E * (kp0 + 2 * hmax)  # noqa: E731  table, head rows, x and two images
    if env_tile == 0:
        env_tile = 64 if lds(64) <= MAX_LDS and n >= 64 * max(cus, 1) else 32
    if lds(env_tile) > MAX_LDS:
        return ("error",)
    return ("ok", env_tile, lds(env_tile), packed)


def test_bf16_plan_equals_the_documented_layout():
    seen = {"ok": 0, "error": 0, 32: 0, 64: 0}
    for c in GOLDEN["cases"]:
        lstms, shapes = structs(c)
        args = (c["obs_dim"], c["n"], CUS, lstms, shapes, activation_id(c), c["env_tile"])
        got = outcome(lambda: C.policy_plan(*args, precision=C.PE_PREC_BF16))
        if lstms is not None:
            assert got == ("error", "a recurrent policy has no reduced precision"), c
            continue
        f32 = outcome(lambda: C.policy_plan(*args))
        shape_error = f32[0] == "error" and "LDS" not in f32[1]
        if shape_error:   # the argument checks are the f32 plan's, with its messages
            assert got == f32, c
            continue
        want = bf16_plan(c["obs_dim"], c["n"], CUS, c["towers"], c["env_tile"])
        if want[0] == "error":
            assert got[0] == "error" and "bf16 obs and activation images do not fit 160 KiB of LDS" in got[1], c
        else:
            assert got == want + (0,), c
            assert got[2] <= MAX_LDS
            seen[got[1]] += 1
        seen[want[0]] += 1
    assert seen["ok"] and seen["error"] and seen[32] and seen[64], seen
    # the automatic rule flips at 64 CUs envs, and a 512-wide net gets 64 envs at D = 107
    t = P._tower_structs([[512, 512, 256, 5]])
    assert C.policy_plan(107, 64 * CUS - 1, CUS, None, t, C.PE_ACT_RELU, 0, precision=C.PE_PREC_BF16).env_tile == 32
    assert C.policy_plan(107, 64 * CUS, CUS, None, t, C.PE_ACT_RELU, 0, precision=C.PE_PREC_BF16).env_tile == 64


def test_unknown_precision_is_refused():
    t = P._tower_structs([[32, 5]])
    for bad in (-1, 2, 7):
        with pytest.raises(ValueError, match="precision must be PE_PREC_F32 or PE_PREC_BF16"):
            C.policy_plan(107, 64, CUS, None, t, C.PE_ACT_TANH, 0, precision=bad)
    with pytest.raises(ValueError, match="precision"):
        P.host_forward([[32, 5]], BU.lattice_tensors([[32, 5]], 52, 1), "tanh", np.zeros((1, 52), np.float32),
                       precision="f16")


# ---------------------------------------------------------------- 2: the twin against torch
TWIN_NETS = [("a2c", (256, 256), "tanh"), ("dqn", (512, 512, 256), "relu"), ("a2c", (32,), "tanh")]


@pytest.mark.parametrize("D", [77, 107, 347])
@pytest.mark.parametrize("kind,hidden,act", TWIN_NETS)
def test_twin_is_no_worse_than_torch_bf16(D, kind, hidden, act):
    """70 rows, torch default init.  Reference: f64 torch on the f32 weights.  Yardstick: torch's own
    bf16 modules on the CPU, which round the biases, the head and every output too.  The twin's worst
    head deviation is at most 1.0 x the yardstick's (measured: 0.65 .. 0.91)."""
    sd = a2c_state_dict(D, hidden, seed=D) if kind == "a2c" else dqn_state_dict(D, hidden, seed=D)
    towers, activation, tensors = P.parse_state_dict(sd)
    assert activation == act
    tensors = BU.np_tensors(tensors)
    obs = obs_rows(D, n=70, seed=D)
    ref = BU.reference_heads(tensors, act, obs)
    yard = BU.torch_bf16_heads(tensors, act, obs)
    _, logits, values = P.host_forward(towers, tensors, act, obs, precision="bf16")
    twin = BU.worst_deviation((logits, values), ref)
    torch_bf16 = BU.worst_deviation((yard[0], yard[1][:, 0] if len(yard) == 2 else None), ref)
    print(f"D={D} {kind}{list(hidden)} {act}: twin {twin:.3e} torch-bf16 {torch_bf16:.3e} ratio {twin / torch_bf16:.3f}")
    assert 0 < twin <= 1.0 * torch_bf16
    # and the twin is a bf16 evaluation, not the f32 one: it differs from the f32 twin
    _, l32, _ = P.host_forward(towers, tensors, act, obs)
    assert not np.array_equal(l32, logits)


def test_twin_executes_the_definition():
    """The twin against the definition restated in numpy on one small net: operands rounded once to
    bf16, f64 sums rounded to f32 once, pe_tanhf, activations rounded to bf16, f32 fmaf head."""
    towers, D = [[32, 5], [32, 1]], 52
    tensors = BU.np_tensors(P.parse_state_dict(a2c_state_dict(D, (32,), seed=3))[2])
    obs = obs_rows(D, n=9, seed=3, geometry=(8, 4))
    _, logits, values = P.host_forward(towers, tensors, "tanh", obs, precision="bf16")
    xb = BU.bf16_round(obs).astype(np.float64)
    for tw, got in zip(tensors, (logits, values[:, None])):
        (W, b), (Wh, bh) = tw
        z = (b.astype(np.float64) + xb @ BU.bf16_round(W).astype(np.float64).T).astype(np.float32)
        a = BU.bf16_round(P.math_host("tanh", z))
        # the head's fmaf chain rounds after every step; in f64 it is within a few f32 ulps
        want = bh.astype(np.float64) + a.astype(np.float64) @ Wh.astype(np.float64).T
        assert np.abs(got - want).max() < 1e-5


# ---------------------------------------------------------------- 3: the lattice generator
@pytest.mark.parametrize("name,form", [(g, f) for g in BU.GEO for f in BU.GEO[g]["obs"]])
def test_lattice_cases_are_exact(name, form):
    """Every exact case of the GPU test: for every hidden layer the terms of every pre-activation
    share a grid 2^-g and sum |terms| + |bias| < 2^(20 - g) (policy_bf16_util.lattice_check), with
    the obs values the case feeds -- the lattice rows, or the geometry's code table in bf16."""
    D = BU.obs_dim(name)
    xs = BU.exact_x_values(name, form)
    if form == "f32":
        rows = BU.lattice_obs(70, D, BU.LATTICE_SEED)
        assert np.isin(rows, xs).all() and (rows != 0).all()
    for towers, act in BU.EXACT_NETS:
        tensors = BU.lattice_tensors(towers, D, BU.LATTICE_SEED)
        checked = BU.lattice_check(towers, tensors, act, xs)
        assert len(checked) == sum(len(t) - 1 for t in towers)
        assert all(g <= 20 and bound < limit for _, _, g, bound, limit in checked)


def test_lattice_twin_sums_are_exact():
    """On a lattice case the twin's f64 sum is exact, so any summation order gives its bits: the
    pre-activations of the first layer in f32, summed forwards and backwards, equal the f64 ones."""
    D = 107
    towers, act = BU.EXACT_NETS[3]
    (W, b), *_ = BU.lattice_tensors(towers, D, BU.LATTICE_SEED)[0]
    x = BU.lattice_obs(5, D, 1)
    want = b.astype(np.float64) + x.astype(np.float64) @ W.astype(np.float64).T
    for order in (np.arange(D), np.arange(D)[::-1]):
        acc = np.broadcast_to(b, want.shape).astype(np.float32).copy()
        for k in order:
            acc = (acc + x[:, k:k + 1] * W[None, :, k]).astype(np.float32)
        assert np.array_equal(acc.astype(np.float64), want)
