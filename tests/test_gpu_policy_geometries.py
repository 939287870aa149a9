"""GPU checks of the policy kernels at the obs lengths of tests/policy_geometries.py -- what g20
(D = 107) and g21 (D = 77), both odd with D % 8 in {3, 5}, cannot tell apart:

- D even, where the staging pitch D | 1 differs from D (e52, e72);
- no padded k-group (e72: Kp0 == D), 7 padded columns (p57), 1 (p87);
- the staging image as the widest LDS image (HB = D | 1) and only 32 envs per workgroup (w347,
  far347, max417), the library's fallback to 32 at n >= 64 CUs, the LDS limit (max417 / over422);
- obs codes written by the byte-tile and far step kernels (w347, far347: R = 32 in the table);
- the LSTM chain [obs padded to 8 | h] with H < D | 1 < Kp0 + H, H > D | 1 and Kp0 == D.

Everything is bit for bit against the host twins (Policy.host_forward,
RecurrentPolicy.host_forward), which test_policy_geometries_host.py holds against f64 at the
same lengths.  The step kernel each geometry runs is asserted by policy_geometries.make (the
table in that module's docstring); all eight rows were accepted as stated.
"""
import ctypes

import numpy as np
import pytest
import torch

import policy_geometries as PG
from lstm_util import make_lstm_tensors
from policy_util import make_tensors
from test_gpu_policy import check_equal, guarded, np_, rollout_obs
from test_gpu_policy_lstm import check_states, record, u8

pytestmark = pytest.mark.gpu

DEV = PG.DEV
NETS = [([[32, 5]], "tanh"), ([[64, 64, 5], [64, 64, 1]], "tanh"), ([[64, 32, 5]], "relu")]
ACCEPTED = [(g, form) for g in PG.GEO if g != "over422" for form in PG.GEO[g]["obs"]]
SEED = 81


def cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count


def ff_tiles(D, n, towers, act):
    """the env tiles the plan accepts: 32, and 64 where its LDS images fit"""
    from plantos_amd import _capi as C
    from plantos_amd import policy as P
    out = []
    for et in (32, 64):
        try:
            C.policy_plan(D, n, cu_count(), None, P._tower_structs(towers), P.ACTIVATIONS[act], et)
            out.append(et)
        except ValueError:
            assert et == 64
    return out


def lstm_tiles(D, n, H, towers):
    from plantos_amd import _capi as C
    from plantos_amd import policy as P
    out = []
    for et in (32, 64):
        try:
            C.policy_plan(D, n, cu_count(), P._lstm_structs(H, len(towers)), P._tower_structs(towers),
                          P.ACTIVATIONS["tanh"], et)
            out.append(et)
        except ValueError:
            assert et == 64
    return out


# ---------------------------------------------------------------- MLP, value, rows
@pytest.mark.parametrize("name,form,n", [(g, f, n) for g, f in ACCEPTED for n in (33, 65)])
def test_mlp_kernel_equals_twin(name, form, n):
    """act() on the reset obs and on the obs after 12 synthetic steps (codes and their f32
    expansion), argmax and sampled, every tile the plan accepts; value() against act()'s values;
    act_rows() on the last 17 rows (they cross a tile boundary at n = 65)."""
    from plantos_amd import Policy
    codes = form == "codes"
    b = PG.make(name, n, codes, seed=3, env_id_offset=1000)
    D = b.obs_dim
    first, stepped, stepped_f32 = rollout_obs(b, steps=12)
    assert stepped.dtype is (torch.uint8 if codes else torch.float32)
    inputs = [("reset", first, first), ("stepped", stepped, stepped_f32)]
    if codes:
        inputs.append(("stepped f32", stepped_f32, stepped_f32))
    rows = stepped[n - 17:]
    rows32 = np_(stepped_f32)[n - 17:]
    wide = D > 128
    for towers, act in NETS:
        tensors = make_tensors(towers, D, SEED, "var")
        tiles = ff_tiles(D, n, towers, act)
        assert tiles == ([32] if wide else [32, 64]), (name, towers, tiles)
        want = {}
        for et in tiles:
            pol = Policy(b, towers, act, seed=99, env_tile=et).load(tensors)
            assert pol.env_tile == et
            got_bytes = {}
            for what, x, x32 in inputs:
                for det in (True, False):
                    key = (what, det)
                    if key not in want:
                        want[key] = pol.host_forward(np_(x32), tensors, deterministic=det, t=7)
                    tag = f"{name} {form} n={n} {towers} tile {et} {what} det={det}"
                    got = pol.act(x, deterministic=det, t=7)
                    check_equal(got, want[key], tag)
                    got_bytes[key] = [np_(g).tobytes() if g is not None else None for g in got]
                    if len(towers) == 2:   # the value-only forward: act()'s values, bit for bit
                        pol.values.fill_(-7.0)
                        assert pol.value(x) is pol.values
                        assert np_(pol.values).tobytes() == want[key][2].tobytes(), f"{tag}: value()"
            if codes:
                for det in (True, False):
                    assert got_bytes[("stepped", det)] == got_bytes[("stepped f32", det)], f"{name} tile {et}: codes vs f32"
            w = pol.host_forward(rows32, tensors)
            for x in ([rows, torch.as_tensor(rows32, device=DEV)] if codes else [rows]):
                a, lg, v = pol.act_rows(x.contiguous())
                tag = f"{name} {form} n={n} {towers} tile {et} act_rows {x.dtype}"
                assert np_(a).tobytes() == w[0].tobytes() and np_(lg).tobytes() == w[1].tobytes(), tag
                assert (v is None) == (w[2] is None) and (v is None or np_(v).tobytes() == w[2].tobytes()), tag
            pol.close()
        assert not np.array_equal(want[("reset", True)][1], want[("stepped", True)][1])   # the batch moved
    b.close()


# ---------------------------------------------------------------- LSTM
LSTM_CASES = [("e52", "codes"), ("e72", "codes"), ("p57", "codes"), ("p57", "f32"), ("w347", "codes")]
LSTM_NETS = [(32, [[32, 5], [32, 1]]), (256, [[64, 64, 5], [64, 1]])]


@pytest.mark.parametrize("name,form", LSTM_CASES)
def test_lstm_kernel_equals_twin_over_a_sequence(name, form):
    """Four steps with carried state, a third of the envs flagged as episode starts at step 2
    (index 1), argmax and sampled: outputs and every tower's (h, c) after every step.  H = 32 <
    D | 1 < Kp0 + H everywhere; H = 256 > D | 1 at e52 / e72 / p57 and < D | 1 at w347."""
    from plantos_amd import RecurrentPolicy
    n = 65
    b = PG.make(name, n, form == "codes", seed=3, env_id_offset=1000)
    D = b.obs_dim
    seq = record(b, steps=4)
    assert seq[1][0].dtype is (torch.uint8 if form == "codes" else torch.float32)
    start = (np.arange(n) % 3 == 1).astype(np.uint8) * 5
    starts = [None, start, None, None]
    for H, towers in LSTM_NETS:
        tensors = make_lstm_tensors(D, H, towers, SEED)
        tiles = lstm_tiles(D, n, H, towers)
        assert tiles == ([32] if D > 128 else [32, 64]), (name, H, tiles)
        want = None
        for et in tiles:
            pols = {det: RecurrentPolicy(b, H, towers, "tanh", seed=99, env_tile=et).load(tensors) for det in (True, False)}
            assert pols[True].env_tile == et
            if want is None:   # the twin's sequence, once per net
                want, st = [], None
                for t, ((_, x32), s) in enumerate(zip(seq, starts)):
                    outs = {}
                    for det in (True, False):
                        outs[det], new = pols[det].host_forward(x32, st, s, tensors, deterministic=det, t=7 + t)
                    st = new
                    want.append((outs, st))
                # the flags mattered: the flagged rows differ from a run without them
                _, unflagged = pols[True].host_forward(seq[1][1], want[0][1], None, tensors)
                assert (unflagged[0][0][start != 0] != want[1][1][0][0][start != 0]).any()
            for t, ((x, _), s) in enumerate(zip(seq, starts)):
                for det in (True, False):
                    what = f"{name} {form} H={H} tile {et} step {t + 1} det={det}"
                    got = pols[det].act(x, episode_start=None if s is None else u8(s), deterministic=det, t=7 + t)
                    check_equal(got, want[t][0][det], what)
                    check_states(pols[det], want[t][1], what)
            for p in pols.values():
                p.close()
    b.close()


# ---------------------------------------------------------------- the library's tile choice
def test_tile_falls_back_to_32_where_64_does_not_fit():
    """n = 64 CUs envs: the batch size from which the library picks 64 envs per workgroup -- where
    they fit.  At D = 347 they do not: env_tile=None gives 32, asking for 64 is refused, and the
    forward over all 64 CUs x 2 workgroups equals the twin."""
    from plantos_amd import Policy, _capi as C
    from plantos_amd import policy as P
    towers, act = NETS[0]
    n = 64 * cu_count()
    short = C.policy_plan(PG.obs_dim("p87"), n, cu_count(), None, P._tower_structs(towers), P.ACTIVATIONS[act], 0)
    assert short.env_tile == 64   # the rule this case falls out of
    b = PG.make("w347", n, True, seed=5)
    b.step(b.synth_actions(5, 0))
    codes = b.obs
    x32 = np_(b.expand_codes(b.io)[0])
    tensors = make_tensors(towers, b.obs_dim, SEED, "var")
    pol = Policy(b, towers, act, seed=3, env_tile=None).load(tensors)
    assert pol.env_tile == 32
    with pytest.raises(ValueError, match="LDS"):
        Policy(b, towers, act, env_tile=64)
    check_equal(pol.act(codes, deterministic=False, t=2), pol.host_forward(x32, tensors, deterministic=False, t=2),
                f"w347 n={n}")
    pol.close()
    b.close()


# ---------------------------------------------------------------- the LDS limit
def test_lds_edge_accepts_417_and_refuses_422():
    """[[32, 5]]: the LDS images of 32 envs hold an obs of 417 values (C = 78) and not of 422
    (C = 79).  The sizes are the plan's own (lds_bytes); the refusal launches nothing and leaves
    the batch as it was: its next step equals that of a batch that never saw the refusal."""
    from plantos_amd import Policy, _capi as C
    from plantos_amd import policy as P
    towers, act = NETS[0]
    shapes = P._tower_structs(towers)
    n = 33
    info = C.policy_plan(PG.obs_dim("max417"), n, cu_count(), None, shapes, P.ACTIVATIONS[act], 0)
    assert info.env_tile == 32 and info.lds_bytes <= 160 * 1024
    with pytest.raises(ValueError, match="LDS"):
        C.policy_plan(PG.obs_dim("over422"), n, cu_count(), None, shapes, P.ACTIVATIONS[act], 0)

    b = PG.make("max417", n, False, seed=7, env_id_offset=50)
    first, stepped, _ = rollout_obs(b, steps=12)
    tensors = make_tensors(towers, b.obs_dim, SEED, "var")
    pol = Policy(b, towers, act, seed=9).load(tensors)
    assert pol.env_tile == 32
    for what, x in (("reset", first), ("stepped", stepped)):
        for det in (True, False):
            check_equal(pol.act(x, deterministic=det, t=4), pol.host_forward(np_(x), tensors, deterministic=det, t=4),
                        f"max417 {what} det={det}")
    pol.close()
    b.close()

    b, twin = (PG.make("over422", n, False, seed=7) for _ in range(2))
    for et in (None, 32, 64):
        with pytest.raises(ValueError, match="LDS"):
            Policy(b, towers, act, env_tile=et)
    p = ctypes.c_void_p()
    assert C.lib().pe_policy_create(b.handle, 1, shapes, P.ACTIVATIONS[act], 0, ctypes.byref(p)) == C.PE_ERR_ARG
    assert not p.value and b"LDS" in C.lib().pe_last_error()
    for t in range(2):
        out = [np_(x).copy() for x in b.step(b.synth_actions(5, t))]
        ref = [np_(x).copy() for x in twin.step(twin.synth_actions(5, t))]
        for u, v in zip(out, ref):
            assert u.tobytes() == v.tobytes(), f"step {t} after the refusals"
    assert np.isfinite(out[0]).all() and out[0].any()
    b.close()
    twin.close()


# ---------------------------------------------------------------- padding
@pytest.mark.parametrize("name", ["e52", "e72"])
def test_padding_reads_and_writes_nothing_outside(name):
    """test_gpu_policy's guarded-buffer check where the staging pitch is D + 1: NaN / sentinel
    bytes around the weights, the obs (f32 and codes) and the outputs; the outputs equal the twin
    (a read of a guard would put NaN into them) and every guard is as it was."""
    from plantos_amd import Policy
    n = 65
    b = PG.make(name, n, True, seed=9)
    D = b.obs_dim
    _, codes, f32 = rollout_obs(b, steps=9)
    nan = float("nan")
    towers, act = NETS[1]
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
            check_equal(got, pol.host_forward(np_(f32), tensors, deterministic=False, t=1), f"{name} tile {et} {x.dtype}")
            assert (np_(a_whole)[:5] == -7).all() and (np_(a_whole)[-5:] == -7).all()
            for whole in (lg_whole, v_whole):
                assert np.isnan(np_(whole)[:3]).all() and np.isnan(np_(whole)[-3:]).all()
        pol.close()
    for whole, before in wholes:  # inputs untouched, surroundings included
        assert np_(whole).tobytes() == np_(before).tobytes()
    b.close()
