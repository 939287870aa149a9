"""The policy twins and plans at the obs lengths of tests/policy_geometries.py, without a GPU.

test_gpu_policy_geometries.py shows that the kernels equal the host twins at these lengths; this
file shows that the twins are right there: against test_policy_host.py's f64 reference and its
derived running bound (TAU = 3.16), test_policy_lstm_host.py's torch-f64 scheme (MARGIN = 8.0),
and the documented layouts of test_policy_plan_host.py.  No new bound or margin: all three are
imported.  The obs rows come from each geometry's own code table (policy_util.obs_rows with
(G, R)): distances up to R = 32, positions up to 96 + 32, visit values.
"""
import numpy as np
import pytest

import policy_geometries as PG
from plantos_amd import _capi as C
from plantos_amd import policy as P
from policy_util import make_tensors, obs_rows
from test_policy_host import N, SHAPES, reference
from test_policy_lstm_host import check_twin_against_f64
from test_policy_plan_host import CUS, packed_floats

# D -> (G, R) of the geometry whose rows are drawn; 347: far347's, the longest code table
LENGTHS = {PG.obs_dim(g): (PG.GEO[g]["cfg"][0], PG.GEO[g]["cfg"][3]) for g in ("e52", "p57", "e72", "p87", "far347", "max417")}
ALL_LENGTHS = sorted({PG.obs_dim(g) for g in PG.GEO})
WEIGHT_SEED = 20251   # test_policy_host's; see test_argmax_matches_f64_reference for the count it gives here
# the nets of the GPU tests at these lengths, then test_policy_host's
NETS = [([[64, 32, 5]], "relu")] + SHAPES


def test_lengths_are_the_stated_residues():
    assert sorted(LENGTHS) == [52, 57, 72, 87, 347, 417] and ALL_LENGTHS == [52, 57, 72, 87, 347, 417, 422]
    pad = {D: ((D + 7) & ~7) - D for D in ALL_LENGTHS}
    assert pad[72] == 0 and pad[57] == 7 and pad[87] == 1 and pad[52] == 4
    assert {D | 1 != D for D in (52, 72)} == {True} and {D % 4 for D in (52, 72, 57, 87)} == {0, 1, 3}
    assert LENGTHS[347] == (33, 32)


def test_obs_rows_default_is_unchanged_and_geometry_rows_use_their_table():
    """Without (G, R) obs_rows returns what it always did (the golden rows, or (21, 2) codes for a
    length without a trajectory); with it every real row is made of the geometry's own codes."""
    from plantos_amd.codes import code_table
    for D in (77, 107, 52):
        rng = np.random.default_rng(7)
        a = obs_rows(D)
        assert a.shape == (N, D) and a.dtype == np.float32 and a.tobytes() == obs_rows(D, 37, 7, None).tobytes()
        if D == 52:   # no trajectory: the draw order of the rule as it was
            real = code_table(21, 2)[rng.integers(0, 4, (25, D))]
            want = np.concatenate([real, rng.random((12, D), np.float32)]).astype(np.float32)
            assert a.tobytes() == want.tobytes()
    for D, (G, R) in LENGTHS.items():
        x = obs_rows(D, geometry=(G, R))
        C5 = D - 27
        real = x[:N - N // 3]
        tab = code_table(G, R)
        assert x.shape == (N, D) and np.isin(real, tab).all()
        assert set(np.unique(real[:, 0:C5:5])) == set(tab[:R + 1])            # every distance r / R
        assert set(np.unique(real[:, 1:C5:5])) == {0.0, 1.0}                   # code R + 1
        assert real[:, C5:C5 + 2].max() > 0.5 and real[:, C5 + 2:].max() == 1.0   # the 96.. and 80.. ranges
        assert not np.isin(x[N - N // 3:], tab).all()                          # the uniform third


@pytest.fixture(scope="module")
def cases():
    """Every (scale, D, net): twin outputs and the f64 reference, computed once."""
    res = []
    for scale in ("std", "var"):
        for D, geo in LENGTHS.items():
            x = obs_rows(D, geometry=geo)
            for towers, act in NETS:
                tensors = make_tensors(towers, D, WEIGHT_SEED, scale)
                a, lg, v = P.host_forward(towers, tensors, act, x)
                res.append(dict(scale=scale, D=D, towers=towers, act=act, actions=a, logits=lg, values=v,
                                ref=reference(towers, tensors, act, x)))
    return res


def test_twin_within_bound_of_f64_reference(cases):
    assert {c["scale"] for c in cases} == {"std", "var"} and len(cases) == 2 * len(LENGTHS) * len(NETS)
    for c in cases:
        z, ez = c["ref"][0]
        err = np.abs(c["logits"].astype(np.float64) - z)
        print(f"{c['scale']} D={c['D']} {c['towers']} {c['act']}: max |twin-ref| {err.max():.3e}, "
              f"max err/bound {(err / ez).max():.3f}")
        assert c["logits"].shape == (N, 5)
        assert (err <= ez).all(), (c["scale"], c["D"], c["towers"])
        if len(c["towers"]) == 2:
            zv, ev = c["ref"][1]
            errv = np.abs(c["values"].astype(np.float64) - zv[:, 0])
            assert (errv <= ev[:, 0]).all(), (c["scale"], c["D"], c["towers"])
        else:
            assert c["values"] is None


def test_argmax_matches_f64_reference(cases):
    """Rows whose f64 top-two gap exceeds twice the row's bound must agree; the undecided rows of
    the new lengths as a group are at most 1 % of their rows.  The count depends on the f64
    reference and the bound alone, not on the twin: with WEIGHT_SEED = 20251 it is 0 of 1110."""
    rows = excluded = 0
    for c in cases:
        if c["scale"] != "std":
            continue
        z, ez = c["ref"][0]
        srt = np.sort(z, axis=1)
        decided = (srt[:, -1] - srt[:, -2]) > 2.0 * ez.max(axis=1)
        rows += len(z)
        excluded += int((~decided).sum())
        assert np.array_equal(c["actions"][decided], np.argmax(z, axis=1)[decided].astype(np.int32)), (c["D"], c["towers"])
        assert np.array_equal(c["actions"], np.argmax(c["logits"], axis=1).astype(np.int32))
    print(f"excluded {excluded} of {rows} rows")
    assert rows == N * len(LENGTHS) * len(NETS)
    assert excluded <= 0.01 * rows


@pytest.mark.parametrize("H,D", [(32, 52), (96, 72), (256, 347)])
def test_lstm_twin_against_f64(H, D):
    """test_policy_lstm_host.test_twin_against_f64's scheme and margin at the new lengths: H < D | 1
    < Kp0 + H at (32, 52), no padded k-group between obs and h at (96, 72), the far kernel's table
    at (256, 347)."""
    check_twin_against_f64(H, D, 1.0, geometry=LENGTHS[D])


def plan(D, towers, hidden=None, n=65, env_tile=0):
    lstms = P._lstm_structs(hidden, len(towers)) if hidden else None
    return C.policy_plan(D, n, CUS, lstms, P._tower_structs(towers), P.ACTIVATIONS["tanh"], env_tile)


def test_plan_sizes_equal_the_documented_layouts():
    """test_policy_plan_host.test_sizes_equal_the_documented_layouts' formulas at the eight lengths,
    feed-forward and with H = 256: the LDS images, the packed buffer, the LSTM state."""
    seen = 0
    for D in ALL_LENGTHS:
        for towers in ([[32, 5]], [[64, 64, 5], [64, 64, 1]], [[64, 32, 5]]):
            for H in (0, 256):
                for n in (33, 65, 64 * CUS):
                    kp0 = (D + 7) // 8 * 8
                    hb = max([w for t in towers for w in t[:-1]] + [H, D | 1])
                    fits = {E: 4 * (256 + E * (9 + kp0 + 2 * hb)) <= 160 * 1024 for E in (32, 64)}
                    if not fits[32]:
                        assert D == 422
                        with pytest.raises(ValueError, match="LDS"):
                            plan(D, towers, H, n)
                        continue
                    info = plan(D, towers, H, n)
                    E = info.env_tile
                    assert E == (64 if fits[64] and n >= 64 * CUS else 32), (D, towers, H, n)
                    assert info.lds_bytes == 4 * (256 + E * (9 + kp0 + 2 * hb)) <= 160 * 1024
                    assert info.packed_floats == packed_floats(D, H, towers), (D, towers, H)
                    assert info.state_floats == (n + E - 1) // E * H * E
                    if not fits[64]:
                        with pytest.raises(ValueError, match="LDS"):
                            plan(D, towers, H, n, env_tile=64)
                    seen += 1
    assert seen == 6 * 3 * 2 * 3   # every length but 422
    # 64 envs per workgroup stop fitting between the short and the long lengths
    assert plan(87, [[32, 5]], n=64 * CUS).env_tile == 64 and plan(347, [[32, 5]], n=64 * CUS).env_tile == 32
    assert plan(417, [[32, 5]]).lds_bytes <= 160 * 1024
    for D, towers in ((422, [[32, 5]]), (347, [[512, 512, 256, 5]])):
        for H in (None, 256):
            with pytest.raises(ValueError, match="LDS"):
                plan(D, towers, H)


def test_step_kernels_of_the_table():
    """The step kernel pe_internal_plan gives every geometry in every obs form the tests feed, and
    that obs_codes is refused where the table has no codes (the wave kernel)."""
    for (name, codes), kernel in PG.KERNEL.items():
        for n in (1, 33, 65, 64 * CUS):
            cfg = C.default_config(*PG.GEO[name]["cfg"])
            cfg.obs_codes = int(codes)
            assert C.plan(cfg, n, CUS).kernel_name.decode() == kernel, (name, codes, n)
    assert set(PG.KERNEL) == {(name, form == "codes") for name, g in PG.GEO.items() for form in g["obs"]}
    for name in ("max417", "over422"):
        cfg = C.default_config(*PG.GEO[name]["cfg"])
        cfg.obs_codes = 1
        with pytest.raises(ValueError, match="obs_codes"):
            C.plan(cfg, 33, CUS)
