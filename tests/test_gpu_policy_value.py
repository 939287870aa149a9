"""GPU checks of the value-only forward (pe_policy_value / pe_policy_value_lstm;
Policy.value, RecurrentPolicy.value, RecurrentPolicy.get_states(out=)): the values equal
act()'s and the host twin's bit for bit, at sizes around the env tiles, with every legal tile,
towers of different depths, codes and f32 obs; the recurrent one reads the state and the start
flags and leaves state and sampler alone; selection writes the selected entries only, whole
tiles skipped included; argument checks; graph capture of act -> step -> value(select).
"""
import ctypes

import numpy as np
import pytest
import torch

from lstm_util import make_lstm_tensors
from policy_util import make_tensors
from rollout_util import record_inputs

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GEO = {"g20": dict(cfg=(20, 10, 12, 6, 16), codes=True), "g21": dict(cfg=(21, 8, 50, 2, 10), codes=False)}
# the last: towers of different depths -- tower 1's own offsets, and its head reads either buffer
FF_TOWERS = ([[32, 5], [32, 1]], [[64, 64, 5], [64, 64, 1]], [[32, 5], [64, 32, 64, 1]])
SEED = 79
FILL = -7.0


def np_(t):
    return None if t is None else t.detach().cpu().numpy()


def u8(x):
    return torch.as_tensor(np.asarray(x, np.uint8), device=DEV)


def make(name, n, **kw):
    from plantos_amd import PlantOSBatch
    G, P, Ob, R, C = GEO[name]["cfg"]
    return PlantOSBatch(n, grid_size=G, num_plants=P, num_obstacles=Ob, lidar_range=R, lidar_channels=C,
                        device=DEV, obs_codes=GEO[name]["codes"], **kw)


def obs_seq(b, steps):
    """[(obs as the batch holds it, obs f32 numpy)] after each of `steps` synthetic steps"""
    act = torch.empty(b.num_envs, dtype=torch.int32, device=DEV)
    seq = []
    for t in range(steps):
        b.synth_actions(5, t, out=act)
        b.step(act)
        x = b.obs.clone()
        f32 = b.expand_codes(b.io)[0] if b.obs_codes else x
        seq.append((x, np_(f32).copy()))
    return seq


def filled(n):
    return torch.full((n,), FILL, dtype=torch.float32, device=DEV)


# ---------------------------------------------------------------- feed-forward
@pytest.mark.parametrize("name,n", [(g, n) for g in GEO for n in (1, 31, 33, 64, 65, 130)])
def test_value_equals_act_and_twin(name, n):
    from plantos_amd import Policy
    b = make(name, n, seed=3)
    (x, x32), = obs_seq(b, 1)
    assert x.dtype is (torch.uint8 if b.obs_codes else torch.float32)
    for towers in FF_TOWERS:
        tensors = make_tensors(towers, b.obs_dim, SEED, "var")
        for act in ("tanh", "relu"):
            want = None
            for et in (32, 64):
                what = f"{name} n={n} {towers} {act} tile {et}"
                pol = Policy(b, towers, act, seed=5, env_tile=et).load(tensors)
                assert pol.env_tile == et
                if want is None:
                    want = pol.host_forward(x32)[2]
                full = np_(pol.act(x, deterministic=False)[2]).copy()
                out = filled(n)
                got = pol.value(x, out=out)
                assert got is out and pol.t == 1, what
                assert np_(out).tobytes() == full.tobytes(), f"{what}: value() vs act()"
                assert np_(out).tobytes() == want.tobytes(), f"{what}: value() vs the twin"
                pol.values.fill_(FILL)   # the default output; obs=None reads the batch's own obs
                assert pol.value() is pol.values and np_(pol.values).tobytes() == want.tobytes(), what
                pol.close()
    b.close()


# ---------------------------------------------------------------- recurrent
def run_recurrent(name, n, H, towers, tiles):
    from plantos_amd import RecurrentPolicy
    b = make(name, n, seed=4, env_id_offset=500)
    seq = obs_seq(b, 5)
    rng = np.random.default_rng(H + n)
    starts = [None] + [(rng.random(n) < 0.3).astype(np.uint8) * 2 for _ in range(4)]
    if n > 2:
        assert starts[3].any() and not starts[3].all()
    tensors = make_lstm_tensors(b.obs_dim, H, towers, SEED)
    for et in tiles:
        what = f"{name} n={n} H={H} tile {et}"
        pol = RecurrentPolicy(b, H, towers, "tanh", seed=11, env_tile=et).load(tensors)
        st = None
        for t in range(3):   # three steps with start flags (the policy's own sampler counter)
            pol.act(seq[t][0], episode_start=None if starts[t] is None else u8(starts[t]), deterministic=False)
            _, st = pol.host_forward(seq[t][1], st, starts[t], deterministic=False, t=t)
        assert pol.t == 3
        before = [(np_(h).copy(), np_(c).copy()) for h, c in pol.get_states()]
        for (h, c), (wh, wc) in zip(before, st):
            assert np.array_equal(h, wh) and np.array_equal(c, wc), f"{what}: the state after three steps"
        x, x32 = seq[3]
        for s in (starts[3], None):
            want = pol.host_forward(x32, [(h.copy(), c.copy()) for h, c in st], s)[0][2]
            out = filled(n)
            assert pol.value(x, episode_start=None if s is None else u8(s), out=out) is out
            assert np_(out).tobytes() == want.tobytes(), f"{what}: value(episode_start={'s' if s is not None else None})"
        # a pair of flags, as act takes them
        pair = (u8(starts[3] & 2), u8(np.zeros(n, np.uint8)))
        assert np_(pol.value(x, episode_start=pair, out=filled(n))).tobytes() == \
            pol.host_forward(x32, st, starts[3])[0][2].tobytes(), what
        if n > 2:
            assert pol.host_forward(x32, st, starts[3])[0][2].tobytes() != pol.host_forward(x32, st, None)[0][2].tobytes()
        # state and sampler untouched; get_states(out=) writes the tensors given
        into = [(torch.full((n, H), FILL, device=DEV), torch.full((n, H), FILL, device=DEV)) for _ in towers]
        ret = pol.get_states(out=into)
        assert all(r[0] is i[0] and r[1] is i[1] for r, i in zip(ret, into))
        for (h, c), (wh, wc) in zip(into, before):
            assert np_(h).tobytes() == wh.tobytes() and np_(c).tobytes() == wc.tobytes(), f"{what}: state after value()"
        assert pol.t == 3
        # the next act equals the twin that never saw the value calls
        got = pol.act(x, episode_start=u8(starts[3]), deterministic=False)
        (wa, wl, wv), st2 = pol.host_forward(x32, st, starts[3], deterministic=False, t=3)
        assert np.array_equal(np_(got[0]), wa) and np.array_equal(np_(got[1]), wl) and np.array_equal(np_(got[2]), wv), what
        for (h, c), (wh, wc) in zip(pol.get_states(), st2):
            assert np.array_equal(np_(h), wh) and np.array_equal(np_(c), wc), f"{what}: the state after the next act"
        pol.close()
    b.close()


@pytest.mark.parametrize("name,n", [(g, n) for g in GEO for n in (1, 33, 65, 130)])
def test_recurrent_value_equals_twin_and_leaves_state(name, n):
    run_recurrent(name, n, 32, [[32, 5], [32, 1]], (32, 64))
    run_recurrent(name, n, 96, [[64, 64, 5], [64, 32, 64, 1]], (32, 64))


def test_recurrent_value_h512():
    run_recurrent("g20", 33, 512, [[32, 5], [64, 1]], (32,))


# ---------------------------------------------------------------- selection
def selections(n, seed):
    """(name, want or None, unless or None) over n = 130 envs: tiles of 32 are [0,32) .. [128,130),
    tiles of 64 are [0,64), [64,128), [128,130)"""
    z = np.zeros(n, np.uint8)

    def at(*idx):
        w = z.copy()
        w[list(idx)] = 1
        return w

    _, _, _, te, tr, *_ = record_inputs(n, 5, seed)
    assert {(int(x), int(y)) for x, y in zip(te, tr)} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    return [("none", z, None), ("all", np.ones(n, np.uint8), None), ("all (no flags)", None, None),
            ("one env in the last partial tile", at(n - 1), None),
            ("one env per tile", at(5, 40, 70, 100, 128) * 9, None),
            ("an empty tile between two", at(3, n - 1), None),
            ("truncated unless terminated", tr, te), ("unless alone", None, te),
            ("want, none of them unless", at(3, 64), z)]


@pytest.mark.parametrize("kind", ["mlp", "lstm"])
def test_selection_writes_selected_entries_only(kind):
    from plantos_amd import Policy, RecurrentPolicy
    n = 130
    b = make("g20", n, seed=6)
    (x, x32), (y, _) = obs_seq(b, 2)
    for et in (32, 64):
        if kind == "mlp":
            towers = FF_TOWERS[2]
            pol = Policy(b, towers, "tanh", env_tile=et).load(make_tensors(towers, b.obs_dim, SEED, "var"))
            value = pol.value
        else:
            towers = [[32, 5], [32, 1]]
            pol = RecurrentPolicy(b, 32, towers, env_tile=et).load(make_lstm_tensors(b.obs_dim, 32, towers, SEED))
            pol.act(y)   # a state that is not zero
            value = lambda obs, **kw: pol.value(obs, episode_start=u8(np.arange(n) % 5 == 0), **kw)  # noqa: E731
        full = np_(value(x, out=filled(n))).copy()
        assert (full != FILL).all()
        for what, want, unless in selections(n, 17):
            sel = np.ones(n, bool) if want is None else want != 0
            if unless is not None:
                sel &= unless == 0
            for as_bool in (False, True):
                conv = (lambda a: None if a is None else (u8(a).bool() if as_bool else u8(a)))  # noqa: E731
                select = conv(want) if unless is None else (conv(want), conv(unless))
                out = filled(n)
                value(x, select=select, out=out)
                got = np_(out)
                assert got[sel].tobytes() == full[sel].tobytes(), f"{kind} tile {et} {what}: selected entries"
                assert (got[~sel] == FILL).all(), f"{kind} tile {et} {what}: an unselected entry was written"
        pol.close()
    b.close()


# ---------------------------------------------------------------- argument checks
def test_argument_checks_launch_nothing():
    from plantos_amd import Policy, RecurrentPolicy, _capi as C
    L, P = C.lib(), ctypes.c_void_p
    b = make("g21", 64, seed=1)   # no obs_codes
    n = b.num_envs
    x = b.reset()
    tw2, tw1 = [[32, 5], [32, 1]], [[32, 5]]
    ff, ff1 = Policy(b, tw2, "tanh"), Policy(b, tw1, "tanh")
    rec, rec1 = RecurrentPolicy(b, 32, tw2), RecurrentPolicy(b, 32, tw1)
    out = filled(n)
    flag = torch.ones(n, dtype=torch.uint8, device=DEV)
    for pol in (ff1, rec1):   # no value tower
        with pytest.raises(ValueError):
            pol.value(x, out=out)
    s = b._stream()
    X, V, F = P(x.data_ptr()), P(out.data_ptr()), P(flag.data_ptr())
    for args in ((rec._p, X, 0, F, None, V, s),     # the wrong kind
                 (ff1._p, X, 0, F, None, V, s),     # one tower
                 (ff._p, X, 0, F, None, None, s),   # null values
                 (ff._p, None, 0, F, None, V, s),   # null obs
                 (ff._p, X, 1, F, None, V, s),      # codes, no obs_codes
                 (ff._p, X, 2, F, None, V, s),
                 (None, X, 0, F, None, V, s)):
        assert L.pe_policy_value(*args) == C.PE_ERR_ARG
    for args in ((ff._p, X, 0, None, None, F, None, V, s),
                 (rec1._p, X, 0, None, None, F, None, V, s),
                 (rec._p, X, 0, None, None, F, None, None, s),
                 (rec._p, None, 0, None, None, F, None, V, s),
                 (rec._p, X, 1, None, None, F, None, V, s),
                 (None, X, 0, None, None, F, None, V, s)):
        assert L.pe_policy_value_lstm(*args) == C.PE_ERR_ARG
    bad_flags = [flag.to(torch.int32), flag.to(torch.float32), flag[:-1], torch.zeros((n, 1), dtype=torch.uint8, device=DEV),
                 flag.cpu(), np.ones(n, np.uint8), (flag, flag, flag), (flag, flag.to(torch.int64)), (flag,)]
    bad_out = [out[:-1], out.to(torch.float64), out.cpu(), torch.zeros((n, 1), device=DEV), torch.zeros(2 * n, device=DEV)[::2]]
    for pol in (ff, rec):
        for f in bad_flags:
            with pytest.raises(ValueError):
                pol.value(x, select=f, out=out)
        for o in bad_out:
            with pytest.raises(ValueError):
                pol.value(x, out=o)
        with pytest.raises(ValueError):
            pol.value(x[:-1], out=out)
        with pytest.raises(ValueError):
            pol.value(torch.zeros((n, b.obs_dim), dtype=torch.uint8, device=DEV), out=out)
    for f in bad_flags[:-1]:
        with pytest.raises(ValueError):
            rec.value(x, episode_start=f, out=out)
    H = rec.hidden
    good = [(torch.zeros((n, H), device=DEV), torch.zeros((n, H), device=DEV)) for _ in range(2)]
    for bad in (good[:1], [(good[0][0],), good[1]], [(good[0][0][:-1], good[0][1]), good[1]],
                [(good[0][0].double(), good[0][1]), good[1]], [(good[0][0].cpu(), good[0][1]), good[1]]):
        with pytest.raises(ValueError):
            rec.get_states(out=bad)
    torch.cuda.synchronize()
    assert (np_(out) == FILL).all()
    for pol in (ff, ff1, rec, rec1):
        pol.close()
    b.close()


# ---------------------------------------------------------------- graph capture
@pytest.mark.parametrize("kind", ["mlp", "lstm"])
def test_act_step_value_in_a_graph(kind):
    """act(); step(); value(terminal obs, select=(truncated, terminated)) captured as one chain and
    replayed twice against the eager run on a twin batch.  max_steps=3 and one env stepped ahead:
    truncations fall into both replays, in some tiles only."""
    from plantos_amd import Policy, RecurrentPolicy
    res = []
    for graphed in (True, False):
        b = make("g20", 130, seed=12, prefetch_every=0, max_steps=3)
        if kind == "mlp":
            towers = FF_TOWERS[1]
            pol = Policy(b, towers, "tanh").load(make_tensors(towers, b.obs_dim, SEED, "var"))
            act = lambda: pol.act()[0]  # noqa: E731
        else:
            towers = [[32, 5], [32, 1]]
            pol = RecurrentPolicy(b, 32, towers).load(make_lstm_tensors(b.obs_dim, 32, towers, SEED))
            act = lambda: pol.act(episode_start=(b.terminated, b.truncated))[0]  # noqa: E731
        b.step(b.synth_actions(1, 0))   # the io buffer now holds codes
        mask = torch.zeros(130, dtype=torch.uint8, device=DEV)
        mask[64:] = 1
        b.reset(mask=mask)              # envs 64.. are one step behind: they time out a step later
        out = filled(130)

        def one():
            b.step(act())
            pol.value(obs=b.terminal_obs, select=(b.truncated, b.terminated), out=out)

        one()   # every kernel of the chain has run once before the capture
        torch.cuda.synchronize()
        if graphed:
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                one()
        log = []
        for _ in range(2):
            gr.replay() if graphed else one()
            torch.cuda.synchronize()
            log.append([np_(out).copy(), np_(b.truncated).copy(), np_(b.io).copy()])
        res.append(log)
        if graphed:
            del gr
        pol.close()
        b.close()
    for it, (u, v) in enumerate(zip(*res)):
        for p, q in zip(u, v):
            assert p.tobytes() == q.tobytes(), f"replay {it}"
    trunc = [l[1] != 0 for l in res[0]]
    assert all(t.any() and not t.all() for t in trunc) and (trunc[0] != trunc[1]).any()
    assert ((res[0][1][0] != FILL) == (trunc[0] | trunc[1])).all()   # written exactly where a time limit fell
