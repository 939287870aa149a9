"""GPU checks of the rollout minibatches (csrc/pe_rollout_minibatch.h; Rollout.minibatches /
env_minibatches / next_minibatch): the gather kernel on synthetic storage equals numpy fancy
indexing at the host twin's indices byte for byte, in row and env mode, with padded field rows and
guard bytes around every output; the normalisation kernels equal their twin bit for bit on both of
their paths; the generators reproduce a collected rollout through both collectors; device counters
under graph capture; argument checks launch nothing.
"""
import ctypes

import numpy as np
import pytest
import torch

from lstm_util import make_lstm_tensors
from policy_util import make_tensors

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GEO = {"g20": dict(cfg=(20, 10, 12, 6, 16), codes=True), "g21": dict(cfg=(21, 8, 50, 2, 10), codes=False)}
TOWERS = [[32, 5], [32, 1]]
GUARD = 64  # elements of poison on either side of every output (keeps 16-byte alignment)
F_IN = ("actions", "values", "log_probs", "advantages", "returns", "starts")
PADS = dict(actions=2, values=3, log_probs=5, advantages=8, returns=1, starts=6)


def np_(t):
    return t.detach().cpu().numpy()


def dev(x):
    return torch.as_tensor(x, device=DEV)


def collector_stride(n, D, codes):
    """The row stride RolloutCollector gives its storage."""
    from plantos_amd.codes import io_layout
    io_b = io_layout(n, D)[3] if codes else 4 * n * (D + 1) + 2 * n
    return (io_b + n + 511) // 512 * 512


def make_storage(T, n, D, codes, seed):
    """(buf u8 device tensor, stride, obs numpy [T, n, D], table or None): obs rows at the
    collector's stride, the rest of every row poisoned; the buffer ends with the last obs row."""
    from plantos_amd.codes import code_table
    rng = np.random.default_rng(seed)
    stride = collector_stride(n, D, codes)
    row = n * D * (1 if codes else 4)
    host = np.full((T - 1) * stride + row, 0xA5, np.uint8)
    if codes:
        table = code_table(20, 6)
        used = np.flatnonzero((table != 0) | (np.arange(256) == 0)).astype(np.uint8)
        obs = used[rng.integers(0, len(used), (T, n, D))]
        for t in range(T):
            host[t * stride:t * stride + row] = obs[t].reshape(-1)
    else:
        table = None
        obs = rng.standard_normal((T, n, D)).astype(np.float32)
        for t in range(T):
            host[t * stride:t * stride + row] = obs[t].reshape(-1).view(np.uint8)
    return dev(host), stride, obs, table


def make_fields(T, n, seed, with_starts):
    """({name: device view [T, n] of a padded, poisoned array}, {name: numpy [T, n]})."""
    rng = np.random.default_rng(seed)
    views, host = {}, {}
    for name in F_IN:
        if name == "starts" and not with_starts:
            continue
        if name == "actions":
            x, poison = rng.integers(0, 5, (T, n)).astype(np.int32), -99
        elif name == "starts":
            x, poison = rng.integers(0, 2, (T, n)).astype(np.uint8), 77
        else:
            x, poison = rng.standard_normal((T, n)).astype(np.float32), np.nan
        wide = np.full((T, n + PADS[name]), poison, x.dtype)
        wide[:, :n] = x
        views[name], host[name] = dev(wide)[:, :n], x
    return views, host


class Guarded:
    """Contiguous device outputs with GUARD poisoned elements on either side."""

    def __init__(self):
        self.full, self.poison = {}, {}

    def new(self, name, shape, dtype):
        poison = {torch.float32: -123.5, torch.int32: -77, torch.uint8: 0xEE}[dtype]
        size = int(np.prod(shape))
        full = torch.full((size + 2 * GUARD,), poison, dtype=dtype, device=DEV)
        self.full[name], self.poison[name] = full, poison
        return full[GUARD:GUARD + size].view(shape)

    def check(self, what):
        for name, full in self.full.items():
            p = self.poison[name]
            assert bool((full[:GUARD] == p).all()) and bool((full[-GUARD:] == p).all()), f"{what}: guard of {name}"


def make_outs(shape, D, codes, with_starts, B):
    g = Guarded()
    f32, i32, u8 = torch.float32, torch.int32, torch.uint8
    outs = dict(indices=g.new("indices", (B,), i32), obs=g.new("obs", shape + (D,), f32),
                actions=g.new("actions", shape, i32), values=g.new("values", shape, f32),
                log_probs=g.new("log_probs", shape, f32), advantages=g.new("advantages", shape, f32),
                returns=g.new("returns", shape, f32))
    if codes:
        outs["codes"] = g.new("codes", shape + (D,), u8)
    if with_starts:
        outs["starts"] = g.new("starts", shape, u8)
    return outs, g


def expected_rows(idx, n, obs, table, fields):
    """numpy fancy indexing at rollout rows idx: {output name: array [len(idx), ..]}."""
    t, e = idx // n, idx % n
    want = {k: v[t, e] for k, v in fields.items()}
    want["obs"] = obs[t, e] if table is None else table[obs[t, e]]
    if table is not None:
        want["codes"] = obs[t, e]
    return want


# ---------------------------------------------------------------- 1. standalone gather, row mode
@pytest.mark.parametrize("T", [1, 2, 9])
@pytest.mark.parametrize("n", [1, 63, 65, 200])
def test_row_gather_equals_fancy_indexing(T, n):
    from plantos_amd.rollout import host_minibatch_indices, mb_args, minibatch_device
    M = T * n
    for codes, D in ((True, 107), (False, 77)):
        buf, stride, obs, table = make_storage(T, n, D, codes, 100 * T + n)
        fviews, fhost = make_fields(T, n, 7 * T + n, False)
        d_table = None if table is None else dev(table)
        for B in sorted({1, 7, 64, 65, M}):
            nmb = -(-M // B)
            outs, guards = make_outs((B,), D, codes, False, B)
            a = mb_args("rows", T, n, D, B, buf, stride, fviews, outs, obs_f32=not codes, table=d_table, seed=11)
            acc = {k: torch.zeros((nmb * B,) + tuple(v.shape[1:]), dtype=v.dtype, device=DEV) for k, v in outs.items()}
            for epoch in (0, 3):
                what = f"T={T} n={n} D={D} B={B} epoch={epoch}"
                for k in range(nmb):
                    a.epoch, a.k = epoch, k
                    minibatch_device(a, DEV)
                    for name, v in outs.items():
                        acc[name][k * B:(k + 1) * B] = v
                idx = np.concatenate([host_minibatch_indices(M, B, epoch, k, 11) for k in range(nmb)])
                assert np.array_equal(np.sort(idx), np.arange(M))
                want = expected_rows(idx, n, obs, table, fhost)
                got = {k: np_(v) for k, v in acc.items()}
                assert np.array_equal(got["indices"][:M], idx), f"{what}: indices"
                for name, w in want.items():
                    assert got[name][:M].tobytes() == w.tobytes(), f"{what}: {name}"
                # the fixed-size form: rows past count are zeros, their indices -1
                assert np.all(got["indices"][M:] == -1), f"{what}: indices past count"
                for name in want:
                    assert not got[name][M:].any(), f"{what}: {name} past count"
                guards.check(what)


# ---------------------------------------------------------------- 2. standalone gather, env mode
@pytest.mark.parametrize("T", [1, 5])
@pytest.mark.parametrize("n", [1, 70])
def test_env_gather_equals_fancy_indexing(T, n):
    from plantos_amd.rollout import host_minibatch_indices, mb_args, minibatch_device
    H, D = 32, 107
    buf, stride, obs, table = make_storage(T, n, D, True, 5 * T + n)
    fviews, fhost = make_fields(T, n, 3 * T + n, True)
    d_table = dev(table)
    rng = np.random.default_rng(T + n)
    for towers in (1, 2):
        for S in sorted({1, T}):
            snaps = [rng.standard_normal((S, n, H)).astype(np.float32) for _ in range(2 * towers)]
            d_snaps = [dev(s) for s in snaps]
            for Be in (1, 32, 33, 70):
                nmb = -(-n // Be)
                outs, guards = make_outs((T, Be), D, True, True, Be)
                dst = [guards.new(f"state{i}", (Be, H), torch.float32) for i in range(2 * towers)]
                a = mb_args("envs", T, n, D, Be, buf, stride, fviews, outs, table=d_table, seed=5,
                            states=list(zip(d_snaps, dst)))
                for epoch in (0, 2):
                    seen = []
                    for k in range(nmb):
                        what = f"T={T} n={n} towers={towers} S={S} Be={Be} epoch={epoch} k={k}"
                        a.epoch, a.k = epoch, k
                        minibatch_device(a, DEV)
                        env = host_minibatch_indices(n, Be, epoch, k, 5, "envs")
                        c = len(env)
                        seen.append(env)
                        got = {name: np_(v) for name, v in outs.items()}
                        assert np.array_equal(got["indices"][:c], env) and np.all(got["indices"][c:] == -1), what
                        want = {name: v[:, env] for name, v in fhost.items()}
                        want["codes"], want["obs"] = obs[:, env], table[obs[:, env]]
                        for name, w in want.items():
                            assert got[name].shape[:2] == (T, Be), f"{what}: {name} is not time-major"
                            assert got[name][:, :c].tobytes() == np.ascontiguousarray(w).tobytes(), f"{what}: {name}"
                            assert not got[name][:, c:].any(), f"{what}: {name} past count"
                        for i, (s, d) in enumerate(zip(snaps, dst)):
                            g = np_(d)
                            assert g[:c].tobytes() == s[0, env].tobytes(), f"{what}: state {i}"
                            assert not g[c:].any(), f"{what}: state {i} past count"
                        guards.check(what)
                    assert np.array_equal(np.sort(np.concatenate(seen)), np.arange(n))


# ---------------------------------------------------------------- 3. normalisation kernel
@pytest.mark.parametrize("B", [1, 2, 255, 256, 257, 4096, 4097, 8193, 70001])
def test_adv_norm_kernel_equals_twin(B):
    from plantos_amd.rollout import adv_norm_device, host_adv_norm
    rng = np.random.default_rng(B)
    for scale, off in ((1.0, 0.0), (1e-3, 0.1), (1e3, -2e4)):
        a = (rng.standard_normal(B) * scale + off).astype(np.float32)
        want = host_adv_norm(a)
        d_a = dev(a)
        out = torch.full((B + 2 * GUARD,), -123.5, device=DEV)
        adv_norm_device(d_a, out=out[GUARD:GUARD + B])
        assert np_(out[GUARD:GUARD + B]).tobytes() == want.tobytes(), f"B={B} scale={scale}: out of place"
        assert bool((out[:GUARD] == -123.5).all()) and bool((out[-GUARD:] == -123.5).all())
        assert np_(d_a).tobytes() == a.tobytes()
        adv_norm_device(d_a)
        assert np_(d_a).tobytes() == want.tobytes(), f"B={B} scale={scale}: in place"
    const = torch.full((B,), 2.5, device=DEV)
    adv_norm_device(const)
    assert bool((const == (2.5 if B == 1 else 0.0)).all())


@pytest.mark.parametrize("T,cap,count", [(5, 33, 4), (5, 33, 33), (3, 7000, 6999), (1, 64, 1), (4, 64, 0)])
def test_adv_norm_kernel_on_valid_columns(T, cap, count):
    """The [T, cap] form with `count` valid columns, by value (a view) and from a device word:
    the twin on the valid block; the other columns untouched."""
    from plantos_amd.rollout import adv_norm_device, host_adv_norm
    a = np.random.default_rng(T * cap + count).standard_normal((T, cap)).astype(np.float32)
    want = a.copy()
    want[:, :count] = host_adv_norm(a[:, :count])
    if count:
        by_value = dev(a)
        adv_norm_device(by_value[:, :count])
        assert np_(by_value).tobytes() == want.tobytes()
    by_word = dev(a)
    adv_norm_device(by_word, count=dev(np.int32([count])))
    assert np_(by_word).tobytes() == want.tobytes()


# ---------------------------------------------------------------- 4. through the collectors
def make(name, n, **kw):
    from plantos_amd import PlantOSBatch
    G, P, Ob, R, C = GEO[name]["cfg"]
    return PlantOSBatch(n, grid_size=G, num_plants=P, num_obstacles=Ob, lidar_range=R, lidar_channels=C,
                        device=DEV, obs_codes=GEO[name]["codes"], max_steps=3, **kw)


PAIRS = (("actions", "actions"), ("old_values", "values"), ("old_log_prob", "log_probs"), ("advantages", "advantages"),
         ("returns", "returns"))


def check_row_epoch(ro, T, n, B, epoch, what):
    from plantos_amd import host_adv_norm, host_minibatch_indices
    M = T * n
    flat = {src: np_(getattr(ro, src)).reshape(M) for _, src in PAIRS}
    flat["observations"] = np_(ro.obs_f32())
    got = {k: np.zeros_like(v) for k, v in flat.items()}
    seen = np.zeros(M, np.int32)
    raw = []
    for k, mb in enumerate(ro.minibatches(B, epoch=epoch, seed=3, normalize_advantage=False)):
        idx = np_(mb.indices)
        assert mb.count == len(idx) == min(B, M - k * B)
        assert np.array_equal(idx, host_minibatch_indices(M, B, epoch, k, 3)), f"{what}: indices of minibatch {k}"
        seen[idx] += 1
        got["observations"][idx] = np_(mb.observations)
        for dst, src in PAIRS:
            got[src][idx] = np_(getattr(mb, dst))
        raw.append(np_(mb.advantages).copy())
    assert np.all(seen == 1), f"{what}: an epoch is no partition"
    for k, v in flat.items():
        assert got[k].tobytes() == v.tobytes(), f"{what}: {k}"
    for k, mb in enumerate(ro.minibatches(B, epoch=epoch, seed=3, normalize_advantage=True)):
        assert np_(mb.advantages).tobytes() == host_adv_norm(raw[k]).tobytes(), f"{what}: normalised minibatch {k}"
        assert np_(mb.returns).tobytes() == flat["returns"][np_(mb.indices)].tobytes()


@pytest.mark.parametrize("name", list(GEO))
def test_minibatches_reproduce_the_rollout(name):
    from plantos_amd import Policy, RolloutCollector
    n, T = 70, 5
    b = make(name, n, seed=21)
    pol = Policy(b, TOWERS, "tanh", seed=99).load(make_tensors(TOWERS, b.obs_dim, 77, "var"))
    col = RolloutCollector(b, pol, T)
    for it in range(2):
        ro = col.collect()
        check_row_epoch(ro, T, n, 64, it, f"{name} collect {it}")
    # batch_size None: one minibatch of every row; the codes on request
    (mb,) = list(ro.minibatches(None, epoch=1))
    assert mb.count == T * n and tuple(mb.observations.shape) == (T * n, b.obs_dim)
    assert np_(mb.observations).tobytes() == np_(ro.obs_f32())[np_(mb.indices)].tobytes()
    if b.obs_codes:
        (mc,) = list(ro.minibatches(None, epoch=1, obs="codes"))
        assert np.array_equal(np_(mc.codes), np_(ro.obs).reshape(T * n, -1)[np_(mc.indices)])
        assert np_(mc.observations).tobytes() == np_(mb.observations).tobytes()
    else:
        with pytest.raises(ValueError):
            ro.minibatches(64, obs="codes")
    for kw in (dict(batch_size=0), dict(batch_size=-3), dict(batch_size=1.5), dict(batch_size=64, epoch=-1),
               dict(batch_size=64, epoch=0.5), dict(batch_size=64, seed=-1), dict(batch_size=64, obs="bytes")):
        with pytest.raises(ValueError):
            ro.minibatches(**kw)
    with pytest.raises(ValueError):
        ro.env_minibatches(0)
    pol.close(), b.close()


@pytest.mark.parametrize("name", list(GEO))
@pytest.mark.parametrize("mode", ["first", "all"])
def test_env_minibatches_reproduce_the_recurrent_rollout(name, mode):
    from plantos_amd import RecurrentPolicy, RecurrentRolloutCollector, host_adv_norm, host_minibatch_indices
    n, T, H, Be = 70, 5, 32, 33
    b = make(name, n, seed=21)
    pol = RecurrentPolicy(b, H, TOWERS, "tanh", seed=99).load(make_lstm_tensors(b.obs_dim, H, TOWERS, 80))
    col = RecurrentRolloutCollector(b, pol, T, state_snapshots=mode)
    for it in range(2):
        ro = col.collect()
        what = f"{name} {mode} collect {it}"
        obs = np_(ro.obs_f32()).reshape(T, n, -1)
        full = {dst: np_(getattr(ro, src)) for dst, src in PAIRS}
        full["episode_starts"] = np_(ro.episode_starts)
        seen = []
        for k, mb in enumerate(ro.env_minibatches(Be, epoch=it, seed=8)):
            env = np_(mb.env_indices)
            assert np.array_equal(env, host_minibatch_indices(n, Be, it, k, 8, "envs")) and mb.count == len(env)
            seen.append(env)
            assert np_(mb.observations).tobytes() == np.ascontiguousarray(obs[:, env]).tobytes(), f"{what}: obs"
            for key, v in full.items():
                g = np_(getattr(mb, key))
                assert g.shape == (T, len(env)) and g.tobytes() == np.ascontiguousarray(v[:, env]).tobytes(), f"{what}: {key}"
            assert len(mb.lstm_states) == 2
            for (h0, c0), (h, c) in zip(mb.lstm_states, ro.lstm_states):
                assert tuple(h0.shape) == (len(env), H)
                assert np_(h0).tobytes() == np_(h)[0, env].tobytes() and np_(c0).tobytes() == np_(c)[0, env].tobytes(), \
                    f"{what}: lstm_states"
        assert np.array_equal(np.sort(np.concatenate(seen)), np.arange(n))
        for k, mb in enumerate(ro.env_minibatches(Be, epoch=it, seed=8, normalize_advantage=True)):
            want = host_adv_norm(full["advantages"][:, seen[k]])
            assert np_(mb.advantages).tobytes() == want.tobytes(), f"{what}: normalised minibatch {k}"
    pol.close(), b.close()


def test_env_minibatches_without_states():
    from plantos_amd import Policy, RolloutCollector
    b = make("g20", 70, seed=2)
    pol = Policy(b, TOWERS, "tanh", seed=9).load(make_tensors(TOWERS, b.obs_dim, 77, "var"))
    ro = RolloutCollector(b, pol, 5).collect()
    mbs = [(np_(mb.env_indices).copy(), np_(mb.returns).copy(), mb.lstm_states) for mb in ro.env_minibatches(32)]
    assert [len(e) for e, _, _ in mbs] == [32, 32, 6] and all(s is None for _, _, s in mbs)
    for env, ret, _ in mbs:
        assert ret.tobytes() == np.ascontiguousarray(np_(ro.returns)[:, env]).tobytes()
    pol.close(), b.close()


# ---------------------------------------------------------------- 5. device counters, graph capture
def test_next_minibatch_in_a_graph():
    from plantos_amd import Policy, RolloutCollector
    n, T, B = 70, 5, 64
    M = T * n
    nmb = -(-M // B)
    b = make("g20", n, seed=12)
    pol = Policy(b, TOWERS, "tanh", seed=1).load(make_tensors(TOWERS, b.obs_dim, 77, "var"))
    ro = RolloutCollector(b, pol, T).collect()
    names = ("observations", "actions", "old_values", "old_log_prob", "advantages", "returns", "indices")

    def full(mb, count):
        """The fixed-size form of a generator's minibatch: zeros and -1 past count."""
        out = []
        for k in names:
            x = np_(getattr(mb, k))
            pad = np.full((B - count,) + x.shape[1:], -1 if k == "indices" else 0, x.dtype)
            out.append(np.concatenate([x, pad]))
        return out

    want = [full(mb, mb.count) for mb in ro.minibatches(B, epoch=0, seed=4, normalize_advantage=True)]
    want.append(full(next(iter(ro.minibatches(B, epoch=1, seed=4, normalize_advantage=True))), B))
    assert len(want) == nmb + 1 and M % B != 0
    mb = ro.next_minibatch(B, seed=4, normalize_advantage=True)  # every kernel has run before the capture
    torch.cuda.synchronize()
    assert np_(ro.minibatch_ctrl).tolist() == [0, 1] and int(mb.count) == B
    ro.minibatch_ctrl.zero_()
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        mb = ro.next_minibatch(B, seed=4, normalize_advantage=True)
    ro.minibatch_ctrl.zero_()  # whatever the capture did to it
    for i in range(nmb + 1):
        gr.replay()
        torch.cuda.synchronize()
        assert int(mb.count) == min(B, M - (i % nmb) * B)
        for k, w in zip(names, want[i]):
            assert np_(getattr(mb, k)).tobytes() == w.tobytes(), f"replay {i}: {k}"
    assert np_(ro.minibatch_ctrl).tolist() == [1, 1]
    del gr
    pol.close(), b.close()


# ---------------------------------------------------------------- 6. argument checks
def test_argument_checks_launch_nothing():
    from plantos_amd import _capi as C
    from plantos_amd.rollout import mb_args, minibatch_device
    T, n, D, B = 2, 65, 107, 7
    buf, stride, obs, table = make_storage(T, n, D, True, 1)
    fviews, _ = make_fields(T, n, 2, True)
    outs, guards = make_outs((B,), D, True, False, B)
    before = {k: np_(v).copy() for k, v in outs.items()}
    L = C.lib()
    stream = C.stream_ptr(torch.device(DEV))

    def args(**kw):
        a = mb_args("rows", T, n, D, B, buf, stride, fviews, outs, table=dev(table), seed=1)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    with torch.cuda.device(DEV):
        for kw in (dict(B=0), dict(B=-1), dict(k=-(-T * n // B)), dict(out_obs=None), dict(values=None), dict(buf=None),
                   dict(table=None), dict(n_states=2, H=32), dict(T=2 ** 16, n=2 ** 15)):
            assert L.pe_internal_rollout_minibatch(ctypes.byref(args(**kw)), stream) == C.PE_ERR_ARG, kw
        env = mb_args("envs", T, n, D, B, buf, stride, fviews, make_outs((T, B), D, True, True, B)[0], table=dev(table))
        env.n_states, env.H = 1, 32  # states requested, none given
        assert L.pe_internal_rollout_minibatch(ctypes.byref(env), stream) == C.PE_ERR_ARG
        f = torch.full((64,), -7.0, device=DEV)
        P = ctypes.c_void_p
        for bad in ((0, 64, 64, None, P(f.data_ptr()), P(f.data_ptr()), None, stream),
                    (1, 64, 63, None, P(f.data_ptr()), P(f.data_ptr()), None, stream),
                    (1, 64, 64, None, None, P(f.data_ptr()), None, stream),
                    (1, 64, 64, None, P(f.data_ptr()), None, None, stream),
                    (2, 16384, 16384, None, P(f.data_ptr()), P(f.data_ptr()), None, stream)):
            assert L.pe_internal_rollout_adv_norm(*bad) == C.PE_ERR_ARG
    with pytest.raises(ValueError):
        minibatch_device(args(k=99), DEV)
    torch.cuda.synchronize()
    for k, v in outs.items():
        assert np_(v).tobytes() == before[k].tobytes(), f"{k} was written"
    assert bool((f == -7.0).all())
    guards.check("argument checks")
    from plantos_amd import host_minibatch_indices
    last = -(-T * n // B) - 1
    minibatch_device(args(k=last), DEV)  # the last valid k runs
    idx = host_minibatch_indices(T * n, B, 0, last, 1)
    got = np_(outs["indices"])
    assert np.array_equal(got[:len(idx)], idx) and np.all(got[len(idx):] == -1)
