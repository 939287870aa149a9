"""GPU parity of the step kernel's whole-batch (dense) auto-reset -- a synchronized
batch truncating together, the lane-per-env path of quad_done_path -- against the
oracle: every output of every step bit for bit, the terminal obs / info / return /
length of the done envs and the final state.  Shapes are the smallest that reach
each kernel: the 64-env f32 headline kernel is chosen only above 32768 envs.
"""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from oracle_rollout import OracleVec
from test_gpu_coop_reset import CFG, info_rows, np_

pytestmark = pytest.mark.gpu

N_HEAD = 32855  # 513 full 64-env blocks + one of 23 live envs (> kCoopMaxDone done: dense too)
HEADLINE = "pe_step_quad<C16,R6,1word>"


def _make(name, n, seed, **kw):
    from plantos_amd import PlantOSBatch
    G, P, Ob, R, C = CFG[name]
    return PlantOSBatch(n, grid_size=G, num_plants=P, num_obstacles=Ob, lidar_range=R, lidar_channels=C, seed=seed,
                        device="cuda:0", **kw)


def _set_steps(b, ov, start):
    sc = np_(b.get_state(parts=("scalars",))["scalars"])
    sc[:, O.S_STEP] = start
    b.set_state(scalars=sc)
    ov.b.scal[:, O.S_STEP] = start


def _dense_run(name, n, start, steps, want_tobs=True, autoreset=True, again_at=None, kernel=None):
    """start: every env's step counter before the first step (array or int); again_at:
    set them to 999 again before that step (a second whole-batch reset, the other
    visit slot).  Returns the number of resets."""
    cfg = CFG[name]
    seed = aseed = 31
    b = _make(name, n, seed, autoreset=autoreset)
    if kernel is not None:
        assert b.kernel_name == kernel, b.kernel_name
    ov = OracleVec(cfg, np.arange(n), seed)
    _set_steps(b, ov, np.broadcast_to(np.asarray(start, np.int32), (n,)).copy())
    act = torch.empty(n, dtype=torch.int32, device="cuda:0")
    tobs0 = np_(b.terminal_obs).copy()
    resets = 0
    for t in range(steps):
        if t == again_at:
            _set_steps(b, ov, np.full(n, 999, np.int32))
        b.synth_actions(aseed, t, out=act)
        a_np = np_(act)
        obs, rew, te, tr = b.step(act, want_terminal_obs=want_tobs)
        o_obs, o_rew, o_te, o_tr = ov.b.step(a_np)
        done = o_te | o_tr
        didx = np.nonzero(done)[0]
        o_info = info_rows(ov.b, didx)
        o_tobs = o_obs.copy()
        ov.ret += o_rew
        o_ret, o_len = ov.ret.copy(), ov.b.scal[:, O.S_STEP].copy()
        if autoreset:
            for k in didx:
                ov.b.reset_philox(int(k), seed, int(k), int(ov.b.scal[k, O.S_EPISODE]))
                ov.ret[k] = 0.0
            if len(didx):
                o_obs[done] = ov.b.obs(didx)[done]
        resets += len(didx)
        assert (np_(rew) == o_rew.astype(np.float32)).all(), t
        assert (np_(te).astype(bool) == o_te).all() and (np_(tr).astype(bool) == o_tr).all(), t
        assert (np_(obs) == o_obs).all(), t  # (the rows of the envs that are not done: the ordinary ones)
        if len(didx):
            if want_tobs:
                assert (np_(b.terminal_obs)[didx] == o_tobs[didx]).all(), t
            else:
                assert (np_(b.terminal_obs) == tobs0).all(), t  # untouched
            assert (np_(b.episode_return)[didx] == o_ret[didx]).all(), t
            assert (np_(b.episode_length)[didx] == o_len[didx]).all(), t
            assert (np_(b.terminal_info)[didx] == o_info).all(), t
    st = b.get_state()
    assert (np_(st["cells"]) == ov.b.cells).all()
    assert (np_(st["visits"]) == ov.b.visits).all()
    assert (np_(st["scalars"]) == ov.b.scal).all()
    b.close()
    return resets


def test_headline_every_env_at_once():
    assert _dense_run("g20", N_HEAD, 999, 3, kernel=HEADLINE) == N_HEAD


def test_headline_partly_done_blocks():
    """Start steps spread over 4 values: about 16 of a block's 64 envs are done in each
    of the first 4 steps -- done and ordinary rows mixed in one tile."""
    start = 999 - (np.random.default_rng(7).integers(0, 4, N_HEAD)).astype(np.int32)
    assert _dense_run("g20", N_HEAD, start, 6, kernel=HEADLINE) == N_HEAD


@pytest.mark.parametrize("name,n", [
    ("g20", 256),     # 16 envs per workgroup, 8 waves
    ("g20", 8256),    # 32 envs per workgroup
    ("g15", 256), ("g12r2", 256), ("g21", 256),
    ("g25", 256),     # two-word rows; the image fills its tile row exactly
    ("g7", 256),      # the runtime sector kernel
])
def test_lane_path_every_env_at_once(name, n):
    assert _dense_run(name, n, 999, 3) == n


def test_two_whole_batch_resets():
    """Both visit slots (episode & 1) get a fresh episode's rows."""
    assert _dense_run("g20", N_HEAD, 999, 5, again_at=2, kernel=HEADLINE) == 2 * N_HEAD


def test_without_terminal_obs():
    assert _dense_run("g20", N_HEAD, 999, 3, want_tobs=False, kernel=HEADLINE) == N_HEAD


def test_without_autoreset():
    """Terminal outputs are written and no env is reset (the done step is the last)."""
    assert _dense_run("g20", N_HEAD, 998, 2, autoreset=False, kernel=HEADLINE) == N_HEAD


def test_reset_step_in_a_graph():
    """Four steps holding the whole-batch reset, captured in one graph and replayed
    once, against the same four steps launched one by one on a twin batch."""
    n, K = N_HEAD, 4
    outs = []
    for graphed in (True, False):
        b = _make("g20", n, 31)
        assert b.kernel_name == HEADLINE, b.kernel_name
        sc = np_(b.get_state(parts=("scalars",))["scalars"])
        sc[:, O.S_STEP] = 997
        ep0 = sc[:, O.S_EPISODE].copy()
        b.set_state(scalars=sc)
        acts = torch.empty((K, n), dtype=torch.int32, device="cuda:0")
        for t in range(K):
            b.synth_actions(31, t, out=acts[t])
        ios = [b.new_io() for _ in range(K)]
        torch.cuda.synchronize()
        if graphed:
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                for t in range(K):
                    b.step(acts[t], io=ios[t])
            gr.replay()
        else:
            for t in range(K):
                b.step(acts[t], io=ios[t])
        torch.cuda.synchronize()
        res = [np_(v).copy() for io in ios for v in b.io_views(io)]
        res += [np_(x).copy() for x in (b.terminal_obs, b.episode_return, b.episode_length, b.terminal_info)]
        st = b.get_state()
        res += [np_(st[k]).copy() for k in sorted(st)]
        assert (np_(st["scalars"])[:, O.S_EPISODE] == ep0 + 1).all()  # the reset step was in the window
        outs.append(res)
        if graphed:
            del gr
        b.close()
    assert len(outs[0]) == len(outs[1])
    for u, v in zip(*outs):
        assert u.shape == v.shape and (u == v).all()
