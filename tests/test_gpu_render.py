"""GPU checks of pe_render / PlantOSBatch.render (rl-env_amd/csrc/pe_render.hip).  Every
comparison is exact equality of uint8 arrays:

- golden: the reference's own frames (tests/golden/render_*.npz) from set_state;
- against tests/render_ref.py (pinned to those frames on the CPU) after real stepping
  with auto-resets, at seven geometries, and with the explored map decoupled from the
  visits (the explored-bitmap path);
- indexing (k = 1, no index, repeated / unordered indices with env n-1), strided output
  into a prefilled mosaic canvas (nothing outside the frames is touched), the state is
  left unchanged, bad arguments.
"""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

import render_ref

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def np_(t):
    return t.detach().cpu().numpy()


def make(cfg, n, **kw):
    from plantos_amd import PlantOSBatch
    G, P, Ob, R, C = cfg
    return PlantOSBatch(n, grid_size=G, num_plants=P, num_obstacles=Ob, lidar_range=R, lidar_channels=C,
                        device=DEV, **kw)


def state(b):
    return {k: np_(v) for k, v in b.get_state().items()}


def ref(b, st, idx, s):
    return render_ref.render_batch(st["cells"], st["explored"], st["scalars"], idx, b.cfg.lidar_channels,
                                   b.cfg.lidar_range, s)


def stepped(cfg, n, steps=60, seed=3, max_steps=25):
    """a batch after `steps` random-action steps (max_steps small: auto-resets occur)"""
    b = make(cfg, n, seed=seed, max_steps=max_steps)
    rng = np.random.default_rng(seed)
    for _ in range(steps):
        b.step(torch.as_tensor(rng.integers(0, 5, n).astype(np.int32), device=DEV))
    if steps >= 2 * max_steps:
        assert int(np_(b.get_state(("scalars",))["scalars"])[:, 7].min()) >= 2  # every env was reset
    return b


# ------------------------------------------------------------------ golden frames
@pytest.mark.parametrize("geo", ["g7", "g20", "g21", "g25"])
def test_golden_frames(geo):
    paths = sorted(glob.glob(os.path.join(REPO, "tests", "golden", f"render_{geo}_*.npz")))
    fx = [np.load(p, allow_pickle=False) for p in paths]
    assert len(fx) >= 8
    b = make(tuple(int(v) for v in fx[0]["cfg"]), len(fx))
    b.set_state(cells=np.stack([d["cells"] for d in fx]), visits=np.stack([d["visits"] for d in fx]),
                explored=np.stack([d["explored"] for d in fx]), scalars=np.stack([d["scalars"] for d in fx]))
    for s in sorted({int(d["cell_size"]) for d in fx}):
        frames = np_(b.render(cell_size=s))
        for i, (p, d) in enumerate(zip(paths, fx)):
            if int(d["cell_size"]) == s:
                assert np.array_equal(frames[i], d["frame"]), os.path.basename(p)
    b.close()


# ------------------------------------------------------------------ render_ref after stepping
STEPPED = {
    "g7": ((7, 3, 3, 3, 12), 8),
    "g20": ((20, 10, 12, 6, 16), 6),
    "g25": ((25, 10, 12, 6, 16), 4),
    "g21": ((21, 8, 50, 2, 10), 5),
    "g32": ((32, 20, 30, 9, 24), 3),
    "g64": ((64, 100, 120, 6, 64), 4),
    "g64r32": ((64, 100, 120, 32, 64), 2),
    "g128": ((128, 10, 12, 6, 16), 2),  # the largest grid side: frames of 256 x 256
}


@pytest.mark.parametrize("geo", list(STEPPED))
def test_equals_render_ref_after_stepping(geo):
    cfg, s = STEPPED[geo]
    n = 70
    b = stepped(cfg, n)
    st = state(b)
    idx = [0, 1, 17, 33, 64, 65, 68, n - 1]
    frames = np_(b.render(idx, cell_size=s))
    assert frames.shape == (8, cfg[0] * s, cfg[0] * s, 3) and frames.dtype == np.uint8
    want = ref(b, st, idx, s)
    for j, e in enumerate(idx):
        assert np.array_equal(frames[j], want[j]), (geo, e)
    b.close()


def test_explored_bitmap_path():
    """visit_counts injected without explored (CurriculumWrapper, A2C_training.py:88-93):
    the explored map no longer follows the visits and is drawn from the bitmap"""
    cfg, s = STEPPED["g20"]
    n = 9
    b = stepped(cfg, n, steps=20, max_steps=1000, seed=8)
    before = state(b)
    assert ((before["explored"] > 0).sum(axis=(1, 2)) >= 2).any()
    visits = np.zeros_like(before["visits"])
    visits[:, 5, 5] = 3
    b.set_state(visits=visits)
    st = state(b)
    assert np.array_equal(st["explored"], before["explored"]) and np.array_equal(st["visits"], visits)
    frames = np_(b.render(cell_size=s))
    assert np.array_equal(frames, ref(b, st, range(n), s))
    derived = dict(st, explored=(visits > 0).astype(np.int8))
    assert not np.array_equal(frames, ref(b, derived, range(n), s))
    b.close()


# ------------------------------------------------------------------ indexing
def test_indexing():
    cfg, s = STEPPED["g7"]
    n = 70
    b = stepped(cfg, n)
    st = state(b)
    full = ref(b, st, range(n), s)
    assert np.array_equal(np_(b.render(cell_size=s)), full)                 # no index: env j in frame j
    assert np.array_equal(np_(b.render([n - 1], cell_size=s)), full[[n - 1]])  # k = 1
    idx = [n - 1, 3, 3, 64, 0, n - 1, 41]
    assert np.array_equal(np_(b.render(idx, cell_size=s)), full[idx])
    assert np.array_equal(np_(b.render(np.array(idx, np.int64), cell_size=s)), full[idx])
    dev_idx = torch.as_tensor(idx, dtype=torch.int32, device=DEV)
    assert np.array_equal(np_(b.render(dev_idx, cell_size=s)), full[idx])
    assert tuple(b.render([], cell_size=s).shape) == (0, 56, 56, 3)
    b.close()


# ------------------------------------------------------------------ strides
@pytest.mark.parametrize("geo", ["g21", "g7"])
def test_strided_mosaic_touches_nothing_else(geo):
    """5 frames into a 3-column mosaic canvas prefilled with 0xAB, at an odd byte offset:
    one render per tile row; every byte outside the frames (the sixth tile included) keeps
    0xAB.  g21 with s = 5 has 315-byte frame rows."""
    cfg, s = STEPPED[geo]
    n, pad, cols = 6, 5, 3
    b = stepped(cfg, n)
    st = state(b)
    H = W = cfg[0] * s
    idx = [4, 0, 5, 2, 4]
    flat = torch.full((pad + 2 * H * cols * W * 3 + pad,), 0xAB, dtype=torch.uint8, device=DEV)
    canvas = flat[pad:pad + 2 * H * cols * W * 3].view(2 * H, cols * W, 3)
    for r, part in enumerate((idx[:3], idx[3:])):
        tiles = canvas[r * H:(r + 1) * H, :len(part) * W].unflatten(1, (len(part), W)).permute(1, 0, 2, 3)
        assert tiles.stride() == (3 * W, 3 * cols * W, 3, 1)
        assert b.render(part, cell_size=s, out=tiles) is tiles
    want = np.full((2 * H, cols * W, 3), 0xAB, np.uint8)
    frames = ref(b, st, idx, s)
    for i in range(5):
        want[(i // cols) * H:(i // cols + 1) * H, (i % cols) * W:(i % cols + 1) * W] = frames[i]
    got = np_(flat)
    assert np.array_equal(got[pad:-pad].reshape(2 * H, cols * W, 3), want)
    assert (got[:pad] == 0xAB).all() and (got[-pad:] == 0xAB).all()
    b.close()


def test_vec_env_mosaic_on_device():
    from plantos_amd.vec_env import PlantOSVecEnv
    cfg, s = STEPPED["g21"]
    G, P, Ob, R, C = cfg
    envs = [6, 2, 4, 0, 6]
    v = PlantOSVecEnv(7, grid_size=G, num_plants=P, num_obstacles=Ob, lidar_range=R, lidar_channels=C, seed=4,
                      device=DEV, render_mode="rgb_array", render_envs=envs, cell_size=s)
    v.reset()
    for t in range(5):
        v.step(np.full(7, t % 5))
    st = state(v.batch)
    frames = ref(v.batch, st, envs, s)
    imgs = v.get_images()
    assert len(imgs) == 5 and all(np.array_equal(a, f) for a, f in zip(imgs, frames))
    assert np.array_equal(v.render(), render_ref.mosaic(frames))
    v.close()


# ------------------------------------------------------------------ the state is only read
def test_render_leaves_state_and_next_step_unchanged():
    cfg, s = STEPPED["g20"]
    n = 70
    a, twin = stepped(cfg, n), stepped(cfg, n)
    before = state(a)
    a.render(cell_size=s)
    a.render([5, 5, n - 1], cell_size=3)
    after = state(a)
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    rng = np.random.default_rng(99)
    for _ in range(3):
        act = torch.as_tensor(rng.integers(0, 5, n).astype(np.int32), device=DEV)
        outs_a = [np_(t).copy() for t in a.step(act)]
        outs_t = [np_(t).copy() for t in twin.step(act)]
        for x, y in zip(outs_a, outs_t):
            assert np.array_equal(x, y)
        a.render(cell_size=s)
    sa, stw = state(a), state(twin)
    for k in sa:
        assert np.array_equal(sa[k], stw[k]), k
    a.close()
    twin.close()


def test_width_limit_at_the_largest_grid():
    """grid_size * cell_size <= 4096: at G = 128 cell_size 32 is the last one drawn, 33 is rejected
    and draws nothing"""
    cfg, _ = STEPPED["g128"]
    b = make(cfg, 2, seed=3)
    st = state(b)
    assert np.array_equal(np_(b.render([1], cell_size=32)), ref(b, st, [1], 32))
    out = torch.full((1, 8, 8, 3), 0xCD, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match=r"grid_size \* cell_size <= 4096"):
        b.render([1], cell_size=33)
    from plantos_amd import _capi
    assert _capi.lib().pe_render(b.handle, 1, None, 33, ctypes.c_void_p(out.data_ptr()), 3 * 4224 * 4224, 3 * 4224,
                                 b._stream()) == _capi.PE_ERR_ARG
    torch.cuda.synchronize()
    assert (np_(out) == 0xCD).all()  # nothing was launched
    b.close()


# ------------------------------------------------------------------ arguments
def test_bad_arguments():
    from plantos_amd import _capi
    cfg, s = STEPPED["g7"]
    n = 5
    b = make(cfg, n)
    L = _capi.lib()
    W = cfg[0] * s
    out = torch.full((n, W, W, 3), 0xCD, dtype=torch.uint8, device=DEV)
    ptr, stream = ctypes.c_void_p(out.data_ptr()), b._stream()

    def call(k, cell, fs, rs):
        return L.pe_render(b.handle, k, None, cell, ptr, fs, rs, stream)

    assert call(n, 0, 3 * W * W, 3 * W) == _capi.PE_ERR_ARG
    assert call(n, 1, 3 * W * W, 3 * W) == _capi.PE_ERR_ARG
    assert call(-1, s, 3 * W * W, 3 * W) == _capi.PE_ERR_ARG
    assert call(n, s, 3 * W * W, 3 * W - 1) == _capi.PE_ERR_ARG      # rows would overlap
    assert call(n, s, -1, 3 * W) == _capi.PE_ERR_ARG
    assert call(n + 1, s, 3 * W * W, 3 * W) == _capi.PE_ERR_ARG      # no index: k <= n
    assert call(n, 65, 3 * 65 * 7 * 65 * 7, 3 * 65 * 7) == _capi.PE_ERR_ARG
    assert call(0, s, 3 * W * W, 3 * W) == _capi.PE_OK
    for bad in ([n], [-1], [0, n + 3, 1]):
        with pytest.raises(ValueError):
            b.render(bad, cell_size=s, out=out[:len(bad)])
    with pytest.raises(ValueError):
        b.render(cell_size=1)
    with pytest.raises(ValueError):
        b.render([0.5], cell_size=s)
    with pytest.raises(ValueError):
        b.render(cell_size=s, out=out[:, :, :, :2])
    torch.cuda.synchronize()
    assert (np_(out) == 0xCD).all()  # nothing was launched
    b.close()
