"""Visit counts past 15 (pe_device.hpp: a saturating nibble, the exact count in vx from
the 15th visit on) in the kernels that defer the vx write by a step -- the 64-env f32
headline kernel and its byte-coded twin -- against the oracle: counts injected around
the nibble's saturation, around 270 (where a byte beside the nibble would hand over to
vx: the representation profiles/visit_overflow/ measured and did not keep) and past 16
bits, then stepped, exported, carried across auto-resets (vx is never cleared) and
cloned by the MCTS.  Shapes are the smallest that reach each kernel: the f32 headline
kernel is chosen only above 32768 envs; the byte-coded twin keeps 64-env workgroups at
any size.
"""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from oracle_rollout import OracleVec

pytestmark = pytest.mark.gpu

CFG = (20, 10, 12, 6, 16)
G = CFG[0]
N_HEAD = 32855  # 513 full 64-env blocks + one of 23 live envs
N_TWIN = 130    # two full blocks + a ragged one
HEADLINE = "pe_step_quad<C16,R6,1word>"
TWIN = "pe_step_quad<C16,R6,1word,bytetile>"
KERNELS = [pytest.param(N_HEAD, False, HEADLINE, id="headline"), pytest.param(N_TWIN, True, TWIN, id="codes_twin")]
# below / at / past the nibble's saturation, around the byte's last value (15 + 254 = 269), the
# first counts vx holds (270, 271), and one far past 16 bits
BOUNDARY = np.array([0, 13, 14, 15, 16, 268, 269, 270, 271, 70000], np.int32)
SEED = 31


def np_(t):
    return t.detach().cpu().numpy()


class Pair:
    """a batch on the GPU and its oracle twin, stepped together and compared bit for bit"""

    def __init__(self, n, codes, kernel):
        from plantos_amd import PlantOSBatch
        Gs, P, Ob, R, C = CFG
        self.n, self.codes = n, codes
        self.b = PlantOSBatch(n, grid_size=Gs, num_plants=P, num_obstacles=Ob, lidar_range=R, lidar_channels=C,
                              seed=SEED, device="cuda:0", obs_codes=codes)
        assert self.b.kernel_name == kernel, self.b.kernel_name
        self.ov = OracleVec(CFG, np.arange(n), SEED)
        dev = "cuda:0"
        self.act = torch.empty(n, dtype=torch.int32, device=dev)
        if codes:
            self.obs = torch.empty((n, self.b.obs_dim), dtype=torch.float32, device=dev)
            self.rew = torch.empty(n, dtype=torch.float32, device=dev)
            self.te = torch.empty(n, dtype=torch.uint8, device=dev)
            self.tr = torch.empty(n, dtype=torch.uint8, device=dev)
        self.t = 0

    def set_visits(self, v):
        """visit counts alone, as CurriculumWrapper injects them: the explored map stays"""
        v = np.array(np.broadcast_to(np.asarray(v, np.int32), (self.n, G, G)))  # (a writable copy)
        self.b.set_state(visits=v)
        self.ov.b.visits[...] = v
        return v

    def set_steps(self, steps):
        sc = np_(self.b.get_state(parts=("scalars",))["scalars"])
        sc[:, O.S_STEP] = steps
        self.b.set_state(scalars=sc)
        self.ov.b.scal[:, O.S_STEP] = steps

    def step(self, k):
        resets = 0
        for _ in range(k):
            t = self.t
            self.b.synth_actions(SEED, t, out=self.act)
            out = self.b.step(self.act)
            if self.codes:
                self.b.expand_codes(self.b.io, 1, self.obs, self.rew, self.te, self.tr)
                obs, rew, te, tr = self.obs, self.rew, self.te, self.tr
            else:
                obs, rew, te, tr = out
            o_obs, o_rew, o_te, o_tr, *_ = self.ov.step(np_(self.act))
            assert np.array_equal(np_(obs), o_obs), f"step {t}: obs"
            assert np.array_equal(np_(rew), o_rew.astype(np.float32)), f"step {t}: reward"
            assert np.array_equal(np_(te).astype(bool), o_te) and np.array_equal(np_(tr).astype(bool), o_tr), t
            resets += int((o_te | o_tr).sum())
            self.t += 1
        return resets

    def check_state(self):
        st = self.b.get_state()
        assert np.array_equal(np_(st["visits"]), self.ov.b.visits)
        assert np.array_equal(np_(st["cells"]), self.ov.b.cells)
        assert np.array_equal(np_(st["explored"]), self.ov.b.explored)
        assert np.array_equal(np_(st["scalars"]), self.ov.b.scal)

    def close(self):
        self.b.close()


@pytest.mark.parametrize("n,codes,kernel", KERNELS)
def test_boundaries_under_stepping(n, codes, kernel):
    """every cell of env e preset to BOUNDARY[e % 10], then 40 steps: the moves cross 14 -> 15
    (the exact count's first write) and 269 -> 270, and bump the counts past both"""
    p = Pair(n, codes, kernel)
    v0 = p.set_visits(BOUNDARY[np.arange(n) % 10][:, None, None])
    assert p.step(40) == 0
    # (the window does cross them: some cell went 13 -> 16 and more, 268 -> 271 and more)
    final, cls = p.ov.b.visits, np.arange(n) % 10
    assert final[cls == 1].max() >= 16 and final[cls == 5].max() >= 271 and final[cls == 6].max() >= 271
    p.check_state()
    p.close()


@pytest.mark.parametrize("n,codes,kernel", KERNELS)
def test_import_export_round_trip(n, codes, kernel):
    p = Pair(n, codes, kernel)
    cell = np.arange(G * G).reshape(1, G, G)
    v = p.set_visits(BOUNDARY[(cell + np.arange(n)[:, None, None]) % 10])
    assert np.array_equal(np_(p.b.get_state()["visits"]), v)
    # a second import over the first one's counts, every cell at another value
    v = p.set_visits(BOUNDARY[(cell + 3 + np.arange(n)[:, None, None]) % 10])
    assert np.array_equal(np_(p.b.get_state()["visits"]), v)
    p.check_state()
    p.close()


@pytest.mark.parametrize("whole_batch", [True, False], ids=["whole_batch", "a_few_envs"])
@pytest.mark.parametrize("n,codes,kernel", KERNELS)
def test_stale_bytes_across_auto_reset(n, codes, kernel, whole_batch):
    """the first episode leaves exact counts of 100 and more behind (never cleared); after the
    auto-reset (every env at once: the lane-per-env path, whose map scratch is vx; a few envs,
    one or two per block: the cooperative path with prefetched records) a count of 14
    injected everywhere makes every move a 15th visit, which must overwrite its cell's
    stale count"""
    p = Pair(n, codes, kernel)
    p.set_visits(100)
    assert p.step(10) == 0
    if whole_batch:
        steps = np.full(n, 999, np.int32)
    else:
        steps = np_(p.b.get_state(parts=("scalars",))["scalars"])[:, O.S_STEP].copy()
        steps[[1, 64 + 7, 64 + 40, n - 1]] = 999  # one done env in a block, two in the next, the last env
    p.set_steps(steps)
    assert p.step(1) == (n if whole_batch else 4)
    p.check_state()
    p.set_visits(14)
    p.step(20)
    assert (p.ov.b.visits >= 16).any()  # (a cell entered twice: its fresh count bumped)
    p.check_state()
    p.close()


def test_mcts_clone_reads_the_counts():
    """the MCTS clone's exact counts (its rollouts move to the least-visited neighbour) of
    a handle carrying 15, 200, 270 and 300, bumped by a few steps: every search equals the
    oracle's on the exported state"""
    from plantos_amd.mcts import MCTS
    p = Pair(N_TWIN, True, TWIN)
    n = p.n
    cell = np.arange(G * G).reshape(1, G, G)
    p.set_visits(np.array([15, 200, 270, 300], np.int32)[(cell + cell // G + np.arange(n)[:, None, None]) % 4])
    assert p.step(6) == 0
    p.check_state()
    st = p.b.get_state()
    cells, visits, expl, sc = (np_(st[k]) for k in ("cells", "visits", "explored", "scalars"))
    m = MCTS(p.b, n_simulations=20, max_depth=30, seed=77)
    a, order, cv, cval = m.search(root_stats=True)
    torch.cuda.synchronize()
    a, order, cv, cval = np_(a), np_(order), np_(cv), np_(cval)
    cfg = O.config(*CFG)
    for e in range(n):
        r = O.NpMT(77 + e)
        oa, oo, ocv, ocval = O.mcts_search(cfg, cells[e], visits[e], expl[e], sc[e], r, 20, 1.414, 30)
        assert oa == a[e] and (oo == order[e]).all() and (ocv == cv[e]).all() and (ocval == cval[e]).all(), e
    m.close()
    p.close()
