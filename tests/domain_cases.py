"""Parity over the whole geometry domain that pe_create accepts (TEST INFRA): grid_size up to
128, lidar_range up to 64 (G + 2R <= 256: up to 8 row words), more than 128 plants, the maze on
every step-kernel family, and the small corners G = 1..4 and C < 4.

  features()   what a geometry exercises, from the device-free plan: the step kernel with its
               row-word class, and the kernel with the path its auto-resets take and the map
               generator.
  lattice()    the sample of the domain (LATTICE_G x LATTICE_R x LATTICE_C, few and many plants,
               both map generators) over which tests/test_domain_cases.py shows that every
               reachable feature is reached by a geometry of an older table (today()) or of CASES.
  CASES        the new GPU cases: hand-picked edges, and a greedy cover (toward the largest G) of
               the lattice features that neither today() nor the edges reach.
  run_case()   one case on the oracle twin alone (test_domain_cases.py: the conditions) or on the
               twin and a GPU batch (test_gpu_domain.py), every step compared bit for bit, with a
               masked reset, a load_maps and a set_state(visits) mid-run on both sides.
"""
import numpy as np

import curriculum_cases as CC
import rules_util as U
from oracle import oracle as O
from plantos_amd import _capi as C

N = 133        # two full 64-env workgroups and a ragged third
SEED = 47      # the batches' seed
LOAD_SEED = 1047  # the seed of the layouts that load_maps installs
CUS = 256
ALGOS = ("original", "maze")


# ---------------------------------------------------------------- features
def plan_of(cfg, algo="original", n=N, codes=False):
    """pe_internal_plan of a geometry (raises ValueError where pe_create would)"""
    G, P, Ob, R, Ch = cfg
    c = C.default_config(G, P, Ob, R, Ch)
    c.map_generation_algo = C.MAP_ALGOS[algo]
    c.obs_codes = int(codes)
    return C.plan(c, n, CUS)


def kernel_base(name):
    """the plan's kernel name without the workgroup-shape suffixes of small batches"""
    for s in (",W8", ",E16", ",E32"):
        name = name.replace(s, "")
    return name


def row_words(G, R):
    return (2 * (G + 2 * R) + 63) // 64


def wpr_class(G, R):
    w = row_words(G, R)
    return "1" if w == 1 else ("2" if w == 2 else ("3-4" if w <= 4 else "5-8"))


def reset_scratch_bytes(G, WPR, P):
    """pe_device.hpp reset_scratch_bytes / maze_scratch_bytes"""
    maze = (((G - 1) // 6) ** 2 + 3) // 4
    return 8 + G * WPR * 8 + max(2 * P, maze)


def reset_path(cfg, info):
    """Where an auto-reset of the planned step kernel generates the map:
    coop      the wave-cooperative reset (the plan's coop_max_done > 0; above that many done envs
              per block the lane-per-env reset of the same kernel);
    lane-lds  one lane per env, the map built in the env's obs-tile row in LDS: the sector kernels
              with an f32 tile that can hold the image (pe_quad_done.hpp quad_done_path:
              scratch_ok = !BT && reset_scratch_bytes(G, WPR, P) <= 4 D);
    lane-hbm  one lane per env, the map built in place (pe_device.hpp reset_env): the byte-tile
              sector kernels and pe_step_far (the same line), and pe_step_wave, whose lane 0 runs
              reset_env whenever the plan has no cooperative reset (pe_step_wave.hpp wave_done)."""
    G, P, _, R, Ch = cfg
    if info.coop_max_done > 0:
        return "coop"
    if info.kernel_name.decode() == "pe_step_wave":
        return "lane-hbm"
    D = 5 * Ch + 27
    return "lane-lds" if not info.tile_codes and reset_scratch_bytes(G, row_words(G, R), P) <= 4 * D else "lane-hbm"


def features(cfg, algo="original", n=N, codes=False):
    info = plan_of(cfg, algo, n, codes)
    k = kernel_base(info.kernel_name.decode())
    return {("kw", k, wpr_class(cfg[0], cfg[3])), ("kra", k, reset_path(cfg, info), algo)}


# ---------------------------------------------------------------- the lattice
LATTICE_G = (1, 2, 3, 4, 5, 7, 8, 12, 15, 16, 20, 21, 24, 25, 30, 32, 33, 40, 48, 52, 53, 64, 65, 96, 100, 128)
LATTICE_R = (1, 2, 4, 6, 9, 12, 14, 15, 20, 32, 33, 48, 64)
LATTICE_C = (1, 3, 4, 10, 16, 24, 32, 33, 40, 48, 64, 65, 100, 120)


def lattice():
    """(cfg, algo) over the sample; geometries that pe_create rejects included (the closure test
    skips them and counts them)"""
    for G in LATTICE_G:
        plants = [max(0, min(3, G * G - 2))] + ([129] if G >= 32 else [])
        for R in LATTICE_R:
            for Ch in LATTICE_C:
                for P in plants:
                    for algo in ALGOS:
                        if algo == "maze" and G < 7:
                            continue
                        yield (G, P, 12 if G >= 8 else 0, R, Ch), algo


def lattice_features():
    """{feature: [(cfg, algo), ...]} over the lattice, and the number of rejected geometries"""
    out, rejected = {}, 0
    for cfg, algo in lattice():
        try:
            fs = features(cfg, algo)
        except ValueError:
            rejected += 1
            continue
        for f in fs:
            out.setdefault(f, []).append((cfg, algo))
    return out, rejected


def today():
    """(cfg, algo, n, codes) of the tables that predate this module: rules_util.CFG with its batch
    sizes and code-mode entries, the four lists of test_gpu_geometry_sweep.py with its code-mode
    list, and the three maze rollouts of test_gpu_maze.py"""
    import test_gpu_geometry_sweep as GS
    import test_gpu_maze as GM
    out = [(U.CFG[g], "original", 133, False) for g in U.CFG]
    out += [(U.CFG["g20"], "original", n, False) for n in U.G20_BY_N]
    out += [(U.CFG[c["name"]], "original", c["n"], True) for c in U.FAMILY_CASES if c["codes"]]
    out += [(g, "original", 133, False) for g in GS.GEOS + GS.WIDE + GS.FAR + GS.MIXED]
    out += [(g, "original", 133, True) for g in GS.CODES]
    out += [(GM.CFG[g], "maze", n, False) for g, n in (("g20", 2048), ("g7fallback", 300), ("g64", 128))]
    return out


def features_of(table):
    out = set()
    for cfg, algo, n, codes in table:
        out |= features(cfg, algo, n, codes)
    return out


# ---------------------------------------------------------------- the cases
def dom_case(cfg, kernel, wpr, path, algo="original", codes=False, cur=False, steps=40):
    """kernel, wpr, path: the plan's kernel name at n = 133, the row-word class and the reset
    path, written out (test_domain_cases.py holds them against the plan); codes: obs_codes;
    cur: the curriculum (a2c) with thresholds in explored cells (curriculum_cases.K_CELLS style)."""
    return dict(cfg=cfg, kernel=kernel, wpr=wpr, path=path, algo=algo, codes=codes, cur=cur, steps=steps)


def case_id(c):
    return ("G{}P{}O{}R{}C{}".format(*c["cfg"]) + ("-maze" if c["algo"] == "maze" else "") +
            ("-codes" if c["codes"] else "") + ("-cur" if c["cur"] else ""))


WAVE, HBM, LDS, COOP = "pe_step_wave", "lane-hbm", "lane-lds", "coop"
RT, RT_BT = "pe_step_quad<runtime C,R>", "pe_step_quad<runtime C,R,bytetile>"
C64, FAR = "pe_step_quad<C64,R6,bytetile>", "pe_step_far<C64,R32,bytetile>"
HEAD = "pe_step_quad<C16,R6,1word,W8,E16>"

# the edges picked by hand.  Code mode where the plan accepts it and keeps the kernel (the byte-tile
# kernels), and on (128, 20, 30, 9, 24), which then runs the byte-tile twin of its f32 kernel.
EDGES = [
    dom_case((128, 20, 30, 64, 16), WAVE, "5-8", HBM, cur=True),          # 8 row words, R = 64
    dom_case((8, 3, 3, 64, 16), WAVE, "5-8", HBM),                        # the window far wider than the map
    dom_case((64, 100, 120, 33, 64), WAVE, "5-8", HBM),                   # one past the far kernel's range
    dom_case((100, 200, 300, 20, 16), WAVE, "5-8", HBM),                  # P > 128
    dom_case((32, 129, 30, 9, 24), RT, "2", HBM, cur=True),               # P > 128: picks in the explored words
    dom_case((20, 150, 12, 6, 16), HEAD, "1", HBM),                       # P > 128 on the headline kernel
    dom_case((1, 0, 0, 1, 1), WAVE, "1", COOP),                           # one cell, no plant
    dom_case((1, 0, 0, 2, 4), "pe_step_quad<runtime C,R,1word>", "1", COOP),
    dom_case((2, 1, 0, 3, 4), "pe_step_quad<runtime C,R,1word>", "1", COOP),
    dom_case((3, 2, 0, 2, 8), "pe_step_quad<runtime C,R,1word>", "1", COOP),
    dom_case((4, 3, 0, 6, 16), HEAD, "1", COOP),
    dom_case((20, 5, 12, 6, 2), WAVE, "1", COOP),                         # C < 4
    dom_case((30, 10, 12, 7, 120), WAVE, "2", HBM),                       # C = 120 at R <= 7
    dom_case((128, 100, 120, 6, 64), C64, "5-8", HBM, codes=True),
    dom_case((128, 20, 30, 9, 24), RT, "5-8", HBM),
    dom_case((128, 20, 30, 9, 24), RT_BT, "5-8", HBM, codes=True),
]
# the greedy cover of the lattice features that neither TODAY nor EDGES reach: at every turn the
# lattice geometry with the most features still missing, ties toward the largest G, then the maze
COVER = [
    dom_case((128, 3, 12, 14, 64), RT_BT, "5-8", HBM, algo="maze", codes=True),
    dom_case((128, 3, 12, 6, 16), "pe_step_quad<C16,R6>", "5-8", HBM, algo="maze", cur=True),
    dom_case((128, 3, 12, 4, 16), "pe_step_quad<C16,R4>", "5-8", HBM, algo="maze"),
    dom_case((128, 3, 12, 2, 10), "pe_step_quad<C10,R2>", "5-8", HBM, algo="maze"),
    dom_case((100, 3, 12, 14, 32), RT, "3-4", HBM, algo="maze", cur=True),
    dom_case((100, 3, 12, 6, 16), "pe_step_quad<C16,R6>", "3-4", HBM),
    dom_case((100, 3, 12, 4, 16), "pe_step_quad<C16,R4>", "3-4", HBM),
    dom_case((100, 3, 12, 2, 10), "pe_step_quad<C10,R2>", "3-4", HBM),
    dom_case((25, 3, 12, 2, 32), RT, "1", LDS, algo="maze"),
    dom_case((24, 3, 12, 4, 16), "pe_step_quad<C16,R4>", "1", LDS, algo="maze"),
    dom_case((128, 3, 12, 64, 100), WAVE, "5-8", HBM, algo="maze"),
    dom_case((128, 3, 12, 14, 64), RT_BT, "5-8", HBM, codes=True),
    dom_case((64, 3, 12, 32, 64), FAR, "3-4", HBM, algo="maze", codes=True),
    dom_case((64, 129, 12, 32, 64), FAR, "3-4", HBM, codes=True),
    dom_case((52, 3, 12, 6, 64), C64, "2", HBM, algo="maze", codes=True),
    dom_case((25, 3, 12, 6, 16), "pe_step_quad<C16,R6>", "2", LDS, algo="maze"),
    dom_case((25, 3, 12, 2, 64), RT_BT, "1", HBM, algo="maze", codes=True),
    dom_case((25, 3, 12, 2, 10), "pe_step_quad<C10,R2>", "1", LDS, algo="maze"),
    dom_case((20, 3, 12, 6, 64), C64, "1", HBM, algo="maze", codes=True),
    dom_case((20, 3, 12, 6, 48), "pe_step_quad<runtime C,R,1word,bytetile>", "1", HBM, algo="maze", codes=True),
    dom_case((20, 3, 12, 4, 16), "pe_step_quad<C16,R4,1word>", "1", LDS, algo="maze"),
    dom_case((20, 3, 12, 2, 10), "pe_step_quad<C10,R2,1word>", "1", LDS, algo="maze"),
]
CASES = EDGES + COVER


def case_table(cases=None):
    return [(c["cfg"], c["algo"], N, c["codes"]) for c in (CASES if cases is None else cases)]


# ---------------------------------------------------------------- the run
MAX_STEPS = 12   # episodes of at most 12 steps: every env resets several times in 40 steps
SPREAD = 10      # env e starts at step MAX_STEPS - 1 - k(e), k in [0, SPREAD)
MASK_AT, LOAD_AT, VISITS_AT = 14, 24, 32
K_CELLS, INC_CELLS, MAX_EPS = 9, 3, 3   # the curriculum cases' first threshold and its increment, in explored cells
# distinct f64 step rewards of a case's run: at least 4, except where fewer are reachable (allowed
# at G <= 2 and G = 128 only) -- there exactly the twin's count.  One cell: the first step ends the
# episode (the map is explored) with a blocked move or an empty watering, plus r_complete.
MIN_REWARDS = 4
FEWER_REWARDS = {"G1P0O0R1C1": 2, "G1P0O0R2C4": 2}


class Side:
    """The oracle side of a case: rules_util.Twin (a quarter of the plants thirsty), or
    curriculum_cases.CurriculumTwin for the curriculum cases, behind one interface; the `adv`
    rewards on both."""

    def __init__(self, c):
        from collections import Counter
        self.cur = c["cur"]
        algo = 1 if c["algo"] == "maze" else 0
        if self.cur:
            tw = CC.CurriculumTwin(c["cfg"], N, SEED, max_steps=MAX_STEPS, max_eps=MAX_EPS, terminate=True,
                                   map_algo=algo)
            for k, v in U.PRESETS["adv"].items():  # (the rewards take no part in the maps drawn above)
                setattr(tw.c, k, v)
            T = Counter(tw.totals().tolist()).most_common(1)[0][0]
            initial, inc = (K_CELLS / T) * 100, (INC_CELLS / T) * 100
            tw.set_thresholds(initial, inc, (initial + inc) + inc)
            self.bt = tw.b
        else:
            tw = U.Twin(c["cfg"], N, SEED, MAX_STEPS, 0.25, U.PRESETS["adv"], map_algo=algo)
            self.bt = tw.ov.b
        self.tw = tw

    def snapshot(self):
        b = self.bt
        return {"cells": b.cells.copy(), "visits": b.visits.copy(), "explored": b.explored.copy(),
                "scalars": b.scal.copy()}

    def actions(self, synth):
        return np.array(synth, np.int32) if self.cur else self.tw.actions(synth)

    def _reset_env(self, e, seed):
        """one env's reset() on the map stream of `seed`; its reset obs (curriculum: the fresh map's,
        before the carried counts are put back)"""
        tw, b = self.tw, self.bt
        if self.cur:
            keep, tw.seed = tw.seed, seed
            try:
                return tw.reset_env(e)
            finally:
                tw.seed = keep
        b.reset_philox(e, seed, e, int(b.scal[e, O.S_EPISODE]))
        tw.ov.ret[e] = 0.0
        tw.watered[e] = False
        return b.obs([e])[e]

    def reset(self, mask):
        """pe_reset(mask): the obs of every env, the masked ones' fresh"""
        rows = {int(e): self._reset_env(int(e), SEED) for e in np.nonzero(mask)[0]}
        obs = self.bt.obs([e for e in range(N) if e not in rows])
        for e, r in rows.items():
            obs[e] = r
        return obs

    def load(self, idx):
        """pe_load_maps of layouts that the oracle's reset_philox draws under LOAD_SEED for (env,
        episode counter): (cells [k, G, G], rover [k, 2], reset obs [k, D]).  The twin takes the
        same layouts through its own reset logic (a curriculum env may carry its counts over)."""
        obs = np.array([self._reset_env(int(e), LOAD_SEED) for e in idx])
        return self.bt.cells[idx].copy(), self.bt.scal[idx, :2].copy(), obs


def pick_envs(rng, fresh, parity, frac=None, k=None):
    """a seeded subset (a mask of about `frac` of the envs, or `k` shuffled indices).  Where the
    batch holds them, the subset gets an env of either parity of the episode counter (an odd and
    an even number of resets before: the two visit slots), an env standing on a fresh map (step 0)
    and one in mid-episode: the first env of a kind that the draw missed is added."""
    n = len(fresh)
    sel = rng.random(n) < frac if k is None else np.isin(np.arange(n), rng.permutation(n)[:k])
    for kind in (fresh, ~fresh, parity, ~parity):
        if not (sel & kind).any() and kind.any():
            sel[np.nonzero(kind)[0][0]] = True
    return sel


def kinds_of(sel, fresh, parity):
    """(inside the subset, outside it) per kind"""
    return {name: (int((sel & kind).sum()), int((~sel & kind).sum()))
            for name, kind in (("fresh", fresh), ("mid", ~fresh), ("odd", parity), ("even", ~parity))}


def make_batch(c):
    from plantos_amd import PlantOSBatch
    G, P, Ob, R, Ch = c["cfg"]
    kw = dict(grid_size=G, num_plants=P, num_obstacles=Ob, lidar_range=R, lidar_channels=Ch, seed=SEED,
              device="cuda:0", max_steps=MAX_STEPS, map_generation_algo=c["algo"], obs_codes=c["codes"])
    if not c["cur"]:
        kw["thirsty_plant_prob"] = 0.25
    return PlantOSBatch(N, rewards=U.PRESETS["adv"], **kw)


def _rows_equal(got, want, tag, idx=None):
    bad = np.nonzero((got != want).reshape(len(want), -1).any(1))[0]
    assert len(bad) == 0, (tag, (bad if idx is None else np.asarray(idx)[bad])[:8].tolist())


def run_case(c, gpu=None):
    """One case on the twin; with gpu=True also on a PlantOSBatch, bit for bit: at creation
    get_state (all four parts) and the obs of reset(mask = 0); every step through
    rules_util.compare_step; the obs of the masked reset before step MASK_AT, the rows load_maps
    returns before step LOAD_AT, set_state(visits) before step VISITS_AT (a seeded tenth of the
    visited cells raised to counts in 16..40: the overflow array and the explored bitmap); at the
    end the state, get_info and the curriculum records.  Returns what the run exercised."""
    tag = case_id(c)
    side = Side(c)
    tw, bt = side.tw, side.bt
    b = act = f_obs = None
    if gpu:
        import torch
        b = make_batch(c)
        assert b.kernel_name == c["kernel"], b.kernel_name
        U.compare_state(b, side.snapshot(), (tag, "creation"))
        _rows_equal(U.np_(b.reset(mask=np.zeros(N, np.uint8))), bt.obs(), (tag, "reset(mask = 0) obs"))
    if c["cur"]:
        obs0 = tw.reset()
        if gpu:
            b.enable_curriculum("a2c", initial_threshold=float(tw.thr[0]), threshold_increment=tw.inc,
                                max_threshold=tw.maximum, max_episodes_per_maze=MAX_EPS)
            _rows_equal(U.np_(b.reset()), obs0, (tag, "reset() obs"))
    start = (MAX_STEPS - 1 - np.random.default_rng(5).integers(0, SPREAD, N)).astype(np.int32)
    bt.scal[:, O.S_STEP] = start
    if gpu:
        sc = U.np_(b.get_state(parts=("scalars",))["scalars"])
        sc[:, O.S_STEP] = start
        b.set_state(scalars=sc)
        act = torch.empty(N, dtype=torch.int32, device="cuda:0")
        f_obs = torch.empty((N, b.obs_dim), dtype=torch.float32, device="cuda:0") if c["codes"] else None
    out = dict(resets=np.zeros(N, np.int64), rewards=set(), raised=0)
    for t in range(c["steps"]):
        fresh, parity = bt.scal[:, O.S_STEP] == 0, (bt.scal[:, O.S_EPISODE] & 1) == 1
        if t == MASK_AT:
            mask = pick_envs(np.random.default_rng(MASK_AT), fresh, parity, frac=0.25)
            out["mask"] = kinds_of(mask, fresh, parity)
            want = side.reset(mask)
            if gpu:
                _rows_equal(U.np_(b.reset(torch.as_tensor(mask))), want, (tag, "masked reset obs"))
        if t == LOAD_AT:
            sel = pick_envs(np.random.default_rng(LOAD_AT), fresh, parity, k=20)
            idx = np.random.default_rng(LOAD_AT + 1).permutation(np.nonzero(sel)[0])
            out["load"] = kinds_of(sel, fresh, parity)
            cells, rover, want = side.load(idx)
            if gpu:
                _rows_equal(U.np_(b.load_maps(idx, cells, rover)), want, (tag, "load_maps obs"), idx)
        if t == VISITS_AT:
            rng = np.random.default_rng(VISITS_AT)
            raise_ = (bt.visits > 0) & (rng.random(bt.visits.shape) < 0.1)
            bt.visits[raise_] = rng.integers(16, 41, int(raise_.sum()))
            out["raised"] = int(raise_.sum())
            if gpu:
                b.set_state(visits=bt.visits)
        if gpu:
            b.synth_actions(U.ASEED, t, out=act)
            a = side.actions(U.np_(act))
            got = b.step(torch.as_tensor(a, device="cuda:0"))
            want = tw.step(a)
            U.compare_step(b, got, want, (tag, t), f_obs)
        else:
            want = tw.step(side.actions(U.host_synth(N, t)))
        out["rewards"].update(want[1].tolist())
        out["resets"][want[4]] += 1
    if gpu:
        U.compare_state(b, side.snapshot(), (tag, "end"))
        _rows_equal(U.np_(b.get_info()), U.info_rows(bt, np.arange(N)), (tag, "get_info"))
        if c["cur"]:
            CC.compare_curriculum(b, tw, (tag, "end"))
        assert b.poll_errors() & 4 == 0, (tag, "F_NOROOM")
        b.close()
    out["keep_over15"] = tw.n_keep_over15 if c["cur"] else None
    return out


def conditions(c, out):
    """What a finished case must have exercised (asserted by the GPU test and, with the twin
    alone, by the host test).  No F_NOROOM: the twin's resets raise where a map has no room."""
    assert out["resets"].min() >= 2, out["resets"].min()   # every env auto-reset at least twice
    G = c["cfg"][0]
    for k in ("mask", "load"):
        # Envs that had reset before and envs that had not: with episodes of at most 12 steps every
        # env has auto-reset once by step 10, so "before" is counted in resets -- the subset holds
        # envs with an odd and with an even number of resets behind them (the two visit slots: a
        # reset writes the slot that the episode before it left), and so does its complement.
        # (G = 1: one cell, every step ends the episode, every env has the same count.)
        m = out[k]
        if G > 1:
            assert min(m["odd"]) >= 1 and min(m["even"]) >= 1, (k, m)
        assert sum(m["odd"]) + sum(m["even"]) == N and m["odd"][0] + m["even"][0] >= 20, (k, m)
    assert out["raised"] >= 10, out["raised"]
    if case_id(c) in FEWER_REWARDS:
        assert G <= 2 or G == 128
        assert len(out["rewards"]) == FEWER_REWARDS[case_id(c)], sorted(out["rewards"])
    else:
        assert len(out["rewards"]) >= MIN_REWARDS, sorted(out["rewards"])
    if c["cur"]:
        assert out["keep_over15"] >= 1, out["keep_over15"]   # a carried reset holding a count above 15
