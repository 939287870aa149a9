"""Non-default rules for the parity tests (TEST INFRA): reward presets, a helper
that leaves an oracle env one move away from termination, and the checked hand-over
of the oracle's state to a GPU batch.

Why `adv`: the step reward is float32(f64 sum of r_step, one action outcome and,
when the map completes, r_complete).  With the reference's presets a sum carried in
f32 rounds to the same float32 in all 12 cases, and r_invalid == r_water_empty hides
a swap of those two branches; `adv` has 12 distinct float32 sums, more than half of
which differ between the two summations (tests/test_rules_presets.py).
"""
import numpy as np

from oracle import oracle as O
from oracle_rollout import OracleVec

REWARD_KEYS = ("r_goal", "r_mistake", "r_invalid", "r_water_empty", "r_step", "r_exploration", "r_revisit",
               "r_complete")


def _preset(goal, mistake, invalid, water_empty, step, exploration, revisit, complete):
    return dict(zip(REWARD_KEYS, (goal, mistake, invalid, water_empty, step, exploration, revisit, complete)))


PRESETS = {
    "default": _preset(20.0, -10.0, -5.0, -5.0, -0.1, 10.0, -1.0, 50.0),   # plantos_env.py:76-83
    "alt": _preset(50.0, -5.0, -2.0, -5.0, -0.05, 5.0, -0.5, 200.0),       # commented out in the reference
    "old": _preset(200.0, -20.0, -11.0, -20.0, -0.1, 10.0, -3.0, 100.0),
    "adv": _preset(0.7, -0.3, -1.1, -0.9, -0.01, 0.3, -0.07, 33.301),
}

# the six action outcomes of a step (plantos_env.py:166-222)
OUTCOMES = ("r_goal", "r_mistake", "r_invalid", "r_water_empty", "r_exploration", "r_revisit")


def step_rewards(rules, bonus=(False, True)):
    """The possible step rewards as f64 sums in the reference's order:
    (r_step + outcome) [+ r_complete]."""
    out = []
    for k in OUTCOMES:
        for b in bonus:
            r = rules["r_step"] + rules[k]
            if b:
                r += rules["r_complete"]
            out.append(r)
    return np.array(out, np.float64)


def step_rewards_f32(rules):
    """The same sums carried in float32 (what a kernel must NOT do)."""
    out = []
    for k in OUTCOMES:
        for b in (False, True):
            r = np.float32(rules["r_step"]) + np.float32(rules[k])
            if b:
                r = np.float32(r + np.float32(rules["r_complete"]))
            out.append(r)
    return np.array(out, np.float32)


DIRS = ((-1, 0), (0, 1), (1, 0), (0, -1))  # N, E, S, W (plantos_env.py:186)
PE_EMPTY, PE_OBST = 0, 1


def inject_last_cell(ov, envs):
    """Leave each listed env of the OracleVec `ov` one move away from a fully explored
    map: the first in-grid neighbour (N/E/S/W) of the rover is cleared and is the only
    unexplored, never-visited non-obstacle cell.  Returns the action per env that moves
    into it (terminates with r_step + r_exploration + r_complete)."""
    b = ov.b
    G = b.cfg.grid_size
    acts = np.zeros(len(envs), np.int32)
    for i, e in enumerate(envs):
        x, y = int(b.scal[e, O.S_X]), int(b.scal[e, O.S_Y])
        for a, (dx, dy) in enumerate(DIRS):
            nx, ny = x + dx, y + dy
            if 0 <= nx < G and 0 <= ny < G:
                break
        else:
            raise AssertionError("no neighbour inside the grid")
        b.cells[e, nx, ny] = PE_EMPTY
        free = b.cells[e] != PE_OBST
        b.visits[e][free] = 1
        b.explored[e][free] = 1
        b.visits[e, nx, ny] = 0
        b.explored[e, nx, ny] = 0
        b.explored[e, x, y] = 2
        acts[i] = a
    return acts


def info_rows(b, idx):
    """terminal_info rows (PE_I_* order) of envs `idx` of an oracle Batch"""
    rows = np.zeros((len(idx), 11), np.int32)
    for k, e in enumerate(idx):
        th, hy, tot, ex, tc = b.info(e)
        s = b.scal[e]
        rows[k] = [s[O.S_X], s[O.S_Y], th, hy, tot, s[O.S_STEP], ex, tc, s[O.S_COLLIDED], s[O.S_COLL], s[O.S_POISONED]]
    return rows


class Twin:
    """The oracle side of a GPU-vs-oracle rollout under given rules: an OracleVec of envs
    0..n-1, the action rule of the rules tests (an env standing on a plant waters when a seeded
    host draw is below 0.5), every output a GPU step has to reproduce, and the bookkeeping for
    the conditions on the inputs (which rewards occurred, which plants were watered)."""

    def __init__(self, cfg, n, seed, max_steps, p, rules, water_seed=9, map_algo=0):
        self.cfg, self.n, self.seed, self.max_steps, self.p, self.rules = cfg, n, seed, max_steps, p, rules
        self.ov = OracleVec(cfg, np.arange(n), seed, max_steps=max_steps, map_algo=map_algo, thirsty_plant_prob=p,
                            **rules)
        self.wrng = np.random.default_rng(water_seed)
        self.seen = set()       # f64 step rewards that occurred
        self.watered = np.zeros((n, cfg[0], cfg[0]), bool)  # plants watered in the current episode
        self.n_term = self.n_trunc = 0

    def set_steps(self, start):
        self.ov.b.scal[:, O.S_STEP] = start

    def _at_rover(self):
        b = self.ov.b
        return b.cells[np.arange(self.n), b.scal[:, O.S_X], b.scal[:, O.S_Y]]

    def actions(self, synth):
        """the synthetic actions, with action 4 where an env stands on a plant and the draw says so"""
        a = np.array(synth, np.int32)
        draw = self.wrng.random(self.n) < 0.5
        a[(self._at_rover() >= 2) & draw] = 4
        return a

    def step(self, a, autoreset=True):
        """(obs, f64 reward, terminated, truncated, done idx, terminal obs, returns, lengths,
        terminal info rows of the done envs) -- obs holds the fresh rows of auto-reset envs"""
        ov, b = self.ov, self.ov.b
        e_all = np.arange(self.n)
        x, y, pre = b.scal[:, O.S_X].copy(), b.scal[:, O.S_Y].copy(), self._at_rover()
        obs, rew, te, tr = b.step(a)
        self.watered[e_all, x, y] |= (np.asarray(a) >= 4) & (pre == 3)
        self.seen.update(rew.tolist())
        self.n_term += int(te.sum())
        self.n_trunc += int((tr & ~te).sum())
        done = te | tr
        didx = np.nonzero(done)[0]
        info = info_rows(b, didx)
        tobs = obs.copy()
        ov.ret += rew
        ret, ln = ov.ret.copy(), b.scal[:, O.S_STEP].copy()
        if autoreset:
            for k in didx:
                b.reset_philox(int(k), self.seed, int(k), int(b.scal[k, O.S_EPISODE]))
                ov.ret[k] = 0.0
                self.watered[k] = False
            if len(didx):
                obs[done] = b.obs(didx)[done]
        return obs, rew, te, tr, didx, tobs, ret, ln, info

    def plant_census(self):
        """(thirsty plants, hydrated plants that were never watered) over the oracle's cells"""
        c = self.ov.b.cells
        return int((c == 3).sum()), int(((c == 2) & ~self.watered).sum())

    def assert_input_conditions(self, outcomes=True):
        """The run exercised what it is there for: every non-bonus reward value that the rules
        allow occurred, and the maps hold the plants that thirsty_plant_prob implies."""
        thirsty, dry_hyd = self.plant_census()
        if self.p == 0.0:
            assert thirsty == 0 and dry_hyd > 0, (thirsty, dry_hyd)
        elif self.p == 1.0:
            assert dry_hyd == 0 and thirsty > 0, (thirsty, dry_hyd)
        else:
            assert thirsty > 0 and dry_hyd > 0, (thirsty, dry_hyd)
        if outcomes:
            want = set(step_rewards(self.rules, bonus=(False,)).tolist())
            if self.p == 0.0:  # no plant is ever thirsty: r_goal cannot occur
                want.discard(self.rules["r_step"] + self.rules["r_goal"])
            assert want <= self.seen, sorted(want - self.seen)


def np_(t):
    return t.detach().cpu().numpy()


def compare_step(b, out, want, tag, f_obs=None):
    """One GPU step's outputs (`out` = PlantOSBatch.step's return) against Twin.step's `want`:
    obs (codes expanded), reward as float32(oracle f64), both flags; for the done envs the
    terminal obs, terminal info, f64 return and length -- all bit for bit."""
    obs, rew, te, tr = out
    o_obs, o_rew, o_te, o_tr, didx, o_tobs, o_ret, o_len, o_info = want
    if b.obs_codes:  # the step wrote byte codes: expand them (pe_expand_obs_codes)
        obs = b.expand_codes(b.io, 1, f_obs)[0]
    g_rew = np_(rew)
    bad = np.nonzero(g_rew != o_rew.astype(np.float32))[0]
    assert len(bad) == 0, (tag, "reward", bad[:8].tolist(), g_rew[bad[:8]].tolist(), o_rew[bad[:8]].tolist())
    g_te, g_tr = np_(te).astype(bool), np_(tr).astype(bool)
    assert (g_te == o_te).all(), (tag, "terminated", np.nonzero(g_te != o_te)[0][:8].tolist())
    assert (g_tr == o_tr).all(), (tag, "truncated", np.nonzero(g_tr != o_tr)[0][:8].tolist())
    bad = np.nonzero((np_(obs) != o_obs).any(1))[0]
    assert len(bad) == 0, (tag, "obs", bad[:8].tolist())
    if len(didx):
        for name, got, exp in (("terminal_obs", b.terminal_obs, o_tobs), ("episode_return", b.episode_return, o_ret),
                               ("episode_length", b.episode_length, o_len)):
            g = np_(got)[didx]
            e = exp[didx]
            bad = np.nonzero((g != e).reshape(len(didx), -1).any(1))[0]
            assert len(bad) == 0, (tag, name, didx[bad[:8]].tolist())
        g = np_(b.terminal_info)[didx]
        bad = np.nonzero((g != o_info).any(1))[0]
        assert len(bad) == 0, (tag, "terminal_info", didx[bad[:8]].tolist(), g[bad[:2]].tolist(),
                               o_info[bad[:2]].tolist())


STATE_KEYS = ("cells", "visits", "explored", "scalars")


def snapshot(ov):
    """Copies of the oracle's four state arrays, under get_state()'s names."""
    b = ov.b
    return {"cells": b.cells.copy(), "visits": b.visits.copy(), "explored": b.explored.copy(),
            "scalars": b.scal.copy()}


def compare_state(b, want, tag):
    """b.get_state() against the oracle's four arrays (`want`: an OracleVec or a snapshot())"""
    if not isinstance(want, dict):
        want = snapshot(want)
    got = b.get_state()
    for k in STATE_KEYS:
        g = np_(got[k])
        bad = np.nonzero((g != want[k]).reshape(len(g), -1).any(1))[0]
        assert len(bad) == 0, (tag, k, bad[:8].tolist())


def make_batch(cfg, n, seed, max_steps, p, rules, **kw):
    from plantos_amd import PlantOSBatch
    G, P, Ob, R, C = cfg
    return PlantOSBatch(n, grid_size=G, num_plants=P, num_obstacles=Ob, lidar_range=R, lidar_channels=C, seed=seed,
                        device="cuda:0", max_steps=max_steps, thirsty_plant_prob=p, rewards=rules, **kw)


def push(ov, b, before=None):
    """The oracle's state into the GPU batch `b`.  First the batch's own state is read back
    and must equal the oracle's -- `before` (a snapshot() taken ahead of the caller's edits of
    the oracle), or the oracle's arrays as they are when nothing was edited -- so that a state
    bug left by the steps before cannot be overwritten unseen; then set_state()."""
    compare_state(b, ov if before is None else before, "before the push")
    ob = ov.b
    b.set_state(ob.cells, ob.visits, ob.explored, ob.scal)


# ---------------------------------------------------------------- the rules rollouts
# (test_gpu_rules.py runs them on the GPU; test_rules_presets.py checks their input
# conditions with the oracle alone)
CFG = {
    "g20": (20, 10, 12, 6, 16), "g64": (64, 100, 120, 6, 64), "g7": (7, 3, 3, 3, 12), "g32": (32, 20, 30, 9, 24),
    "g21": (21, 8, 50, 2, 10), "g25": (25, 10, 12, 6, 16), "g15": (15, 6, 8, 4, 16), "g12r2": (12, 4, 6, 2, 10),
    "g64r32": (64, 100, 120, 32, 64), "g30r2": (30, 12, 40, 2, 10), "g16c40": (16, 6, 8, 5, 40),
    "g40c48": (40, 100, 120, 8, 48), "g25r4": (25, 10, 12, 4, 16), "g8r12": (8, 3, 3, 12, 16),
    "g8r20": (8, 3, 3, 20, 16), "g24c100": (24, 10, 12, 8, 100),
}  # the geometries of test_gpu_parity.CFG and test_gpu_coop_reset.CFG, by their names there

KERNELS = {
    "g20": "pe_step_quad<C16,R6,1word,W8,E16>", "g25": "pe_step_quad<C16,R6>",
    "g64": "pe_step_quad<C64,R6,bytetile>", "g21": "pe_step_quad<C10,R2>", "g12r2": "pe_step_quad<C10,R2,1word>",
    "g30r2": "pe_step_quad<C10,R2>", "g15": "pe_step_quad<C16,R4,1word>", "g25r4": "pe_step_quad<C16,R4>",
    "g64r32": "pe_step_far<C64,R32,bytetile>", "g7": "pe_step_quad<runtime C,R,1word>",
    "g32": "pe_step_quad<runtime C,R>", "g8r12": "pe_step_quad<runtime C,R,1word>", "g24c100": "pe_step_wave",
    "g8r20": "pe_step_wave", "g16c40": "pe_step_quad<runtime C,R,1word,bytetile>",
    "g40c48": "pe_step_quad<runtime C,R,bytetile>",
}
G20_BY_N = {4200: "pe_step_quad<C16,R6,1word,E16>", 8256: "pe_step_quad<C16,R6,1word,E32>",
            32855: "pe_step_quad<C16,R6,1word>"}
CODES_KERNELS = {"g20": "pe_step_quad<C16,R6,1word,bytetile>"}  # (the others are byte-coded already)


def kernel_of(name, n=133, codes=False):
    if codes and name in CODES_KERNELS:
        return CODES_KERNELS[name]
    if name == "g20" and n in G20_BY_N:
        return G20_BY_N[n]
    return KERNELS[name]


def rules_case(name, n=133, codes=False, preset="adv", p=0.25, max_steps=1000, coop=None, every=None, seed=31,
               steps=40):
    return dict(name=name, n=n, codes=codes, preset=preset, p=p, max_steps=max_steps, coop=coop, every=every,
                seed=seed, steps=steps)


def case_id(c):
    s = f"{c['name']}-n{c['n']}-{c['preset']}-p{c['p']}-ms{c['max_steps']}"
    if c["codes"]:
        s += "-codes"
    if c["coop"] is not None:
        s += f"-coop{c['coop']}"
    if c["every"] is not None:
        s += f"-every{c['every']}"
    return s


# every kernel family once: adv rewards, a quarter of the plants thirsty
FAMILY_CASES = (
    [rules_case("g20"), rules_case("g20", n=4200), rules_case("g20", n=8256)] +
    [rules_case(g) for g in ("g25", "g64", "g21", "g12r2", "g30r2", "g15", "g25r4", "g64r32", "g7", "g32", "g8r12",
                             "g16c40", "g40c48", "g24c100", "g8r20")] +
    [rules_case(g, codes=True) for g in ("g20", "g64", "g16c40", "g64r32")])
# the other presets, both ends of thirsty_plant_prob, episodes of 1 and 3 steps and every forced reset path
SWEEP_GEOMS = ("g20", "g64", "g21", "g7", "g24c100", "g64r32")
SWEEP_CASES = []
for _g in SWEEP_GEOMS:
    SWEEP_CASES += [rules_case(_g, preset="alt", p=0.0), rules_case(_g, preset="old", p=1.0),
                    rules_case(_g, max_steps=1), rules_case(_g, max_steps=3)]
    for _p in (0.0, 0.25, 1.0):
        SWEEP_CASES += [rules_case(_g, p=_p, coop=0), rules_case(_g, p=_p, coop=64), rules_case(_g, p=_p, every=0),
                        rules_case(_g, p=_p, every=1)]
RULES_CASES = FAMILY_CASES + SWEEP_CASES
ASEED = 31  # synth_actions' seed


def rules_twin(c):
    """the oracle twin of a rules case, desynchronized: env e starts at step
    max_steps - 1 - k(e), k in [0, 30), so that resets fall inside the window"""
    tw = Twin(CFG[c["name"]], c["n"], c["seed"], c["max_steps"], c["p"], PRESETS[c["preset"]])
    start = np.clip(c["max_steps"] - 1 - np.random.default_rng(5).integers(0, 30, c["n"]), 0, None).astype(np.int32)
    tw.set_steps(start)
    return tw, start


def rules_conditions(c, tw):
    """what a finished rules rollout must have exercised (asserted by the GPU test and, with
    the oracle alone, by the host test)"""
    # episodes of 1 or 3 steps start beside no plant: the action outcomes cannot all occur
    tw.assert_input_conditions(outcomes=c["max_steps"] >= 1000)
    assert tw.n_trunc >= c["n"] and tw.n_term == 0  # every env reset in the window, by truncation
    if c["max_steps"] == 1:
        assert tw.n_trunc == c["n"] * c["steps"]


def host_synth(n, t):
    return np.array([O.synth_action(ASEED, e, t) for e in range(n)], np.int32)
