"""The curriculum parity cases (TEST INFRA): the batched CurriculumWrapper
(pe_curriculum_enable) on every step-kernel family, with episodes short enough that the
paths only it uses run many times -- carried visits, time-outs, the threshold ladder up to
max_threshold, carried counts past 15, a masked pe_reset mid-run.

  CurriculumTwin      the oracle side: test_oracle_curriculum.OracleCurriculumVec restated
                      with a `carry` flag per env in place of the per-step copy of every env's
                      visit counts (the persistent copy always equals the live counts: it is
                      taken at the first reset on a maze and refreshed after every step), plus
                      the terminal outputs of rules_util.Twin.step and the counters that the
                      conditions below are asserted on.  tests/test_curriculum_cases.py shows
                      it equal to OracleCurriculumVec and to the reference's recorded runs
                      (tests/golden/curriculum_*.npz).
  CASES               the case table; run_case() drives one case on the twin alone
                      (test_curriculum_cases.py) or on the twin and a GPU batch, comparing
                      every step (test_gpu_curriculum_kernels.py).
  conditions()        what a finished case must have exercised, from the twin's counters.
"""
from collections import Counter

import numpy as np

import rules_util as U
from oracle import oracle as O
from test_oracle_curriculum import OracleCurriculumVec

BLOCK = 64  # envs per workgroup of the sector kernels' largest form


class PhiloxCurriculumVec(OracleCurriculumVec):
    """The same wrapper over the device-rng map stream: env e's k-th map is
    reset_philox(seed, e, k) (what pe_create / pe_reset / the auto-reset draw)."""

    def __init__(self, cfg, n, seed, **kw):
        super().__init__(cfg, n, 0, **kw)
        self.seed = seed
        for e in range(n):
            self.b.reset_philox(e, seed, e, 0)  # pe_create

    def _new_map(self, e):
        self.b.reset_philox(e, self.seed, e, int(self.b.scal[e, O.S_EPISODE]))


class CurriculumTwin:
    """DummyVecEnv([CurriculumWrapper(env)]) over the oracle, flag form (module docstring).
    stream "philox": env e's k-th map is reset_philox(seed, e, k); "cpython": the shared
    CPython stream of the reference's fixtures."""

    def __init__(self, cfg, n, seed, stream="philox", max_steps=None, initial=40.0, maximum=100.0, inc=10.0,
                 max_eps=3, terminate=True, map_algo=0):
        self.c = O.config(*cfg, map_algo=map_algo)
        if max_steps is not None:
            self.c.max_steps = max_steps
        self.b = O.Batch(self.c, n)
        self.n, self.seed, self.stream = n, seed, stream
        self.mt = O.MT(seed) if stream == "cpython" else None
        if stream == "philox":
            for e in range(n):
                self.b.reset_philox(e, seed, e, 0)  # pe_create
        self.thr = np.full(n, float(initial))
        self.maximum, self.inc, self.max_eps, self.terminate = float(maximum), float(inc), max_eps, terminate
        self.episodes = np.zeros(n, np.int64)
        self.successes = np.zeros(n, np.int64)
        self.on_maze = np.zeros(n, np.int64)
        self.completed = np.zeros(n, bool)
        self.carry = np.zeros(n, bool)
        self.ret = np.zeros(n, np.float64)
        self._row = np.zeros(O.obs_dim(self.c), np.float32)
        self._row_p, self._cref, self._addr = self._row.ctypes.data, O.ctypes.byref(self.c), None
        # ---- what the run exercised
        self.resets = np.zeros(n, np.int64)  # auto-resets per env
        self.n_keep = 0           # resets that carried the visit counts over
        self.keep_cells = []      # visited cells of each carried map
        self.n_keep_over15 = 0    # ... whose carried counts hold one above 15
        self.n_timeout = 0        # resets by max_episodes_per_maze alone (maze not completed)
        self.n_completed = 0      # resets of completed mazes (threshold raised)
        self.n_term = self.n_trunc = self.n_both = 0
        self.n_hit = 0            # env-steps at or above the threshold
        self.n_exact = 0          # ... with pct == thr exactly
        self.thr_seen = {float(initial)}
        self.blocks_one = self.blocks_gt8 = 0  # (step, 64-env block) pairs with 1 / more than 8 done envs

    def set_thresholds(self, initial, inc, maximum):
        """before the first reset()"""
        self.thr[:] = initial
        self.inc, self.maximum = float(inc), float(maximum)
        self.thr_seen = {float(initial)}

    def totals(self):
        return (self.b.cells != 1).reshape(self.n, -1).sum(1)

    def _new_map(self, e):
        if self.stream == "cpython":
            self.b.reset_cpython(e, self.mt)
        else:
            b = self.b
            if self._addr is None:  # the arrays are written in place, never replaced
                self._addr = [(a.ctypes.data, a.strides[0]) for a in (b.cells, b.visits, b.explored, b.scal)]
            rc = O.lib().po_reset_philox(self._cref, self.seed, e, int(b.scal[e, O.S_EPISODE]),
                                         *[p + e * s for p, s in self._addr])
            assert rc == 0, "Not enough available positions"

    def _obs_row(self, e):
        if self._addr is None:
            b = self.b
            self._addr = [(a.ctypes.data, a.strides[0]) for a in (b.cells, b.visits, b.explored, b.scal)]
        (pc, sc), (pv, sv), _, (ps, ss) = self._addr
        O.lib().po_obs(self._cref, pc + e * sc, pv + e * sv, ps + e * ss, self._row_p)
        return self._row.copy()

    def reset_env(self, e):
        """CurriculumWrapper.reset (A2C_training.py:56-95); the obs is the fresh map's, computed
        before the carried counts are put back"""
        self.episodes[e] += 1
        self.on_maze[e] += 1
        timeout = self.on_maze[e] >= self.max_eps
        if self.completed[e] or timeout:
            if self.completed[e]:
                self.thr[e] = min(self.thr[e] + self.inc, self.maximum)
                self.thr_seen.add(float(self.thr[e]))
                self.successes[e] += 1
                self.n_completed += 1
            else:
                self.n_timeout += 1
            self.completed[e] = False
            self.on_maze[e] = 0
            self.carry[e] = False
            self._new_map(e)
            obs = self._obs_row(e)
        else:
            old = self.b.visits[e].copy() if self.carry[e] else None
            self._new_map(e)
            obs = self._obs_row(e)
            if old is not None:
                self.b.visits[e] = old
                self.n_keep += 1
                self.keep_cells.append(int((old > 0).sum()))
                self.n_keep_over15 += int((old > 15).any())
            self.carry[e] = True
        self.ret[e] = 0.0
        return obs

    def reset(self, mask=None):
        """reset() of the batch; with a mask, pe_reset's: the masked envs through reset_env, the
        others' obs rebuilt from their current state"""
        return np.array([self.reset_env(e) if mask is None or mask[e] else self._obs_row(e) for e in range(self.n)])

    def set_steps(self, start):
        self.b.scal[:, O.S_STEP] = start

    def fin(self):
        """get_curriculum()'s counters: episodes, successes, episodes on the maze, flags"""
        return np.stack([self.episodes, self.successes, self.on_maze, self.completed.astype(int) | 2 * self.carry], 1)

    def step(self, a):
        """rules_util.Twin.step's tuple: (obs, f64 reward, terminated, truncated, done idx,
        terminal obs, returns, lengths, terminal info rows of the done envs)"""
        b, n = self.b, self.n
        obs, rew, te, tr = b.step(np.asarray(a, np.int64))
        te = te.copy()
        tobs = obs.copy()
        ex = (b.explored > 0).reshape(n, -1).sum(1).astype(np.float64)   # plantos_env.py:320
        tc = (b.cells != 1).reshape(n, -1).sum(1).astype(np.float64)     # :321
        pct = (ex / tc) * 100
        hit = pct >= self.thr                                   # A2C_training.py:101, trainingCode.py:87
        self.completed |= hit
        if self.terminate:                                      # A2C_training.py:103 only
            te |= hit
        self.n_hit += int(hit.sum())
        self.n_exact += int((hit & (pct == self.thr)).sum())
        self.n_term += int(te.sum())
        self.n_trunc += int((tr & ~te).sum())
        self.n_both += int((te & tr).sum())
        done = te | tr
        per_block = np.add.reduceat(done.astype(np.int64), np.arange(0, n, BLOCK))
        self.blocks_one += int((per_block == 1).sum())
        self.blocks_gt8 += int((per_block > 8).sum())
        didx = np.nonzero(done)[0]
        info = U.info_rows(b, didx)
        self.ret += rew
        ret, ln = self.ret.copy(), b.scal[:, O.S_STEP].copy()
        for e in didx:
            obs[e] = self.reset_env(int(e))
        self.resets[didx] += 1
        return obs, rew, te, tr, didx, tobs, ret, ln, info


# ---------------------------------------------------------------- the cases
VARIANTS = {"a2c": True, "trainingCode": False}  # terminate_on_threshold


def cur_case(name, n=133, codes=False, variant="a2c", kind="plan", k=12, inc_cells=3, max_steps=20, max_eps=3,
             steps=120, spread=20, coop=None, every=None, seed=41):
    """kind "plan": the episode plan (thresholds of k, k+3, k+6 explored cells of the most common
    map size, episodes of 20 steps, 3 episodes per maze, env e starting at step
    max_steps - 1 - k(e), k(e) in [0, spread); spread 0: every env at step 0, whole blocks finish
    together).  "over15": every fourth env walks up and down (actions 0 and 2), so carried counts pass 15.
    "masked": a plan run with a masked reset() after MASK_AT steps."""
    return dict(name=name, n=n, codes=codes, variant=variant, kind=kind, k=k, inc_cells=inc_cells,
                max_steps=max_steps, max_eps=max_eps, steps=steps, spread=spread, coop=coop, every=every, seed=seed)


def case_id(c):
    s = f"{c['kind']}-{c['name']}-n{c['n']}-{c['variant']}"
    if c["codes"]:
        s += "-codes"
    if c["spread"] == 0:
        s += "-sync"
    if c["coop"] is not None:
        s += f"-coop{c['coop']}"
    if c["every"] is not None:
        s += f"-every{c['every']}"
    return s


# explored cells of the first threshold, per geometry: few enough that an episode of 20 steps
# reaches it, enough that most do not (tuned with the twin alone; the conditions hold it)
K_CELLS = {"g20": 12, "g25": 12, "g64": 12, "g21": 9, "g12r2": 9, "g30r2": 9, "g15": 11, "g25r4": 11,
           "g64r32": 12, "g7": 9, "g32": 11, "g8r12": 9, "g16c40": 12, "g40c48": 11, "g24c100": 11, "g8r20": 9}
BIG = 32855  # the headline 64-env kernel (rules_util.G20_BY_N)
BIG_STEPS = 45  # the time is the host twin's: the shortest windows in which the conditions still hold
MID_STEPS = 60  # (n = 4200 and 8256)


def _plan(name, n=133, **kw):
    kw.setdefault("k", K_CELLS[name])
    if n == BIG:
        kw.setdefault("steps", BIG_STEPS)
    elif n > 133:
        kw.setdefault("steps", MID_STEPS)
    return cur_case(name, n=n, **kw)


# 1. every family once (a2c): rules_util.FAMILY_CASES' geometries, sizes and code-mode entries, and
#    the headline kernel
FAMILY = [_plan(c["name"], n=c["n"], codes=c["codes"]) for c in U.FAMILY_CASES] + [_plan("g20", n=BIG)]
# 2. the variant whose threshold marks the maze completed and does not terminate
TRAINING_CODE = [_plan(g, variant="trainingCode") for g in U.SWEEP_GEOMS] + [_plan("g20", n=BIG,
                                                                                   variant="trainingCode")]
# 3. every reset path forced, and whole blocks finishing on one step
FORCED = []
for _g in U.SWEEP_GEOMS:
    FORCED += [_plan(_g, coop=0), _plan(_g, coop=64), _plan(_g, every=0), _plan(_g, every=1), _plan(_g, spread=0)]
# 4. carried counts past 15
OVER15 = [cur_case(g, n=n, variant="trainingCode", kind="over15", k=K_CELLS[g], max_steps=40, max_eps=6,
                   steps=130 if n == 133 else 60, spread=40)
          for g, n in (("g20", 133), ("g20", BIG), ("g64", 133), ("g64r32", 133), ("g24c100", 133))]
# 5. a masked pe_reset mid-run (trainingCode: a completed maze stays completed until its episode
#    ends, so the mask can hold one; under a2c the hit ends the episode on the spot), once through
#    the lane-per-env reset kernel.  4 episodes per maze: at the reset, envs in their second
#    episode on a maze carry their counts over (keep) and envs in their third time out
MASKED = ([_plan(g, variant="trainingCode", kind="masked", steps=60, max_eps=4) for g in ("g20", "g64", "g24c100")] +
          [_plan("g20", variant="trainingCode", kind="masked", steps=60, max_eps=4, coop=0),
           _plan("g20", kind="masked", steps=60, max_eps=4)])
MASK_AT = 30
CASES = FAMILY + TRAINING_CODE + FORCED + OVER15 + MASKED


def kernel_of(c):
    return U.kernel_of(c["name"], c["n"], c["codes"])


def host_twin(c):
    """the twin of a case after its first reset(), thresholds and start steps set:
    (twin, reset obs, start steps)"""
    cfg = U.CFG[c["name"]]
    tw = CurriculumTwin(cfg, c["n"], c["seed"], max_steps=c["max_steps"], max_eps=c["max_eps"],
                        terminate=VARIANTS[c["variant"]])
    # obstacles overlap, so the cell totals differ from env to env: thresholds in cells of the
    # most common total land on pct == thr exactly in those envs
    T = Counter(tw.totals().tolist()).most_common(1)[0][0]
    initial = (c["k"] / T) * 100
    inc = (c["inc_cells"] / T) * 100
    tw.T = T
    tw.set_thresholds(initial, inc, (initial + inc) + inc)
    obs0 = tw.reset()
    spread = np.random.default_rng(9).integers(0, c["spread"], c["n"]) if c["spread"] else c["max_steps"] - 1
    start = (c["max_steps"] - 1 - spread) * np.ones(c["n"], np.int32)
    tw.set_steps(start.astype(np.int32))
    return tw, obs0, start.astype(np.int32)


def actions(c, synth, t):
    a = np.array(synth, np.int32)
    if c["kind"] == "over15":
        a[::4] = 0 if t % 2 == 0 else 2  # opposite moves: the env revisits two cells
    return a


def pick_mask(tw):
    """the masked reset's envs, and the three kinds it must hold: completed mazes, carried counts,
    one episode from the time-out; two envs of three, so that each kind also stays unmasked"""
    kinds = {"completed": tw.completed.copy(), "carrying": tw.carry & ~tw.completed,
             "before time-out": (tw.on_maze == tw.max_eps - 1) & ~tw.completed}
    mask = (np.arange(tw.n) % 3 != 0) & (kinds["completed"] | kinds["carrying"] | kinds["before time-out"])
    return mask, kinds


def make_batch(c, tw):
    """the GPU batch of a case, curriculum enabled with the twin's thresholds"""
    from plantos_amd import PlantOSBatch
    G, P, Ob, R, C = U.CFG[c["name"]]
    b = PlantOSBatch(c["n"], grid_size=G, num_plants=P, num_obstacles=Ob, lidar_range=R, lidar_channels=C,
                     seed=c["seed"], device="cuda:0", max_steps=c["max_steps"], coop_max_done=c["coop"],
                     prefetch_every=c["every"], obs_codes=c["codes"])
    b.enable_curriculum(c["variant"], initial_threshold=float(tw.thr[0]), threshold_increment=tw.inc,
                        max_threshold=tw.maximum, max_episodes_per_maze=c["max_eps"])
    return b


def compare_curriculum(b, tw, tag):
    """get_curriculum() against the twin: thresholds with tolerance 0, the four counters"""
    thr, cnt = b.get_curriculum()
    bad = np.nonzero(U.np_(thr) != tw.thr)[0]
    assert len(bad) == 0, (tag, "thresholds", bad[:8].tolist())
    bad = np.nonzero((U.np_(cnt) != tw.fin()).any(1))[0]
    assert len(bad) == 0, (tag, "counters", bad[:8].tolist(), U.np_(cnt)[bad[:2]].tolist(), tw.fin()[bad[:2]].tolist())


def run_case(c, gpu=False):
    """One case on the twin; with gpu=True also on a PlantOSBatch, every step compared bit for
    bit (obs -- codes expanded --, float32(f64 reward), both flags, terminal obs / info / f64
    return / length of the done envs), the state and the curriculum records at the end (kind
    "over15": also at two points mid-run).  Returns the twin."""
    n, tag = c["n"], case_id(c)
    tw, obs0, start = host_twin(c)
    b = act = f_obs = None
    if gpu:
        import torch
        b = make_batch(c, tw)
        assert b.kernel_name == kernel_of(c), b.kernel_name
        assert (U.np_(b.reset()) == obs0).all(), (tag, "reset obs")
        sc = U.np_(b.get_state(parts=("scalars",))["scalars"])
        sc[:, O.S_STEP] = start
        b.set_state(scalars=sc)
        act = torch.empty(n, dtype=torch.int32, device="cuda:0")
        f_obs = torch.empty((n, b.obs_dim), dtype=torch.float32, device="cuda:0") if c["codes"] else None
    mid = (c["steps"] // 3, 2 * c["steps"] // 3) if c["kind"] == "over15" else ()
    tw.mask_kinds = None
    for t in range(c["steps"]):
        if c["kind"] == "masked" and t == MASK_AT:
            mask, kinds = pick_mask(tw)
            tw.mask_kinds = {k: (int((v & mask).sum()), int((v & ~mask).sum())) for k, v in kinds.items()}
            before = (tw.n_keep, tw.n_timeout, tw.n_completed)
            want = tw.reset(mask)
            tw.mask_resets = dict(zip(("keep", "timeout", "completed"),
                                      np.subtract((tw.n_keep, tw.n_timeout, tw.n_completed), before).tolist()))
            if gpu:
                got = U.np_(b.reset(torch.as_tensor(mask)))
                bad = np.nonzero((got != want).any(1))[0]
                assert len(bad) == 0, (tag, "masked reset obs", bad[:8].tolist(), mask[bad[:8]].tolist())
        if gpu:
            b.synth_actions(U.ASEED, t, out=act)
            a = actions(c, U.np_(act), t)
            out = b.step(torch.as_tensor(a, device="cuda:0"))
            U.compare_step(b, out, tw.step(a), (tag, t), f_obs)
        else:
            tw.step(actions(c, U.host_synth(n, t), t))
        if gpu and t in mid:
            U.compare_state(b, tw, (tag, "state after step", t))
            compare_curriculum(b, tw, (tag, t))
    if gpu:
        compare_curriculum(b, tw, (tag, "end"))
        U.compare_state(b, tw, (tag, "end"))
        b.close()
    return tw


def counts(c, tw):
    """the figures the conditions are asserted on"""
    return dict(term=tw.n_term, trunc=tw.n_trunc, both=tw.n_both, hit=tw.n_hit, exact=tw.n_exact, keep=tw.n_keep,
                keep_over15=tw.n_keep_over15, keep_cells_median=int(np.median(tw.keep_cells)) if tw.keep_cells else 0,
                keep_cells_max=max(tw.keep_cells, default=0), timeout=tw.n_timeout, completed_resets=tw.n_completed,
                at_max=int((tw.thr == tw.maximum).sum()), thresholds=len(tw.thr_seen),
                min_resets=int(tw.resets.min()), blocks_one=tw.blocks_one, blocks_gt8=tw.blocks_gt8,
                over15_end=int((tw.b.visits > 15).reshape(tw.n, -1).any(1).sum()), max_count=int(tw.b.visits.max()))


def conditions(c, tw):
    """What a finished case must have exercised (asserted by the GPU test and, with the twin
    alone, by the host test).  The episode-plan conditions hold for kinds "plan" and "masked" up
    to the window: a masked case runs half of it, so it answers for its mask alone."""
    n, k = c["n"], counts(c, tw)
    if c["kind"] == "plan":
        assert k["min_resets"] >= 2, k                 # every env reset at least twice
        assert k["keep"] >= n / 2, k                   # carried visits
        assert k["timeout"] >= n / 4, k                # max_episodes_per_maze ran out
        assert k["at_max"] >= 1 and k["thresholds"] >= 3, k   # the ladder up to max_threshold (the fmin)
        assert k["exact"] >= 1, k                      # pct == thr: >= and > differ
        if VARIANTS[c["variant"]]:
            assert k["term"] >= n / 4, k
            assert k["both"] >= 1, k                   # terminated and truncated on one step (a hit on the last)
        else:
            assert k["term"] == 0 and k["completed_resets"] >= n / 4, k
        assert k["blocks_one"] >= 1, k                 # a block with one done env (the cooperative reset's least)
        if c["spread"] == 0:
            assert k["blocks_gt8"] >= 1, k             # ... and with more than the cooperative reset takes
    elif c["kind"] == "over15":
        assert k["keep_over15"] >= 20 and k["over15_end"] >= 10, k
    else:
        m = tw.mask_kinds
        assert m["carrying"][0] >= 1 and m["before time-out"][0] >= 1, m
        assert m["carrying"][1] >= 1, m                # and the mask is not everyone
        if not VARIANTS[c["variant"]]:
            assert m["completed"][0] >= 1, m
        r = tw.mask_resets  # what the masked reset itself did: carried counts over, timed out, raised thresholds
        assert r["keep"] >= 1 and r["timeout"] >= 1 and (VARIANTS[c["variant"]] or r["completed"] >= 1), r
    return k
