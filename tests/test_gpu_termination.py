"""GPU parity of TERMINATIONS inside a block, with the curriculum off.

A random policy never finishes a map, so every auto-reset of the other GPU tests is a
truncation -- which the step kernels predict from the step count and speculate on.  Here
envs are made to terminate (rules_util.inject_last_cell: one unexplored cell left, then the
move into it) beside, below, between and on envs that are about to truncate, under the
`adv` rewards with max_steps = 50.  T: an env made to terminate; P: an env whose step
counter is set to 49, so it truncates in the event step and the kernel can know it.

What the code does with each scenario (pe_step_quad.hpp pe_step_quad, pe_quad_done.hpp
quad_done_path, pe_far.hpp; the tests cannot observe which path a block took, this is read from the code):

  the prediction   pm = __ballot(s.step + 1 >= rl.max_steps); npred (npk) = popcount(pm);
                   ndone = popcount(ballot(terminated || truncated)) after the transition.
  stage_ok         byte-coded kernels with C >= 64 (g64, the runtime byte-tile kernels g16c40 /
                   g40c48) and pe_step_far (g64r32), full blocks only (e0 + 64 <= n: never the
                   ragged group), prefetch on, coop_max_done >= 1: with npred == 1 the commit
                   wave stages P's prefetched record into LDS by LDS-DMA during round 2 (and the
                   info wave P's grid rows, info_reg).  The staged data is used only when
                   `staged = stage_ok && npred == 1 && ndone == 1`.
  kEarlyRec        one-word 64-env kernels with D <= 128 (g15, g12r2, g7; g20 at n > 32768 and,
                   byte-coded, g20 with obs_codes): with npk == 1 the commit wave loads P's
                   record into registers (e_early = P), the info wave P's rows (e_info = P).  The
                   single-done path takes them only if the done env IS e_early (early_hit); the
                   cooperative path (2 <= ndone <= coop_max_done) hands the k-th done env to wave
                   k % 4 and a wave uses its early record only for el == e_early.
  no prediction    the multi-word f32 kernels (g25, g21, g32) and the 16-env workgroups of g20 at
                   n = 279 make none (the round-6 A/B paths that did -- two early records, the
                   register-staged record -- were removed): every done env's record is loaded in
                   the done path.  The scenarios still run there: they pin the unstaged paths, and
                   a later change that adds a prediction meets them.
  pe_step_wave     (g24c100, g8r20) one wave per env, no speculation: `reset_now = done && autoreset`.

  S1  T at 5                 npred 0, ndone 1: nothing staged; the single-done path loads T's record.
  S2  P at 9, T at 3         npred 1 -> P's record staged / early; ndone 2 -> staged = false, the
                             cooperative path: T (the LOWER index) is the 0th done env, P the 1st.
  S3  P at 3, T at 9         the same with T above P.
  S4  P at 2 and 11, T at 6  npred 2: nothing staged (only a single prediction is); ndone 3.
  S5  7 is both P and T      npred 1, ndone 1, the done env is the predicted one: the staged /
                             early record IS used, by an env with terminated and truncated both
                             set, whose return includes r_complete.
  S6  P at 4, T at 20, 40    npred 1, ndone 3, the T envs in other waves' sectors.
  S7  a whole group T        ndone 64 (23 in the ragged group) > coop_max_done = 8: the lane-per-env
                             dense path with terminated flags (g64 / g64r32 / the byte-tile runtime
                             kernels: coop_max_done = 64, so the cooperative path, 16 envs a wave).
  S8  every env T            the same in every block at once.
  S0  P at 7 alone           (after the rotation, with S5 in every block at once) npred 1, ndone 1:
                             the plain predicted truncation, staged data used.

Offsets are within a 64-env group and below 16 (but S6's T), so they share a workgroup in the
16- and 32-env shapes too.  Each round edits the oracle, hands its state to the batch
(rules_util.push, which first checks that the batch still equals the oracle), steps once with
the injected actions (pe_synth_actions' for every other env) and three more times with
synthetic actions -- which checks that the fresh episodes were committed and the prefetch
refills.  All four steps are compared in full, as test_gpu_rules does.
"""
import numpy as np
import pytest
import torch

import rules_util as U
from oracle import oracle as O

pytestmark = pytest.mark.gpu

MAX_STEPS, P_THIRSTY, SEED, N = 50, 0.25, 17, 279
RULES = U.PRESETS["adv"]
R_TERM = np.float32((RULES["r_step"] + RULES["r_exploration"]) + RULES["r_complete"])

# scenario -> (T offsets, P offsets) within a 64-env group
SCEN = {0: ([], [7]), 1: ([5], []), 2: ([3], [9]), 3: ([9], [3]), 4: ([6], [2, 11]), 5: ([7], [7]), 6: ([20, 40], [4]),
        7: (list(range(64)), [])}


def groups_of(n):
    return (n + 63) // 64


def small_plan(n):
    """rounds of {group: scenario}: S1..S6 rotated over the groups, S5 and S0 in every group at
    once, S7 on a full and on the ragged group with quiet neighbours, S8 ("all")"""
    ng = groups_of(n)
    plan = [{g: 1 + (g + r) % 6 for g in range(ng)} for r in range(6)]
    # the one case in which the staged data IS used, in every block at once -- S5, then a plain
    # predicted truncation (P at 7 alone): with prefetch_every = 1 the records are there to take
    plan.append({g: 5 for g in range(ng)})
    plan.append({g: 0 for g in range(ng)})
    plan.append({1: 7, ng - 1: 7})
    plan.append("all")
    seen = {g: set() for g in range(ng)}
    for rnd in plan[:6]:
        for g, k in rnd.items():
            seen[g].add(k)
    assert all(s == {1, 2, 3, 4, 5, 6} for s in seen.values())
    assert n % 64 != 0  # the last group is ragged
    return plan


def big_plan(n):
    ng = groups_of(n)
    return [{g: 1 + g % 7 for g in range(ng)}, {g: 1 + (g + 3) % 7 for g in range(ng)}, "all"]


def envs_of(rnd, n):
    if rnd == "all":
        return np.arange(n), np.zeros(0, np.int64)
    T, P = [], []
    for g, k in sorted(rnd.items()):
        size = min(64, n - 64 * g)
        T += [64 * g + o for o in SCEN[k][0] if o < size]
        P += [64 * g + o for o in SCEN[k][1] if o < size]
    return np.array(T, np.int64), np.array(P, np.int64)


class Run:
    def __init__(self, name, n, codes=False, every=None, autoreset=True):
        self.n, self.name, self.autoreset = n, name, autoreset
        self.tw = U.Twin(U.CFG[name], n, SEED, MAX_STEPS, P_THIRSTY, RULES)
        self.b = U.make_batch(U.CFG[name], n, SEED, MAX_STEPS, P_THIRSTY, RULES, obs_codes=codes,
                              prefetch_every=every, autoreset=autoreset)
        self.f_obs = torch.empty((n, self.b.obs_dim), dtype=torch.float32, device="cuda:0") if codes else None
        self.act = torch.empty(n, dtype=torch.int32, device="cuda:0")
        self.t = 0

    def synth(self):
        self.b.synth_actions(U.ASEED, self.t, out=self.act)
        return U.np_(self.act).copy()

    def step(self, a, tag):
        out = self.b.step(torch.as_tensor(a, device="cuda:0"))
        want = self.tw.step(a, autoreset=self.autoreset)
        U.compare_step(self.b, out, want, (self.name, tag, self.t), self.f_obs)
        self.t += 1
        return want

    def event(self, T, P, tag):
        """edit the oracle (P: step counter 49; T: one cell left), push, step once"""
        ob = self.tw.ov.b
        before = U.snapshot(self.tw.ov)
        ob.scal[P, O.S_STEP] = MAX_STEPS - 1
        t_act = U.inject_last_cell(self.tw.ov, T)
        U.push(self.tw.ov, self.b, before)
        a = self.synth()
        a[T] = t_act
        both = np.intersect1d(T, P)
        obs, rew, te, tr, didx, *_ = self.step(a, tag)
        # the inputs did what the scenario says (oracle side)
        assert te[T].all() and (rew[T].astype(np.float32) == R_TERM).all()
        assert tr[P].all() and tr[both].all() and te[both].all()
        assert (np.sort(didx) == np.union1d(T, P)).all()
        return didx

    def round(self, rnd, tag, follow=3):
        T, P = envs_of(rnd, self.n)
        self.event(T, P, tag)
        for _ in range(follow):
            self.step(self.synth(), tag)

    def close(self):
        U.compare_state(self.b, self.tw.ov, (self.name, "end"))
        self.b.close()


FAMILIES = [  # (geometry, obs_codes)
    ("g20", False), ("g15", False), ("g12r2", False), ("g7", False),   # one-word kernels (g20: 16-env groups here)
    ("g25", False), ("g21", False), ("g32", False),                    # multi-word f32 kernels
    ("g64", False), ("g16c40", False), ("g40c48", False),              # byte-coded, LDS-DMA staging
    ("g64r32", False), ("g24c100", False), ("g8r20", False),           # far, wave
    ("g20", True), ("g64", True),
]


@pytest.mark.parametrize("every", [None, 1], ids=["prefetch_default", "prefetch_every1"])
@pytest.mark.parametrize("name,codes", FAMILIES, ids=[f"{g}{'-codes' if c else ''}" for g, c in FAMILIES])
def test_terminations_inside_blocks(name, codes, every):
    r = Run(name, N, codes, every)
    assert r.b.kernel_name == U.kernel_of(name, N, codes), r.b.kernel_name
    for k, rnd in enumerate(small_plan(N)):
        r.round(rnd, f"round{k}")
    assert r.tw.n_term >= N + 64 + N % 64 + 7 * 5  # S8, S7 twice, one T or more per group and round before
    r.close()


def test_terminations_headline_kernel():
    """the 64-env headline kernel (early record): 513 full blocks and one of 23 envs, three
    rounds -- S1..S7 spread over the blocks twice, then every env at once"""
    n = 32855
    r = Run("g20", n)
    assert U.kernel_of("g20", n) == "pe_step_quad<C16,R6,1word>" == r.b.kernel_name, r.b.kernel_name
    for k, rnd in enumerate(big_plan(n)):
        r.round(rnd, f"round{k}")
    r.close()


@pytest.mark.parametrize("name", ["g20", "g64", "g24c100"])
def test_termination_without_autoreset(name):
    """autoreset=False: S1 and S5, then three more steps on the finished envs -- terminated
    (and S5's truncated) stays set, the bonus is not paid again, PE_S_BONUS stays 1"""
    r = Run(name, N, autoreset=False)
    ng = groups_of(N)
    rnd = {g: (1 if g % 2 == 0 else 5) for g in range(ng)}
    T, P = envs_of(rnd, N)
    r.event(T, P, "event")
    fin = np.union1d(T, P)
    for k in range(3):
        obs, rew, te, tr, *_ = r.step(r.synth(), f"after{k}")
        assert te[T].all() and tr[P].all()
        assert (rew[fin] < 1.0).all()  # no second r_complete (33.301)
        sc = U.np_(r.b.get_state(parts=("scalars",))["scalars"])
        assert (sc[T, O.S_BONUS] == 1).all() and (r.tw.ov.b.scal[T, O.S_BONUS] == 1).all()
    r.close()
