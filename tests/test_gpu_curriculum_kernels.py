"""GPU parity of EVERY step-kernel family with the batched CurriculumWrapper on
(pe_curriculum_enable), against the oracle twin of tests/curriculum_cases.py.

With st.cur set the step kernels take paths that nothing else runs: a done env stores its
last move and watering (the visit counts are carried), those stores are ordered before the
info rows are read and before the reset rewrites the rows, the LDS-DMA staging of the env's
rows is off, and a reset -- lane-per-env, wave-cooperative or a taken prefetched record --
may keep the visit rows of the episode before (copied from visit slot episode-1 into slot
episode, explored bitmap restarted).  tests/test_gpu_curriculum_autoreset.py reaches them on
three kernels, with episodes of 1000 steps: one truncation per env, never a time-out, never
max_threshold, a dozen carried cells, no count past 15.  Here the episodes are 20 steps long
(curriculum_cases.cur_case), so in ~120 steps every env resets at least twice; thresholds sit
at k, k+3 and k+6 explored cells of the most common map size, 3 episodes per maze:

  1. every family of rules_util.FAMILY_CASES once (a2c: the threshold terminates), their
     sizes and code-mode entries, and the headline 64-env kernel (32855 envs); the kernel is
     asserted by name.  No geometry refuses the curriculum together with obs_codes.
  2. the trainingCode variant (the threshold only marks the maze completed).
  3. every reset path forced (coop_max_done 0 / 64, prefetch_every 0 / 1), and a synchronized
     start, where whole blocks finish on one step.  The API does not report taken records;
     that records are taken with `keep` follows from prefetch_every = 1 (a record is ready
     for every env on every step) and the twin's count of keep resets (>= n/2).
  4. carried counts past 15 (every fourth env walks back and forth; 6 episodes of 40 steps
     per maze), the state read back at two points mid-run and at the end.
  5. a masked reset() mid-run whose mask holds completed mazes, envs that carry their counts
     (keep) and envs one episode from the time-out, through both reset kernels.

Every step, bit for bit: obs (codes expanded), reward as float32(f64), both flags; for the done
envs the terminal obs, terminal info, f64 return and length.  At the end: get_curriculum()
(thresholds with tolerance 0, the four counters) and the whole state.  What each case must
have exercised is asserted on the twin's counters (curriculum_cases.conditions; on the host
alone in tests/test_curriculum_cases.py).

Mutation check (scratch builds of the library, MI355X; failing ids of the 70 here / of the 13
curriculum ids the suite had before, in test_gpu_curriculum_autoreset, test_gpu_coop_reset and
test_gpu_vec_env):
  coop_apply_reset copies from slot s.episode      55 / 6   (pass: pe_step_wave's ids and the
                                                             coop_max_done = 0 ids, which never
                                                             run the cooperative reset)
  pct > thr in curriculum_hit                      68 / 3   (pass: two over15 ids)
  on_maze > cur_max_eps in curriculum_on_reset     65 / 0   (pass: the over15 ids, no time-out)
  commit stores without `&& !st.cur`, sector       51 / 4   (every sector-kernel id)
  ... far kernel                                    9 / 2   (the nine g64r32 ids, no other)
  ... wave kernel                                  10 / 0   (the ten g24c100 / g8r20 ids, no other)
Unmutated: 70 passed in 18.5 s, the slowest id (over15-g20-n32855) 3.4 s, the host twin's time.
"""
import pytest

import curriculum_cases as CC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", CC.CASES, ids=CC.case_id)
def test_curriculum_kernel_parity(case):
    tw = CC.run_case(case, gpu=True)
    CC.conditions(case, tw)
