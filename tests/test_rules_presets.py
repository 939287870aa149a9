"""Why the non-default-rules GPU tests (test_gpu_rules.py, test_gpu_termination.py) use the
`adv` reward preset, recorded as a host test: the reference's presets cannot tell a reward
summed in f32 from float32(f64 sum), nor r_invalid from r_water_empty; `adv` can.  Plus the
test infrastructure's own behaviour on the oracle (no GPU)."""
import numpy as np
import pytest

from oracle import oracle as O
from oracle_rollout import OracleVec
from rules_util import (CFG, FAMILY_CASES, PRESETS, REWARD_KEYS, RULES_CASES, case_id, host_synth, inject_last_cell,
                        rules_conditions, rules_twin, step_rewards, step_rewards_f32)


def counts(rules):
    f64 = step_rewards(rules).astype(np.float32)
    f32 = step_rewards_f32(rules)
    return len(set(f64.tolist())), int((f64 != f32).sum())


def test_adv_preset_separates_what_the_defaults_cannot():
    assert len(step_rewards(PRESETS["adv"])) == 12
    distinct, differ = counts(PRESETS["adv"])
    assert distinct == 12   # every (outcome, bonus) pair has its own float32 reward
    assert differ >= 6      # an f32 summation gives another float32 in at least half of them
    assert counts(PRESETS["default"]) == (10, 0)
    # the presets the reference keeps commented out are as blind to the summation type
    assert counts(PRESETS["alt"])[1] == 0


def test_presets_name_every_reward_of_the_oracle_config():
    fields = {f[0] for f in O.POConfig._fields_ if f[0].startswith("r_")}
    for name, p in PRESETS.items():
        assert set(p) == fields == set(REWARD_KEYS), name
    c = O.config(20, 10, 12, 6, 16)
    assert {k: getattr(c, k) for k in REWARD_KEYS} == PRESETS["default"]


def test_oracle_vec_takes_rules():
    ov = OracleVec((12, 4, 6, 2, 10), np.arange(3), 1, max_steps=7, thirsty_plant_prob=0.25, **PRESETS["adv"])
    assert ov.cfg.max_steps == 7 and ov.cfg.thirsty_plant_prob == 0.25
    assert {k: getattr(ov.cfg, k) for k in REWARD_KEYS} == PRESETS["adv"]
    with pytest.raises(TypeError):
        OracleVec((12, 4, 6, 2, 10), np.arange(3), 1, grid_size=3)  # not a rule: refused, not set silently


@pytest.mark.parametrize("cfg", [(20, 10, 12, 6, 16), (7, 3, 3, 3, 12), (12, 4, 6, 2, 10)])
def test_inject_last_cell_terminates_every_env(cfg):
    """64 freshly reset envs, none skipped: each terminates on the returned action and takes
    the bonus once -- float32(r_step + r_exploration + r_complete) is 33.591."""
    n = 64
    adv = PRESETS["adv"]
    ov = OracleVec(cfg, np.arange(n), 3, max_steps=50, **adv)
    acts = inject_last_cell(ov, np.arange(n))
    obs, rew, te, tr, tobs, ret, ln = ov.step(acts)
    assert te.all() and not tr.any()
    assert (rew == (adv["r_step"] + adv["r_exploration"]) + adv["r_complete"]).all()
    assert (rew.astype(np.float32) == np.float32(33.591)).all()
    assert (ov.b.scal[:, O.S_EPISODE] == 2).all() and (ov.b.scal[:, O.S_BONUS] == 0).all()  # reset after it


def _oracle_key(c):
    return tuple(c[k] for k in ("name", "n", "preset", "p", "max_steps", "seed", "steps"))


# one oracle run per distinct input (the forced reset paths and code mode share theirs)
ORACLE_RUNS = list({_oracle_key(c): c for c in RULES_CASES}.values())


@pytest.mark.parametrize("case", ORACLE_RUNS, ids=case_id)
def test_rules_rollouts_exercise_what_they_claim(case):
    """The input conditions of test_gpu_rules.py, with the oracle alone: all six action
    outcomes occur in every family's run, the maps hold no thirsty plant at p = 0, no
    never-watered hydrated one at p = 1 and both at 0.25, every env resets in the window."""
    tw, start = rules_twin(case)
    assert (start >= 0).all() and (case["max_steps"] - 1 - start < 30).all()
    for t in range(case["steps"]):
        tw.step(tw.actions(host_synth(case["n"], t)))
    rules_conditions(case, tw)


def test_rules_cases_cover_the_issue():
    fam = {(c["name"], c["n"], c["codes"]) for c in FAMILY_CASES}
    assert {("g20", 133, False), ("g20", 4200, False), ("g20", 8256, False)} <= fam
    assert {g for g, n, codes in fam if not codes} == set(CFG)
    assert {g for g, n, codes in fam if codes} == {"g20", "g64", "g16c40", "g64r32"}
    assert len(RULES_CASES) == len(FAMILY_CASES) + 6 * 16
