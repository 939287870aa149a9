"""GPU parity of every step-kernel family under NON-DEFAULT rules (pe_device.hpp Rules: the
eight f64 rewards, p_thirsty, max_steps) against the oracle given the same po_config.

Every other GPU test runs the reference's default rules, whose rewards cannot tell
"summed in f64, cast once" from a sum carried in f32, nor r_invalid from r_water_empty
(rules_util.py, test_rules_presets.py).  Here the batches are built with
PlantOSBatch(rewards=..., thirsty_plant_prob=..., max_steps=...): the `adv` preset, whose 12
possible step rewards are 12 distinct float32 values, the reference's two other presets,
thirsty_plant_prob 0 / 0.25 / 1 (read by the lane reset, the cooperative reset and the
prefetch kernel), episodes of 1 and 3 steps (every env truncates every step / every third),
and every reset path forced through coop_max_done / prefetch_every.

Shape of test_gpu_coop_reset._desync_run: 133 envs (two 64-env blocks and a ragged one; the
headline geometry also at the 16- and 32-env workgroup sizes), 40 steps, each env starting
within 30 steps of its truncation.  Actions are pe_synth_actions', except that an env standing
on a plant waters when a seeded host draw is below 0.5 -- which reaches r_goal and r_mistake
without waiting for luck.  Every step: obs (expanded from codes in code mode), reward, both
flags, and the terminal obs / info / f64 return / length of the done envs; at the end the
whole state.  The conditions on the inputs (all six action outcomes occurred, the plants that
thirsty_plant_prob implies are on the maps, every env reset) are asserted on the oracle.
"""
import pytest
import torch

import rules_util as U

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", U.RULES_CASES, ids=U.case_id)
def test_rules_rollout_parity(case):
    c = case
    n = c["n"]
    tw, start = U.rules_twin(c)
    b = U.make_batch(U.CFG[c["name"]], n, c["seed"], c["max_steps"], c["p"], U.PRESETS[c["preset"]],
                     coop_max_done=c["coop"], prefetch_every=c["every"], obs_codes=c["codes"])
    assert b.kernel_name == U.kernel_of(c["name"], n, c["codes"]), b.kernel_name
    f_obs = torch.empty((n, b.obs_dim), dtype=torch.float32, device="cuda:0") if c["codes"] else None
    sc = U.np_(b.get_state(parts=("scalars",))["scalars"])
    sc[:, U.O.S_STEP] = start
    b.set_state(scalars=sc)
    # the batch was created by the rules under test: its maps carry thirsty_plant_prob already
    U.compare_state(b, tw.ov, "create")
    act = torch.empty(n, dtype=torch.int32, device="cuda:0")
    for t in range(c["steps"]):
        b.synth_actions(U.ASEED, t, out=act)
        a = tw.actions(U.np_(act))
        out = b.step(torch.as_tensor(a, device="cuda:0"))
        U.compare_step(b, out, tw.step(a), (U.case_id(c), t), f_obs)
    U.compare_state(b, tw.ov, "end")
    U.rules_conditions(c, tw)
    b.close()
