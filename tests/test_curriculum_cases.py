"""Host checks (no GPU) of tests/curriculum_cases.py, the twin and the cases of
tests/test_gpu_curriculum_kernels.py.

- CurriculumTwin, which keeps a `carry` flag per env, equals OracleCurriculumVec, which copies
  every env's visit counts every step as the reference's wrapper does, in every output, every
  counter and the final state (and the copies equal the live counts, which is why a flag is
  enough), and reproduces the reference's six recorded runs (tests/golden/curriculum_*.npz) in
  the assertions of test_oracle_curriculum.py.
- every case reaches what it is there for, by the twin's counters alone (conditions()).
- the cases name every step kernel of rules_util.
"""
import numpy as np
import pytest

import curriculum_cases as CC
import rules_util as U
from golden_util import cfg_tuple, load
from oracle import oracle as O
from test_oracle_curriculum import OracleCurriculumVec


@pytest.mark.parametrize("case", [CC.cur_case("g7", k=9), CC.OVER15[0]], ids=CC.case_id)
def test_flag_twin_equals_the_copying_wrapper(case):
    c = case
    tw, obs0, start = CC.host_twin(c)
    ov = CC.PhiloxCurriculumVec(U.CFG[c["name"]], c["n"], c["seed"], initial=float(tw.thr[0]), maximum=tw.maximum,
                                inc=tw.inc, max_eps=c["max_eps"], terminate=tw.terminate)
    ov.c.max_steps = c["max_steps"]
    assert (ov.reset() == obs0).all()
    ov.b.scal[:, O.S_STEP] = start
    ret = np.zeros(c["n"])
    for t in range(c["steps"]):
        a = CC.actions(c, U.host_synth(c["n"], t), t)
        obs, rew, te, tr, didx, tobs, t_ret, t_len, info = tw.step(a)
        o_obs, o_rew, o_te, o_tr, o_tobs = ov.step(a)
        assert (rew == o_rew).all() and (te == o_te).all() and (tr == o_tr).all(), t
        assert (obs == o_obs).all() and (tobs == o_tobs).all(), t
        assert (didx == np.nonzero(o_te | o_tr)[0]).all()
        ret += o_rew                             # the terminal outputs that the wrapper does not return
        assert (t_ret[didx] == ret[didx]).all(), t
        ret[didx] = 0.0
        carrying = np.array([p is not None for p in ov.persistent])
        assert (carrying == tw.carry).all(), t
        for e in np.nonzero(carrying)[0]:        # the copy is the live counts: a flag says as much
            assert (ov.persistent[e] == ov.b.visits[e]).all(), (t, e)
    for got, want in ((tw.thr, ov.thr), (tw.episodes, ov.episodes), (tw.successes, ov.successes),
                      (tw.on_maze, ov.on_maze), (tw.completed, ov.completed), (tw.b.cells, ov.b.cells),
                      (tw.b.visits, ov.b.visits), (tw.b.explored, ov.b.explored), (tw.b.scal, ov.b.scal)):
        assert (got == want).all()
    CC.conditions(c, tw)


@pytest.mark.parametrize("name", ["curriculum_g20_explore", "curriculum_g7_explore", "curriculum_g20_random",
                                  "curriculum_tc_g20_explore", "curriculum_tc_g7_explore", "curriculum_tc_g20_random"])
def test_flag_twin_matches_reference(name):
    """test_oracle_curriculum.test_curriculum_restatement_matches_reference, on the flag twin"""
    f = load(name)
    T, N = f["actions"].shape
    v = CC.CurriculumTwin(cfg_tuple(f), N, int(f["seed"]), stream="cpython",
                          **OracleCurriculumVec.VARIANTS["tc" if "_tc_" in name else "a2c"])
    assert (v.reset() == f["obs0"]).all()
    for t in range(T):
        obs, rew, te, tr, didx, tobs = v.step(f["actions"][t])[:6]
        assert (rew == f["reward"][t]).all(), t
        assert (te == f["terminated"][t].astype(bool)).all() and (tr == f["truncated"][t].astype(bool)).all(), t
        done = te | tr
        assert (tobs[done] == f["terminal_obs"][t][done]).all(), t
        assert (obs == f["obs"][t]).all(), t
        assert (v.thr == f["threshold"][t]).all(), t
        assert (v.b.visits.reshape(N, -1).sum(1) == f["visits_sum"][t]).all(), t
    assert (v.fin() == f["final_counters"]).all()
    assert v.mt.u32() == int(f["next_u32"])


def _oracle_key(c):
    return tuple(v for k, v in c.items() if k not in ("codes", "coop", "every"))


# one twin run per distinct input (the forced reset paths and code mode share theirs)
ORACLE_RUNS = list({_oracle_key(c): c for c in CC.CASES}.values())


@pytest.mark.parametrize("case", ORACLE_RUNS, ids=CC.case_id)
def test_cases_exercise_what_they_claim(case):
    """The conditions of test_gpu_curriculum_kernels.py with the twin alone: carried visits,
    time-outs, the threshold ladder up to max_threshold, pct == thr, both flags on one step, blocks
    with one done env and with more than 8, counts past 15, what the masked reset holds."""
    tw = CC.run_case(case)
    CC.conditions(case, tw)
    G, _, Ob = U.CFG[case["name"]][:3]
    assert tw.T <= G * G - Ob  # cells of a map size that occurs (obstacles overlap: hardly ever the nominal one)


def test_cases_cover_every_kernel():
    names = set(U.KERNELS.values()) | set(U.G20_BY_N.values()) | set(U.CODES_KERNELS.values())
    for group, variant in ((CC.FAMILY, "a2c"),):
        assert {CC.kernel_of(c) for c in group if c["variant"] == variant} == names
    fam = {(c["name"], c["n"], c["codes"]) for c in CC.FAMILY}
    assert fam == {(c["name"], c["n"], c["codes"]) for c in U.FAMILY_CASES} | {("g20", CC.BIG, False)}
    assert {c["name"] for c in CC.TRAINING_CODE} == set(U.SWEEP_GEOMS) and len(CC.TRAINING_CODE) == 7
    assert len(CC.FORCED) == 5 * len(U.SWEEP_GEOMS)
    for g in U.SWEEP_GEOMS:
        assert {(c["coop"], c["every"], c["spread"]) for c in CC.FORCED if c["name"] == g} == {
            (0, None, 20), (64, None, 20), (None, 0, 20), (None, 1, 20), (None, None, 0)}
    assert {(c["name"], c["n"]) for c in CC.OVER15} == {("g20", 133), ("g20", CC.BIG), ("g64", 133), ("g64r32", 133),
                                                        ("g24c100", 133)}
    assert {c["name"] for c in CC.MASKED} == {"g20", "g64", "g24c100"} and any(c["coop"] == 0 for c in CC.MASKED)
    ids = [CC.case_id(c) for c in CC.CASES]
    assert len(set(ids)) == len(ids)
