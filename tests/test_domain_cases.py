"""The domain cases (tests/domain_cases.py) without a device: the case table reaches, together
with the older tables, every (kernel, row-word class) and (kernel, reset path, map generator)
that the plan can give over a sample of the accepted geometry domain; the table agrees with the
plan; and each case's run, on the oracle twin alone, exercises what the case is there for."""
import pytest

import domain_cases as D

# features of the lattice that no table reaches.  Allowed only where the plan rejects every
# lattice geometry with the feature -- which cannot hold for a feature found by planning one, so
# the table stays empty
EXCLUDED = {}


def test_every_reachable_feature_is_reached():
    lat, rejected = D.lattice_features()
    assert len(lat) >= 60 and rejected > 0  # (the lattice crosses G + 2R <= 256 and the LDS limits)
    have = D.features_of(D.today()) | D.features_of(D.case_table())
    missing = {f: lat[f][:3] for f in lat if f not in have and f not in EXCLUDED}
    assert not missing, missing
    assert not EXCLUDED


def test_cases_add_what_the_older_tables_lack():
    """the cases are there for the features the older tables do not reach: each row-word class up
    to 8 words on every sector kernel, the in-place lane-per-env reset and the maze on every family"""
    new = D.features_of(D.case_table()) - D.features_of(D.today())
    assert len(new) >= 30, len(new)
    assert ("kw", D.WAVE, "5-8") in new and ("kra", D.FAR, D.HBM, "maze") in new
    ids = [D.case_id(c) for c in D.CASES]
    assert len(set(ids)) == len(ids)
    assert {"G128P100O120R6C64-codes", "G128P20O30R9C24-codes"} <= set(ids)
    cur = [c for c in D.CASES if c["cur"]]
    assert len(cur) == 4
    assert any(c["wpr"] == "5-8" for c in cur) and any(c["algo"] == "maze" for c in cur)
    assert any(c["cfg"][1] > 128 for c in cur)


@pytest.mark.parametrize("c", D.CASES, ids=D.case_id)
def test_plan_and_table_agree(c):
    info = D.plan_of(c["cfg"], c["algo"], D.N, c["codes"])
    assert info.kernel_name.decode() == c["kernel"]
    assert D.reset_path(c["cfg"], info) == c["path"]
    assert D.wpr_class(c["cfg"][0], c["cfg"][3]) == c["wpr"]
    if c["path"] != D.COOP:  # no cooperative reset: no prefetched records either
        assert info.coop_max_done == 0 and info.prefetch_every == 0


@pytest.mark.parametrize("c", D.CASES, ids=D.case_id)
def test_case_conditions(c):
    D.conditions(c, D.run_case(c))
