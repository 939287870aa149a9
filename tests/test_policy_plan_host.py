"""Policy creation's decisions without a GPU: pe_internal_policy_plan (csrc/pe_policy_plan.hpp:
everything pe_policy_create / pe_policy_create_lstm decide before their first allocation, as a
function of the obs length, the batch size, the CU count and the net) against two records that
the code under test did not produce:

- tests/golden/policy_plan_parent.json: the env tile Policy / RecurrentPolicy got, or the
  ValueError their constructors raised, on an MI355X with the library of the commit before these
  decisions moved into the plan (tools/gen_golden_policy_plan.py), over a sweep that crosses
  every branch of the plan;
- the documented layouts, restated here in Python: the LDS images, the packed weight buffer and
  the LSTM state.
"""
import json
import os

from plantos_amd import _capi as C
from plantos_amd import policy as P

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(REPO, "tests", "golden", "policy_plan_parent.json")) as _f:
    GOLDEN = json.load(_f)
CUS = GOLDEN["cu_count"]


def planned(case, cus=CUS):
    """(the constructors' outcome in the fixture's form, the plan's info or None): their own
    argument checks in their order, then the library's plan where they go on to create"""
    try:
        lstms = None
        if case["hidden"] is not None:
            lstms = P._lstm_structs(P.check_lstm_hidden(case["hidden"]), len(case["towers"]))
        towers = P.check_towers(case["towers"])
        if case["activation"] not in P.ACTIVATIONS:
            raise ValueError(f"activation must be one of {sorted(P.ACTIVATIONS)}")
        info = C.policy_plan(case["obs_dim"], case["n"], cus, lstms, P._tower_structs(towers),
                             P.ACTIVATIONS[case["activation"]], case["env_tile"])
    except ValueError as e:
        return {"error": str(e)}, None
    return {"result": info.env_tile}, info


def recorded(case):
    return {k: case[k] for k in ("result", "error") if k in case}


def test_fixture_crosses_the_plan():
    cases = GOLDEN["cases"]
    ok = [c for c in cases if "result" in c]
    # both tiles, chosen and asked for, feed-forward and recurrent, one and two towers, 1..3 hidden layers
    for rec in (False, True):
        for asked in (0, 32, 64):
            for nt in (1, 2):
                got = {c["result"] for c in ok if (c["hidden"] is not None) == rec and c["env_tile"] == asked
                       and len(c["towers"]) == nt}
                assert got == ({asked} if asked else {32, 64}), (rec, asked, nt)
    assert {1, 2, 3} == {len(t) - 1 for c in ok for t in c["towers"]}
    assert {32, 256, 288, 512} <= {w for c in ok for t in c["towers"] for w in t[:-1]}
    assert {32, 256, 512} == {c["hidden"] for c in ok if c["hidden"] is not None}
    assert len({c["obs_dim"] for c in ok}) >= 2
    # the automatic rule flips between 64 CUs - 1 and 64 CUs envs
    auto = {(c["n"], c["result"]) for c in ok if c["env_tile"] == 0 and c["towers"] == [[32, 5]] and c["geometry"] == "g20"}
    assert {(64, 32), (64 * CUS - 1, 32), (64 * CUS, 64)} <= auto
    # D = 107: 64 envs fit beside hidden buffers of 256 rows and not of 288
    by = {(c["n"], json.dumps(c["towers"])): c for c in cases if c["geometry"] == "g20" and c["hidden"] is None
          and c["env_tile"] == 64}
    assert by[(64, "[[256, 256, 5], [256, 256, 1]]")]["result"] == 64 and "error" in by[(64, "[[288, 5]]")]
    # the 32-env tile that does not fit either
    assert any("error" in c and c["env_tile"] == 32 and c["obs_dim"] >= 265 for c in cases)
    errors = {c["error"] for c in cases if "error" in c}
    assert len(errors) == 8, errors
    for part in ("K-streamed", "activation must be", "head must have", "env_tile must be 0, 32 or 64",
                 "pe_policy_create: the env tile's activations do not fit",
                 "pe_policy_create_lstm: the env tile's obs, h and activation images do not fit"):
        assert any(part in e for e in errors), part


def test_plan_reproduces_the_parent():
    bad = [(c, got) for c in GOLDEN["cases"] for got in [planned(c)[0]] if got != recorded(c)]
    assert not bad, (len(bad), bad[:3])


def test_plan_depends_on_the_cu_count():
    case = dict(hidden=None, towers=[[32, 5]], activation="tanh", env_tile=0, obs_dim=107, n=64 * 100)
    assert planned(case, 100)[0] == {"result": 64} and planned(case, 101)[0] == {"result": 32}
    assert planned(case, 0)[0] == {"result": 64}  # (an unknown CU count counts as one)


def packed_floats(obs_dim, hidden, towers):
    """the packed buffer (include/plantos_batch.h): per LSTM tower the gate weights over
    the chain [obs padded to 8 | h] and the summed biases; per layer N rows of K padded to 8
    (heads: K as it is) and the bias rounded up to 4 floats"""
    total = 0
    if hidden:
        kp0 = (obs_dim + 7) // 8 * 8
        total += len(towers) * (4 * hidden * (kp0 + hidden) + 4 * hidden)
    for t in towers:
        k = hidden or obs_dim
        for i, n in enumerate(t):
            total += n * (k if i == len(t) - 1 else (k + 7) // 8 * 8) + (n + 3) // 4 * 4
            k = n
    return total


def test_sizes_equal_the_documented_layouts():
    seen = 0
    for c in GOLDEN["cases"]:
        got, info = planned(c)
        if info is None:
            continue
        E, D, H, nt = info.env_tile, c["obs_dim"], c["hidden"] or 0, len(c["towers"])
        kp0 = (D + 7) // 8 * 8
        hb = max([w for t in c["towers"] for w in t[:-1]] + [H, D | 1])
        assert info.lds_bytes == 4 * (256 + E * (9 + kp0 + 2 * hb)) <= 160 * 1024, c
        assert info.packed_floats == packed_floats(D, H, c["towers"]), c
        state = 2 * nt * ((c["n"] + E - 1) // E) * H * E
        assert info.state_floats == state // (2 * nt), c
        seen += 1
    assert seen == sum("result" in c for c in GOLDEN["cases"])
