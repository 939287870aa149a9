"""GPU parity of both MCTS search kernels (rl-env_amd/csrc/pe_mcts.hip) at the shapes and budgets
where they can go wrong, every env bit for bit against the oracle (oracle/plantos_mcts.c).

pe_mcts_search_lds_kernel keeps the sim envs in LDS and runs up to G = 29;
pe_mcts_search_kernel keeps them in global memory with an undo log and runs above that
(tests/mcts_cases.py states the 64 KiB rule).  Every test asserts by name which kernel it ran.
Compared per env: the action, the root's children (order, visits, f64 value sums), the np.random
stream after the search, and the live batch state, which a search must leave alone.  What a case
is there for -- the kernel boundary, truncation / termination / watering inside the search on the
product's large grids, masked and chained searches, backpropagation paths of more than 8 nodes,
visit counts around the LDS byte's limit of 31, budgets of 0 -- is asserted from the oracle's
statistics of the very searches compared (mcts_cases.*_conditions; with the oracle alone:
test_mcts_cases.py).

Batches of 70 envs: one full workgroup and a ragged one of 6.
"""
import contextlib

import numpy as np
import pytest
import torch

import mcts_cases as MC
import rules_util as U
from mcts_cases import same_stream
from rules_util import np_

pytestmark = pytest.mark.gpu

SENTINEL = MC.SENTINEL


def gpu_side(cs, tw, before):
    """the GPU batch of a case: the same WARM synthetic steps as the oracle twin took, then the
    oracle's (edited) state pushed over it -- U.push first checks that the batch's own state
    equals the twin's before the edits"""
    n = cs["n"]
    b = U.make_batch(cs["cfg"], n, MC.SEED, cs["max_steps"], cs["p"], U.PRESETS[cs["rules"]])
    acts = torch.empty(n, dtype=torch.int32, device="cuda:0")
    for t in range(MC.WARM):
        b.synth_actions(U.ASEED, t, out=acts)
        b.step(acts)
    U.push(tw.ov, b, before)
    return b


@contextlib.contextmanager
def searcher(cs, b, n_sims=None, depth=None):
    """an MCTS over `b` with the case's budget, asserted to run the case's kernel; closed on the way
    out, also when a comparison fails, so that it never outlives its batch"""
    from plantos_amd.mcts import MCTS
    m = MCTS(b, n_simulations=cs["n_sims"] if n_sims is None else n_sims, c_param=cs["c"],
             max_depth=cs["depth"] if depth is None else depth, seed=cs["mseed"])
    try:
        assert m.kernel_name == cs["kernel"] == MC.expected_kernel(cs["cfg"][0])
        yield m
    finally:
        m.close()


@contextlib.contextmanager
def open_case(cs):
    """(twin, batch, MCTS) of a case; the MCTS, then the batch, closed on the way out"""
    tw, before = MC.host_side(cs)
    b = gpu_side(cs, tw, before)
    try:
        with searcher(cs, b) as m:
            yield tw, b, m
    finally:
        b.close()


def search_and_compare(m, b, ov, rngs, tag, live=None):
    """One GPU search (of the `live` envs, or all) against the oracle's searches from the oracle's
    state; `rngs` (the oracle's streams) advance with it.  Returns the oracle's results and
    statistics (MC.oracle_searches)."""
    n = b.num_envs
    want = MC.oracle_searches(ov, rngs, m.n_simulations, m.c_param, m.max_depth, live)
    m.actions.fill_(SENTINEL)
    a, order, cv, cval = m.search(mask=live, root_stats=True)
    torch.cuda.synchronize()
    a, order, cv, cval = np_(a), np_(order), np_(cv), np_(cval)
    on = np.ones(n, bool) if live is None else np.asarray(live, bool)
    bad = np.nonzero(a != want["action"])[0]  # (masked-out envs: the sentinel on both sides)
    assert len(bad) == 0, (tag, "action", bad[:8].tolist(), a[bad[:8]].tolist(), want["action"][bad[:8]].tolist())
    for name, got in (("order", order), ("visits", cv), ("value", cval)):  # value: f64 sums, bit for bit
        bad = np.nonzero(((got != want[name]).any(1)) & on)[0]
        assert len(bad) == 0, (tag, name, bad[:8].tolist(), got[bad[:2]].tolist(), want[name][bad[:2]].tolist())
    key, pos = m.get_rng_state()
    bad = [e for e in range(n) if not same_stream(key[e], pos[e], *rngs[e].state())]
    assert not bad, (tag, "stream", bad[:8])  # (masked-out envs: neither stream moved)
    U.compare_state(b, ov, f"{tag}: the search left the state alone")
    return want


@pytest.mark.parametrize("cs", MC.BOUNDARY, ids=MC.case_id)
def test_kernel_boundary(cs):
    """G = 28 (LDS, the even dword count padded to an odd stride), 29 (LDS, the largest shape:
    62208 B), 30 (the first global shape: the LDS kernel would need 65792 B) and 32 (global)."""
    G = cs["cfg"][0]
    assert (MC.lds_bytes(G) <= 65536) == (G <= 29) and cs["kernel"] == (MC.LDS_KERNEL if G <= 29 else MC.GLOBAL_KERNEL)
    with open_case(cs) as (tw, b, m):
        search_and_compare(m, b, tw.ov, MC.streams(cs["mseed"]), cs["geom"])


@pytest.mark.parametrize("cs", MC.LARGE, ids=MC.case_id)
def test_global_kernel_large_geometries(cs):
    """32x32, 40x40 and 64x64 under the `adv` rewards: a third of the envs 3, 2 or 1 steps before
    max_steps (every rollout truncates, the undo log is short), a third one move from a finished
    map (termination and r_complete inside the search), a third with rollouts of the full depth.
    Oracle statistics over the 70 envs (envs with a count > 0, largest count): selection steps that
    ended the episode 14 / 16 / 13 envs (15), thirsty plants watered 20 / 10 / 14 envs (5 / 4 / 7)."""
    with open_case(cs) as (tw, b, m):
        st = search_and_compare(m, b, tw.ov, MC.streams(cs["mseed"]), cs["geom"])
    MC.large_conditions(st)


def test_global_kernel_above_64():
    """G = 100 (10000 cells per sim env, 4 row words): pe_mcts_search_kernel takes any grid side"""
    cs = MC.ABOVE_64
    with open_case(cs) as (tw, b, m):
        assert m.kernel_name == MC.GLOBAL_KERNEL and b.grid_size == 100
        search_and_compare(m, b, tw.ov, MC.streams(cs["mseed"], cs["n"]), cs["geom"])


def test_global_kernel_masked_and_chained():
    """G = 32: a search of every third env leaves the other envs' actions and streams alone; then
    three rounds of search -> step(actions) with continuing streams, every env each round."""
    cs = MC.CHAIN
    with open_case(cs) as (tw, b, m):
        assert m.kernel_name == MC.GLOBAL_KERNEL
        rngs = MC.streams(cs["mseed"])
        key0, pos0 = m.get_rng_state()
        live = np.zeros(MC.N, np.uint8)
        live[::3] = 1
        st = search_and_compare(m, b, tw.ov, rngs, "masked", live)
        off = live == 0
        assert (np_(m.actions)[off] == SENTINEL).all() and (st["action"][~off] >= 0).all()
        key1, pos1 = m.get_rng_state()
        assert (pos1[off] == pos0[off]).all() and (key1[off] == key0[off]).all()
        assert (pos1[~off] != pos0[~off]).any()
        for rnd in range(3):
            st = search_and_compare(m, b, tw.ov, rngs, f"round {rnd}")
            tw.step(st["action"])
            b.step(m.actions)
        U.compare_state(b, tw.ov, "after the chain")


@pytest.mark.parametrize("cs", MC.DEEP, ids=MC.case_id)
def test_deep_trees_walk_the_parent_links(cs):
    """c_param = 0 (pure exploitation) and 400 simulations at max_depth 30 grow narrow, deep trees:
    the backpropagation of a path of more than 8 nodes walks the parent links instead of the
    packed path.  Envs of the 70 whose longest path has 9 nodes or more: 17 on g20 (LDS kernel,
    longest 11), 12 on g32 (global kernel, longest 10); the test needs 5."""
    with open_case(cs) as (tw, b, m):
        st = search_and_compare(m, b, tw.ov, MC.streams(cs["mseed"]), cs["geom"])
    MC.deep_conditions(st)


@pytest.mark.parametrize("cs", MC.SATURATION, ids=MC.case_id)
def test_visit_counts_at_the_byte_limit(cs):
    """Visit counts of {0, 28, 29, 30, 31, 32, 33, 40} in a pattern (mcts_cases.saturation_pattern)
    in which every cell has neighbours whose LDS bytes both read 31 while their exact counts
    differ, and the rover stands beside a 30: the rollout's least-visited choice needs the exact
    counts, and moves cross 30 -> 31 (the first write of the exact count beside the byte) and
    bump cells at 31 or more twice in a simulation.  g20 and G = 29 run the LDS kernel; G = 32
    runs the global kernel, whose words are exact, on the same pattern.  Oracle statistics: all
    70 envs moved into a 30 (up to 154 times) and into an already bumped saturated cell (up to
    353 times); the test needs half of the envs."""
    with open_case(cs) as (tw, b, m):
        st = search_and_compare(m, b, tw.ov, MC.streams(cs["mseed"]), cs["geom"])
    MC.saturation_conditions(st)


@pytest.mark.parametrize("geom", MC.DEGENERATE_GEOMS, ids=[MC.case_id(MC.case(g)) for g in MC.DEGENERATE_GEOMS])
def test_degenerate_budgets(geom):
    """n_simulations in {0, 1, 4, 5, 6, 40} x max_depth in {0, 1, 2}, one MCTS each over the same
    batch.  Without simulations or depth the root has no children: the action is the stream's
    np.random.randint(5) and the stream has advanced by exactly that draw.  (6, 1) and (40, 2)
    stop selections at depth == max_depth with nothing to expand or roll out (in all 70 envs)."""
    cs = MC.case(geom)
    tw, before = MC.host_side(cs)
    b = gpu_side(cs, tw, before)
    try:
        for n_sims, depth in MC.DEGENERATE_BUDGETS:
            with searcher(cs, b, n_sims, depth) as m:
                tag = f"{geom} n_sims {n_sims} max_depth {depth}"
                st = search_and_compare(m, b, tw.ov, MC.streams(cs["mseed"]), tag)
                MC.degenerate_conditions(n_sims, depth, st)
                if n_sims == 0 or depth == 0:  # numpy itself: one randint(5) from np.random.seed(seed + e)
                    a = np_(m.actions)
                    key, pos = m.get_rng_state()
                    for e in range(MC.N):
                        r = np.random.RandomState(cs["mseed"] + e)
                        assert a[e] == r.randint(5), (tag, e)
                        s = r.get_state()
                        assert same_stream(key[e], pos[e], s[1], s[2]), (tag, e)
    finally:
        b.close()


def test_create_limits():
    from plantos_amd.mcts import MCTS
    b = U.make_batch(MC.GEOM["g7"], 4, MC.SEED, 1000, 0.7, U.PRESETS["default"])
    try:
        for kw, text in ((dict(n_simulations=-1), r"n_simulations must be in \[0, 65534\]"),
                         (dict(n_simulations=65535), r"n_simulations must be in \[0, 65534\]"),
                         (dict(max_depth=-1), r"max_depth must be in \[0, 2\^20\]"),
                         (dict(max_depth=2**20 + 1), r"max_depth must be in \[0, 2\^20\]")):
            with pytest.raises(ValueError, match="pe_mcts_create: " + text):
                MCTS(b, **{"n_simulations": 5, "max_depth": 10, **kw})
        MCTS(b, n_simulations=5, max_depth=10).close()
    finally:
        b.close()


@pytest.mark.parametrize("geom", MC.DEGENERATE_GEOMS, ids=[MC.case_id(MC.case(g)) for g in MC.DEGENERATE_GEOMS])
def test_kernel_name_is_the_plans(geom):
    """the kernel a handle reports is the one the device-free plan (tests/test_mcts_plan_host.py)
    names for its grid side, env count and budget: g7 the LDS kernel, G30 the global one"""
    from plantos_amd import _capi as C
    from plantos_amd.mcts import MCTS
    cs = MC.case(geom)
    b = U.make_batch(cs["cfg"], MC.N, MC.SEED, 1000, 0.7, U.PRESETS["default"])
    try:
        m = MCTS(b, n_simulations=cs["n_sims"], max_depth=cs["depth"])
        try:
            assert m.kernel_name == C.mcts_plan(cs["cfg"][0], MC.N, cs["n_sims"], cs["depth"]).kernel_name == cs["kernel"]
        finally:
            m.close()
    finally:
        b.close()


def test_mcts_may_be_closed_after_its_batch():
    """pe_mcts_destroy needs nothing of the env handle (a collector may finalize a batch before the
    MCTS over it): closing in that order succeeds and leaves no HIP error behind."""
    from plantos_amd.mcts import MCTS
    b = U.make_batch(MC.GEOM["g7"], 4, MC.SEED, 1000, 0.7, U.PRESETS["default"])
    m = MCTS(b, n_simulations=5, max_depth=10)
    m.search()
    torch.cuda.synchronize()
    b.close()
    m.close()
    torch.cuda.synchronize()
    assert torch.zeros(4, device="cuda:0").sum().item() == 0.0
