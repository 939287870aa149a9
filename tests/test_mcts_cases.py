"""Host checks (no GPU) of the oracle's search statistics and of the cases of
tests/test_gpu_mcts_kernels.py (tests/mcts_cases.py).

- oracle.mcts_search(..., stats=True) returns exactly what the search returns without statistics
  (the reference's recorded searches, tests/golden/mcts_*.npz, are the fixed point) and leaves the
  stream where that search leaves it; a backpropagation path has at least 2 nodes whenever a
  simulation can expand (n_sims >= 1, max_depth >= 1).
- the kernel rule of mcts_cases (64 KiB of LDS) puts the boundary between G = 29 and G = 30.
- every case reaches what it is there for, by the oracle's statistics alone.
"""
import zlib

import numpy as np
import pytest

import mcts_cases as MC
from golden_util import cfg_tuple, load
from oracle import oracle as O


@pytest.mark.parametrize("name", ["mcts_g7", "mcts_g20d", "mcts_g32"])
def test_stats_leave_the_search_alone(name):
    f = load(name)
    cfg = O.config(*cfg_tuple(f))
    ns, md, cp = int(f["n_sims"]), int(f["max_depth"]), float(f["c_param"])
    plain = with_stats = None
    for i in range(min(len(f["action"]), 12)):
        if f["cseed"][i] >= 0:
            plain, with_stats = O.NpMT(int(f["cseed"][i])), O.NpMT(int(f["cseed"][i]))
        args = (cfg, f["cells"][i], f["visits"][i], f["explored"][i], f["scal"][i])
        a0, o0, v0, q0 = O.mcts_search(*args, plain, ns, cp, md)
        a1, o1, v1, q1, st = O.mcts_search(*args, with_stats, ns, cp, md, stats=True)
        assert a0 == a1 == f["action"][i]
        for got0, got1, want in ((o0, o1, f["order"][i]), (v0, v1, f["cvisits"][i]), (q0, q1, f["cvalue"][i])):
            assert (got0 == want).all() and (got1 == want).all(), (name, i)  # f64 sums bit for bit
        for r in (plain, with_stats):
            key, pos = r.state()
            assert pos == f["pos_out"][i] and zlib.crc32(key.tobytes()) == f["crc_out"][i], (name, i)
        assert sorted(st) == sorted(O.MCTS_STATS)
        # n_sims >= 5 expands all root actions: paths of 2 nodes at least; a fully expanded root
        # is descended from (depth 1) and its child expanded: 3 nodes once n_sims >= 7
        assert 3 <= st["max_path_nodes"] <= min(ns + 1, md + 2), (name, i, st)


def test_path_length_statistic():
    """(a) counts the root: 0 without simulations, 1 when nothing can expand (max_depth 0), at
    least 2 whenever n_sims >= 1 and max_depth >= 1, and never more than max_depth + 2 nodes
    (root, max_depth selected nodes, one expanded) or n_sims + 1 (the nodes that exist)."""
    tw, _ = MC.host_side(MC.case("g7"))
    b = tw.ov.b
    for n_sims in (0, 1, 2, 5, 6, 7, 40):
        for depth in (0, 1, 2, 3, 10):
            for e in (0, 1, 69):
                st = O.mcts_search(tw.ov.cfg, b.cells[e], b.visits[e], b.explored[e], b.scal[e], O.NpMT(e), n_sims,
                                   1.414, depth, stats=True)[4]
                a = st["max_path_nodes"]
                if n_sims == 0:
                    assert a == 0
                elif depth == 0:
                    assert a == 1
                else:
                    assert 2 <= a <= min(depth + 2, n_sims + 1), (n_sims, depth, e, a)


def test_kernel_rule():
    assert MC.lds_bytes(28) == 64 * (4 * 197 + 128)  # 196 dwords: even, padded to 197
    assert MC.lds_bytes(29) == 62208 and MC.lds_bytes(30) == 65792
    for name, cfg in MC.GEOM.items():
        assert MC.expected_kernel(cfg[0]) == MC.KERNEL[name], name
    assert [MC.expected_kernel(G) for G in (28, 29, 30, 32)] == [MC.LDS_KERNEL] * 2 + [MC.GLOBAL_KERNEL] * 2


def test_saturation_pattern_layout():
    """every interior cell has two neighbours at 31 or more with different exact counts, and the
    rover's first free neighbour holds 30"""
    for cs in MC.SATURATION:
        tw, _ = MC.host_side(cs)
        b = tw.ov.b
        G = cs["cfg"][0]
        for e in range(MC.N):
            v = b.visits[e]
            assert set(np.unique(v)) <= set(MC.SAT_VALUES) | {1}
            nb = np.stack([v[:-2, 1:-1], v[2:, 1:-1], v[1:-1, :-2], v[1:-1, 2:]])
            x, y = int(b.scal[e, O.S_X]), int(b.scal[e, O.S_Y])
            ok = np.zeros((G - 2, G - 2), bool)
            for p in range(4):
                for q in range(p + 1, 4):
                    ok |= (nb[p] >= 31) & (nb[q] >= 31) & (nb[p] != nb[q])
            assert ok.all(), (cs["geom"], e, np.argwhere(~ok)[:4].tolist())
            free = [(x + dx, y + dy) for dx, dy in MC.U.DIRS
                    if 0 <= x + dx < G and 0 <= y + dy < G and b.cells[e, x + dx, y + dy] != 1]
            assert not free or v[free[0]] == 30, (cs["geom"], e)
            assert ((b.explored[e] > 0) == (v > 0)).all() and b.explored[e, x, y] == 2


def searched(cs):
    tw, _ = MC.host_side(cs)
    return MC.oracle_searches(tw.ov, MC.streams(cs["mseed"]), cs["n_sims"], cs["c"], cs["depth"])


@pytest.mark.parametrize("cs", MC.LARGE, ids=MC.case_id)
def test_large_cases_reach_termination_truncation_and_watering(cs):
    MC.large_conditions(searched(cs))


@pytest.mark.parametrize("cs", MC.DEEP, ids=MC.case_id)
def test_deep_cases_walk_the_parent_links(cs):
    MC.deep_conditions(searched(cs))


@pytest.mark.parametrize("cs", MC.SATURATION, ids=MC.case_id)
def test_saturation_cases_cross_the_byte_limit(cs):
    MC.saturation_conditions(searched(cs))


@pytest.mark.parametrize("geom", MC.DEGENERATE_GEOMS)
def test_degenerate_cases_stop_at_the_depth_limit(geom):
    tw, _ = MC.host_side(MC.case(geom))
    for n_sims, depth in MC.DEGENERATE_BUDGETS:
        st = MC.oracle_searches(tw.ov, MC.streams(41), n_sims, 1.414, depth)
        MC.degenerate_conditions(n_sims, depth, st)
