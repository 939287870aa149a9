"""The cases of tests/test_gpu_mcts_kernels.py (TEST INFRA): the oracle side of every case --
the env states a search starts from, the oracle's searches with their statistics
(oracle.mcts_search(..., stats=True)) and the conditions those statistics must meet -- so that
the host test (test_mcts_cases.py) can show with the oracle alone that each case reaches the
code path it is there for, and the GPU test asserts the same conditions on the searches it
compares.

Which search kernel runs (pe_mcts_plan.hpp, pe_mcts_kernel_name): the LDS kernel keeps, per workgroup
of 64 envs, each env's cells as bytes -- G*G rounded up to whole dwords, plus one dword when that
count is even (odd stride between lanes) -- and a ring of 32 draws (128 B); it runs when G <= 64
and the 64 envs fit 64 KiB, which holds up to G = 29 (62208 B; G = 30 needs 65792 B).
"""
import numpy as np

import rules_util as U
from oracle import oracle as O

LDS_KERNEL, GLOBAL_KERNEL = "pe_mcts_search_lds_kernel", "pe_mcts_search_kernel"
N = 70        # one full workgroup of 64 envs plus a ragged one of 6
WARM = 6      # synth_actions steps that move the envs off their reset states
SEED = 8      # the batch's seed
SENTINEL = -7  # the action of an env that a masked search leaves out


def lds_bytes(G):
    """dynamic LDS of one workgroup of the LDS search kernel at grid side G (the documented rule)"""
    dwords = (G * G + 3) // 4
    dwords += dwords % 2 == 0
    return 64 * (4 * dwords + 4 * 32)


def expected_kernel(G):
    return LDS_KERNEL if G <= 64 and lds_bytes(G) <= 64 * 1024 else GLOBAL_KERNEL


GEOM = {
    "g7": (7, 3, 3, 3, 12), "g20": (20, 10, 12, 6, 16),
    "G28": (28, 10, 12, 6, 16), "G29": (29, 10, 12, 6, 16), "G30": (30, 10, 12, 6, 16), "G32": (32, 10, 12, 6, 16),
    "g32": (32, 20, 30, 9, 24), "g40": (40, 30, 40, 8, 48), "g64": (64, 100, 120, 6, 64),
    "G100": (100, 20, 30, 6, 16),
}
# written out, not derived: a drift of the rule in expected_kernel() or in the library shows here
KERNEL = {"g7": LDS_KERNEL, "g20": LDS_KERNEL, "G28": LDS_KERNEL, "G29": LDS_KERNEL, "G30": GLOBAL_KERNEL,
          "G32": GLOBAL_KERNEL, "g32": GLOBAL_KERNEL, "g40": GLOBAL_KERNEL, "g64": GLOBAL_KERNEL,
          "G100": GLOBAL_KERNEL}


def case(geom, n_sims=20, depth=40, c=1.414, rules="default", max_steps=1000, p=0.7, edit=None, mseed=41, n=N):
    return dict(geom=geom, cfg=GEOM[geom], kernel=KERNEL[geom], n_sims=n_sims, depth=depth, c=c, rules=rules,
                max_steps=max_steps, p=p, edit=edit, mseed=mseed, n=n)


def host_side(cs):
    """(twin, snapshot before the edits): the oracle's envs after WARM synthetic steps -- the state
    the GPU batch must be in after the same steps -- then the case's edits of that state."""
    tw = U.Twin(cs["cfg"], cs["n"], SEED, cs["max_steps"], cs["p"], U.PRESETS[cs["rules"]])
    for t in range(WARM):
        tw.step(U.host_synth(cs["n"], t))
    before = U.snapshot(tw.ov)
    if cs["edit"] is not None:
        cs["edit"](tw.ov)
    return tw, before


def streams(seed, n=N):
    """env e's np.random stream as MCTS(seed=seed) starts it: np.random.seed(seed + e)"""
    return [O.NpMT(seed + e) for e in range(n)]


def same_stream(key_a, pos_a, key_b, pos_b, draws=700):
    """Two numpy MT states (key, pos) produce the same future draws (numpy reports a round
    boundary as pos 624 over the untwisted words, the device as pos 0 over the twisted ones)."""
    ra, rb = np.random.RandomState(), np.random.RandomState()
    ra.set_state(("MT19937", np.asarray(key_a, np.uint32), int(pos_a), 0, 0.0))
    rb.set_state(("MT19937", np.asarray(key_b, np.uint32), int(pos_b), 0, 0.0))
    return (ra.randint(0, 2**32, draws, dtype=np.uint64) == rb.randint(0, 2**32, draws, dtype=np.uint64)).all()


def oracle_searches(ov, rngs, n_sims, c, depth, live=None):
    """One oracle search per live env from the oracle's current state; the streams advance.
    Returns action [n], order [n,5], visits [n,5], value f64 [n,5] and the statistics as arrays [n]
    (zero rows for envs that are not live)."""
    b = ov.b
    n = b.n
    out = dict(action=np.full(n, SENTINEL, np.int32), order=np.full((n, 5), -1, np.int32),
               visits=np.zeros((n, 5), np.int32), value=np.zeros((n, 5), np.float64))
    out.update({k: np.zeros(n, np.int64) for k in O.MCTS_STATS})
    for e in range(n):
        if live is not None and not live[e]:
            continue
        a, order, cv, cval, st = O.mcts_search(ov.cfg, b.cells[e], b.visits[e], b.explored[e], b.scal[e], rngs[e],
                                               n_sims, c, depth, stats=True)
        out["action"][e], out["order"][e], out["visits"][e], out["value"][e] = a, order, cv, cval
        for k, v in st.items():
            out[k][e] = v
    return out


# ---------------------------------------------------------------- the edits of a case's state
def late_and_last_cell(ov):
    """a third of the envs 3, 2 or 1 steps before max_steps (every rollout truncates, the undo log
    stays short; at max_steps - 1 the first selection step truncates); another third one move away
    from a fully explored map (termination and r_complete inside the search)"""
    late, inj = late_envs(), last_cell_envs()
    ov.b.scal[late, O.S_STEP] = ov.cfg.max_steps - 3 + (late // 3) % 3
    U.inject_last_cell(ov, inj)


def late_envs():
    return np.arange(0, N, 3)


def last_cell_envs():
    return np.arange(1, N, 3)


SAT_VALUES = (0, 28, 29, 30, 31, 32, 33, 40)


def saturation_pattern(G, x, y, cells):
    """visit counts [G, G] for an env whose rover stands at (x, y): cell (i, j) holds
    SAT_VALUES[(i + 3 j + k) % 8].  Along a row step the index moves by 1, along a column step by
    3, so the four neighbours of a cell at index m sit at m +- 1 and m +- 3: for every m at least
    two of them hold different values of {31, 32, 33, 40} -- both bytes of the LDS kernel read 31,
    the exact counts differ (checked by test_mcts_cases.py).  k puts a 30 on the rover's first
    neighbour that it can move to.  The rover's own cell is visited: at least 1."""
    k = 0
    for dx, dy in U.DIRS:
        nx, ny = x + dx, y + dy
        if 0 <= nx < G and 0 <= ny < G and cells[nx, ny] != U.PE_OBST:
            k = (SAT_VALUES.index(30) - (nx + 3 * ny)) % 8
            break
    i, j = np.meshgrid(np.arange(G), np.arange(G), indexing="ij")
    v = np.array(SAT_VALUES, np.int32)[(i + 3 * j + k) % 8]
    v[x, y] = max(int(v[x, y]), 1)
    return v


def saturate(ov):
    """every env's visit counts replaced by saturation_pattern(); explored_map follows the counts
    (explored where visited, the rover's cell 2), as the env itself keeps them"""
    b = ov.b
    G = b.cfg.grid_size
    for e in range(b.n):
        x, y = int(b.scal[e, O.S_X]), int(b.scal[e, O.S_Y])
        b.visits[e] = saturation_pattern(G, x, y, b.cells[e])
        b.explored[e] = (b.visits[e] > 0).astype(np.int8)
        b.explored[e, x, y] = 2


# ---------------------------------------------------------------- the cases
BOUNDARY = [case(g) for g in ("G28", "G29", "G30", "G32")]
LARGE = [case(g, rules="adv", edit=late_and_last_cell) for g in ("g32", "g40", "g64")]
CHAIN = case("g32")
DEEP_SIMS = 400
DEEP = [case(g, n_sims=DEEP_SIMS, depth=30, c=0.0) for g in ("g20", "g32")]
SATURATION = [case(g, n_sims=30, edit=saturate) for g in ("g20", "G29", "G32")]
# the global kernel is documented for any G: a grid side above 64 (16 envs, a small budget)
ABOVE_64 = case("G100", n_sims=8, depth=10, n=16)
DEGENERATE_GEOMS = ("g7", "G30")
DEGENERATE_BUDGETS = [(s, d) for s in (0, 1, 4, 5, 6, 40) for d in (0, 1, 2)]


def case_id(cs):
    return f"{cs['geom']}-{cs['kernel']}"


# ---------------------------------------------------------------- what the statistics must show
def large_conditions(st):
    """some env ended a selection step terminated or truncated, some env watered a thirsty plant;
    the late envs' rollouts are short, the last-cell envs meet r_complete"""
    assert (st["select_ended"] > 0).any() and (st["waters_thirsty"] > 0).any(), \
        (int(st["select_ended"].sum()), int(st["waters_thirsty"].sum()))
    assert (st["select_ended"][late_envs()[(late_envs() // 3) % 3 == 2]] > 0).all()  # one step from max_steps
    # r_complete (33.301, `adv`) is in a value sum of every last-cell env; a late env's value sums
    # are at most n_sims rollouts of at most 3 steps of at most 0.69 each
    best = st["value"].max(1)
    assert (best[last_cell_envs()] > 33.0).all() and (best[late_envs()] < 20 * 3 * 0.7).all()


def deep_conditions(st):
    """the parent-link walk of the backpropagation (paths of more than 8 nodes) is taken in at
    least 5 envs"""
    deep = int((st["max_path_nodes"] >= 9).sum())
    assert deep >= 5, deep
    return deep


def saturation_conditions(st):
    """at least half of the envs moved into a cell at exactly 30 and moved again into a cell at
    31 or more that the same simulation had bumped"""
    b30, bsat = int((st["moves_into_30"] > 0).sum()), int((st["moves_into_bumped_sat"] > 0).sum())
    assert 2 * b30 >= N and 2 * bsat >= N, (b30, bsat)
    return b30, bsat


def degenerate_conditions(n_sims, depth, st):
    """selection stopped by depth == max_depth, with nothing to expand or roll out: the sixth
    simulation of a (6, 1) budget descends from the fully expanded root to the depth limit; a
    (40, 2) budget gets there once a child of the root is fully expanded"""
    stops = st["select_depth_stop"]
    if (n_sims, depth) == (6, 1):
        assert (stops == 1).all(), stops
    if (n_sims, depth) == (40, 2):
        assert (stops > 0).any(), stops
    if depth == 0:
        assert (stops == n_sims).all(), stops
    if n_sims == 0 or depth == 0:  # a root without children
        assert (st["order"] == -1).all() and (st["visits"] == 0).all() and (st["value"] == 0.0).all()
        assert (st["max_path_nodes"] == (1 if n_sims else 0)).all()
