"""pe_mcts_create's decisions and the np.random stream conversions without a GPU.

pe_internal_mcts_plan (csrc/pe_mcts_plan.hpp: the argument checks, the search kernel, its LDS and
the layout of the handle's one allocation, as a function of the grid side, the env count and the
budget) against statements that the code under test did not produce: the kernel rule as
tests/mcts_cases.py restates it (lds_bytes, expected_kernel) and writes it out (KERNEL), and the
documented per-env sizes, restated here.  pe_internal_mcts_rng_to_device_host / _from_device_host
(csrc/pe_mcts_rng.hpp: what pe_mcts_set_rng / pe_mcts_get_rng convert with) against numpy's own
streams.
"""
import itertools

import numpy as np
import pytest

import mcts_cases as MC
from plantos_amd import _capi as C

ARRAYS = C.MCTS_ARRAYS
LDS_ONLY, GLOBAL_ONLY = ("cellb", "csim", "csg"), ("ulog",)


def test_kernel_rule_for_every_grid_side():
    for G in range(1, 129):
        p = C.mcts_plan(G, MC.N, 20, 40)
        assert p.kernel_name == MC.expected_kernel(G), G
        assert p.lds_bytes == MC.lds_bytes(G), G
        assert p.ldsp * 64 + 64 * 4 * 32 == p.lds_bytes and p.ldsp % 8 == 4, G  # an odd dword stride
        assert p.ggp == (G * G + 15) // 16 * 16 and p.ggp + 4 >= p.ldsp, G


def test_kernel_of_every_case_geometry():
    for geom, cfg in MC.GEOM.items():
        assert C.mcts_plan(cfg[0], MC.N, 20, 40).kernel_name == MC.KERNEL[geom], geom


def test_rule_flips_between_29_and_30():
    p29, p30 = C.mcts_plan(29, MC.N, 20, 40), C.mcts_plan(30, MC.N, 20, 40)
    assert (p29.lds_bytes, p29.kernel_name) == (62208, MC.LDS_KERNEL)
    assert (p30.lds_bytes, p30.kernel_name) == (65792, MC.GLOBAL_KERNEL)
    names = [C.mcts_plan(G, MC.N, 20, 40).kernel_name for G in range(1, 129)]
    assert names == [MC.LDS_KERNEL] * 29 + [MC.GLOBAL_KERNEL] * 99


def documented_bytes(G, n, n_sims, depth, lds):
    """the arrays of a handle by the per-env sizes of include/plantos_batch.h; None: not allocated"""
    GG = G * G
    return {"cellw": n * GG * 4, "ulog": None if lds else n * (depth + 4) * 8, "nodes": n * (n_sims + 1) * 32,
            "rng": n * 628 * 4, "logt": (n_sims + 1) * 8, "cellb": n * ((GG + 15) // 16 * 16) if lds else None,
            "csim": n * GG * 4 if lds else None, "csg": n * GG * 4 if lds else None}


@pytest.mark.parametrize("G", (7, 29, 30, 64))
def test_layout(G):
    for n, n_sims, depth in itertools.product((1, 70), (0, 1, 65534), (0, 1, 2**20)):
        p = C.mcts_plan(G, n, n_sims, depth)
        tag = (G, n, n_sims, depth)
        lds = p.kernel_name == MC.LDS_KERNEL
        assert lds == (G <= 29), tag
        want = documented_bytes(G, n, n_sims, depth, lds)
        end = 0
        for i, name in enumerate(ARRAYS):
            off, size = p.offset[i], p.size[i]
            if want[name] is None:
                assert size == 0, (tag, name)
            else:
                assert size == (want[name] + 255) // 256 * 256 and size > 0, (tag, name)
            assert off % 256 == 0 and off == end, (tag, name)  # ascending, no gap, no overlap
            end = off + size
        assert p.total == end, tag
        for name in LDS_ONLY:
            assert (p.size[ARRAYS.index(name)] == 0) == (not lds), (tag, name)
        for name in GLOBAL_ONLY:
            assert (p.size[ARRAYS.index(name)] == 0) == lds, (tag, name)
        assert p.clone_blocks == (n * G * G + 255) // 256 and p.search_blocks == (n + 63) // 64, tag


@pytest.mark.parametrize("kw, text", [
    (dict(n_simulations=-1), r"n_simulations must be in \[0, 65534\]"),
    (dict(n_simulations=65535), r"n_simulations must be in \[0, 65534\]"),
    (dict(max_depth=-1), r"max_depth must be in \[0, 2\^20\]"),
    (dict(max_depth=2**20 + 1), r"max_depth must be in \[0, 2\^20\]")])
def test_errors_are_pe_mcts_creates(kw, text):
    """the strings tests/test_gpu_mcts_kernels.py::test_create_limits matches"""
    args = {"n_simulations": 5, "max_depth": 10, **kw}
    with pytest.raises(ValueError, match="^pe_mcts_create: " + text + "$"):
        C.mcts_plan(7, 4, args["n_simulations"], args["max_depth"])


@pytest.mark.parametrize("seed", (0, 1, 12345))
def test_stream_conversion_round_trip(seed):
    for k in (0, 1, 15, 16, 17, 396, 397, 623, 624, 625, 1300):
        r = np.random.RandomState(seed)
        if k:
            r.randint(0, 2**32, size=k, dtype=np.uint32)
        _, key, pos = r.get_state()[:3]
        assert pos == (624 if k == 0 else (k - 1) % 624 + 1), (k, pos)
        dev = C.mcts_rng_to_device(key, pos)
        assert dev.shape == (C.MCTS_RNG_WORDS,) and dev[624] == pos % 624 == (0 if pos == 624 else pos), k
        assert (dev[pos:624] == key[pos:]).all() and (dev[626:] == 0).all(), k  # this round's words, the pad
        key2, pos2 = C.mcts_rng_from_device(dev)
        assert pos2 == pos % 624, k
        assert MC.same_stream(key2, pos2, key, pos), k
        if pos < 624:  # inside a round the way back is exact (at a round's end numpy holds the untwisted words)
            assert (key2 == key).all() and (C.mcts_rng_to_device(key2, pos2) == dev).all(), k


def test_stream_positions_out_of_range_are_refused():
    key = np.random.RandomState(3).get_state()[1]
    for pos in (-1, 625):
        with pytest.raises(ValueError, match=r"^pe_mcts_set_rng: pos must be in \[0, 624\]$"):
            C.mcts_rng_to_device(key, pos)
    for pos in (0, 624):
        C.mcts_rng_to_device(key, pos)
