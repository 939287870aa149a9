"""Seed-exact CPython map stream of the product library (pe_pystream_*, host code,
no GPU) against the reference's own outputs: consecutive reset() layouts after
random.seed(s) for 6 geometries (tests/golden/maps_*.npz, incl. the MT state
afterwards via getrandbits(32)), the KAT's map, and the reset layouts of the
reference DummyVecEnv trajectories in consumption order."""
import numpy as np
import pytest

from golden_util import MAP_CFGS, TRAJ_FILES, cfg_tuple, load
from plantos_amd._capi import PyStream


@pytest.mark.parametrize("cfg", MAP_CFGS)
def test_reset_stream_matches_reference(cfg):
    f = load(f"maps_{cfg}")
    G, P, O, R, C = cfg_tuple(f)
    n_resets = f["cells"].shape[1]
    for si, seed in enumerate(f["seeds"]):
        s = PyStream(G, P, O, int(seed))
        cells, rover = s.next(n_resets)
        assert (cells == f["cells"][si]).all(), (cfg, seed)
        assert (rover == f["rover"][si]).all(), (cfg, seed)
        assert s.getrandbits32() == int(f["next_u32"][si]), (cfg, seed)
        s.close()


def test_kat_map():
    k = load("kat_seed0")
    G, P, O, R, C = cfg_tuple(k)
    s = PyStream(G, P, O, 0)
    cells, rover = s.next(1)
    assert (cells[0] == k["cells0"]).all() and (rover[0] == k["rover0"]).all()


@pytest.mark.parametrize("name", TRAJ_FILES)
def test_dummyvecenv_reset_order(name):
    """maps0 (env-index order at reset) then every auto-reset map in (step, env) order."""
    f = load(name)
    G, P, O, R, C = cfg_tuple(f)
    s = PyStream(G, P, O, int(f["seed"]))
    n = f["maps0"].shape[0]
    cells, rover = s.next(n)
    assert (cells == f["maps0"]).all() and (rover == f["rover0"]).all()
    k = len(f["reset_t"])
    if k:
        cells, rover = s.next(k)
        assert (cells == f["reset_cells"]).all() and (rover == f["reset_rover"]).all()
    assert s.getrandbits32() == int(f["next_u32"])


def test_reset_order_with_non_default_thirsty_prob():
    """thirsty_plant_prob = 0.5 on the host path (pe_pystream.cpp): the reference's fork env
    built with it (tests/golden/traj_g12r2_rules.npz) -- maps0, then every auto-reset map."""
    f = load("traj_g12r2_rules")
    G, P, O, R, C = cfg_tuple(f)
    p = float(f["thirsty_plant_prob"])
    assert p == 0.5
    s = PyStream(G, P, O, int(f["seed"]), thirsty_plant_prob=p)
    cells, rover = s.next(f["maps0"].shape[0])
    assert (cells == f["maps0"]).all() and (rover == f["rover0"]).all()
    k = len(f["reset_t"])
    assert k >= 8
    cells, rover = s.next(k)
    assert (cells == f["reset_cells"]).all() and (rover == f["reset_rover"]).all()
    assert s.getrandbits32() == int(f["next_u32"])
    # the maps tell 0.5 from the default: the default stream draws other plants thirsty
    d = PyStream(G, P, O, int(f["seed"]))
    assert (d.next(f["maps0"].shape[0])[0] != f["maps0"]).any()


def test_no_room_is_value_error():
    s = PyStream(5, 22, 3, 0)
    with pytest.raises(ValueError):
        s.next(1)
