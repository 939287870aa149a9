"""Kernel selection without a GPU: pe_internal_plan (csrc/pe_plan.hpp: everything pe_create
decides before its first allocation, as a function of the config, the batch size and the CU
count) against two records that the code under test did not produce:

- the project's own tables of which kernel a geometry runs (tests/rules_util.py), which
  predate the plan;
- tests/golden/plan_parent.json: what pe_create gave, on an MI355X, at the commit before
  selection moved into the plan (tools/gen_golden_plan.py) -- kernel name, variant number,
  prefetch period, state bytes, or the error text -- over a sweep that crosses every
  threshold of the selection ladder, and the same for a -DPE_DEBUG_KNOBS library under each
  A/B knob.
"""
import ctypes
import json
import os
import shutil
import subprocess
import sys
import tempfile

import pytest

import rules_util as RU
from plantos_amd import _capi as C

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "rl-env_amd", "csrc")
with open(os.path.join(REPO, "tests", "golden", "plan_parent.json")) as _f:
    GOLDEN = json.load(_f)
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _plan_named(name, n, codes):
    G, P, O, R, Ch = RU.CFG[name]
    cfg = C.default_config(G, P, O, R, Ch)
    cfg.obs_codes = int(codes)
    return C.plan(cfg, n, 256)


NAMED = ([(g, 133, False) for g in RU.CFG] + [("g20", n, False) for n in RU.G20_BY_N] + [("g20", 133, True)])


@pytest.mark.parametrize("name,n,codes", NAMED, ids=[f"{g}-n{n}{'-codes' if c else ''}" for g, n, c in NAMED])
def test_plan_matches_the_kernel_tables(name, n, codes):
    assert _plan_named(name, n, codes).kernel_name.decode() == RU.kernel_of(name, n, codes)


def config_of(case):
    """the pe_config of a fixture row, as PlantOSBatch fills it"""
    cfg = C.default_config(case["grid_size"], case["num_plants"], case["num_obstacles"], case["lidar_range"],
                           case["lidar_channels"])
    cfg.max_steps = case["max_steps"]
    cfg.autoreset = case["autoreset"]
    cfg.map_generation_algo = C.map_algo_id(case["map_generation_algo"])
    cfg.coop_max_done = case["coop_max_done"]
    cfg.prefetch_every = case["prefetch_every"]
    cfg.obs_codes = case["obs_codes"]
    return cfg


def planned(lib, case, cu_count):
    """the plan of a fixture row in the fixture's form: {"result": ...} or {"error": text}"""
    info = C.PEPlanInfo()
    rc = lib.pe_internal_plan(ctypes.byref(config_of(case)), case["n"], cu_count, ctypes.byref(info))
    if rc != C.PE_OK:
        assert rc == C.PE_ERR_ARG, rc
        return {"error": lib.pe_last_error().decode()}
    return {"result": dict(kernel_name=info.kernel_name.decode(), kernel_variant=info.variant,
                           prefetch_every=info.prefetch_every, state_bytes=info.state_bytes)}


def recorded(case):
    return {k: case[k] for k in ("result", "error") if k in case}


def test_fixture_crosses_the_ladder():
    """the recorded sweep holds every kernel variant, every shape of the headline kernel, both
    tile forms of the runtime kernel and every rejection the plan can give a PlantOSBatch"""
    res = [c["result"] for c in GOLDEN["cases"] + GOLDEN["knob_cases"] if "result" in c]
    assert {r["kernel_variant"] for r in res} == set(range(14)) - {2}  # (2: pe_step_fast<C16,R6>, G > 20 with the lane knob)
    names = {r["kernel_name"] for r in res}
    for n in list(RU.KERNELS.values()) + list(RU.G20_BY_N.values()) + list(RU.CODES_KERNELS.values()):
        assert n in names, n
    assert len({c["error"] for c in GOLDEN["cases"] + GOLDEN["knob_cases"] if "error" in c}) == 12
    assert 200 <= len(GOLDEN["cases"]) <= 400


def test_plan_reproduces_the_parent():
    lib = C.lib()
    bad = []
    for case in GOLDEN["cases"]:
        got = planned(lib, case, GOLDEN["cu_count"])
        if got != recorded(case):
            bad.append((case, got))
    assert not bad, (len(bad), bad[:3])


def test_plan_depends_on_the_cu_count():
    """32x32 / 24 rays at 32768 envs: 512 workgroups, two f32-tile workgroups per CU -- one
    round on 256 CUs (f32 tile), more than one on 255 (byte tile)"""
    cfg = C.default_config(*RU.CFG["g32"])
    assert C.plan(cfg, 32768, 256).tile_codes == 0 and C.plan(cfg, 32768, 255).tile_codes == 1
    assert C.plan(cfg, 32769, 256).tile_codes == 1


_CHILD = r"""
import ctypes, json, os, sys
sys.path[:0] = sys.argv[1:4]
import test_plan_host as T
from plantos_amd import _capi as C
lib = ctypes.CDLL(sys.argv[4])  # (the plan alone is called in it: the configs come from the product library)
lib.pe_internal_plan.argtypes = [ctypes.POINTER(C.PEConfig), ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(C.PEPlanInfo)]
lib.pe_last_error.restype = ctypes.c_char_p
out = []
for case in T.GOLDEN["knob_cases"]:
    for v in ("PE_STEP_KERNEL", "PE_QUAD_EPB", "PE_TILE_CODES", "PE_STAGGER", "PE_LDS_FLOOR"):
        os.environ.pop(v, None)
    os.environ.update(case["knobs"])
    out.append(T.planned(lib, case, T.GOLDEN["cu_count"]))
print(json.dumps(out))
"""


@pytest.mark.skipif(not (shutil.which(HIPCC) or os.path.exists(HIPCC)), reason="needs hipcc")
def test_plan_reproduces_the_parent_under_the_knobs():
    """a -DPE_DEBUG_KNOBS build of the plan's translation unit (and pe_render.hip, which it
    links against), loaded in a child process; the knob variables set there before each plan"""
    with tempfile.TemporaryDirectory(prefix="pe_plan_knobs_", dir="/tmp") as d:
        so = os.path.join(d, "libplantos_knobs.so")
        subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-std=c++17", "-fPIC", "-w", "-shared",
                        "-DPE_DEBUG_KNOBS", "-o", so, os.path.join(CSRC, "plantos_batch.hip"),
                        os.path.join(CSRC, "pe_render.hip")], check=True)
        env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
        r = subprocess.run([sys.executable, "-c", _CHILD, os.path.join(REPO, "rl-env_amd"),
                            os.path.join(REPO, "tests"), REPO, so], env=env, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert len(got) == len(GOLDEN["knob_cases"]) == 42
    bad = [(c["knobs"], c["grid_size"], c["n"], g) for c, g in zip(GOLDEN["knob_cases"], got) if g != recorded(c)]
    assert not bad, bad[:3]
    # the knobs took effect in that library: these rows differ from the product's choice
    assert any(c["knobs"] and recorded(c) != planned(C.lib(), c, GOLDEN["cu_count"]) for c in GOLDEN["knob_cases"])
