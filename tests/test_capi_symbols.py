"""CPU-side checks of the C-ABI boundary (no GPU, no compute calls).

- libplantos_hip.so loads and exports every function include/*.h declares;
- the ctypes layer (plantos_amd._capi) binds exactly that set, and every entry of its signature
  table has the return type and the parameters of the header's prototype;
- struct layout of pe_config, pe_policy_tower and pe_policy_lstm agrees between C and ctypes;
- without a usable device, the product path fails loudly (no CPU fallback).
"""
import ctypes
import glob
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = sorted(glob.glob(os.path.join(REPO, "include", "*.h")))
DECL = re.compile(r"^\s*(?:const\s+)?[A-Za-z_][A-Za-z0-9_]*\s*\*?\s*(pe_[a-z0-9_]+)\s*\(", re.M)
PROTO = re.compile(r"^\s*((?:const\s+)?[A-Za-z_][A-Za-z0-9_]*\s*\*?)\s*(pe_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", re.M)
SCALARS = {"int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "int64_t": ctypes.c_int64,
           "uint64_t": ctypes.c_uint64, "float": ctypes.c_float, "double": ctypes.c_double, "int": ctypes.c_int}
STRUCTS = {"pe_config": "PEConfig", "pe_policy_tower": "PEPolicyTower", "pe_policy_lstm": "PEPolicyLstm"}


def declared():
    names = []
    for h in HEADERS:
        src = open(h).read()
        src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
        names += DECL.findall(src)
    return sorted(set(names))


def prototypes():
    """{name: (return type, [parameter types])} of every prototype, as C text without the
    parameter names ("const float*", "int64_t", "pe_handle**")."""
    out = {}
    for h in HEADERS:
        src = re.sub(r"/\*.*?\*/", "", open(h).read(), flags=re.S)
        for ret, name, params in PROTO.findall(src):
            params = [" ".join(p.split()) for p in params.split(",")]
            params = [] if params == ["void"] else [re.sub(r"\s*[A-Za-z_][A-Za-z0-9_]*$", "", p) for p in params]
            out[name] = (" ".join(ret.split()), params)
    return out


def _type_mismatch(c_type, bound, capi):
    """None if the ctypes type `bound` fits the C type text, else what is wrong with it."""
    base = c_type.replace("const", "").replace("*", "").strip()
    stars = c_type.count("*")
    if stars == 0:
        if c_type == "void":
            return None if bound is None else f"void bound as {bound}"
        return None if bound is SCALARS[base] else f"{c_type} bound as {bound}"
    if bound in (ctypes.c_void_p, ctypes.c_char_p):
        return None
    if not (isinstance(bound, type) and issubclass(bound, ctypes._Pointer)):
        return f"{c_type} bound as {bound}, which is no pointer type"
    if stars == 1 and base in STRUCTS and bound._type_ is not getattr(capi, STRUCTS[base]):
        return f"{c_type} bound as a pointer to {bound._type_}"
    if stars == 1 and base in SCALARS and bound._type_ is not SCALARS[base]:
        return f"{c_type} bound as a pointer to {bound._type_}"
    return None


def signature_mismatches(protos, table, capi):
    """Every disagreement between the header's prototypes and a name -> (restype, [argtypes]) table."""
    bad = []
    for name, (ret, params) in sorted(protos.items()):
        if name not in table:
            bad.append(f"{name}: not in the table")
            continue
        restype, argtypes = table[name]
        why = _type_mismatch(ret, restype, capi)
        if why:
            bad.append(f"{name} returns {why}")
        if len(argtypes) != len(params):
            bad.append(f"{name}: {len(params)} parameters, {len(argtypes)} argtypes")
            continue
        for i, (c_type, bound) in enumerate(zip(params, argtypes)):
            why = _type_mismatch(c_type, bound, capi)
            if why:
                bad.append(f"{name} parameter {i}: {why}")
    return bad


@pytest.fixture(scope="module")
def lib_path():
    from plantos_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        subprocess.run(["python", os.path.join(REPO, "rl-env_amd", "build.py")], check=True)
    return _capi.LIB_PATH


def test_headers_declare_the_boundary():
    names = declared()
    for must in ("pe_create", "pe_reset", "pe_step", "pe_get_state", "pe_set_state", "pe_destroy",
                 "pe_last_error"):
        assert must in names


def test_library_exports_every_declared_symbol(lib_path):
    out = subprocess.run(["nm", "-D", "--defined-only", lib_path], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    missing = [n for n in declared() if n not in exported]
    assert not missing, missing
    L = ctypes.CDLL(lib_path)
    for n in declared():
        assert hasattr(L, n), n


def test_ctypes_binding_matches_header(lib_path):
    from plantos_amd import _capi
    assert sorted(_capi.EXPORTS) == declared()
    L = _capi.lib()
    for n in _capi.EXPORTS:
        assert getattr(L, n).restype is not None or n == "pe_default_config"


def test_signatures_match_header():
    """Every prototype of include/*.h against _capi.SIGNATURES: the return type, the number of
    parameters, and each parameter's width and kind (a pointer for anything with a `*`, the
    matching struct behind a POINTER)."""
    from plantos_amd import _capi
    protos = prototypes()
    assert sorted(protos) == declared()
    assert len(protos) == len(_capi.EXPORTS) == 70
    assert sorted(_capi.SIGNATURES) == sorted(protos)
    assert signature_mismatches(protos, _capi.SIGNATURES, _capi) == []
    # the comparison sees a wrong width: an int64_t stride bound as c_int32
    restype, argtypes = _capi.SIGNATURES["pe_rollout_gae"]
    assert protos["pe_rollout_gae"][1][2] == "int64_t" and argtypes[2] is ctypes.c_int64
    wrong = dict(_capi.SIGNATURES, pe_rollout_gae=(restype, argtypes[:2] + [ctypes.c_int32] + argtypes[3:]))
    bad = signature_mismatches(protos, wrong, _capi)
    assert len(bad) == 1 and bad[0].startswith("pe_rollout_gae parameter 2: int64_t bound as")
    # ... and a double bound as c_float, a struct pointer to the wrong struct, a dropped parameter
    for name, i, other in (("pe_replay_target", 5, ctypes.c_float),
                           ("pe_policy_load", 1, ctypes.POINTER(_capi.PEPolicyLstm)), ("pe_seed", 3, None)):
        restype, argtypes = _capi.SIGNATURES[name]
        changed = argtypes[:i] + ([other] if other is not None else []) + argtypes[i + 1:]
        assert len(signature_mismatches(protos, dict(_capi.SIGNATURES, **{name: (restype, changed)}), _capi)) == 1


def test_library_binding_is_the_table(lib_path):
    """lib() binds what the table says, the plan entry points included."""
    from plantos_amd import _capi
    L = _capi.lib()
    for name, (restype, argtypes) in {**_capi.SIGNATURES, **_capi.INTERNAL_SIGNATURES}.items():
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


def test_config_struct_layout(lib_path):
    """pe_default_config writes the reference defaults (plantos_env.py:25-27,76-83,120)
    through the C struct; pe_obs_dim = 5C+27 (plantos_env.py:55-57)."""
    from plantos_amd import _capi
    c = _capi.default_config(20, 10, 12, 6, 16)
    assert (c.abi_version, c.grid_size, c.num_plants, c.num_obstacles, c.lidar_range,
            c.lidar_channels) == (_capi.PE_ABI_VERSION, 20, 10, 12, 6, 16)
    assert c.max_steps == 1000 and c.autoreset == 1
    assert c.thirsty_plant_prob == 0.7
    assert (c.r_goal, c.r_mistake, c.r_invalid, c.r_water_empty) == (20, -10, -5, -5)
    assert (c.r_step, c.r_exploration, c.r_revisit, c.r_complete) == (-0.1, 10, -1, 50)
    assert _capi.lib().pe_obs_dim(ctypes.byref(c)) == 107


def _assert_layout_matches_c_compiler(tmp_path, c_name, struct):
    """sizeof of the struct, and offsetof and sizeof of every field, from gcc on
    include/plantos_batch.h == ctypes."""
    fields = [f[0] for f in struct._fields_]
    src = ["#include <stdio.h>", "#include <stddef.h>", '#include "plantos_batch.h"', "int main(void){",
           f'printf("%zu\\n", sizeof({c_name}));']
    src += [f'printf("%zu\\n", offsetof({c_name}, {f}));' for f in fields]
    src += [f'printf("%zu\\n", sizeof((({c_name}*)0)->{f}));' for f in fields]
    src += ["return 0;}"]
    c = tmp_path / f"layout_{c_name}.c"
    c.write_text("\n".join(src))
    exe = tmp_path / f"layout_{c_name}"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), "-o", str(exe), str(c)], check=True)
    vals = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert len(vals) == 1 + 2 * len(fields)
    assert vals[0] == ctypes.sizeof(struct)
    for f, off, size in zip(fields, vals[1:], vals[1 + len(fields):]):
        assert getattr(struct, f).offset == off, f
        assert getattr(struct, f).size == size, f


def test_config_struct_matches_c_compiler(tmp_path):
    """sizeof/offsetof of pe_config from gcc on include/plantos_batch.h == ctypes."""
    from plantos_amd import _capi
    _assert_layout_matches_c_compiler(tmp_path, "pe_config", _capi.PEConfig)


@pytest.mark.parametrize("c_name, struct", [("pe_policy_tower", "PEPolicyTower"), ("pe_policy_lstm", "PEPolicyLstm")])
def test_policy_structs_match_c_compiler(tmp_path, c_name, struct):
    """... and of pe_policy_tower / pe_policy_lstm, whose pointers the policy calls pass."""
    from plantos_amd import _capi
    _assert_layout_matches_c_compiler(tmp_path, c_name, getattr(_capi, struct))


def test_no_cpu_fallback_without_device(lib_path):
    """pe_create must fail with PE_ERR_DEVICE (or ARG) rather than run on the host."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from plantos_amd import _capi
    c = _capi.default_config(20, 10, 12, 6, 16)
    h = ctypes.c_void_p()
    rc = _capi.lib().pe_create(ctypes.byref(c), 0, 64, ctypes.byref(h))
    assert rc == _capi.PE_ERR_DEVICE
    assert b"no HIP device" in _capi.lib().pe_last_error()
    from plantos_amd import PlantOSBatch
    with pytest.raises(Exception):
        PlantOSBatch(64, device="cpu")
