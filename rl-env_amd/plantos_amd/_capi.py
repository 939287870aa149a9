"""ctypes binding of the C-ABI in include/plantos_batch.h (libplantos_hip.so).

This is the binding a Python maintainer of the reference would add
(INTEGRATION.md): plain pointers and sizes, device buffers owned by torch.
There is no CPU fallback: if the library or a gfx950 device is missing,
loading / pe_create raises.
"""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libplantos_hip.so")
# diagnostics only (tools/ablate.py): load a differently built library
if os.environ.get("PLANTOS_HIP_LIB"):
    LIB_PATH = os.environ["PLANTOS_HIP_LIB"]

PE_ABI_VERSION = 4
PE_OK, PE_ERR_ARG, PE_ERR_DEVICE, PE_ERR_NOMEM, PE_ERR_NOROOM = 0, -1, -2, -3, -4
PE_NSCAL = 8
PE_NINFO = 11
(PE_S_X, PE_S_Y, PE_S_STEP, PE_S_COLL, PE_S_COLLIDED, PE_S_BONUS, PE_S_POISONED, PE_S_EPISODE) = range(8)
(PE_I_X, PE_I_Y, PE_I_THIRSTY, PE_I_HYDRATED, PE_I_TOTAL_PLANTS, PE_I_STEP, PE_I_EXPLORED,
 PE_I_TOTAL_CELLS, PE_I_COLLIDED, PE_I_COLLISIONS, PE_I_POISONED) = range(11)

PE_CELL_EMPTY, PE_CELL_OBSTACLE, PE_CELL_HYDRATED, PE_CELL_THIRSTY = range(4)
PE_MAP_ORIGINAL, PE_MAP_MAZE = 0, 1
MAP_ALGOS = {"original": PE_MAP_ORIGINAL, "maze": PE_MAP_MAZE}


def map_algo_id(name):
    """map_generation_algo of the fork's constructor (plantos_env_new.py:28, 355-358):
    'maze' selects the maze; anything else is 'original', as there."""
    return PE_MAP_MAZE if name == "maze" else PE_MAP_ORIGINAL


PE_REPLAY_CTRL_WORDS = 4
PE_RC_STEPS, PE_RC_DRAWS = 0, 1
PE_ACT_TANH, PE_ACT_RELU = 0, 1
PE_POLICY_ARGMAX, PE_POLICY_SAMPLE = 0, 1
PE_PREC_F32, PE_PREC_BF16 = 0, 1


class PEConfig(ctypes.Structure):
    _fields_ = [
        ("abi_version", ctypes.c_int32), ("grid_size", ctypes.c_int32), ("num_plants", ctypes.c_int32),
        ("num_obstacles", ctypes.c_int32), ("lidar_range", ctypes.c_int32), ("lidar_channels", ctypes.c_int32),
        ("max_steps", ctypes.c_int32), ("autoreset", ctypes.c_int32), ("thirsty_plant_prob", ctypes.c_double),
        ("r_goal", ctypes.c_double), ("r_mistake", ctypes.c_double), ("r_invalid", ctypes.c_double),
        ("r_water_empty", ctypes.c_double), ("r_step", ctypes.c_double), ("r_exploration", ctypes.c_double),
        ("r_revisit", ctypes.c_double), ("r_complete", ctypes.c_double), ("seed", ctypes.c_uint64),
        ("env_id_offset", ctypes.c_uint32), ("map_generation_algo", ctypes.c_int32),
        ("coop_max_done", ctypes.c_int32), ("prefetch_every", ctypes.c_int32), ("obs_codes", ctypes.c_int32),
        ("reserved", ctypes.c_int32 * 3),
    ]


class PEPolicyTower(ctypes.Structure):
    _fields_ = [
        ("n_hidden", ctypes.c_int32), ("hidden", ctypes.c_int32 * 3), ("n_out", ctypes.c_int32),
        ("reserved", ctypes.c_int32 * 3), ("weight", ctypes.c_void_p * 4), ("bias", ctypes.c_void_p * 4),
    ]


class PEPolicyLstm(ctypes.Structure):
    _fields_ = [
        ("hidden", ctypes.c_int32), ("reserved", ctypes.c_int32 * 3), ("weight_ih", ctypes.c_void_p),
        ("weight_hh", ctypes.c_void_p), ("bias_ih", ctypes.c_void_p), ("bias_hh", ctypes.c_void_p),
    ]


class PEPlanInfo(ctypes.Structure):
    """pe_plan_info (csrc/pe_handle.hpp): what pe_create would decide, without a device."""
    _fields_ = [
        ("variant", ctypes.c_int32), ("kernel_name", ctypes.c_char * 64), ("tile_codes", ctypes.c_int32),
        ("stagger", ctypes.c_int32), ("quad_epb", ctypes.c_int32), ("quad_waves", ctypes.c_int32),
        ("coop_max_done", ctypes.c_int32), ("prefetch_every", ctypes.c_int32), ("state_bytes", ctypes.c_uint64),
        ("prefetch_bytes", ctypes.c_uint64),
    ]


class PEPolicyPlanInfo(ctypes.Structure):
    """pe_policy_plan_info (csrc/pe_handle.hpp): what pe_policy_create[_lstm] would decide, without a device."""
    _fields_ = [("env_tile", ctypes.c_int32), ("lds_bytes", ctypes.c_uint64), ("packed_floats", ctypes.c_uint64),
                ("state_floats", ctypes.c_uint64)]


MCTS_ARRAYS = ("cellw", "ulog", "nodes", "rng", "logt", "cellb", "csim", "csg")
MCTS_RNG_WORDS = 628  # one stream in device form: mt[624], pos, saved mt[0], 2 pad


class PEMctsPlanInfo(ctypes.Structure):
    """pe_mcts_plan_info (csrc/pe_handle.hpp): what pe_mcts_create would decide, without a device.
    offset / size: the arrays of MCTS_ARRAYS in the handle's one allocation (size 0: not allocated)."""
    _fields_ = [("kernel", ctypes.c_int32), ("ldsp", ctypes.c_int32), ("ggp", ctypes.c_int32),
                ("clone_blocks", ctypes.c_uint32), ("search_blocks", ctypes.c_uint32),
                ("lds_bytes", ctypes.c_uint64), ("offset", ctypes.c_uint64 * 8), ("size", ctypes.c_uint64 * 8),
                ("total", ctypes.c_uint64)]

    @property
    def kernel_name(self):
        return "pe_mcts_search_lds_kernel" if self.kernel else "pe_mcts_search_kernel"


PE_MB_ROWS, PE_MB_ENVS = 0, 1
PE_MB_MAX_STATES = 4


class PERolloutMb(ctypes.Structure):
    """pe_rollout_mb (csrc/pe_rollout_minibatch.h): one rollout minibatch gather."""
    _fields_ = [
        ("mode", ctypes.c_int32), ("T", ctypes.c_int32), ("n", ctypes.c_int32), ("D", ctypes.c_int32),
        ("B", ctypes.c_int32), ("obs_f32", ctypes.c_int32), ("n_states", ctypes.c_int32), ("H", ctypes.c_int32),
        ("seed", ctypes.c_uint64), ("epoch", ctypes.c_uint64), ("k", ctypes.c_uint64),
        ("buf", ctypes.c_void_p), ("stride", ctypes.c_int64), ("buf_bytes", ctypes.c_int64),
        ("table", ctypes.c_void_p), ("actions", ctypes.c_void_p), ("values", ctypes.c_void_p),
        ("log_probs", ctypes.c_void_p), ("advantages", ctypes.c_void_p), ("returns", ctypes.c_void_p),
        ("starts", ctypes.c_void_p), ("s_actions", ctypes.c_int64), ("s_values", ctypes.c_int64),
        ("s_log_probs", ctypes.c_int64), ("s_advantages", ctypes.c_int64), ("s_returns", ctypes.c_int64),
        ("s_starts", ctypes.c_int64), ("state_src", ctypes.c_void_p * 4), ("ctrl", ctypes.c_void_p),
        ("count", ctypes.c_void_p), ("indices", ctypes.c_void_p), ("out_obs", ctypes.c_void_p),
        ("out_codes", ctypes.c_void_p), ("out_actions", ctypes.c_void_p), ("out_values", ctypes.c_void_p),
        ("out_log_probs", ctypes.c_void_p), ("out_advantages", ctypes.c_void_p), ("out_returns", ctypes.c_void_p),
        ("out_starts", ctypes.c_void_p), ("state_dst", ctypes.c_void_p * 4),
    ]


class PELearnerPlanInfo(ctypes.Structure):
    """pe_learner_plan_info (csrc/pe_learner.h): what an A2C learner is made of, without a device."""
    _fields_ = [("env_tile", ctypes.c_int32), ("n_layers", ctypes.c_int32), ("grad_chunk", ctypes.c_int32),
                ("max_chunks", ctypes.c_int32), ("wgrad_groups", ctypes.c_int32), ("sum_chunks", ctypes.c_int32),
                ("lds_bytes", ctypes.c_uint64), ("n_params", ctypes.c_uint64), ("ws_floats", ctypes.c_uint64),
                ("partial_floats", ctypes.c_uint64), ("sums_doubles", ctypes.c_uint64),
                ("packed_floats", ctypes.c_uint64), ("packed_t_floats", ctypes.c_uint64)]


class PELearnerBufs(ctypes.Structure):
    """pe_learner_bufs (csrc/pe_learner.h): the device buffers a learner works in."""
    _fields_ = [(name, ctypes.c_void_p) for name in
                ("params", "grads", "square_avg", "out", "n_updates", "ws", "partials", "sums", "packed", "packed_t")]


class PlantOSNativeError(RuntimeError):
    pass


def _signatures():
    P, I32, U32, I64, U64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint32, ctypes.c_int64, ctypes.c_uint64
    INT, F, D, STR = ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_char_p
    CP, TP, LP, PP = (ctypes.POINTER(t) for t in (PEConfig, PEPolicyTower, PEPolicyLstm, P))
    step = [P, P, I32] + [P] * 9
    forward_host = [I32, I32, I32, TP, I32, P, I32, U64, U32, U32, P, P, P]
    record = [I32, I32] + [P] * 8 + [D] + [P] * 6
    gae = [I32, I32, I64, I64, I64, I64, P, P, P, P, D, D, P, P]
    abi = {  # in the header's order
        "pe_default_config": (None, [CP, I32, I32, I32, I32, I32]),
        "pe_obs_dim": (I32, [CP]),
        "pe_create": (INT, [CP, I32, I32, PP]),
        "pe_destroy": (INT, [P]),
        "pe_seed": (INT, [P, U64, I32, P]),
        "pe_reset": (INT, [P, P, P, P]),
        "pe_step": (INT, step),
        "pe_step_codes": (INT, step),
        "pe_obs_code_table": (INT, [P, P]),
        "pe_expand_obs_codes": (INT, [P, I32, I32, P, I64, P, P, P, P, P]),
        "pe_get_info": (INT, [P, P, P]),
        "pe_get_state": (INT, [P] * 6),
        "pe_set_state": (INT, [P] * 6),
        "pe_load_maps": (INT, [P, I32, P, P, P, P, P]),
        "pe_synth_actions": (INT, [P, U64, U32, P, P]),
        "pe_poll_errors": (INT, [P, ctypes.POINTER(I32), P]),
        "pe_curriculum_enable": (INT, [P, D, D, D, I32, I32, P]),
        "pe_curriculum_disable": (INT, [P]),
        "pe_curriculum_get": (INT, [P, P, P, P]),
        "pe_pystream_create": (INT, [CP, I64, PP]),
        "pe_pystream_next": (INT, [P, I32, P, P]),
        "pe_pystream_getrandbits32": (U32, [P]),
        "pe_pystream_destroy": (INT, [P]),
        "pe_mcts_create": (INT, [P, I32, D, I32, PP]),
        "pe_mcts_destroy": (INT, [P]),
        "pe_mcts_seed": (INT, [P, P, U32, P]),
        "pe_mcts_set_rng": (INT, [P, P, P]),
        "pe_mcts_get_rng": (INT, [P, P, P]),
        "pe_mcts_search": (INT, [P] * 7),
        "pe_mcts_kernel_name": (INT, [P, ctypes.POINTER(STR)]),
        "pe_render_tables": (INT, [CP, I32, P, P]),
        "pe_render": (INT, [P, I32, P, I32, P, I64, I64, P]),
        "pe_policy_create": (INT, [P, I32, TP, I32, I32, PP]),
        "pe_policy_destroy": (INT, [P]),
        "pe_policy_load": (INT, [P, TP, P]),
        "pe_policy_forward": (INT, [P, P, I32, I32, U64, U32, P, P, P, P]),
        "pe_policy_forward_rows": (INT, [P, I32, P, I32, P, P, P, P]),
        "pe_policy_forward_host": (INT, forward_host),
        "pe_policy_math_host": (INT, [I32, I32, P, P]),
        "pe_policy_env_tile": (I32, [P]),
        "pe_policy_create_lstm": (INT, [P, I32, LP, TP, I32, I32, PP]),
        "pe_policy_load_lstm": (INT, [P, LP, TP, P]),
        "pe_policy_forward_lstm": (INT, [P, P, I32, P, P, I32, U64, U32, P, P, P, P]),
        "pe_policy_lstm_reset_state": (INT, [P, P]),
        "pe_policy_lstm_get_state": (INT, [P, I32, P, P, P]),
        "pe_policy_lstm_set_state": (INT, [P, I32, P, P, P]),
        "pe_policy_lstm_forward_host": (INT, [I32, I32, I32, LP, TP, I32, P, P, P, P, I32, U64, U32, U32, P, P, P]),
        "pe_policy_value": (INT, [P, P, I32, P, P, P, P]),
        "pe_policy_value_lstm": (INT, [P, P, I32, P, P, P, P, P, P]),
        "pe_policy_create_prec": (INT, [P, I32, TP, I32, I32, I32, PP]),
        "pe_policy_precision": (I32, [P]),
        "pe_policy_forward_host_bf16": (INT, forward_host),
        "pe_rollout_record": (INT, record + [P]),
        "pe_rollout_record_host": (INT, record),
        "pe_logf_host": (INT, [I32, P, P]),
        "pe_rollout_gae": (INT, gae + [P]),
        "pe_rollout_gae_host": (INT, gae),
        "pe_replay_select": (INT, [I32, I32, P, P, P, U64, U32, P, P, P]),
        "pe_replay_select_host": (INT, [I32, I32, P, F, U64, U64, U32, P, P]),
        "pe_replay_store": (INT, [I32] * 5 + [P] * 19),
        "pe_replay_sample": (INT, [I32] * 4 + [P] * 5 + [U64] + [P] * 8),
        "pe_replay_sample_indices_host": (INT, [I32, I32, I32, U64, U64, U64, P]),
        "pe_replay_target": (INT, [I32, I32, P, P, P, D, P, P]),
        "pe_replay_target_host": (INT, [I32, I32, P, P, P, D, P]),
        "pe_num_envs": (I32, [P]),
        "pe_kernel_variant": (I32, [P]),
        "pe_kernel_name": (STR, [P]),
        "pe_prefetch_every": (I32, [P]),
        "pe_state_bytes": (U64, [P]),
        "pe_last_error": (STR, []),
    }
    plan = [I32, I32, I32, I32, LP, TP, I32, I32]
    internal = {
        "pe_internal_plan": (INT, [CP, I32, I32, ctypes.POINTER(PEPlanInfo)]),
        "pe_internal_policy_plan": (INT, plan + [ctypes.POINTER(PEPolicyPlanInfo)]),
        "pe_internal_policy_plan_prec": (INT, plan + [I32, ctypes.POINTER(PEPolicyPlanInfo)]),
        "pe_internal_mcts_plan": (INT, [I32, I32, I32, I32, ctypes.POINTER(PEMctsPlanInfo)]),
        "pe_internal_mcts_rng_to_device_host": (INT, [P, I32, P]),
        "pe_internal_mcts_rng_from_device_host": (INT, [P, P, P]),
        # csrc/pe_rollout_minibatch.h
        "pe_internal_rollout_minibatch_check": (INT, [ctypes.POINTER(PERolloutMb)]),
        "pe_internal_rollout_minibatch": (INT, [ctypes.POINTER(PERolloutMb), P]),
        "pe_internal_rollout_perm_host": (INT, [I64, U64, U64, I32, I64, I64, P]),
        "pe_internal_rollout_adv_norm": (INT, [I32, I32, I64, P, P, P, P, P]),
        "pe_internal_rollout_adv_norm_host": (INT, [I32, I32, I64, P, P]),
        # csrc/pe_learner.h
        "pe_internal_learner_plan": (INT, [I32, I32, I32, I32, TP, I32, I32, ctypes.POINTER(PELearnerPlanInfo)]),
        "pe_internal_learner_create": (INT, [P, I32, ctypes.POINTER(PELearnerBufs), PP]),
        "pe_internal_learner_destroy": (INT, [P]),
        "pe_internal_learner_repack": (INT, [P, P]),
        "pe_internal_learner_update": (INT, [P, I32, P, I32, P, P, P] + [D] * 6 + [P]),
        "pe_internal_learner_update_host": (INT, [I32, I32, I32, TP, I32, P, P, P, P] + [D] * 6 + [I32, P, P, P]),
    }
    return abi, internal


# name -> (restype, [argtypes]).  SIGNATURES: every function of include/plantos_batch.h
# (tests/test_capi_symbols.py checks each entry against the header's prototype);
# INTERNAL_SIGNATURES: the plan entry points of csrc/pe_handle.hpp (with the MCTS stream
# conversions declared beside pe_internal_mcts_plan), the rollout minibatches of
# csrc/pe_rollout_minibatch.h and the A2C learner of csrc/pe_learner.h, which are not part of the ABI.
SIGNATURES, INTERNAL_SIGNATURES = _signatures()
EXPORTS = list(SIGNATURES)

_lib = None


def lib():
    """Load libplantos_hip.so (built by rl-env_amd/build.py); raise if absent.  A function the
    loaded library lacks (an older build given through PLANTOS_HIP_LIB) stays unbound: using it
    raises AttributeError."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PlantOSNativeError(
            f"{LIB_PATH} not found: build it with `python rl-env_amd/build.py` "
            "(there is no CPU fallback for the PlantOS hot path)")
    L = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in {**SIGNATURES, **INTERNAL_SIGNATURES}.items():
        fn = getattr(L, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


def check(rc, what):
    if rc != PE_OK:
        msg = lib().pe_last_error().decode(errors="replace")
        if rc == PE_ERR_ARG:
            raise ValueError(f"{what}: {msg}")
        if rc == PE_ERR_NOROOM:
            raise ValueError(f"{what}: {msg}")
        raise PlantOSNativeError(f"{what} failed ({rc}): {msg}")


def ptr(x):
    """The data pointer of a numpy array or a torch tensor as a c_void_p; None for None."""
    if x is None:
        return None
    return ctypes.c_void_p(x.data_ptr() if hasattr(x, "data_ptr") else x.ctypes.data)


def stream_ptr(device):
    """torch's current stream on `device` (a torch.device or an index) as a c_void_p."""
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


_TENSOR = None  # torch.Tensor, once torch is in use (this module imports without it)


def on_device(x, dev_index, dtypes, shape=None):
    """Whether x is a plain torch tensor on device `dev_index`, contiguous, of one of `dtypes` and
    of `shape` (None: any shape)."""
    global _TENSOR
    if _TENSOR is None:
        import torch
        _TENSOR = torch.Tensor
    return (type(x) is _TENSOR and x.is_cuda and x.get_device() == dev_index and x.is_contiguous()
            and x.dtype in dtypes and (shape is None or tuple(x.shape) == shape))


def plan(cfg, n_envs, num_cus):
    """pe_internal_plan: the kernel, reset paths and allocation sizes pe_create would choose for
    `cfg` and `n_envs` on a device of `num_cus` CUs.  Needs no device; raises as pe_create does."""
    info = PEPlanInfo()
    check(lib().pe_internal_plan(ctypes.byref(cfg), int(n_envs), int(num_cus), ctypes.byref(info)), "pe_create")
    return info


def policy_plan(obs_dim, n_envs, num_cus, lstms, shapes, activation, env_tile=0, precision=None):
    """pe_internal_policy_plan: the env tile, LDS and buffer sizes pe_policy_create (lstms None) or
    pe_policy_create_lstm would choose for obs rows of `obs_dim` values, `n_envs` envs and a device of
    `num_cus` CUs.  lstms / shapes: PEPolicyLstm / PEPolicyTower arrays.  precision: None, or a
    PE_PREC_* for pe_internal_policy_plan_prec (what pe_policy_create_prec would choose).  Needs no
    device; raises as the create call does."""
    info = PEPolicyPlanInfo()
    if precision is not None:
        check(lib().pe_internal_policy_plan_prec(int(obs_dim), int(n_envs), int(num_cus), len(shapes), lstms, shapes,
                                                 int(activation), int(env_tile), int(precision), ctypes.byref(info)),
              "pe_policy_create_prec" if lstms is None else "pe_policy_create_lstm")
        return info
    check(lib().pe_internal_policy_plan(int(obs_dim), int(n_envs), int(num_cus), len(shapes), lstms, shapes,
                                        int(activation), int(env_tile), ctypes.byref(info)),
          "pe_policy_create" if lstms is None else "pe_policy_create_lstm")
    return info


def mcts_plan(grid_size, n_envs, n_simulations, max_depth):
    """pe_internal_mcts_plan: the search kernel, its LDS and grids and the layout of the allocation
    pe_mcts_create would choose over a batch of `n_envs` envs of grid side `grid_size`.  Needs no
    device; raises as pe_mcts_create does."""
    info = PEMctsPlanInfo()
    check(lib().pe_internal_mcts_plan(int(grid_size), int(n_envs), int(n_simulations), int(max_depth),
                                      ctypes.byref(info)), "pe_mcts_create")
    return info


def mcts_rng_to_device(key, pos):
    """One np.random stream, numpy's (key uint32 [624], pos) -> the device form uint32 [628], as
    pe_mcts_set_rng stores it (and refuses it).  Host only."""
    import numpy as np
    key = np.ascontiguousarray(key, np.uint32).reshape(624)
    dev = np.zeros(MCTS_RNG_WORDS, np.uint32)
    check(lib().pe_internal_mcts_rng_to_device_host(ptr(key), int(pos), ptr(dev)), "pe_mcts_set_rng")
    return dev


def mcts_rng_from_device(dev):
    """The device form uint32 [628] -> numpy's (key uint32 [624], pos), as pe_mcts_get_rng reports it.
    Host only."""
    import numpy as np
    dev = np.ascontiguousarray(dev, np.uint32).reshape(MCTS_RNG_WORDS)
    key, pos = np.zeros(624, np.uint32), ctypes.c_int32()
    check(lib().pe_internal_mcts_rng_from_device_host(ptr(dev), ptr(key), ctypes.byref(pos)), "pe_mcts_get_rng")
    return key, pos.value


def default_config(grid_size, num_plants, num_obstacles, lidar_range, lidar_channels):
    c = PEConfig()
    lib().pe_default_config(ctypes.byref(c), grid_size, num_plants, num_obstacles, lidar_range, lidar_channels)
    return c


class PyStream:
    """Host-side CPython `random` map stream (seed-exact reset layouts,
    plantos_env.py:338-372 after random.seed(seed)); see include/plantos_batch.h."""

    def __init__(self, grid_size, num_plants, num_obstacles, seed, thirsty_plant_prob=0.7,
                 map_generation_algo="original"):
        import numpy as np
        self._np = np
        self.G = grid_size
        c = default_config(grid_size, num_plants, num_obstacles, 1, 1)
        c.thirsty_plant_prob = float(thirsty_plant_prob)
        c.map_generation_algo = map_algo_id(map_generation_algo)
        h = ctypes.c_void_p()
        check(lib().pe_pystream_create(ctypes.byref(c), int(seed), ctypes.byref(h)), "pe_pystream_create")
        self._h = h

    def next(self, k):
        """next k maps in stream order: cells u8[k,G,G], rover i32[k,2] (numpy)."""
        np = self._np
        cells = np.zeros((k, self.G, self.G), np.uint8)
        rover = np.zeros((k, 2), np.int32)
        check(lib().pe_pystream_next(self._h, int(k), ptr(cells), ptr(rover)), "pe_pystream_next")
        return cells, rover

    def getrandbits32(self):
        return int(lib().pe_pystream_getrandbits32(self._h))

    def close(self):
        if getattr(self, "_h", None):
            lib().pe_pystream_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass
