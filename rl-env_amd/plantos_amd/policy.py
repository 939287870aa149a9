"""Policy: batched MLP policy inference on the device, from a batch's obs to its next actions.

The C-ABI's pe_policy_* (include/plantos_batch.h, "Policy inference"): one fused HIP kernel
reads the obs -- as the byte codes an ``obs_codes`` batch writes, or as f32 --, evaluates an
SB3-shaped MLP (A2C's separate pi / vf towers with Tanh, A2C_training.py:229-247; DQN's
QNetwork with ReLU, trainingCode.py:226-246) and writes actions, logits / Q-values and
values.  Outputs are defined bit for bit by the host twin (`host_forward`), which needs no
device.  Learners stay out of scope: `Policy.load` takes the weights a learner produced.

    policy = Policy.from_state_dict(venv, model.policy.state_dict())
    obs = venv.reset()
    for _ in range(steps):
        actions, logits, values = policy.act()      # reads the batch's current obs
        obs, rewards, dones, infos = venv.step(actions)

RecurrentPolicy is the same stage for sb3_contrib's RecurrentPPO("MlpLstmPolicy") with one
LSTM layer per tower (trainingCode.py:140-162): the LSTM state lives on the device, and the
episode-start flags are the step's own terminated / truncated tensors.

    policy = RecurrentPolicy.from_state_dict(batch, model.policy.state_dict())
    batch.reset()
    actions, _, _ = policy.act()                    # zero state: an episode start
    for _ in range(steps):
        obs, rewards, terminated, truncated = batch.step(actions)
        actions, logits, values = policy.act(episode_start=(terminated, truncated))
"""
import ctypes
import re

import numpy as np

from . import _capi as C
from ._capi import on_device

ACTIVATIONS = {"tanh": C.PE_ACT_TANH, "relu": C.PE_ACT_RELU}
PRECISIONS = {"f32": C.PE_PREC_F32, "bf16": C.PE_PREC_BF16}


def check_towers(towers):
    """ValueError unless `towers` ([[h1, .., out], ..]) is a shape the kernel evaluates:
    1 or 2 towers of 1..3 hidden layers (widths multiples of 32 in 32..512) and a head;
    tower 0's head 2..8 wide, tower 1's 1 wide."""
    towers = [[int(v) for v in t] for t in towers]
    if not 1 <= len(towers) <= 2:
        raise ValueError("a policy has 1 or 2 towers")
    for i, t in enumerate(towers):
        if not 2 <= len(t) <= 4:
            raise ValueError(f"tower {i}: 1..3 hidden layers and a head, got {t}")
        for w in t[:-1]:
            if w < 32 or w > 512 or w % 32:
                raise ValueError(f"tower {i}: hidden widths must be multiples of 32 in 32..512, got {w}")
        if i == 0 and not 2 <= t[-1] <= 8:
            raise ValueError(f"tower 0's head must have 2..8 outputs, got {t[-1]}")
        if i == 1 and t[-1] != 1:
            raise ValueError(f"tower 1's head must have 1 output, got {t[-1]}")
    return towers


def _linears(sd, prefix):
    """[(weight, bias), ..] of `prefix`.{0,2,4,..} (an nn.Sequential of Linear, activation, ..)."""
    idx = sorted({int(m.group(1)) for k in sd for m in [re.fullmatch(re.escape(prefix) + r"\.(\d+)\.weight", k)] if m})
    if idx != list(range(0, 2 * len(idx), 2)):
        raise ValueError(f"{prefix}: expected Linear layers at indices 0, 2, 4, .., found {idx}")
    return [(sd[f"{prefix}.{i}.weight"], sd[f"{prefix}.{i}.bias"]) for i in idx]


def parse_state_dict(sd, activation=None):
    """(towers, activation, tensors) of a Stable-Baselines3 policy state dict:

    - ActorCriticPolicy with separate nets (net_arch=[256,256] in SB3 2.2.1):
      mlp_extractor.policy_net.{0,2,..}, action_net -> tower 0; mlp_extractor.value_net.*,
      value_net -> tower 1; Tanh unless told otherwise;
    - DQN: q_net.q_net.{0,2,..} (the last Linear is the head) -> one tower, ReLU
      (q_net_target.* is ignored).

    tensors[i] = [(weight, bias), ..] of tower i, hidden layers then the head.  A shared
    trunk (mlp_extractor.shared_net.*) or an unsupported width raises ValueError."""
    keys = list(sd)
    if any(k.startswith("mlp_extractor.shared_net") for k in keys):
        raise ValueError("shared-trunk policies (mlp_extractor.shared_net) are not supported: "
                         "separate pi / vf towers only")
    if any(k.startswith("mlp_extractor.policy_net.") for k in keys):
        for need in ("action_net.weight", "action_net.bias", "value_net.weight", "value_net.bias"):
            if need not in sd:
                raise ValueError(f"state dict lacks {need}")
        pi = _linears(sd, "mlp_extractor.policy_net") + [(sd["action_net.weight"], sd["action_net.bias"])]
        vf = _linears(sd, "mlp_extractor.value_net") + [(sd["value_net.weight"], sd["value_net.bias"])]
        tensors, act = [pi, vf], "tanh"
    elif any(k.startswith("q_net.q_net.") for k in keys):
        tensors, act = [_linears(sd, "q_net.q_net")], "relu"
    else:
        raise ValueError("unrecognised state dict: expected mlp_extractor.policy_net.* / action_net / value_net "
                         "(ActorCriticPolicy) or q_net.q_net.* (DQN)")
    for tw in tensors:
        k = tw[0][0].shape[1]
        for w, b in tw:
            if w.dim() != 2 or b.dim() != 1 or w.shape[0] != b.shape[0] or w.shape[1] != k:
                raise ValueError("layer shapes do not chain")
            k = w.shape[0]
    if len({tw[0][0].shape[1] for tw in tensors}) != 1:
        raise ValueError("towers read different obs lengths")
    towers = check_towers([[w.shape[0] for w, _ in tw] for tw in tensors])
    return towers, (activation or act), tensors


def _tower_structs(towers, tensors=None, keep=None):
    """ctypes pe_policy_tower array; tensors[i][l] = (weight, bias) as numpy arrays or torch
    tensors (their pointers are taken; `keep` collects what must stay alive)."""
    arr = (C.PEPolicyTower * len(towers))()
    for i, t in enumerate(towers):
        arr[i].n_hidden = len(t) - 1
        for l, w in enumerate(t[:-1]):
            arr[i].hidden[l] = w
        arr[i].n_out = t[-1]
        if tensors is None:
            continue
        if len(tensors[i]) != len(t):
            raise ValueError(f"tower {i}: expected {len(t)} (weight, bias) pairs, got {len(tensors[i])}")
        for l, (w, b) in enumerate(tensors[i]):
            arr[i].weight[l], arr[i].bias[l] = C.ptr(w), C.ptr(b)
            if keep is not None:
                keep += [w, b]
    return arr


def _check_tensor_shapes(towers, tensors, obs_dim):
    if len(tensors) != len(towers):
        raise ValueError(f"expected {len(towers)} towers of tensors, got {len(tensors)}")
    for i, t in enumerate(towers):
        if len(tensors[i]) != len(t):
            raise ValueError(f"tower {i}: expected {len(t)} (weight, bias) pairs, got {len(tensors[i])}")
        k = obs_dim
        for l, (w, b) in enumerate(tensors[i]):
            if tuple(w.shape) != (t[l], k) or tuple(b.shape) != (t[l],):
                raise ValueError(f"tower {i} layer {l}: expected weight {(t[l], k)} and bias {(t[l],)}, "
                                 f"got {tuple(w.shape)} and {tuple(b.shape)}")
            k = t[l]


def host_forward(towers, tensors, activation, obs, deterministic=True, seed=0, env_id_offset=0, t=0,
                 precision="f32"):
    """The host twin (pe_policy_forward_host; pe_policy_forward_host_bf16 for precision "bf16"):
    the definition of the policy's outputs in plain C++, no device.  obs f32 [n, D] (numpy);
    tensors as parse_state_dict returns them (torch CPU tensors or numpy).  Returns (actions
    i32 [n], logits f32 [n, A], values f32 [n] or None) as numpy arrays."""
    towers = check_towers(towers)
    if precision not in PRECISIONS:
        raise ValueError(f"precision must be one of {sorted(PRECISIONS)}")
    if activation not in ACTIVATIONS:
        raise ValueError(f"activation must be one of {sorted(ACTIVATIONS)}")
    obs = np.ascontiguousarray(obs, np.float32)
    if obs.ndim != 2:
        raise ValueError("obs must be [n, D]")
    n, D = obs.shape
    host = [[(np.ascontiguousarray(_np(w), np.float32), np.ascontiguousarray(_np(b), np.float32)) for w, b in tw]
            for tw in tensors]
    _check_tensor_shapes(towers, host, D)
    keep = []
    arr = _tower_structs(towers, host, keep)
    A = towers[0][-1]
    actions = np.zeros(n, np.int32)
    logits = np.zeros((n, A), np.float32)
    values = np.zeros(n, np.float32) if len(towers) == 2 else None
    twin = C.lib().pe_policy_forward_host_bf16 if precision == "bf16" else C.lib().pe_policy_forward_host
    C.check(twin(
        n, D, len(towers), arr, ACTIVATIONS[activation], C.ptr(obs),
        C.PE_POLICY_ARGMAX if deterministic else C.PE_POLICY_SAMPLE, int(seed) & 0xFFFFFFFFFFFFFFFF,
        int(env_id_offset) & 0xFFFFFFFF, int(t) & 0xFFFFFFFF, C.ptr(actions), C.ptr(logits), C.ptr(values)),
        "pe_policy_forward_host")
    return actions, logits, values


def math_host(which, x):
    """pe_tanhf ("tanh"), pe_expf ("exp"), pe_sigmoidf ("sigmoid") or pe_logf ("log") of a float32
    array, as the twins and the kernels compute them."""
    x = np.ascontiguousarray(x, np.float32)
    y = np.empty_like(x)
    if which == "log":  # (a function of its own: pe_policy_math_host's selectors stay 0..2)
        C.check(C.lib().pe_logf_host(x.size, C.ptr(x), C.ptr(y)), "pe_logf_host")
        return y
    C.check(C.lib().pe_policy_math_host({"tanh": 0, "exp": 1, "sigmoid": 2}[which], x.size, C.ptr(x), C.ptr(y)),
            "pe_policy_math_host")
    return y


def _np(x):
    return x if isinstance(x, np.ndarray) else x.detach().cpu().numpy()


def _to_dev_f32(x, device):
    """x as a contiguous float32 tensor on `device` (one that already is one is returned as it is)."""
    import torch
    return torch.as_tensor(x).detach().to(device=device, dtype=torch.float32).contiguous()


class _PolicyBase:
    """What Policy and RecurrentPolicy share: construction around the subclass's `_create`, the
    handle, and the argument checks of act / value."""

    def __init__(self, batch_or_venv, towers, activation, seed, env_tile):
        import torch
        self._torch = torch
        self.batch = getattr(batch_or_venv, "batch", batch_or_venv)
        self.towers = check_towers(towers)
        if activation not in ACTIVATIONS:
            raise ValueError(f"activation must be one of {sorted(ACTIVATIONS)}")
        self.activation = activation
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.t = 0  # sampler step counter: act(deterministic=False) without t uses and advances it
        b = self.batch
        p = ctypes.c_void_p()
        with torch.cuda.device(b.device):
            self._create(int(env_tile or 0), ctypes.byref(p))
        self._p = p
        n, A, dev = b.num_envs, self.towers[0][-1], b.device
        self.actions = torch.zeros(n, dtype=torch.int32, device=dev)
        self.logits = torch.zeros((n, A), dtype=torch.float32, device=dev)
        self.values = torch.zeros(n, dtype=torch.float32, device=dev) if len(self.towers) == 2 else None
        self._loaded = None

    @property
    def env_tile(self):
        return int(C.lib().pe_policy_env_tile(self._handle()))

    def _handle(self):
        if not self._p:
            raise ValueError(f"{type(self).__name__} is closed")
        return self._p

    def _stream(self):  # (C.stream_ptr's value as a plain int: every act / value call passes through here)
        return self._torch.cuda.current_stream(self.batch._dev_index).cuda_stream

    def close(self):
        if getattr(self, "_p", None):
            C.check(C.lib().pe_policy_destroy(self._p), "pe_policy_destroy")
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def _obs_arg(self, obs, any_rows=False):
        """(obs, codes): the checked obs of a forward -- None reads the batch's own; [n, D], or with
        any_rows any number >= 1 of rows."""
        torch, b = self._torch, self.batch
        n, D = b.num_envs, b.obs_dim
        if obs is None and not any_rows:
            obs = b.obs
        if not (on_device(obs, b._dev_index, (torch.float32, torch.uint8), None if any_rows else (n, D))
                and (not any_rows or (obs.dim() == 2 and obs.shape[0] >= 1 and obs.shape[1] == D))):
            shape = f"(rows >= 1, {D})" if any_rows else (n, D)
            raise ValueError(f"obs must be a contiguous float32 or uint8 tensor of shape {shape} on {b.device}")
        codes = obs.dtype is torch.uint8
        if codes and not b.obs_codes:
            raise ValueError("uint8 obs codes need a batch created with obs_codes=True")
        return obs, codes

    def _out_arg(self, out, rows):
        """(actions, logits, values) of `rows` rows to write: `out`, or the policy's own tensors."""
        torch, b = self._torch, self.batch
        a, lg, v = out if out is not None else (self.actions, self.logits, self.values)
        A = self.towers[0][-1]
        for name, x, dt, shape in (("actions", a, torch.int32, (rows,)), ("logits", lg, torch.float32, (rows, A)),
                                   ("values", v, torch.float32, (rows,))):
            if x is None and name != "actions":
                continue  # an output not asked for
            if not on_device(x, b._dev_index, (dt,), shape):
                raise ValueError(f"{name} must be a contiguous {dt} tensor of shape {shape} on {b.device}")
        if v is not None and len(self.towers) < 2:
            raise ValueError("a one-tower policy has no values")
        return a, lg, v

    def _sampler_step(self, deterministic, t):
        """(mode, step) of a forward; sampling without t uses and advances the policy's counter."""
        if deterministic:
            return C.PE_POLICY_ARGMAX, 0
        if t is None:
            t, self.t = self.t, self.t + 1
        return C.PE_POLICY_SAMPLE, int(t) & 0xFFFFFFFF

    def _flag_arg(self, x, name):
        """The pointer of a per-env flag tensor (uint8 / bool [n]), or None."""
        torch, b = self._torch, self.batch
        if x is None:
            return None
        if not on_device(x, b._dev_index, (torch.uint8, torch.bool), (b.num_envs,)):
            raise ValueError(f"{name} must be a contiguous uint8 or bool tensor of shape {(b.num_envs,)} on {b.device}")
        return x.data_ptr()

    def _value_args(self, obs, select, out):
        """The checked arguments of value(): (obs, codes, want pointer, unless pointer, out).
        ValueError as act's."""
        b = self.batch
        if len(self.towers) < 2:
            raise ValueError("a one-tower policy has no values")
        obs, codes = self._obs_arg(obs)
        if isinstance(select, (tuple, list)):
            if len(select) != 2:
                raise ValueError("select must be a tensor or a pair (want, unless) of tensors")
            want, unless = select
        else:
            want, unless = select, None
        want, unless = self._flag_arg(want, "select / want"), self._flag_arg(unless, "unless")
        if out is None:
            out = self.values
        if not on_device(out, b._dev_index, (self._torch.float32,), (b.num_envs,)):
            raise ValueError(f"out must be a contiguous float32 tensor of shape {(b.num_envs,)} on {b.device}")
        return obs, codes, want, unless, out


class Policy(_PolicyBase):
    """An MLP policy over the obs of a PlantOSBatch (or of a PlantOSVecEnv's batch).

    towers: [[h1, .., A], [h1, .., 1]] (pi and vf nets) or [[h1, .., A]] (a Q-network);
    activation "tanh" or "relu"; seed keys the action sampler (deterministic=False);
    env_tile (32 / 64, None = the library's choice) is the kernel's envs per workgroup: it
    changes speed, never results.  precision "f32" (the default) or "bf16": bf16 rounds the
    obs, the hidden weights and the hidden activations to bf16 and accumulates in f32 on the
    bf16 MFMA (include/plantos_batch.h, "Reduced-precision policy inference"; `host_forward`
    is then the bf16 twin); biases, heads and outputs stay f32.  Weights start at zero: `load`
    them.  Close the policy before its batch."""

    def __init__(self, batch_or_venv, towers=((256, 256, 5), (256, 256, 1)), activation="tanh", seed=0,
                 env_tile=None, precision="f32"):
        if precision not in PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(PRECISIONS)}, got {precision!r}")
        self._precision = precision
        super().__init__(batch_or_venv, towers, activation, seed, env_tile)

    def _create(self, env_tile, out):
        C.check(C.lib().pe_policy_create_prec(self.batch.handle, len(self.towers), _tower_structs(self.towers),
                                              ACTIVATIONS[self.activation], env_tile, PRECISIONS[self._precision], out),
                "pe_policy_create")

    @property
    def precision(self):
        """"f32" or "bf16", as given to the constructor."""
        return self._precision

    @classmethod
    def from_state_dict(cls, env, sd, activation=None, **kw):
        """A Policy shaped and loaded from a Stable-Baselines3 state dict (parse_state_dict)."""
        towers, act, tensors = parse_state_dict(sd, activation)
        p = cls(env, towers, act, **kw)
        p.load(tensors)
        return p

    def load(self, sd_or_tensors):
        """Repack new weights into the policy: one kernel on the current stream, ordered with
        the forwards around it (a learner calls this after every optimizer step).  Takes an
        SB3 state dict or [[(weight, bias), ..], ..] per tower (hidden layers, then the head);
        f32 contiguous tensors on the batch's device are read in place, anything else (CPU
        tensors, numpy, other dtypes) is uploaded first."""
        torch = self._torch
        tensors = sd_or_tensors
        if isinstance(tensors, dict):
            towers, _, tensors = parse_state_dict(tensors)
            if towers != self.towers:
                raise ValueError(f"state dict has towers {towers}, the policy {self.towers}")
        _check_tensor_shapes(self.towers, tensors, self.batch.obs_dim)
        dev = self.batch.device
        devt = [[tuple(_to_dev_f32(x, dev) for x in wb) for wb in tw] for tw in tensors]
        keep = []
        arr = _tower_structs(self.towers, devt, keep)
        with torch.cuda.device(dev):
            C.check(C.lib().pe_policy_load(self._handle(), arr, self.batch._stream()), "pe_policy_load")
        self._loaded = devt  # alive until the next load (the kernel reads them on the stream)
        return self

    def act(self, obs=None, deterministic=True, t=None, out=None):
        """(actions i32 [n], logits f32 [n, A], values f32 [n] or None), device tensors.

        obs: None reads the batch's current obs in its io buffer (byte codes on an
        ``obs_codes`` batch, which holds them from the first step on; f32 otherwise), or a
        contiguous device tensor [n, D], uint8 codes (obs_codes batches) or float32.
        deterministic=False samples with the project's own Philox sampler at step `t` (None:
        the policy's counter, which then advances).  out: (actions, logits, values) tensors to
        write instead of the policy's own (values None for a one-tower policy).  One kernel on
        the current stream; no sync, no allocation: graph-capturable."""
        obs, codes = self._obs_arg(obs)
        a, lg, v = self._out_arg(out, self.batch.num_envs)
        mode, step = self._sampler_step(deterministic, t)
        rc = C.lib().pe_policy_forward(self._handle(), obs.data_ptr(), int(codes), mode, self.seed, step, a.data_ptr(),
                                       lg.data_ptr() if lg is not None else None,
                                       v.data_ptr() if v is not None else None, self._stream())
        if rc:
            C.check(rc, "pe_policy_forward")
        return a, lg, v

    def act_rows(self, obs, out=None):
        """(actions i32 [rows], logits f32 [rows, A], values f32 [rows] or None) of any number of
        obs rows: the argmax forward over a contiguous device tensor [rows, D], rows >= 1,
        uint8 codes (obs_codes batches) or float32 -- a sampled minibatch rather than the
        batch's n envs (pe_policy_forward_rows: the same kernel, the same bits per row as
        `host_forward`).  out: (actions, logits, values) tensors of those shapes to write
        (logits / values may be None: not asked for); without it new tensors are allocated.
        One kernel on the current stream; no sync, and with `out` no allocation:
        graph-capturable."""
        torch, b = self._torch, self.batch
        obs, codes = self._obs_arg(obs, any_rows=True)
        rows, A = int(obs.shape[0]), self.towers[0][-1]
        if out is None:
            out = (torch.empty(rows, dtype=torch.int32, device=b.device),
                   torch.empty((rows, A), dtype=torch.float32, device=b.device),
                   torch.empty(rows, dtype=torch.float32, device=b.device) if len(self.towers) == 2 else None)
        a, lg, v = self._out_arg(out, rows)
        rc = C.lib().pe_policy_forward_rows(self._handle(), rows, obs.data_ptr(), int(codes), a.data_ptr(),
                                            lg.data_ptr() if lg is not None else None,
                                            v.data_ptr() if v is not None else None, self._stream())
        if rc:
            C.check(rc, "pe_policy_forward_rows")
        return a, lg, v

    def value(self, obs=None, select=None, out=None):
        """The values f32 [n] alone: the value tower's head, bit for bit what `act` returns as
        values for the same obs, without the action tower and the sampler (`t` stays).

        obs: as `act`.  select: None (every env), a uint8 / bool device tensor [n] (want), or
        a pair (want, unless): env e is evaluated iff want[e] != 0 and unless[e] == 0 -- a
        step's (truncated, terminated) select the envs cut by the time limit only.  Entries
        of envs not selected are left as they were, and a tile of envs none of which is
        selected costs no work.  out: a float32 tensor [n] to write instead of the policy's
        own values.  ValueError for a one-tower policy.  One kernel on the current stream; no
        sync, no allocation: graph-capturable."""
        obs, codes, want, unless, out = self._value_args(obs, select, out)
        rc = C.lib().pe_policy_value(self._handle(), obs.data_ptr(), int(codes), want, unless, out.data_ptr(),
                                     self._stream())
        if rc:
            C.check(rc, "pe_policy_value")
        return out

    def host_forward(self, obs_np, tensors=None, deterministic=True, t=0):
        """The host twin on f32 obs rows [n, D] (numpy) with the weights last loaded (or
        `tensors`); env ids start at the batch's env_id_offset, the sampler uses the policy's
        seed.  Returns numpy (actions, logits, values or None)."""
        tensors = tensors if tensors is not None else self._loaded
        if tensors is None:
            raise ValueError("no weights loaded")
        return host_forward(self.towers, tensors, self.activation, obs_np, deterministic=deterministic,
                            seed=self.seed, env_id_offset=int(self.batch.cfg.env_id_offset), t=t,
                            precision=self._precision)


# ------------------------------------------------------------------ recurrent policy
LSTM_KEYS = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")


def check_lstm_hidden(hidden):
    """ValueError unless `hidden` is an LSTM size the kernel evaluates: a multiple of 32 in 32..512."""
    hidden = int(hidden)
    if hidden > 512:
        raise ValueError(f"lstm hidden size {hidden} > 512 is not supported: the h tile no longer fits LDS "
                         "(that needs a K-streamed GEMM kernel)")
    if hidden < 32 or hidden % 32:
        raise ValueError(f"lstm hidden size must be a multiple of 32 in 32..512, got {hidden}")
    return hidden


def parse_lstm_state_dict(sd, activation=None):
    """(H, towers, activation, lstm_tensors, mlp_tensors) of an sb3_contrib
    RecurrentActorCriticPolicy state dict with n_lstm_layers=1 and no shared LSTM:

    lstm_actor.{weight_ih_l0, weight_hh_l0, bias_ih_l0, bias_hh_l0}, mlp_extractor.policy_net.*,
    action_net -> tower 0; lstm_critic.*, mlp_extractor.value_net.*, value_net -> tower 1
    (enable_critic_lstm=True).  A dict without lstm_critic.* and value nets is an actor-only
    policy (what predict() evaluates).  lstm_tensors[i] = (w_ih, w_hh, b_ih, b_hh);
    mlp_tensors[i] = [(weight, bias), ..] as parse_state_dict returns them.  ValueError for the
    critic as a Linear (critic.weight: enable_critic_lstm=False, also what shared_lstm=True
    leaves), more LSTM layers (*_l1 keys), a shared trunk, unsupported widths or shapes that
    do not chain.  Tanh unless told otherwise."""
    keys = list(sd)
    if any(k.startswith("critic.") for k in keys):
        raise ValueError("the critic as a Linear layer (critic.*: enable_critic_lstm=False or shared_lstm=True) "
                         "is not supported: enable_critic_lstm=True or an actor-only dict")
    if any(re.fullmatch(r"lstm_(actor|critic)\..*_l[1-9]\d*(_reverse)?", k) for k in keys):
        raise ValueError("n_lstm_layers > 1 (or a bidirectional LSTM) is not supported")
    if any(k.startswith("mlp_extractor.shared_net") for k in keys):
        raise ValueError("shared-trunk policies (mlp_extractor.shared_net) are not supported")
    if not any(k.startswith("lstm_actor.") for k in keys):
        raise ValueError("unrecognised state dict: expected lstm_actor.* (RecurrentActorCriticPolicy)")
    critic = any(k.startswith("lstm_critic.") for k in keys)
    need = [f"lstm_actor.{k}" for k in LSTM_KEYS] + ["action_net.weight", "action_net.bias"]
    if critic:
        need += [f"lstm_critic.{k}" for k in LSTM_KEYS] + ["value_net.weight", "value_net.bias"]
    for k in need:
        if k not in sd:
            raise ValueError(f"state dict lacks {k}")
    lstm = [tuple(sd[f"lstm_actor.{k}"] for k in LSTM_KEYS)]
    mlp = [_linears(sd, "mlp_extractor.policy_net") + [(sd["action_net.weight"], sd["action_net.bias"])]]
    if critic:
        lstm.append(tuple(sd[f"lstm_critic.{k}"] for k in LSTM_KEYS))
        mlp.append(_linears(sd, "mlp_extractor.value_net") + [(sd["value_net.weight"], sd["value_net.bias"])])
    if lstm[0][1].dim() != 2:
        raise ValueError("lstm_actor.weight_hh_l0 must be a matrix")
    H = check_lstm_hidden(lstm[0][1].shape[1])
    D = lstm[0][0].shape[1] if lstm[0][0].dim() == 2 else -1
    for w_ih, w_hh, b_ih, b_hh in lstm:
        if (tuple(w_ih.shape) != (4 * H, D) or tuple(w_hh.shape) != (4 * H, H) or tuple(b_ih.shape) != (4 * H,)
                or tuple(b_hh.shape) != (4 * H,)):
            raise ValueError("lstm shapes do not chain (both towers need the same hidden size and obs length)")
    for tw in mlp:
        if len(tw) < 2:
            raise ValueError("a tower needs at least one hidden layer after the LSTM (net_arch)")
        k = H
        for w, b in tw:
            if w.dim() != 2 or b.dim() != 1 or w.shape[0] != b.shape[0] or w.shape[1] != k:
                raise ValueError("layer shapes do not chain")
            k = w.shape[0]
    towers = check_towers([[w.shape[0] for w, _ in tw] for tw in mlp])
    return H, towers, (activation or "tanh"), lstm, mlp


def _lstm_structs(hidden, n_towers, tensors=None, keep=None):
    arr = (C.PEPolicyLstm * n_towers)()
    for i in range(n_towers):
        arr[i].hidden = hidden
        if tensors is None:
            continue
        for name, x in zip(("weight_ih", "weight_hh", "bias_ih", "bias_hh"), tensors[i]):
            setattr(arr[i], name, C.ptr(x))
            if keep is not None:
                keep.append(x)
    return arr


def _check_lstm_shapes(hidden, n_towers, lstm_tensors, obs_dim):
    if len(lstm_tensors) != n_towers:
        raise ValueError(f"expected {n_towers} towers of lstm tensors, got {len(lstm_tensors)}")
    want = ((4 * hidden, obs_dim), (4 * hidden, hidden), (4 * hidden,), (4 * hidden,))
    for i, tw in enumerate(lstm_tensors):
        if len(tw) != 4 or any(tuple(x.shape) != w for x, w in zip(tw, want)):
            raise ValueError(f"tower {i}: expected lstm tensors (w_ih, w_hh, b_ih, b_hh) of shapes {want}")


def lstm_host_forward(hidden, towers, lstm_tensors, mlp_tensors, activation, obs, states=None, episode_start=None,
                      deterministic=True, seed=0, env_id_offset=0, t=0):
    """The host twin of the recurrent policy (pe_policy_lstm_forward_host), no device.  obs f32
    [n, D]; states: [(h, c), ..] per tower, f32 [n, H] each (None: zeros); episode_start: bool /
    u8 [n] or None.  Returns ((actions, logits, values or None), new_states) as numpy arrays;
    the inputs are left as they are."""
    hidden = check_lstm_hidden(hidden)
    towers = check_towers(towers)
    if activation not in ACTIVATIONS:
        raise ValueError(f"activation must be one of {sorted(ACTIVATIONS)}")
    obs = np.ascontiguousarray(obs, np.float32)
    if obs.ndim != 2:
        raise ValueError("obs must be [n, D]")
    n, D = obs.shape
    nt = len(towers)
    f32 = lambda x: np.ascontiguousarray(_np(x), np.float32)  # noqa: E731
    lt = [tuple(f32(x) for x in tw) for tw in lstm_tensors]
    mt = [[(f32(w), f32(b)) for w, b in tw] for tw in mlp_tensors]
    _check_lstm_shapes(hidden, nt, lt, D)
    _check_tensor_shapes(towers, mt, hidden)
    hs = np.zeros((nt, n, hidden), np.float32)
    cs = np.zeros((nt, n, hidden), np.float32)
    if states is not None:
        if len(states) != nt:
            raise ValueError(f"expected {nt} (h, c) pairs")
        for i, (h, c) in enumerate(states):
            h, c = f32(h), f32(c)
            if h.shape != (n, hidden) or c.shape != (n, hidden):
                raise ValueError(f"states must be [n, H] = {(n, hidden)}")
            hs[i], cs[i] = h, c
    start = None
    if episode_start is not None:
        start = np.ascontiguousarray(np.asarray(_np(episode_start)) != 0, np.uint8)
        if start.shape != (n,):
            raise ValueError("episode_start must be [n]")
    keep = []
    larr = _lstm_structs(hidden, nt, lt, keep)
    tarr = _tower_structs(towers, mt, keep)
    A = towers[0][-1]
    actions = np.zeros(n, np.int32)
    logits = np.zeros((n, A), np.float32)
    values = np.zeros(n, np.float32) if nt == 2 else None
    C.check(C.lib().pe_policy_lstm_forward_host(
        n, D, nt, larr, tarr, ACTIVATIONS[activation], C.ptr(obs), C.ptr(start), C.ptr(hs), C.ptr(cs),
        C.PE_POLICY_ARGMAX if deterministic else C.PE_POLICY_SAMPLE, int(seed) & 0xFFFFFFFFFFFFFFFF,
        int(env_id_offset) & 0xFFFFFFFF, int(t) & 0xFFFFFFFF, C.ptr(actions), C.ptr(logits), C.ptr(values)),
        "pe_policy_lstm_forward_host")
    return (actions, logits, values), [(hs[i], cs[i]) for i in range(nt)]


class RecurrentPolicy(_PolicyBase):
    """An LSTM policy (sb3_contrib MlpLstmPolicy, one LSTM layer per tower) over the obs of a
    PlantOSBatch (or of a PlantOSVecEnv's batch).

    hidden: the LSTM size H (a multiple of 32 in 32..512); towers: the MLP after the LSTM,
    [[h1, .., A], [h1, .., 1]] (actor and critic, each with its own LSTM) or [[h1, .., A]]
    (actor only); activation / seed / env_tile as Policy's.  Weights and state start at zero:
    `load` the weights; the first `act` of a fresh policy behaves as an episode start.  Close
    the policy before its batch."""

    def __init__(self, batch_or_venv, hidden, towers, activation="tanh", seed=0, env_tile=None):
        self.hidden = check_lstm_hidden(hidden)
        super().__init__(batch_or_venv, towers, activation, seed, env_tile)

    def _create(self, env_tile, out):
        nt = len(self.towers)
        C.check(C.lib().pe_policy_create_lstm(self.batch.handle, nt, _lstm_structs(self.hidden, nt),
                                              _tower_structs(self.towers), ACTIVATIONS[self.activation], env_tile, out),
                "pe_policy_create_lstm")

    @classmethod
    def from_state_dict(cls, env, sd, activation=None, **kw):
        """A RecurrentPolicy shaped and loaded from an sb3_contrib state dict (parse_lstm_state_dict)."""
        hidden, towers, act, lstm, mlp = parse_lstm_state_dict(sd, activation)
        p = cls(env, hidden, towers, act, **kw)
        p.load((lstm, mlp))
        return p

    def load(self, sd_or_tensors):
        """Repack new weights: kernels on the current stream, ordered with the forwards around
        them.  Takes an sb3_contrib state dict or (lstm_tensors, mlp_tensors) as
        parse_lstm_state_dict returns them; f32 contiguous tensors on the batch's device are
        read in place, anything else is uploaded first.  The state is left as it is."""
        torch = self._torch
        if isinstance(sd_or_tensors, dict):
            hidden, towers, _, lstm, mlp = parse_lstm_state_dict(sd_or_tensors)
            if hidden != self.hidden or towers != self.towers:
                raise ValueError(f"state dict has hidden {hidden}, towers {towers}; the policy {self.hidden}, {self.towers}")
        else:
            lstm, mlp = sd_or_tensors
        _check_lstm_shapes(self.hidden, len(self.towers), lstm, self.batch.obs_dim)
        _check_tensor_shapes(self.towers, mlp, self.hidden)
        dev = self.batch.device
        dl = [tuple(_to_dev_f32(x, dev) for x in tw) for tw in lstm]
        dm = [[tuple(_to_dev_f32(x, dev) for x in wb) for wb in tw] for tw in mlp]
        keep = []
        larr = _lstm_structs(self.hidden, len(self.towers), dl, keep)
        tarr = _tower_structs(self.towers, dm, keep)
        with torch.cuda.device(dev):
            C.check(C.lib().pe_policy_load_lstm(self._handle(), larr, tarr, self.batch._stream()), "pe_policy_load_lstm")
        self._loaded = (dl, dm)  # alive until the next load (the kernels read them on the stream)
        return self

    def act(self, obs=None, episode_start=None, deterministic=True, t=None, out=None):
        """(actions i32 [n], logits f32 [n, A], values f32 [n] or None), device tensors; the
        LSTM state of every env advances by one step.

        obs, deterministic, t, out: as Policy.act.  episode_start: a uint8 / bool device tensor
        [n], or a pair of them -- the step's (terminated, truncated) as they are; an env whose
        flag (either one) is non-zero reads a zero state in this step.  None: no env starts.
        One kernel on the current stream; no sync, no allocation: graph-capturable."""
        obs, codes = self._obs_arg(obs)
        sa, sb = self._starts(episode_start)
        a, lg, v = self._out_arg(out, self.batch.num_envs)
        mode, step = self._sampler_step(deterministic, t)
        rc = C.lib().pe_policy_forward_lstm(self._handle(), obs.data_ptr(), int(codes), sa, sb, mode, self.seed,
                                            step, a.data_ptr(), lg.data_ptr() if lg is not None else None,
                                            v.data_ptr() if v is not None else None, self._stream())
        if rc:
            C.check(rc, "pe_policy_forward_lstm")
        return a, lg, v

    def _starts(self, episode_start):
        if isinstance(episode_start, (tuple, list)):
            if len(episode_start) != 2:
                raise ValueError("episode_start must be a tensor or a pair of tensors")
            return (self._flag_arg(episode_start[0], "episode_start[0]"),
                    self._flag_arg(episode_start[1], "episode_start[1]"))
        return self._flag_arg(episode_start, "episode_start"), None

    def value(self, obs=None, episode_start=None, select=None, out=None):
        """The values f32 [n] alone, from the LSTM state as it is: bit for bit what `act` would
        return as values for the same obs, flags and state -- but the state of no env and no
        tower changes, the actor tower is not evaluated and the sampler's `t` stays
        (sb3_contrib's predict_values).

        obs, episode_start: as `act`.  select, out: as Policy.value.  ValueError for an
        actor-only policy.  One kernel on the current stream; no sync, no allocation:
        graph-capturable."""
        obs, codes, want, unless, out = self._value_args(obs, select, out)
        sa, sb = self._starts(episode_start)
        rc = C.lib().pe_policy_value_lstm(self._handle(), obs.data_ptr(), int(codes), sa, sb, want, unless,
                                          out.data_ptr(), self._stream())
        if rc:
            C.check(rc, "pe_policy_value_lstm")
        return out

    def reset_states(self):
        """Zero the state of every env and tower (ordered on the current stream)."""
        C.check(C.lib().pe_policy_lstm_reset_state(self._handle(), self._stream()), "pe_policy_lstm_reset_state")

    def get_states(self, out=None):
        """[(h, c), ..] per tower: fresh device tensors f32 [n, H] (SB3's lstm_states, without
        the leading layer axis).  out: [(h, c), ..] of preallocated contiguous float32 device
        tensors [n, H] to write instead (no allocation: graph-capturable); it is returned."""
        torch, b = self._torch, self.batch
        shape = (b.num_envs, self.hidden)
        if out is not None:
            if len(out) != len(self.towers) or any(len(pair) != 2 for pair in out):
                raise ValueError(f"out must be {len(self.towers)} (h, c) pairs")
            for x in (x for pair in out for x in pair):
                if not on_device(x, b._dev_index, (torch.float32,), shape):
                    raise ValueError(f"out tensors must be contiguous float32 of shape {shape} on {b.device}")
        res = []
        for i in range(len(self.towers)):
            if out is not None:
                h, c = out[i]
            else:
                h = torch.empty(shape, dtype=torch.float32, device=b.device)
                c = torch.empty_like(h)
            C.check(C.lib().pe_policy_lstm_get_state(self._handle(), i, h.data_ptr(), c.data_ptr(), self._stream()),
                    "pe_policy_lstm_get_state")
            res.append((h, c))
        return res

    def set_states(self, states):
        """Replace the state: [(h, c), ..] per tower, [n, H] each (device tensors are read in
        place on the current stream; anything else is uploaded first)."""
        b = self.batch
        if len(states) != len(self.towers):
            raise ValueError(f"expected {len(self.towers)} (h, c) pairs")
        dev = []
        for h, c in states:
            pair = tuple(_to_dev_f32(x, b.device) for x in (h, c))
            if any(tuple(x.shape) != (b.num_envs, self.hidden) for x in pair):
                raise ValueError(f"states must be [n, H] = {(b.num_envs, self.hidden)}")
            dev.append(pair)
        for i, (h, c) in enumerate(dev):
            C.check(C.lib().pe_policy_lstm_set_state(self._handle(), i, h.data_ptr(), c.data_ptr(), self._stream()),
                    "pe_policy_lstm_set_state")
        self._states_in = dev  # alive until the next call (the kernels read them on the stream)

    def host_forward(self, obs_np, states_np=None, start_np=None, tensors=None, deterministic=True, t=0):
        """The host twin on f32 obs rows [n, D] (numpy), states [(h, c), ..] (None: zeros) and
        start flags [n] (None: none), with the weights last loaded (or `tensors` =
        (lstm_tensors, mlp_tensors)); env ids start at the batch's env_id_offset, the sampler
        uses the policy's seed.  Returns ((actions, logits, values or None), new_states)."""
        tensors = tensors if tensors is not None else self._loaded
        if tensors is None:
            raise ValueError("no weights loaded")
        return lstm_host_forward(self.hidden, self.towers, tensors[0], tensors[1], self.activation, obs_np,
                                 states=states_np, episode_start=start_np, deterministic=deterministic,
                                 seed=self.seed, env_id_offset=int(self.batch.cfg.env_id_offset), t=t)
