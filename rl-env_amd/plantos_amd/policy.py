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
"""
import ctypes
import re

import numpy as np

from . import _capi as C

ACTIVATIONS = {"tanh": C.PE_ACT_TANH, "relu": C.PE_ACT_RELU}


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
            arr[i].weight[l] = w.ctypes.data if isinstance(w, np.ndarray) else w.data_ptr()
            arr[i].bias[l] = b.ctypes.data if isinstance(b, np.ndarray) else b.data_ptr()
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


def host_forward(towers, tensors, activation, obs, deterministic=True, seed=0, env_id_offset=0, t=0):
    """The host twin (pe_policy_forward_host): the definition of the policy's outputs in plain
    C++, no device.  obs f32 [n, D] (numpy); tensors as parse_state_dict returns them (torch
    CPU tensors or numpy).  Returns (actions i32 [n], logits f32 [n, A], values f32 [n] or
    None) as numpy arrays."""
    towers = check_towers(towers)
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
    P = ctypes.c_void_p
    C.check(C.lib().pe_policy_forward_host(
        n, D, len(towers), arr, ACTIVATIONS[activation], obs.ctypes.data_as(P),
        C.PE_POLICY_ARGMAX if deterministic else C.PE_POLICY_SAMPLE, int(seed) & 0xFFFFFFFFFFFFFFFF,
        int(env_id_offset) & 0xFFFFFFFF, int(t) & 0xFFFFFFFF, actions.ctypes.data_as(P), logits.ctypes.data_as(P),
        values.ctypes.data_as(P) if values is not None else None), "pe_policy_forward_host")
    return actions, logits, values


def math_host(which, x):
    """pe_tanhf ("tanh") or pe_expf ("exp") of a float32 array, as the twin and the kernel compute them."""
    x = np.ascontiguousarray(x, np.float32)
    y = np.empty_like(x)
    P = ctypes.c_void_p
    C.check(C.lib().pe_policy_math_host({"tanh": 0, "exp": 1}[which], x.size, x.ctypes.data_as(P),
                                        y.ctypes.data_as(P)), "pe_policy_math_host")
    return y


def _np(x):
    return x if isinstance(x, np.ndarray) else x.detach().cpu().numpy()


class Policy:
    """An MLP policy over the obs of a PlantOSBatch (or of a PlantOSVecEnv's batch).

    towers: [[h1, .., A], [h1, .., 1]] (pi and vf nets) or [[h1, .., A]] (a Q-network);
    activation "tanh" or "relu"; seed keys the action sampler (deterministic=False);
    env_tile (32 / 64, None = the library's choice) is the kernel's envs per workgroup: it
    changes speed, never results.  Weights start at zero: `load` them.  Close the policy
    before its batch."""

    def __init__(self, batch_or_venv, towers=((256, 256, 5), (256, 256, 1)), activation="tanh", seed=0,
                 env_tile=None):
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
        shapes = _tower_structs(self.towers)
        with torch.cuda.device(b.device):
            C.check(C.lib().pe_policy_create(b.handle, len(self.towers), shapes, ACTIVATIONS[activation],
                                             int(env_tile or 0), ctypes.byref(p)), "pe_policy_create")
        self._p = p
        n, A, dev = b.num_envs, self.towers[0][-1], b.device
        self.actions = torch.zeros(n, dtype=torch.int32, device=dev)
        self.logits = torch.zeros((n, A), dtype=torch.float32, device=dev)
        self.values = torch.zeros(n, dtype=torch.float32, device=dev) if len(self.towers) == 2 else None
        self._loaded = None

    @classmethod
    def from_state_dict(cls, env, sd, activation=None, **kw):
        """A Policy shaped and loaded from a Stable-Baselines3 state dict (parse_state_dict)."""
        towers, act, tensors = parse_state_dict(sd, activation)
        p = cls(env, towers, act, **kw)
        p.load(tensors)
        return p

    @property
    def env_tile(self):
        return int(C.lib().pe_policy_env_tile(self._handle()))

    def _handle(self):
        if not self._p:
            raise ValueError("Policy is closed")
        return self._p

    def close(self):
        if getattr(self, "_p", None):
            C.check(C.lib().pe_policy_destroy(self._p), "pe_policy_destroy")
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

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
        devt = [[tuple(torch.as_tensor(x).detach().to(device=dev, dtype=torch.float32).contiguous() for x in wb)
                 for wb in tw] for tw in tensors]
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
        torch = self._torch
        b = self.batch
        n, D = b.num_envs, b.obs_dim
        if obs is None:
            obs = b.obs
        if not (type(obs) is torch.Tensor and obs.is_cuda and obs.get_device() == b._dev_index
                and obs.is_contiguous() and tuple(obs.shape) == (n, D)
                and (obs.dtype is torch.float32 or obs.dtype is torch.uint8)):
            raise ValueError(f"obs must be a contiguous float32 or uint8 tensor of shape {(n, D)} on {b.device}")
        codes = obs.dtype is torch.uint8
        if codes and not b.obs_codes:
            raise ValueError("uint8 obs codes need a batch created with obs_codes=True")
        a, lg, v = out if out is not None else (self.actions, self.logits, self.values)
        A = self.towers[0][-1]
        for name, x, dt, shape in (("actions", a, torch.int32, (n,)), ("logits", lg, torch.float32, (n, A)),
                                   ("values", v, torch.float32, (n,))):
            if x is None and name != "actions":
                continue  # an output not asked for
            if not (type(x) is torch.Tensor and x.dtype is dt and x.is_cuda and x.get_device() == b._dev_index
                    and x.is_contiguous() and tuple(x.shape) == shape):
                raise ValueError(f"{name} must be a contiguous {dt} tensor of shape {shape} on {b.device}")
        if v is not None and len(self.towers) < 2:
            raise ValueError("a one-tower policy has no values")
        if deterministic:
            mode, step = C.PE_POLICY_ARGMAX, 0
        else:
            mode = C.PE_POLICY_SAMPLE
            if t is None:
                step, self.t = self.t, self.t + 1
            else:
                step = int(t)
        rc = C.lib().pe_policy_forward(self._handle(), obs.data_ptr(), int(codes), mode, self.seed,
                                       step & 0xFFFFFFFF, a.data_ptr(), lg.data_ptr() if lg is not None else None,
                                       v.data_ptr() if v is not None else None,
                                       torch.cuda.current_stream(b._dev_index).cuda_stream)
        if rc:
            C.check(rc, "pe_policy_forward")
        return a, lg, v

    def host_forward(self, obs_np, tensors=None, deterministic=True, t=0):
        """The host twin on f32 obs rows [n, D] (numpy) with the weights last loaded (or
        `tensors`); env ids start at the batch's env_id_offset, the sampler uses the policy's
        seed.  Returns numpy (actions, logits, values or None)."""
        tensors = tensors if tensors is not None else self._loaded
        if tensors is None:
            raise ValueError("no weights loaded")
        return host_forward(self.towers, tensors, self.activation, obs_np, deterministic=deterministic,
                            seed=self.seed, env_id_offset=int(self.batch.cfg.env_id_offset), t=t)
