"""RolloutCollector: on-policy rollouts collected on the device.

What Stable-Baselines3's OnPolicyAlgorithm.collect_rollouts and
RolloutBuffer.compute_returns_and_advantage add to the act / step loop (A2C(n_steps=5,
gamma=0.99, gae_lambda=1.0), A2C_training.py:229-247; the PPO family with n_steps=1024,
gae_lambda=0.95, trainingCode.py:140-162): per-step storage of obs, actions, rewards, episode
starts, values and log-probs, the time-limit bootstrap of truncated episodes and the
reverse-time GAE scan -- the C-ABI's pe_rollout_record / pe_rollout_gae
(include/plantos_batch.h, "Rollout collection") around Policy.act and PlantOSBatch.step.
The Rollout is the data a learner consumes; A2C's learner is plantos_amd.A2CLearner (learner.py).

    collector = RolloutCollector(venv, policy, n_steps=5, gamma=0.99, gae_lambda=1.0)
    learner = A2CLearner(policy, max_rows=5 * venv.num_envs)
    venv.reset()
    while training:
        ro = collector.collect()            # device tensors; no host sync
        learner.train(ro)                   # A2C.train on the device; the policy acts with the new weights

RecurrentRolloutCollector is the same for a two-tower RecurrentPolicy (sb3_contrib's
RecurrentPPO.collect_rollouts): the LSTM state advances with the steps, the bootstrap and
last_values come from the value-only forward, which leaves it alone, and the Rollout carries
snapshots of the state for the learner.

A Rollout also hands out shuffled minibatches on the device (SB3's RolloutBuffer.get and the
advantage normalisation of PPO.train; csrc/pe_rollout_minibatch.h): `ro.minibatches(batch_size,
epoch, seed)` for row minibatches, `ro.env_minibatches(envs_per_batch, ..)` for whole sequences
with their starting LSTM state, `ro.next_minibatch(batch_size)` with counters on the device.

Every output is defined bit for bit by the host twins (`host_record`, `host_gae`,
`RolloutCollector.host_rollout`, `RecurrentRolloutCollector.host_rollout`,
`host_minibatch_indices`, `host_adv_norm`), which need no device.
"""
import numpy as np

from . import _capi as C
from ._capi import ptr as _p
from ._collector import Collector, check_autoreset, check_policy_batch, unwrap
from .policy import Policy, RecurrentPolicy, lstm_host_forward

ROW_ALIGN = 512  # bytes: every row of the buffer starts as aligned as a fresh torch allocation


def host_record(logits, actions, reward, terminated, truncated, gamma, terminal_value=None, episode_return=None,
                episode_length=None, ep_count=None, ep_return_sum=None, ep_length_sum=None):
    """The record step on numpy arrays (pe_rollout_record_host): returns (log_prob f32[n],
    reward f32[n], start_next u8[n]); the accumulators given (i32 / f64 / i32 [n], contiguous)
    are updated in place.  terminal_value None: no bootstrap."""
    logits = np.ascontiguousarray(logits, np.float32)
    n, A = logits.shape
    actions = np.ascontiguousarray(actions, np.int32)
    reward = np.ascontiguousarray(reward, np.float32)
    te = np.ascontiguousarray(np.asarray(terminated) != 0, np.uint8)
    tr = np.ascontiguousarray(np.asarray(truncated) != 0, np.uint8)
    tv = None if terminal_value is None else np.ascontiguousarray(terminal_value, np.float32)
    er = None if episode_return is None else np.ascontiguousarray(episode_return, np.float64)
    el = None if episode_length is None else np.ascontiguousarray(episode_length, np.int32)
    for x, dt in ((ep_count, np.int32), (ep_return_sum, np.float64), (ep_length_sum, np.int32)):
        if x is not None and not (isinstance(x, np.ndarray) and x.dtype == dt and x.flags.c_contiguous and x.shape == (n,)):
            raise ValueError(f"accumulators must be contiguous numpy arrays of shape {(n,)} (i32, f64, i32)")
    for x in (actions, reward, te, tr, tv, er, el):
        if x is not None and x.shape != (n,):
            raise ValueError(f"per-env inputs must have shape {(n,)}")
    lp = np.zeros(n, np.float32)
    ro = np.zeros(n, np.float32)
    st = np.zeros(n, np.uint8)
    C.check(C.lib().pe_rollout_record_host(n, A, _p(logits), _p(actions), _p(reward), _p(te), _p(tr), _p(tv), _p(er),
                                           _p(el), float(gamma), _p(lp), _p(ro), _p(st), _p(ep_count),
                                           _p(ep_return_sum), _p(ep_length_sum)), "pe_rollout_record_host")
    return lp, ro, st


def host_gae(rewards, values, starts, last_values, gamma, gae_lambda):
    """The GAE scan on numpy arrays (pe_rollout_gae_host): rewards / values f32 [T, n], starts
    u8 [T + 1, n] (row T: the last step's done flags), last_values f32 [n]; returns
    (advantages, returns) f32 [T, n]."""
    rewards = np.ascontiguousarray(rewards, np.float32)
    values = np.ascontiguousarray(values, np.float32)
    starts = np.ascontiguousarray(np.asarray(starts) != 0, np.uint8)
    last_values = np.ascontiguousarray(last_values, np.float32)
    if rewards.ndim != 2:
        raise ValueError("rewards must be [T, n]")
    T, n = rewards.shape
    if values.shape != (T, n) or starts.shape != (T + 1, n) or last_values.shape != (n,):
        raise ValueError(f"expected values {(T, n)}, starts {(T + 1, n)}, last_values {(n,)}")
    adv = np.zeros((T, n), np.float32)
    ret = np.zeros((T, n), np.float32)
    C.check(C.lib().pe_rollout_gae_host(T, n, n, n, n, n, _p(rewards), _p(values), _p(starts), _p(last_values),
                                        float(gamma), float(gae_lambda), _p(adv), _p(ret)), "pe_rollout_gae_host")
    return adv, ret


def record_device(logits, actions, reward, terminated, truncated, gamma, log_prob, reward_out, start_next,
                  terminal_value=None, episode_return=None, episode_length=None, ep_count=None, ep_return_sum=None,
                  ep_length_sum=None):
    """pe_rollout_record on device tensors (contiguous, all on logits' device), on torch's
    current stream.  reward_out may be `reward`."""
    import torch
    n, A = logits.shape
    with torch.cuda.device(logits.device):
        C.check(C.lib().pe_rollout_record(
            n, A, _p(logits), _p(actions), _p(reward), _p(terminated), _p(truncated), _p(terminal_value),
            _p(episode_return), _p(episode_length), float(gamma), _p(log_prob), _p(reward_out), _p(start_next),
            _p(ep_count), _p(ep_return_sum), _p(ep_length_sum), C.stream_ptr(logits.device)), "pe_rollout_record")


def gae_device(rewards, values, starts, last_values, gamma, gae_lambda, advantages, returns):
    """pe_rollout_gae on device tensors, on torch's current stream: rewards / values /
    advantages / returns f32 [T, n] and starts u8 [T + 1, n], each with unit stride over envs
    and any row stride (advantages and returns the same one); last_values f32 [n]."""
    import torch
    T, n = rewards.shape
    for name, x, rows in (("rewards", rewards, T), ("values", values, T), ("starts", starts, T + 1),
                          ("advantages", advantages, T), ("returns", returns, T)):
        if tuple(x.shape) != (rows, n) or (n > 1 and x.stride(1) != 1):
            raise ValueError(f"{name} must be [{rows}, {n}] with unit stride over envs")
    if T > 1 and advantages.stride(0) != returns.stride(0):
        raise ValueError("advantages and returns must share their row stride")
    rs = lambda x: x.stride(0) if x.shape[0] > 1 else n  # noqa: E731
    with torch.cuda.device(rewards.device):
        C.check(C.lib().pe_rollout_gae(T, n, rs(rewards), rs(values), starts.stride(0), rs(advantages), _p(rewards),
                                       _p(values), _p(starts), _p(last_values), float(gamma), float(gae_lambda),
                                       _p(advantages), _p(returns), C.stream_ptr(rewards.device)), "pe_rollout_gae")


# ------------------------------------------------------------------ rollout minibatches
U64 = (1 << 64) - 1
NORM_CHUNK = 4096  # pe_rollout_math.hpp kNormChunk: elements per chunk of the normalisation's sums
_MODES = {"rows": C.PE_MB_ROWS, "envs": C.PE_MB_ENVS}
_MB_IN = ("actions", "values", "log_probs", "advantages", "returns", "starts")
_MB_OUT = ("indices", "obs", "codes", "actions", "values", "log_probs", "advantages", "returns", "starts")


def _uint(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or int(v) < 0:
        raise ValueError(f"{name} must be a non-negative int, got {v!r}")
    return int(v)


def check_minibatch_size(B, name="batch_size"):
    if isinstance(B, bool) or not isinstance(B, (int, np.integer)) or int(B) < 1:
        raise ValueError(f"{name} must be an int >= 1, got {B!r}")
    return int(B)


def host_minibatch_indices(M, B, epoch, k, seed=0, domain="rows"):
    """The source indices i32 [count] of minibatch k of epoch `epoch` (pe_rollout_math.hpp
    rollout_perm, no device): positions k B .. k B + count - 1, count = min(B, M - k B), of the
    keyed permutation of [0, M).  domain "rows": M = T * n rows, index = t * n + env; "envs":
    M = n envs.  ValueError for B < 1, k >= ceil(M / B), M outside 1 .. 2^31 - 1, or an epoch /
    seed that is no non-negative int."""
    if domain not in _MODES:
        raise ValueError(f"domain must be 'rows' or 'envs', got {domain!r}")
    M, B, k = _uint("M", M), check_minibatch_size(B, "B"), _uint("k", k)
    epoch, seed = _uint("epoch", epoch), _uint("seed", seed)
    if M < 1 or k >= -(-M // B):
        raise ValueError(f"k must be < ceil(M / B) = {-(-M // B)} and M >= 1, got M={M} k={k}")
    count = min(B, M - k * B)
    out = np.zeros(count, np.int32)
    C.check(C.lib().pe_internal_rollout_perm_host(M, seed & U64, epoch & U64, _MODES[domain], k * B, count, _p(out)),
            "pe_internal_rollout_perm_host")
    return out


def host_adv_norm(a):
    """The advantage normalisation on a numpy array (pe_internal_rollout_adv_norm_host): f32 [N],
    or [T, count] numbered row by row; (a - mean) / (std + 1e-8), unbiased std, sums in f64 in
    the order pe_rollout_math.hpp fixes.  Fewer than 2 elements come back unchanged."""
    a = np.ascontiguousarray(a, np.float32)
    if a.ndim not in (1, 2):
        raise ValueError("a must be [N] or [T, count]")
    rows, count = (1, a.shape[0]) if a.ndim == 1 else a.shape
    out = np.zeros_like(a)
    if a.size:
        C.check(C.lib().pe_internal_rollout_adv_norm_host(max(rows, 1), count, count, _p(a), _p(out)),
                "pe_internal_rollout_adv_norm_host")
    return out


def norm_scratch_len(elements):
    """f64 words of scratch pe_internal_rollout_adv_norm needs for `elements` elements."""
    return 2 * (-(-int(elements) // NORM_CHUNK)) if elements > NORM_CHUNK else 0


def adv_norm_device(a, out=None, count=None, scratch=None):
    """pe_internal_rollout_adv_norm on device tensors, current stream: a f32 [cap] or [T, cap]
    (unit stride over the last axis), out the same layout (None: in place).  count: None (all
    cap columns) or a device i32 [1] holding how many columns are valid.  scratch: a device f64
    tensor of norm_scratch_len(a.numel()) words (None: allocated here when needed)."""
    import torch
    out = a if out is None else out
    rows, cap = (1, a.shape[0]) if a.dim() == 1 else a.shape
    ld = cap if a.dim() == 1 or rows == 1 else a.stride(0)
    if a.dim() == 2 and rows > 1 and out.stride(0) != ld:
        raise ValueError("a and out must share their row stride")
    need = norm_scratch_len(rows * cap)
    if need and scratch is None:
        scratch = torch.zeros(need, dtype=torch.float64, device=a.device)
    if need and scratch.numel() < need:
        raise ValueError(f"scratch must hold {need} float64 words")
    with torch.cuda.device(a.device):
        C.check(C.lib().pe_internal_rollout_adv_norm(rows, cap, ld, _p(count), _p(a), _p(out), _p(scratch),
                                                     C.stream_ptr(a.device)), "pe_internal_rollout_adv_norm")
    return out


def mb_args(mode, T, n, D, B, buf, stride, fields, outs, obs_f32=False, table=None, seed=0, epoch=0, k=0, ctrl=None,
            count=None, states=()):
    """A filled pe_rollout_mb (csrc/pe_rollout_minibatch.h) over device tensors.  mode "rows" /
    "envs"; buf: the u8 storage, obs row t at byte t * stride; fields: dict of the [T, n]
    inputs named actions, values, log_probs, advantages, returns (and starts in env mode), unit
    stride over envs, any row stride; outs: dict of the contiguous outputs named indices, obs,
    actions, values, log_probs, advantages, returns (and codes, starts); states: (src, dst)
    pairs, src f32 [S, n, H] (row 0 is read), dst f32 [B, H].  The tensors are kept alive by the
    struct."""
    a = C.PERolloutMb()
    a.mode, a.T, a.n, a.D, a.B, a.obs_f32 = _MODES[mode], int(T), int(n), int(D), int(B), int(bool(obs_f32))
    a.seed, a.epoch, a.k = int(seed) & U64, int(epoch) & U64, int(k) & U64
    a.buf, a.stride, a.buf_bytes = buf.data_ptr(), int(stride), buf.numel() * buf.element_size()
    keep = [buf, table, ctrl, count]
    a.table = None if table is None else table.data_ptr()
    a.ctrl = None if ctrl is None else ctrl.data_ptr()
    a.count = None if count is None else count.data_ptr()
    for name in _MB_IN:
        x = fields.get(name)
        if x is not None:
            if tuple(x.shape) != (T, n) or (n > 1 and x.stride(1) != 1):
                raise ValueError(f"{name} must be [{T}, {n}] with unit stride over envs")
            setattr(a, name, x.data_ptr())
            setattr(a, "s_" + name, x.stride(0) if T > 1 else n)
            keep.append(x)
    for name in _MB_OUT:
        x = outs.get(name)
        if x is not None:
            if not x.is_contiguous():
                raise ValueError(f"output {name} must be contiguous")
            setattr(a, name if name == "indices" else "out_" + name, x.data_ptr())
            keep.append(x)
    states = list(states)
    if len(states) > C.PE_MB_MAX_STATES:
        raise ValueError(f"at most {C.PE_MB_MAX_STATES} state arrays")
    a.n_states = len(states)
    for i, (src, dst) in enumerate(states):
        a.H = src.shape[-1]
        if src.dim() != 3 or src.shape[1] != n or tuple(dst.shape) != (B, a.H) or not src.is_contiguous() \
                or not dst.is_contiguous():
            raise ValueError(f"states must be contiguous (src [S, {n}, H], dst [{B}, H]) pairs")
        a.state_src[i], a.state_dst[i] = src.data_ptr(), dst.data_ptr()
        keep += [src, dst]
    a._keep = keep
    return a


def minibatch_device(a, device):
    """pe_internal_rollout_minibatch of a filled pe_rollout_mb, on torch's current stream of `device`."""
    import ctypes
    import torch
    with torch.cuda.device(device):
        C.check(C.lib().pe_internal_rollout_minibatch(ctypes.byref(a), C.stream_ptr(device)),
                "pe_internal_rollout_minibatch")


class RolloutMinibatch:
    """One minibatch of a Rollout, named as SB3's RolloutBufferSamples: device tensors owned by the
    collector, one set per (mode, size), overwritten by the next minibatch of that size.

    Row minibatches: observations f32 [B, D], actions i32 [B], old_values, old_log_prob,
    advantages, returns f32 [B], indices i32 [B] (the rollout row t * n + env of each sample).
    Env minibatches: the same time-major, [T, Be(, D)], plus episode_starts u8 [T, Be],
    env_indices (= indices) i32 [Be] and lstm_states [(h0, c0), ..] f32 [Be, H] per tower (None
    without a recurrent collector).  codes: the u8 obs rows where obs="codes" asked for them,
    else None.  count: how many samples (envs) are valid: an int from the generators, which
    yield views of exactly that many; a device i32 [1] from next_minibatch, whose tensors keep
    their full size with zeros (indices -1) past count."""

    NAMES = ("observations", "codes", "actions", "old_values", "old_log_prob", "advantages", "returns",
             "episode_starts")

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def env_indices(self):
        return self.indices

    def _head(self, count):
        """Views of the first `count` samples."""
        ax = (slice(None), slice(0, count)) if self.mode == "envs" else (slice(0, count),)
        kw = {k: None if getattr(self, k) is None else getattr(self, k)[ax] for k in self.NAMES}
        states = self.lstm_states and [(h[:count], c[:count]) for h, c in self.lstm_states]
        return RolloutMinibatch(mode=self.mode, indices=self.indices[:count], lstm_states=states, count=count, **kw)


class Rollout:
    """One collect()'s data: device tensors, most of them views of the collector's storage
    (the next collect() overwrites them).

    obs [T, n, D] (uint8 codes on an ``obs_codes`` batch, else float32; rows strided),
    actions i32 [T, n], rewards f32 [T, n] (strided; with the time-limit bootstrap added
    where it applies), episode_starts u8 [T, n] (strided), values, log_probs, advantages,
    returns f32 [T, n], last_values f32 [n], last_dones u8 [n], and the per-env episode
    accumulators since the collector was made: ep_count i32 [n], ep_return_sum f64 [n],
    ep_length_sum i32 [n].  lstm_states: None, or from a RecurrentRolloutCollector
    [(h, c), ..] per tower, f32 [1, n, H] (the state before step 0) or [T, n, H] (before
    every step), as `state_snapshots` asked."""

    FIELDS = ("obs", "actions", "rewards", "episode_starts", "values", "log_probs", "advantages", "returns",
              "last_values", "last_dones", "ep_count", "ep_return_sum", "ep_length_sum")

    def __init__(self, collector, **fields):
        self._c = collector
        for k in self.FIELDS:
            setattr(self, k, fields[k])
        self.lstm_states = fields.get("lstm_states")

    def obs_f32(self, out=None):
        """The obs as float32 [T * n, D] (step-major).  On an ``obs_codes`` batch: one
        pe_expand_obs_codes launch over the T rows into `out` (or a new tensor).  On a
        float32 batch: a view of the storage where the rows allow one, else one strided copy."""
        return self._c._obs_f32(out)

    def minibatches(self, batch_size=None, epoch=0, seed=0, normalize_advantage=False, obs="f32"):
        """One epoch of shuffled minibatches (SB3's RolloutBuffer.get): a generator of
        ceil(T n / batch_size) RolloutMinibatch, which together hold every row of the rollout
        exactly once, in the order of the keyed permutation rollout_perm(seed, epoch, ..)
        (host_minibatch_indices gives the same indices without a device).  The last one is short
        when batch_size does not divide T n; batch_size None: one minibatch of all rows (A2C's
        get(None)).  Per minibatch one gather kernel reads the collector's storage -- obs codes
        are decoded on the way, so no [T n, D] float tensor is ever made -- and, with
        normalize_advantage, the advantages are normalised as PPO.train does ((a - mean) /
        (std + 1e-8), host_adv_norm bit for bit).  obs="codes" (``obs_codes`` batches) also
        fills mb.codes.  Current stream, no sync; no allocation after the first call of a size.
        ValueError for batch_size < 1 or an epoch / seed that is no non-negative int."""
        return self._c._minibatches("rows", batch_size, epoch, seed, normalize_advantage, obs)

    def env_minibatches(self, envs_per_batch=None, epoch=0, seed=0, normalize_advantage=False, obs="f32"):
        """One epoch of minibatches of whole sequences, for a recurrent learner: a generator of
        ceil(n / envs_per_batch) RolloutMinibatch, each the full [T] sequences of envs_per_batch
        envs drawn by the keyed env permutation, time-major, with episode_starts and -- from a
        RecurrentRolloutCollector -- the LSTM state (h0, c0) each sequence starts from (raw: the
        learner applies episode_starts[0] as the collector's forward did).  All sequences have
        length T, so nothing is padded: this is the project's definition of a recurrent
        minibatch, not sb3_contrib's split-and-pad sampler.  Otherwise as minibatches()."""
        return self._c._minibatches("envs", envs_per_batch, epoch, seed, normalize_advantage, obs)

    def next_minibatch(self, batch_size, seed=0, normalize_advantage=False, obs="f32"):
        """The next row minibatch by the collector's device counters `minibatch_ctrl` = (epoch,
        next k), which the call advances on the device: k + 1, or (epoch + 1, 0) after an
        epoch's last minibatch.  The tensors keep their full size (zeros and indices -1 past
        mb.count, a device i32 [1]).  No host value depends on the counters, so one call can be
        captured with torch.cuda.graph and every replay yields the following minibatch."""
        return self._c._next_minibatch(batch_size, seed, normalize_advantage, obs)

    @property
    def minibatch_ctrl(self):
        """Device i64 [2] = (epoch, next k) of next_minibatch; set it with copy_ / zero_."""
        return self._c.minibatch_ctrl


class _Collector(Collector):
    """What the two collectors share: the argument checks after the policy's kind, the storage
    rows, row 0 and the obs view."""

    def _setup(self, b, policy, n_steps, gamma, gae_lambda, bootstrap_timeouts, deterministic):
        if len(policy.towers) != 2:
            raise ValueError("a rollout needs values: the policy must have a value tower")
        check_policy_batch(policy, b)
        if int(n_steps) < 1:
            raise ValueError(f"n_steps must be >= 1, got {n_steps}")
        self._attach(b, policy)
        check_autoreset(b, "a rollout needs")
        torch = self._torch
        self.n_steps = T = int(n_steps)
        self.gamma, self.gae_lambda = float(gamma), float(gae_lambda)
        self.bootstrap_timeouts, self.deterministic = bool(bootstrap_timeouts), bool(deterministic)
        n, D, A, dev = b.num_envs, b.obs_dim, policy.towers[0][-1], b.device
        io_b = b.io_bytes()
        ro = b._io_offsets()[0]
        # a row: the step's io buffer | start u8 [n] | padding
        self._so = io_b
        self._stride = stride = (io_b + n + ROW_ALIGN - 1) // ROW_ALIGN * ROW_ALIGN
        self._buf = torch.zeros((T + 1) * stride, dtype=torch.uint8, device=dev)
        self._rows = [self._buf[t * stride:t * stride + io_b] for t in range(T + 1)]
        self._row_views = [b.io_views(r) for r in self._rows]
        self._start = [self._buf[t * stride + io_b:t * stride + io_b + n] for t in range(T + 1)]
        m = self._buf.view(T + 1, stride)
        f32, i32 = torch.float32, torch.int32
        if b.obs_codes:
            self._obs = m[:T, :n * D].unflatten(1, (n, D))
        else:
            self._obs = m[:T, :4 * n * D].view(f32).unflatten(1, (n, D))
        self._rewards = m[1:, ro:ro + 4 * n].view(f32)
        self._starts_all = m[:, io_b:io_b + n]
        self.actions = torch.zeros((T, n), dtype=i32, device=dev)
        self.values = torch.zeros((T, n), dtype=f32, device=dev)
        self.log_probs = torch.zeros((T, n), dtype=f32, device=dev)
        self.advantages = torch.zeros((T, n), dtype=f32, device=dev)
        self.returns = torch.zeros((T, n), dtype=f32, device=dev)
        self.last_values = torch.zeros(n, dtype=f32, device=dev)
        self.terminal_values = torch.zeros(n, dtype=f32, device=dev)
        self._logits = torch.zeros((n, A), dtype=f32, device=dev)
        self._rollout = Rollout(
            self, obs=self._obs, actions=self.actions, rewards=self._rewards, episode_starts=self._starts_all[:T],
            values=self.values, log_probs=self.log_probs, advantages=self.advantages, returns=self.returns,
            last_values=self.last_values, last_dones=self._starts_all[T], ep_count=self.ep_count,
            ep_return_sum=self.ep_return_sum, ep_length_sum=self.ep_length_sum)

        # rollout minibatches: the code table on the device (uploaded once), the device counters
        # of next_minibatch, and the output tensors per (mode, size, codes)
        self._mb_table = torch.as_tensor(b.code_table(), device=dev) if b.obs_codes else None
        self.minibatch_ctrl = torch.zeros(2, dtype=torch.int64, device=dev)
        self._mb_cache = {}

    # ----------------------------------------------------------------- minibatches
    def _mb(self, mode, B, codes):
        """The cached RolloutMinibatch (tensors and filled pe_rollout_mb) of a mode and size."""
        key = (mode, B, codes)
        mb = self._mb_cache.get(key)
        if mb is not None:
            return mb
        torch, b = self._torch, self.batch
        T, n, D, dev = self.n_steps, b.num_envs, b.obs_dim, b.device
        shape = (B,) if mode == "rows" else (T, B)
        z = lambda sh, dt: torch.zeros(sh, dtype=dt, device=dev)  # noqa: E731
        f32, i32, u8 = torch.float32, torch.int32, torch.uint8
        states = None
        lstm = getattr(self, "lstm_states", None) if mode == "envs" else None
        if lstm is not None:
            states = [(z((B, h.shape[-1]), f32), z((B, h.shape[-1]), f32)) for h, _ in lstm]
        mb = RolloutMinibatch(
            mode=mode, observations=z(shape + (D,), f32), codes=z(shape + (D,), u8) if codes else None,
            actions=z(shape, i32), old_values=z(shape, f32), old_log_prob=z(shape, f32), advantages=z(shape, f32),
            returns=z(shape, f32), episode_starts=z(shape, u8) if mode == "envs" else None, indices=z((B,), i32),
            lstm_states=states, count=z((1,), i32))
        R = B if mode == "rows" else T * B
        mb._scratch = z((norm_scratch_len(R),), torch.float64) if norm_scratch_len(R) else None
        mb._count_dev = mb.count
        pairs = [] if states is None else [(s, d) for (hs, cs), (hd, cd) in zip(lstm, states) for s, d in ((hs, hd), (cs, cd))]
        mb._args = mb_args(
            mode, T, n, D, B, self._buf, self._stride,
            dict(actions=self.actions, values=self.values, log_probs=self.log_probs, advantages=self.advantages,
                 returns=self.returns, starts=self._starts_all[:T] if mode == "envs" else None),
            dict(indices=mb.indices, obs=mb.observations, codes=mb.codes, actions=mb.actions, values=mb.old_values,
                 log_probs=mb.old_log_prob, advantages=mb.advantages, returns=mb.returns, starts=mb.episode_starts),
            obs_f32=not b.obs_codes, table=self._mb_table, count=mb.count, states=pairs)
        self._mb_cache[key] = mb
        return mb

    def _mb_checks(self, batch_size, seed, obs, M):
        if obs not in ("f32", "codes"):
            raise ValueError(f"obs must be 'f32' or 'codes', got {obs!r}")
        if obs == "codes" and not self.batch.obs_codes:
            raise ValueError("obs='codes' needs an obs_codes batch")
        B = M if batch_size is None else check_minibatch_size(batch_size)
        return B, _uint("seed", seed) & U64

    def _mb_run(self, mb, seed, epoch, k, ctrl, normalize, count):
        a, dev = mb._args, self.batch.device
        a.seed, a.epoch, a.k = seed, epoch, k
        a.ctrl = ctrl.data_ptr() if ctrl is not None else None
        minibatch_device(a, dev)
        if not normalize:
            return
        adv = mb.advantages
        if count is None:  # only the device knows it
            adv_norm_device(adv, count=mb._count_dev, scratch=mb._scratch)
        else:
            adv_norm_device(adv[:count] if mb.mode == "rows" else adv[:, :count], scratch=mb._scratch)

    def _minibatches(self, mode, batch_size, epoch, seed, normalize, obs):
        T, n = self.n_steps, self.batch.num_envs
        M = T * n if mode == "rows" else n
        B, seed = self._mb_checks(batch_size, seed, obs, M)
        epoch = _uint("epoch", epoch) & U64
        mb = self._mb(mode, B, obs == "codes")
        C.check(C.lib().pe_internal_rollout_minibatch_check(mb._args), "pe_internal_rollout_minibatch")

        def gen():
            for k in range(-(-M // B)):
                count = min(B, M - k * B)
                self._mb_run(mb, seed, epoch, k, None, normalize, count)
                yield mb._head(count)
        return gen()

    def _next_minibatch(self, batch_size, seed, normalize, obs):
        T, n = self.n_steps, self.batch.num_envs
        B, seed = self._mb_checks(batch_size, seed, obs, T * n)
        mb = self._mb("rows", B, obs == "codes")
        self._mb_run(mb, seed, 0, 0, self.minibatch_ctrl, normalize, None)
        return mb

    def _begin(self):
        """Row 0 of a collect: primed from the batch the first time, else the previous collect's
        last row (one device copy of a row)."""
        if not self._primed:
            self._prime()
        else:
            s = self._stride
            self._buf[:s].copy_(self._buf[self.n_steps * s:(self.n_steps + 1) * s])

    # ----------------------------------------------------------------- row 0
    def _prime(self):
        """Row 0 of the first collect: the batch's current obs (as codes on an ``obs_codes``
        batch); every env starts an episode."""
        self._prime_obs(self._row_views[0][0])
        self._start[0].fill_(1)

    def _obs_f32(self, out=None):
        torch, b = self._torch, self.batch
        T, n, D = self.n_steps, b.num_envs, b.obs_dim
        if out is not None and not C.on_device(out, b._dev_index, (torch.float32,), (T * n, D)):
            raise ValueError(f"out must be a contiguous float32 tensor of shape {(T * n, D)} on {b.device}")
        if not b.obs_codes:
            if out is None:
                return self._obs.reshape(T * n, D)
            out.view(T, n, D).copy_(self._obs)
            return out
        if out is None:
            out = torch.empty((T * n, D), dtype=torch.float32, device=b.device)
        with torch.cuda.device(b.device):
            C.check(C.lib().pe_expand_obs_codes(b.handle, T, n, _p(self._buf), self._stride, _p(out), None, None, None,
                                                b._stream()), "pe_expand_obs_codes")
        return out


class RolloutCollector(_Collector):
    """Collects `n_steps` steps of every env of a PlantOSBatch (or a PlantOSVecEnv's batch) under
    a two-tower Policy, entirely on the device.

    gamma / gae_lambda: the GAE parameters; bootstrap_timeouts: add gamma * V(terminal obs) to
    the reward of an episode cut by the time limit only (SB3's TimeLimit.truncated handling);
    deterministic: argmax actions instead of the policy's Philox sampler (whose step counter
    advances by one per step, across collects).  Storage is allocated here, once.  ValueError
    for a one-tower policy (no values), a RecurrentPolicy (RecurrentRolloutCollector collects
    those), n_steps < 1, a policy of another batch, or a batch without autoreset.

    The bootstrap and last_values run the value-only forward (Policy.value): the critic tower
    alone, and for the bootstrap only the tiles that hold an env cut by the time limit only.
    `terminal_values` therefore keeps stale entries for every other env; pe_rollout_record
    reads it only where truncated && !terminated (record_reward, pe_rollout_math.hpp), so no
    stale entry reaches a reward."""

    def __init__(self, batch_or_venv, policy, n_steps, gamma=0.99, gae_lambda=0.95, bootstrap_timeouts=True,
                 deterministic=False):
        if isinstance(policy, RecurrentPolicy):
            raise ValueError("a RecurrentPolicy's rollouts are collected by RecurrentRolloutCollector")
        if not isinstance(policy, Policy):
            raise ValueError("policy must be a plantos_amd.Policy")
        self._setup(unwrap(batch_or_venv), policy, n_steps, gamma, gae_lambda, bootstrap_timeouts, deterministic)

    # ----------------------------------------------------------------- hot path
    def collect(self):
        """Run n_steps steps and return the Rollout.  The first call starts from the batch's
        current obs with every env flagged as an episode start; later calls continue from the
        previous call's last row (one device copy of a row).  Everything is launched on
        torch's current stream: no sync, and after the first call no allocation, so one
        collect() can be captured with torch.cuda.graph and replayed (a replay repeats the
        sampler steps of the capture)."""
        b, pol, T = self.batch, self.policy, self.n_steps
        self._begin()
        rows, views, det = self._rows, self._row_views, self.deterministic
        boot = self.bootstrap_timeouts
        for t in range(T):
            a_t = self.actions[t]
            pol.act(obs=views[t][0], deterministic=det, out=(a_t, self._logits, self.values[t]))
            b.step(a_t, io=rows[t + 1])
            _, rew, te, tr = views[t + 1]
            if boot:
                pol.value(obs=b.terminal_obs, select=(tr, te), out=self.terminal_values)
            record_device(self._logits, a_t, rew, te, tr, self.gamma, self.log_probs[t], rew, self._start[t + 1],
                          terminal_value=self.terminal_values if boot else None, episode_return=b.episode_return,
                          episode_length=b.episode_length, ep_count=self.ep_count, ep_return_sum=self.ep_return_sum,
                          ep_length_sum=self.ep_length_sum)
        pol.value(obs=views[T][0], out=self.last_values)
        gae_device(self._rewards, self.values, self._starts_all, self.last_values, self.gamma, self.gae_lambda,
                   self.advantages, self.returns)
        return self._rollout

    # ----------------------------------------------------------------- host twin
    @staticmethod
    def host_rollout(logits, actions, rewards, terminated, truncated, values, last_values, start0, gamma=0.99,
                     gae_lambda=0.95, terminal_values=None, episode_return=None, episode_length=None, ep_count=None,
                     ep_return_sum=None, ep_length_sum=None):
        """The record and GAE host twins over T recorded steps (numpy): logits [T, n, A],
        actions / rewards / terminated / truncated / values [T, n] (rewards as the step gave
        them), last_values [n], start0 [n] (episode starts of step 0); terminal_values [T, n]
        or None (no bootstrap); episode_return / episode_length [T, n] as the step left them,
        or None.  The accumulators given (contiguous numpy i32 / f64 / i32 [n]) are updated
        in place.  Returns a dict: log_probs, rewards, episode_starts, last_dones, advantages,
        returns."""
        logits = np.asarray(logits, np.float32)
        T, n = logits.shape[:2]
        lp = np.zeros((T, n), np.float32)
        rw = np.zeros((T, n), np.float32)
        st = np.zeros((T + 1, n), np.uint8)
        st[0] = np.asarray(start0) != 0
        for t in range(T):
            lp[t], rw[t], st[t + 1] = host_record(
                logits[t], actions[t], rewards[t], terminated[t], truncated[t], gamma,
                terminal_value=None if terminal_values is None else terminal_values[t],
                episode_return=None if episode_return is None else episode_return[t],
                episode_length=None if episode_length is None else episode_length[t],
                ep_count=ep_count, ep_return_sum=ep_return_sum, ep_length_sum=ep_length_sum)
        adv, ret = host_gae(rw, values, st, last_values, gamma, gae_lambda)
        return dict(log_probs=lp, rewards=rw, episode_starts=st[:T], last_dones=st[T], advantages=adv, returns=ret)


class RecurrentRolloutCollector(_Collector):
    """Collects `n_steps` steps of every env of a PlantOSBatch (or a PlantOSVecEnv's batch) under
    a two-tower RecurrentPolicy, entirely on the device: sb3_contrib's
    RecurrentPPO.collect_rollouts and compute_returns_and_advantage.

    gamma / gae_lambda / bootstrap_timeouts / deterministic: as RolloutCollector's.  Per step
    the policy's `act` reads the row's obs and its episode-start flags and advances the LSTM
    state.  The bootstrap is the critic on the terminal obs from the state AFTER that forward,
    with no start flag and the state not advanced (predict_values(terminal_obs,
    terminal_lstm_state, episode_starts=[False])); last_values is the critic on the last obs
    with the last step's done flags as start flags, the state again left alone.  Both are
    RecurrentPolicy.value.

    Row 0 of the first collect flags every env as an episode start, so the first forward reads
    a zero state whatever the policy held; later collects continue from the previous one's
    last row and from the policy's live state.

    state_snapshots: what `Rollout.lstm_states` holds, [(h, c), ..] per tower, raw (before the
    start flags mask it: sb3_contrib's _last_lstm_states).  "first": the state before step 0,
    f32 [1, n, H] each.  "all": the state before every step, f32 [T, n, H] each, which is
    16 * T * n * H bytes for the two towers (h and c, 4 bytes each), allocated here.

    ValueError for a policy that is no RecurrentPolicy or has no critic tower, a
    state_snapshots other than "first" / "all", and what RolloutCollector refuses."""

    def __init__(self, batch_or_venv, policy, n_steps, gamma=0.99, gae_lambda=0.95, bootstrap_timeouts=True,
                 deterministic=False, state_snapshots="first"):
        if not isinstance(policy, RecurrentPolicy):
            raise ValueError("policy must be a plantos_amd.RecurrentPolicy (RolloutCollector collects a Policy's rollouts)")
        if state_snapshots not in ("first", "all"):
            raise ValueError(f"state_snapshots must be 'first' or 'all', got {state_snapshots!r}")
        self._setup(unwrap(batch_or_venv), policy, n_steps, gamma, gae_lambda, bootstrap_timeouts, deterministic)
        torch, b = self._torch, self.batch
        self.state_snapshots = state_snapshots
        S = self.n_steps if state_snapshots == "all" else 1
        shape = (S, b.num_envs, policy.hidden)
        self.lstm_states = [(torch.zeros(shape, dtype=torch.float32, device=b.device),
                             torch.zeros(shape, dtype=torch.float32, device=b.device)) for _ in policy.towers]
        self._snap = [[(h[t], c[t]) for h, c in self.lstm_states] for t in range(S)]
        self._rollout.lstm_states = self.lstm_states

    # ----------------------------------------------------------------- hot path
    def collect(self):
        """Run n_steps steps and return the Rollout: RolloutCollector.collect's contract (current
        stream, no sync, no allocation after the first call, graph-capturable)."""
        b, pol, T = self.batch, self.policy, self.n_steps
        self._begin()
        rows, views, det = self._rows, self._row_views, self.deterministic
        boot = self.bootstrap_timeouts
        for t in range(T):
            if t < len(self._snap):
                pol.get_states(out=self._snap[t])
            a_t = self.actions[t]
            pol.act(obs=views[t][0], episode_start=self._start[t], deterministic=det,
                    out=(a_t, self._logits, self.values[t]))
            b.step(a_t, io=rows[t + 1])
            _, rew, te, tr = views[t + 1]
            if boot:
                pol.value(obs=b.terminal_obs, select=(tr, te), out=self.terminal_values)
            record_device(self._logits, a_t, rew, te, tr, self.gamma, self.log_probs[t], rew, self._start[t + 1],
                          terminal_value=self.terminal_values if boot else None, episode_return=b.episode_return,
                          episode_length=b.episode_length, ep_count=self.ep_count, ep_return_sum=self.ep_return_sum,
                          ep_length_sum=self.ep_length_sum)
        pol.value(obs=views[T][0], episode_start=self._start[T], out=self.last_values)
        gae_device(self._rewards, self.values, self._starts_all, self.last_values, self.gamma, self.gae_lambda,
                   self.advantages, self.returns)
        return self._rollout

    # ----------------------------------------------------------------- host twin
    @staticmethod
    def host_rollout(hidden, towers, lstm_tensors, mlp_tensors, activation, obs, last_obs, terminal_obs, actions,
                     rewards, terminated, truncated, start0, states0=None, gamma=0.99, gae_lambda=0.95,
                     bootstrap_timeouts=True, state_snapshots="first", episode_return=None, episode_length=None,
                     ep_count=None, ep_return_sum=None, ep_length_sum=None):
        """The recurrent collect in numpy, no device: the policy's host twin (lstm_host_forward)
        stepped over T recorded steps with the carried states, then RolloutCollector.host_rollout
        (host_record / host_gae).

        hidden / towers / lstm_tensors / mlp_tensors / activation: the weights, as
        lstm_host_forward takes them.  obs f32 [T, n, D] (what the policy read at each step),
        last_obs f32 [n, D] (the obs after the last step), terminal_obs f32 [T, n, D] (the
        step's terminal obs; rows of envs not cut by the time limit are evaluated too and
        read by nothing), actions i32 [T, n] (the actions taken: the twin does not sample),
        rewards / terminated / truncated [T, n] as the step gave them, start0 [n] (episode
        starts of step 0), states0 [(h, c), ..] per tower f32 [n, H] (None: zeros), the rest
        as RolloutCollector.host_rollout.  The terminal values and last_values are computed on
        COPIES of the carried states: only the per-step forward advances them.

        Returns RolloutCollector.host_rollout's dict plus values [T, n], terminal_values [T, n]
        (None without the bootstrap), last_values [n], lstm_states (the snapshots,
        [(h, c), ..] of [1, n, H] or [T, n, H]) and final_states [(h, c), ..]."""
        if state_snapshots not in ("first", "all"):
            raise ValueError(f"state_snapshots must be 'first' or 'all', got {state_snapshots!r}")
        obs = np.asarray(obs, np.float32)
        T, n = obs.shape[:2]
        nt = len(towers)
        fwd = lambda x, st, start: lstm_host_forward(hidden, towers, lstm_tensors, mlp_tensors, activation, x,  # noqa: E731
                                                     states=st, episode_start=start)
        copy = lambda st: [(h.copy(), c.copy()) for h, c in st]  # noqa: E731
        if states0 is None:
            states = [(np.zeros((n, hidden), np.float32), np.zeros((n, hidden), np.float32)) for _ in range(nt)]
        else:
            states = [(np.array(h, np.float32), np.array(c, np.float32)) for h, c in states0]
        st = np.zeros((T + 1, n), np.uint8)
        st[0] = np.asarray(start0) != 0
        st[1:] = (np.asarray(terminated) != 0) | (np.asarray(truncated) != 0)
        A = towers[0][-1]
        logits = np.zeros((T, n, A), np.float32)
        values = np.zeros((T, n), np.float32)
        tv = np.zeros((T, n), np.float32) if bootstrap_timeouts else None
        snaps = []
        for t in range(T):
            if t == 0 or state_snapshots == "all":
                snaps.append(copy(states))
            (_, logits[t], values[t]), states = fwd(obs[t], states, st[t])
            if bootstrap_timeouts:
                tv[t] = fwd(terminal_obs[t], copy(states), None)[0][2]
        last_values = fwd(last_obs, copy(states), st[T])[0][2]
        out = RolloutCollector.host_rollout(
            logits, actions, rewards, terminated, truncated, values, last_values, start0, gamma, gae_lambda,
            terminal_values=tv, episode_return=episode_return, episode_length=episode_length, ep_count=ep_count,
            ep_return_sum=ep_return_sum, ep_length_sum=ep_length_sum)
        out.update(values=values, terminal_values=tv, last_values=last_values, final_states=states,
                   lstm_states=[(np.stack([s[i][0] for s in snaps]), np.stack([s[i][1] for s in snaps]))
                                for i in range(nt)])
        return out
