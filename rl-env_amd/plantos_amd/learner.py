"""A2CLearner: Stable-Baselines3's A2C.train() on the device.

What A2C.train adds to a collected rollout (A2C("MlpPolicy", n_steps=5, net_arch=[256, 256]),
A2C_training.py:216-267): evaluate_actions, the loss -mean(adv logp) + ent_coef (-mean(H)) +
vf_coef mean((returns - v)^2), the backward pass through both MLP towers, clip_grad_norm_ and one
RMSpropTFLike step -- the private pe_internal_learner_* entry points of csrc/pe_learner.h, whose
kernels are hand-written HIP (csrc/pe_learner.hip).  Every output is defined bit for bit by the
host twin (`host_update`; the definition is written out in csrc/pe_learner_math.hpp), which needs
no device.

    policy = Policy.from_state_dict(venv, model.policy.state_dict())
    collector = RolloutCollector(venv, policy, n_steps=5, gamma=0.99, gae_lambda=1.0)
    learner = A2CLearner(policy, max_rows=5 * venv.num_envs)
    venv.reset()
    while training:
        ro = collector.collect()
        stats = learner.train(ro)           # the policy acts with the new weights from here on

Nothing in that loop leaves the device.  `learner.state_dict()` has SB3's key names.
"""
import ctypes

import numpy as np

from . import _capi as C
from ._capi import on_device
from .policy import ACTIVATIONS, Policy, RecurrentPolicy, _check_tensor_shapes, _np, _tower_structs, check_towers

GRAD_CHUNK = 256  # pe_learner_math.hpp kGradChunk: rows per level-one chain of a parameter gradient
STATS = ("policy_loss", "value_loss", "entropy_loss", "loss", "grad_norm", "clip_coef")
DEFAULTS = dict(learning_rate=7e-4, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5, rms_prop_eps=1e-5, alpha=0.99)


def check_learner_towers(towers):
    """check_towers, and two towers: the learner needs pi and vf."""
    towers = check_towers(towers)
    if len(towers) != 2:
        raise ValueError("the A2C learner needs a two-tower policy (pi and vf), got a one-tower policy")
    return towers


def check_learner_policy(towers, precision="f32", recurrent=False):
    """ValueError unless a policy of these towers, precision and kind is one the learner trains:
    feed-forward, f32, two towers.  Returns the checked towers.  Needs no device."""
    if recurrent:
        raise ValueError("the A2C learner does not train a RecurrentPolicy (no BPTT learner)")
    if precision != "f32":
        raise ValueError(f'the A2C learner trains precision="f32" policies only, not {precision!r}')
    return check_learner_towers(towers)


def check_rows(rows, max_rows):
    """ValueError unless 1 <= rows <= max_rows."""
    if not 1 <= int(rows) <= int(max_rows):
        raise ValueError(f"{rows} rows: an update takes 1..max_rows = {max_rows} rows")
    return int(rows)


def learner_plan(obs_dim, max_rows, num_cus, towers, activation="tanh", env_tile=0):
    """pe_internal_learner_plan: the buffer sizes, chunk counts and grids of a learner of `towers`
    over obs rows of `obs_dim` values and at most `max_rows` rows per update, on a device of
    `num_cus` CUs.  Needs no device; ValueError as the constructor's."""
    info = C.PELearnerPlanInfo()
    C.check(C.lib().pe_internal_learner_plan(int(obs_dim), int(max_rows), int(num_cus), len(towers),
                                             _tower_structs(towers), ACTIVATIONS[activation], int(env_tile or 0),
                                             ctypes.byref(info)), "A2CLearner")
    return info


def param_layout(towers, obs_dim):
    """[[(weight offset, weight shape, bias offset, bias shape), ..], ..] per tower and layer in the
    flat parameter vector (tower, layer, weight then bias), and its length."""
    off, out = 0, []
    for t in towers:
        k, tw = obs_dim, []
        for w in t:
            tw.append((off, (w, k), off + w * k, (w,)))
            off += w * k + w
            k = w
        out.append(tw)
    return out, off


def _hyper(kw):
    h = dict(DEFAULTS)
    for k, v in kw.items():
        if k not in h:
            raise TypeError(f"unexpected hyper-parameter {k!r}")
        if v is not None:
            h[k] = float(v)
    return [h[k] for k in ("learning_rate", "ent_coef", "vf_coef", "max_grad_norm", "alpha", "rms_prop_eps")]


def host_update(towers, tensors, activation, obs, actions, advantages, returns, square_avg=None, apply=True, **hyper):
    """The host twin on numpy arrays (pe_internal_learner_update_host), no device: one A2C update.

    towers / tensors / activation: as policy.host_forward takes them; obs f32 [B, D], actions i32
    [B], advantages / returns f32 [B]; square_avg: [[(w, b), ..], ..] shaped like tensors (None:
    ones, a fresh optimizer); hyper: learning_rate, ent_coef, vf_coef, max_grad_norm, alpha,
    rms_prop_eps (SB3's defaults).  The inputs are left as they are.  Returns a dict: tensors and
    square_avg (the updated copies; with apply=False the inputs' copies), gradients (before the
    clip, shaped like tensors) and the f32 scalars policy_loss, value_loss, entropy_loss, loss,
    grad_norm, clip_coef."""
    towers = check_learner_towers(towers)
    if activation not in ACTIVATIONS:
        raise ValueError(f"activation must be one of {sorted(ACTIVATIONS)}")
    obs = np.ascontiguousarray(obs, np.float32)
    if obs.ndim != 2 or obs.shape[0] < 1:
        raise ValueError("obs must be [B, D] with B >= 1")
    B, D = obs.shape
    actions = np.ascontiguousarray(actions, np.int32)
    advantages = np.ascontiguousarray(advantages, np.float32)
    returns = np.ascontiguousarray(returns, np.float32)
    for name, x in (("actions", actions), ("advantages", advantages), ("returns", returns)):
        if x.shape != (B,):
            raise ValueError(f"{name} must have shape {(B,)}")
    host = [[(np.array(_np(w), np.float32, order="C"), np.array(_np(b), np.float32, order="C")) for w, b in tw]
            for tw in tensors]
    _check_tensor_shapes(towers, host, D)
    layout, P = param_layout(towers, D)
    sq = np.ones(P, np.float32)
    if square_avg is not None:
        for tw, lt in zip(square_avg, layout):
            for (w, b), (ow, sw, ob, sb) in zip(tw, lt):
                sq[ow:ow + sw[0] * sw[1]] = np.asarray(_np(w), np.float32).reshape(-1)
                sq[ob:ob + sb[0]] = np.asarray(_np(b), np.float32).reshape(-1)
    grads = np.zeros(P, np.float32)
    out = np.zeros(8, np.float32)
    keep = []
    arr = _tower_structs(towers, host, keep)
    C.check(C.lib().pe_internal_learner_update_host(
        B, D, 2, arr, ACTIVATIONS[activation], C.ptr(obs), C.ptr(actions), C.ptr(advantages), C.ptr(returns),
        *_hyper(hyper), int(bool(apply)), C.ptr(sq), C.ptr(grads), C.ptr(out)), "pe_internal_learner_update_host")
    shaped = lambda flat: [[(flat[ow:ow + sw[0] * sw[1]].reshape(sw).copy(), flat[ob:ob + sb[0]].copy())  # noqa: E731
                            for ow, sw, ob, sb in lt] for lt in layout]
    res = dict(tensors=host, square_avg=shaped(sq), gradients=shaped(grads), flat_gradients=grads)
    res.update({k: out[i] for i, k in enumerate(STATS)})
    return res


def sb3_state_dict(tensors):
    """[[(w, b), ..], ..] of a two-tower policy under SB3's ActorCriticPolicy key names."""
    sd = {}
    for tw, net, head in zip(tensors, ("policy_net", "value_net"), ("action_net", "value_net")):
        for i, (w, b) in enumerate(tw[:-1]):
            sd[f"mlp_extractor.{net}.{2 * i}.weight"], sd[f"mlp_extractor.{net}.{2 * i}.bias"] = w, b
        sd[f"{head}.weight"], sd[f"{head}.bias"] = tw[-1]
    return sd


class A2CLearner:
    """SB3's A2C.train() for a two-tower f32 Policy, on the policy's device.

    learning_rate .. alpha: SB3's A2C defaults (RMSpropTFLike: square_avg starts at ones, epsilon
    inside the root).  max_rows: the most rows one update may hold -- the workspace (every hidden
    activation and its gradient, row-major, about 8.6 KB per row for [256, 256] towers at D = 107)
    is allocated for it, once; None takes the n_steps * n of `collector`, or of the collector of the
    first rollout given to `train` (allocating then).  The learner copies the
    tensors the policy last loaded into master parameters it owns; after every update the policy
    acts with the new ones.  ValueError for a one-tower policy, precision="bf16", a
    RecurrentPolicy, or a policy nothing was loaded into.  Close the
    learner before its policy.

    While a learner is attached, give new weights to `learner.load`, not to `Policy.load`: the
    policy's `host_forward` reads the learner's master parameters from construction on, a
    `Policy.load` would put other weights into the policy's kernel only, and the next update
    overwrites them with the master parameters' successors.  Beyond SB3's A2C.train the class has
    `load`, the `collector=` keyword (its n_steps * n as max_rows) and the `clip_coef` output."""

    def __init__(self, policy, learning_rate=7e-4, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5, rms_prop_eps=1e-5,
                 alpha=0.99, max_rows=None, collector=None):
        import torch
        self._torch = torch
        if not isinstance(policy, (Policy, RecurrentPolicy)):
            raise ValueError("policy must be a plantos_amd.Policy")
        self.towers = check_learner_policy(policy.towers, getattr(policy, "precision", "f32"),
                                           isinstance(policy, RecurrentPolicy))
        if policy._loaded is None:
            raise ValueError("the policy has no weights loaded: load them before making its learner")
        if max_rows is None and collector is not None:
            max_rows = collector.n_steps * collector.batch.num_envs
        if max_rows is not None and int(max_rows) < 1:
            raise ValueError(f"max_rows must be >= 1, got {max_rows}")
        self.policy, self.batch = policy, policy.batch
        self.hyper = dict(learning_rate=learning_rate, ent_coef=ent_coef, vf_coef=vf_coef,
                          max_grad_norm=max_grad_norm, alpha=alpha, rms_prop_eps=rms_prop_eps)
        _hyper(self.hyper)
        self.max_rows, self._h = None, None
        if max_rows is not None:
            self._build(int(max_rows))

    def _build(self, max_rows):
        """Everything the learner allocates, for updates of at most max_rows rows."""
        torch, policy, b = self._torch, self.policy, self.batch
        self.max_rows = max_rows
        dev, D = b.device, b.obs_dim
        props = torch.cuda.get_device_properties(dev)
        self.plan = info = learner_plan(D, self.max_rows, props.multi_processor_count, self.towers,
                                        policy.activation, policy.env_tile)
        self._layout, P = param_layout(self.towers, D)
        assert P == info.n_params, (P, info.n_params)
        z = lambda n, dt=torch.float32: torch.zeros(int(n), dtype=dt, device=dev)  # noqa: E731
        self._params, self._grads, self._sq = z(P), z(P), torch.ones(P, dtype=torch.float32, device=dev)
        self._out, self.n_updates = z(8), z(1, torch.int64)
        self._work = [z(info.ws_floats), z(info.partial_floats), z(info.sums_doubles, torch.float64),
                      z(info.packed_floats), z(info.packed_t_floats)]
        self.parameters = self._shaped(self._params)
        self.gradients = self._shaped(self._grads)
        self.square_avg = self._shaped(self._sq)
        for tw, src in zip(self.parameters, policy._loaded):
            for (w, bias), (sw, sb) in zip(tw, src):
                w.copy_(sw)
                bias.copy_(sb)
        bufs = C.PELearnerBufs(*(x.data_ptr() for x in (self._params, self._grads, self._sq, self._out,
                                                         self.n_updates, *self._work)))
        h = ctypes.c_void_p()
        with torch.cuda.device(dev):
            C.check(C.lib().pe_internal_learner_create(policy._handle(), self.max_rows, ctypes.byref(bufs),
                                                       ctypes.byref(h)), "A2CLearner")
            self._h = h
            C.check(C.lib().pe_internal_learner_repack(h, b._stream()), "pe_internal_learner_repack")
        policy._loaded = self.parameters  # what the policy acts with from here on (live views)
        self.stats = {k: self._out[i] for i, k in enumerate(STATS)}
        self.stats["n_updates"] = self.n_updates

    def _shaped(self, flat):
        return [[(flat[ow:ow + sw[0] * sw[1]].view(sw), flat[ob:ob + sb[0]]) for ow, sw, ob, sb in lt]
                for lt in self._layout]

    def _handle(self):
        if self.max_rows is None:
            raise ValueError("max_rows is required before an update: give it to the constructor, or call "
                             "train(rollout) first, which takes the n_steps * n of the rollout's collector")
        if not getattr(self, "_h", None):
            raise ValueError("A2CLearner is closed")
        return self._h

    def close(self):
        if getattr(self, "_h", None):
            C.check(C.lib().pe_internal_learner_destroy(self._h), "pe_internal_learner_destroy")
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def load(self, tensors, square_avg=None):
        """Replace the master parameters ([[(weight, bias), ..], ..] per tower, as Policy.load takes
        them) and the optimizer state (square_avg shaped alike; None: ones, a fresh optimizer), zero
        n_updates and repack: the policy acts with `tensors` from here on.  Current stream."""
        torch, b = self._torch, self.batch
        self._handle()
        _check_tensor_shapes(self.towers, tensors, b.obs_dim)
        for dst, src in ((self.parameters, tensors), (self.square_avg, square_avg)):
            if src is None:
                self._sq.fill_(1.0)
                continue
            for tw, stw in zip(dst, src):
                for pair, spair in zip(tw, stw):
                    for x, s in zip(pair, spair):
                        x.copy_(torch.as_tensor(s).to(device=b.device, dtype=torch.float32))
        self.n_updates.zero_()
        with torch.cuda.device(b.device):
            C.check(C.lib().pe_internal_learner_repack(self._h, b._stream()), "pe_internal_learner_repack")
        return self

    def state_dict(self):
        """The master parameters under SB3's ActorCriticPolicy key names (device tensors, live views)."""
        return sb3_state_dict(self.parameters)

    def update(self, mb=None, obs=None, actions=None, advantages=None, returns=None, learning_rate=None):
        """One A2C update over a row RolloutMinibatch (its codes when it has them, else its f32
        observations) or over explicit device tensors: obs uint8 codes or float32 [B, D], actions
        i32 [B], advantages / returns f32 [B], contiguous, B <= max_rows.  learning_rate: this
        call's (None: the constructor's); a host value, baked into a captured graph.  Returns a
        dict of device tensors the next update overwrites: policy_loss, value_loss, entropy_loss,
        loss, grad_norm (before the clip), clip_coef (f32 scalars) and n_updates (i64 [1]).
        Kernels on the current stream only; no sync, no allocation: graph-capturable, and a replay
        performs the next update.  ValueError for more than max_rows rows."""
        torch, b = self._torch, self.batch
        self._handle()
        if mb is not None:
            if getattr(mb, "mode", "rows") != "rows" or not isinstance(mb.count, (int, np.integer)):
                raise ValueError("update takes a row minibatch of a known size (Rollout.minibatches)")
            obs = mb.codes if mb.codes is not None else mb.observations
            actions, advantages, returns = mb.actions, mb.advantages, mb.returns
        D = b.obs_dim
        if not (on_device(obs, b._dev_index, (torch.float32, torch.uint8)) and obs.dim() == 2 and obs.shape[1] == D
                and obs.shape[0] >= 1):
            raise ValueError(f"obs must be a contiguous float32 or uint8 tensor of shape (B >= 1, {D}) on {b.device}")
        B = check_rows(obs.shape[0], self.max_rows)
        codes = obs.dtype is torch.uint8
        if codes and not b.obs_codes:
            raise ValueError("uint8 obs codes need a batch created with obs_codes=True")
        for name, x, dt in (("actions", actions, torch.int32), ("advantages", advantages, torch.float32),
                            ("returns", returns, torch.float32)):
            if not on_device(x, b._dev_index, (dt,), (B,)):
                raise ValueError(f"{name} must be a contiguous {dt} tensor of shape {(B,)} on {b.device}")
        hyper = dict(self.hyper)
        if learning_rate is not None:
            hyper["learning_rate"] = learning_rate
        rc = C.lib().pe_internal_learner_update(self._handle(), B, obs.data_ptr(), int(codes), actions.data_ptr(),
                                                advantages.data_ptr(), returns.data_ptr(), *_hyper(hyper), b._stream())
        if rc:
            C.check(rc, "pe_internal_learner_update")
        return self.stats

    def train(self, rollout, normalize_advantage=False, learning_rate=None):
        """A2C.train on a collected Rollout: its one minibatch of all rows
        (rollout.minibatches(None, normalize_advantage=..), codes on an ``obs_codes`` batch), then
        `update`.  Returns update's dict."""
        if self.max_rows is None:
            self._build(rollout._c.n_steps * rollout._c.batch.num_envs)
        obs = "codes" if self.batch.obs_codes else "f32"
        for mb in rollout.minibatches(None, normalize_advantage=normalize_advantage, obs=obs):
            self.last_minibatch = mb
            return self.update(mb, learning_rate=learning_rate)

    def host_update(self, obs, actions, advantages, returns, tensors=None, square_avg=None, apply=True, **hyper):
        """The twin (module-level host_update) with this learner's towers, activation and
        hyper-parameters on numpy arrays; tensors / square_avg None: the learner's own, read back."""
        h = dict(self.hyper)
        h.update(hyper)
        return host_update(self.towers, tensors if tensors is not None else self.parameters, self.policy.activation,
                           obs, actions, advantages, returns,
                           square_avg=square_avg if square_avg is not None else self.square_avg, apply=apply, **h)
