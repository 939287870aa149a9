"""ReplayCollector: DQN's transition collection on the device.

What Stable-Baselines3's OffPolicyAlgorithm.collect_rollouts, DQN.predict / _sample_action,
ReplayBuffer.add / sample and the target half of DQN.train add to the act / step loop of
DQN("MlpPolicy", buffer_size=2000000, batch_size=64, gamma=0.99, exploration_fraction=0.7,
exploration_initial_eps=1.0, exploration_final_eps=0.05, net_arch=[512,512,256])
(trainingCode.py:203-247): epsilon-greedy exploration, the transition ring with the
terminal-observation and time-limit rules, uniform minibatch sampling and the TD target --
the C-ABI's pe_replay_* (include/plantos_batch.h, "Replay collection") around Policy.act and
PlantOSBatch.step.  The learner (loss, gradients, optimizer, polyak / hard update of the
target net) stays out of scope: what it gets is the sampled batch and its targets, on the
device, and `Policy.load` on a second Policy is how it refreshes the target net.

    q, q_target = Policy.from_state_dict(venv, sd), Policy.from_state_dict(venv, sd)
    rc = ReplayCollector(venv, q, buffer_size=2_000_000)
    venv.reset()
    for it in range(iterations):
        rc.set_eps(linear_eps(it / iterations, 1.0, 0.05, 0.7))
        rc.collect()                               # act -> explore -> step -> store
        mb = rc.sample(64)                         # device tensors; no host sync
        y = rc.targets(mb, q_target, gamma=0.99)
        learner.update(mb.obs_f32(), mb.actions, y)
        q.load(learner.state_dict())

Only ``obs_codes`` batches are supported: the ring stores the obs as byte codes, D = 5C + 27
bytes per obs instead of 4 D, which is what lets SB3's 2 M transitions fit beside the envs
(2 x 214 MB at the headline geometry).  An f32 batch is a ValueError.

Exploration is drawn per env (SB3's DQN.predict draws one number for the whole vector of
envs: all explore or none).  The counters -- rows stored, minibatches drawn -- live on the
device, so a captured collect() or sample() that is replayed writes the next ring slot and
draws fresh random numbers.  Every output is defined bit for bit by the host twins
(`host_select`, `host_sample_indices`, `host_target`, `HostRing`), which need no device.
Multi-GPU: one collector per shard; exploration is keyed by the global env id.
"""
import numpy as np

from . import _capi as C
from ._capi import ptr as _p
from ._collector import Collector, check_autoreset, check_policy_batch, unwrap
from .codes import encode_obs
from .policy import Policy, RecurrentPolicy

U64 = 0xFFFFFFFFFFFFFFFF


def linear_eps(progress, initial=1.0, final=0.05, fraction=0.7):
    """SB3's get_linear_fn(initial, final, fraction) at 1 - progress_remaining = `progress`
    (the share of the training done, 0..1): `final` once progress > fraction, else
    initial + progress * (final - initial) / fraction."""
    progress, initial, final, fraction = float(progress), float(initial), float(final), float(fraction)
    if not fraction > 0.0:
        raise ValueError(f"fraction must be > 0, got {fraction}")
    if progress > fraction:
        return final
    return initial + progress * (final - initial) / fraction


def check_batch_size(B):
    """ValueError unless B is a minibatch size (an integer >= 1)."""
    if int(B) != B or int(B) < 1:
        raise ValueError(f"B must be an integer >= 1, got {B}")
    return int(B)


def check_replay_args(batch, policy, buffer_size):
    """The argument rules of ReplayCollector, before anything touches the device; returns the
    ring's slot count K = max(1, buffer_size // n) (SB3's rule for n_envs > 1)."""
    if isinstance(policy, RecurrentPolicy):
        raise ValueError("a recurrent Q-network is not supported: the policy must be a one-tower Policy")
    if not isinstance(policy, Policy):
        raise ValueError("policy must be a plantos_amd.Policy")
    if len(policy.towers) != 1:
        raise ValueError("a Q-network is one tower: the policy must not have a value tower")
    check_policy_batch(policy, batch)
    if not batch.obs_codes:
        raise ValueError("the replay ring stores obs byte codes: the batch must be created with obs_codes=True")
    check_autoreset(batch, "replay collection needs")
    n = int(batch.num_envs)
    if int(buffer_size) < n:
        raise ValueError(f"buffer_size {buffer_size} holds less than one row of {n} transitions")
    return max(1, int(buffer_size) // n)


# ------------------------------------------------------------------ host twins
def host_select(greedy, A, eps, steps, seed=0, env_id_offset=0, return_explored=False):
    """pe_replay_select_host: the epsilon-greedy actions i32 [n] of step `steps` over the greedy
    actions (numpy); with return_explored also the u8 [n] mask of the envs that explored."""
    greedy = np.ascontiguousarray(greedy, np.int32)
    if greedy.ndim != 1:
        raise ValueError("greedy must be [n]")
    n = greedy.shape[0]
    out = np.zeros(n, np.int32)
    ex = np.zeros(n, np.uint8)
    C.check(C.lib().pe_replay_select_host(n, int(A), _p(greedy), float(eps), int(steps) & U64, int(seed) & U64,
                                          int(env_id_offset) & 0xFFFFFFFF, _p(out), _p(ex)), "pe_replay_select_host")
    return (out, ex) if return_explored else out


def host_sample_indices(B, n, K, steps, draws, seed=0):
    """pe_replay_sample_indices_host: the (slot, env) pairs i32 [B, 2] of draw number `draws`
    from a ring of K slots of n envs that has stored `steps` rows ((-1, -1) when none)."""
    B = check_batch_size(B)
    idx = np.zeros((B, 2), np.int32)
    C.check(C.lib().pe_replay_sample_indices_host(B, int(n), int(K), int(steps) & U64, int(draws) & U64,
                                                  int(seed) & U64, _p(idx)), "pe_replay_sample_indices_host")
    return idx


def host_target(q_next, rewards, dones, gamma):
    """pe_replay_target_host: reward + (g * max_a q_next) * (1 - done), f32 [B] (numpy)."""
    q_next = np.ascontiguousarray(q_next, np.float32)
    if q_next.ndim != 2:
        raise ValueError("q_next must be [B, A]")
    B, A = q_next.shape
    rewards = np.ascontiguousarray(rewards, np.float32)
    dones = np.ascontiguousarray(np.asarray(dones) != 0, np.uint8)
    if rewards.shape != (B,) or dones.shape != (B,):
        raise ValueError(f"rewards and dones must have shape {(B,)}")
    out = np.zeros(B, np.float32)
    C.check(C.lib().pe_replay_target_host(B, A, _p(q_next), _p(rewards), _p(dones), float(gamma), _p(out)),
            "pe_replay_target_host")
    return out


class HostRing:
    """The store's host twin: the ring and its bookkeeping in numpy.  obs / next_obs u8
    [K, n, D], actions i32 [K, n], rewards f32 [K, n], dones u8 [K, n]; steps; the per-env
    episode accumulators ep_count i32 [n], ep_return_sum f64 [n], ep_length_sum i32 [n]."""

    def __init__(self, n, K, grid_size, lidar_channels, lidar_range):
        self.n, self.K = int(n), int(K)
        self.G, self.C, self.R = int(grid_size), int(lidar_channels), int(lidar_range)
        if self.n < 1 or self.K < 1:
            raise ValueError("n and K must be >= 1")
        self.D = D = 5 * self.C + 27
        self.obs = np.zeros((self.K, self.n, D), np.uint8)
        self.next_obs = np.zeros((self.K, self.n, D), np.uint8)
        self.actions = np.zeros((self.K, self.n), np.int32)
        self.rewards = np.zeros((self.K, self.n), np.float32)
        self.dones = np.zeros((self.K, self.n), np.uint8)
        self.steps = 0
        self.ep_count = np.zeros(self.n, np.int32)
        self.ep_return_sum = np.zeros(self.n, np.float64)
        self.ep_length_sum = np.zeros(self.n, np.int32)

    @property
    def filled(self):
        return min(self.steps, self.K)

    def add(self, obs, actions, next_obs, reward, terminated, truncated, terminal_obs, episode_return=None,
            episode_length=None):
        """One step's n transitions into slot steps % K (SB3's _store_transition and
        ReplayBuffer.add): a done env's next_obs is the codes of its terminal obs (f32 rows;
        rows of envs that are not done are not read), done = terminated."""
        s = self.steps % self.K
        te = np.asarray(terminated) != 0
        tr = np.asarray(truncated) != 0
        done = te | tr
        self.obs[s] = obs
        nxt = np.array(next_obs, np.uint8)
        if done.any():
            nxt[done] = encode_obs(np.asarray(terminal_obs, np.float32)[done], self.G, self.C, self.R)
        self.next_obs[s] = nxt
        self.actions[s] = actions
        self.rewards[s] = reward
        self.dones[s] = te
        self.ep_count[done] += 1
        if episode_return is not None:
            self.ep_return_sum[done] += np.asarray(episode_return, np.float64)[done]
        if episode_length is not None:
            self.ep_length_sum[done] += np.asarray(episode_length, np.int32)[done]
        self.steps += 1
        return s


# ------------------------------------------------------------------ the kernels on tensors
def select_device(greedy, A, eps, ctrl, seed, env_id_offset, actions, explored=None):
    """pe_replay_select on device tensors (contiguous, on greedy's device), current stream:
    greedy i32 [n], eps f32 [1], ctrl i64 [PE_REPLAY_CTRL_WORDS], actions i32 [n] (may be
    `greedy`), explored u8 [n] or None."""
    import torch
    with torch.cuda.device(greedy.device):
        C.check(C.lib().pe_replay_select(greedy.shape[0], int(A), _p(greedy), _p(eps), _p(ctrl), int(seed) & U64,
                                         int(env_id_offset) & 0xFFFFFFFF, _p(actions), _p(explored),
                                         C.stream_ptr(greedy.device)), "pe_replay_select")


def store_device(ring, geometry, obs, actions, next_obs, reward, terminated, truncated, terminal_obs, ctrl,
                 episode_return=None, episode_length=None, ep_count=None, ep_return_sum=None, ep_length_sum=None):
    """pe_replay_store on device tensors, current stream.  ring: (obs u8 [K, n, D], next_obs,
    actions i32 [K, n], rewards f32 [K, n], dones u8 [K, n]); geometry: (grid_size,
    lidar_range, lidar_channels) with D = 5 * lidar_channels + 27."""
    import torch
    K, n, D = ring[0].shape
    G, R, Cn = (int(v) for v in geometry)
    if D != 5 * Cn + 27 or tuple(obs.shape) != (n, D) or tuple(next_obs.shape) != (n, D) \
            or tuple(terminal_obs.shape) != (n, D):
        raise ValueError(f"obs, next_obs and terminal_obs must be [{n}, {5 * Cn + 27}] and the ring's rows as wide")
    with torch.cuda.device(obs.device):
        C.check(C.lib().pe_replay_store(n, K, G, R, Cn, _p(obs), _p(actions), _p(next_obs), _p(reward), _p(terminated),
                                        _p(truncated), _p(terminal_obs), _p(episode_return), _p(episode_length),
                                        _p(ring[0]), _p(ring[1]), _p(ring[2]), _p(ring[3]), _p(ring[4]), _p(ep_count),
                                        _p(ep_return_sum), _p(ep_length_sum), _p(ctrl), C.stream_ptr(obs.device)),
                "pe_replay_store")


def sample_device(ring, ctrl, seed, obs, next_obs, actions, rewards, dones, indices):
    """pe_replay_sample on device tensors, current stream: B = obs.shape[0] samples of the ring
    (as store_device's) into obs / next_obs u8 [B, D], actions i32 [B], rewards f32 [B], dones
    u8 [B], indices i32 [B, 2]."""
    import torch
    K, n, D = ring[0].shape
    B = check_batch_size(obs.shape[0])
    with torch.cuda.device(obs.device):
        C.check(C.lib().pe_replay_sample(B, n, K, D, _p(ring[0]), _p(ring[1]), _p(ring[2]), _p(ring[3]), _p(ring[4]),
                                         int(seed) & U64, _p(ctrl), _p(obs), _p(next_obs), _p(actions), _p(rewards),
                                         _p(dones), _p(indices), C.stream_ptr(obs.device)), "pe_replay_sample")


def target_device(q_next, rewards, dones, gamma, out):
    """pe_replay_target on device tensors, current stream: q_next f32 [B, A], rewards f32 [B],
    dones u8 [B], out f32 [B]."""
    import torch
    B, A = q_next.shape
    with torch.cuda.device(q_next.device):
        C.check(C.lib().pe_replay_target(B, A, _p(q_next), _p(rewards), _p(dones), float(gamma), _p(out),
                                         C.stream_ptr(q_next.device)), "pe_replay_target")


class ReplayBatch:
    """One sample()'s minibatch: device tensors owned by the collector (the next sample() of the
    same size overwrites them).  obs / next_obs u8 [B, D] byte codes, actions i32 [B], rewards
    f32 [B], dones u8 [B] (terminated: an episode cut by the time limit alone is not done),
    indices i32 [B, 2] = the (slot, env) drawn; targets f32 [B] once `targets()` ran."""

    def __init__(self, collector, B):
        torch, b = collector._torch, collector.batch
        dev, D, A = b.device, b.obs_dim, collector.policy.towers[0][-1]
        self._c = collector
        self.obs = torch.zeros((B, D), dtype=torch.uint8, device=dev)
        self.next_obs = torch.zeros((B, D), dtype=torch.uint8, device=dev)
        self.actions = torch.zeros(B, dtype=torch.int32, device=dev)
        self.rewards = torch.zeros(B, dtype=torch.float32, device=dev)
        self.dones = torch.zeros(B, dtype=torch.uint8, device=dev)
        self.indices = torch.zeros((B, 2), dtype=torch.int32, device=dev)
        self.targets = torch.zeros(B, dtype=torch.float32, device=dev)
        self._next_actions = torch.zeros(B, dtype=torch.int32, device=dev)
        self._next_q = torch.zeros((B, A), dtype=torch.float32, device=dev)

    def _f32(self, codes, out):
        torch, b = self._c._torch, self._c.batch
        B, D = codes.shape
        if out is None:
            out = torch.empty((B, D), dtype=torch.float32, device=b.device)
        elif not C.on_device(out, b._dev_index, (torch.float32,), (B, D)):
            raise ValueError(f"out must be a contiguous float32 tensor of shape {(B, D)} on {b.device}")
        with torch.cuda.device(b.device):
            C.check(C.lib().pe_expand_obs_codes(b.handle, 1, B, _p(codes), 0, _p(out), None, None, None, b._stream()),
                    "pe_expand_obs_codes")
        return out

    def obs_f32(self, out=None):
        """The obs as float32 [B, D]: one pe_expand_obs_codes launch into `out` (or a new tensor)."""
        return self._f32(self.obs, out)

    def next_obs_f32(self, out=None):
        """The next obs as float32 [B, D] (as obs_f32)."""
        return self._f32(self.next_obs, out)


class ReplayCollector(Collector):
    """Collects DQN transitions of every env of an ``obs_codes`` PlantOSBatch (or a
    PlantOSVecEnv's batch) under a one-tower Q-network Policy, entirely on the device.

    buffer_size: transitions the ring holds, SB3's argument; the ring has K = max(1,
    buffer_size // n) slots of n transitions.  seed keys exploration and sampling.  Storage
    is allocated here, once: 2 K n D bytes of obs codes plus 9 K n bytes of scalars.
    `eps` starts at 1.0 (SB3's exploration_initial_eps).  ValueError for a two-tower or
    recurrent policy, a policy of another batch, a batch without obs_codes or without
    autoreset, and buffer_size < n."""

    def __init__(self, batch_or_venv, q_policy, buffer_size=2_000_000, seed=0):
        b = unwrap(batch_or_venv)
        self.K = K = check_replay_args(b, q_policy, buffer_size)
        self._attach(b, q_policy)
        torch = self._torch
        self.seed = int(seed) & U64
        self.env_id_offset = int(b.cfg.env_id_offset)
        self.geometry = (int(b.cfg.grid_size), int(b.cfg.lidar_range), int(b.cfg.lidar_channels))
        n, D, dev = b.num_envs, b.obs_dim, b.device
        u8, i32, f32 = torch.uint8, torch.int32, torch.float32
        self.obs = torch.zeros((K, n, D), dtype=u8, device=dev)
        self.next_obs = torch.zeros((K, n, D), dtype=u8, device=dev)
        self.ring_actions = torch.zeros((K, n), dtype=i32, device=dev)
        self.rewards = torch.zeros((K, n), dtype=f32, device=dev)
        self.dones = torch.zeros((K, n), dtype=u8, device=dev)
        self.ring = (self.obs, self.next_obs, self.ring_actions, self.rewards, self.dones)
        self.ctrl = torch.zeros(C.PE_REPLAY_CTRL_WORDS, dtype=torch.int64, device=dev)
        self._eps = torch.ones(1, dtype=f32, device=dev)
        self.eps = 1.0
        self.actions = torch.zeros(n, dtype=i32, device=dev)      # the actions last taken
        self.greedy = torch.zeros(n, dtype=i32, device=dev)       # the Q-network's argmax behind them
        self._ios = [b.new_io(), b.new_io()]
        self._views = [b.io_views(io) for io in self._ios]
        self._batches = {}

    # ----------------------------------------------------------------- counters, schedule
    def set_eps(self, v):
        """Set the exploration rate: fills the device scalar on the current stream (no sync; a
        captured collect() reads the value current at replay)."""
        self.eps = float(v)
        self._eps.fill_(self.eps)

    @property
    def steps(self):
        """Rows of transitions stored so far (reads the device counter: synchronizes)."""
        return int(self.ctrl[C.PE_RC_STEPS])

    @property
    def draws(self):
        """Minibatches sampled so far (reads the device counter: synchronizes)."""
        return int(self.ctrl[C.PE_RC_DRAWS])

    @property
    def current_obs(self):
        """u8 [n, D]: the obs codes the next collect() step acts on (after the first collect)."""
        return self._views[0][0]

    # ----------------------------------------------------------------- hot path
    def collect(self, k=1):
        """k times: Q-network argmax on the current obs -> epsilon-greedy select -> step ->
        store.  The first call starts from the batch's current obs.  Two io buffers alternate,
        so the store sees both the obs acted on and the next obs; after an odd k the last
        one is copied back (one device copy of n D + 6 n bytes), an even k costs no copy.
        Everything is launched on torch's current stream: no sync, and after the first call
        no allocation, so collect(k) can be captured with torch.cuda.graph; a replay writes
        the next ring slots and draws fresh exploration numbers."""
        k = int(k)
        if k < 1:
            raise ValueError(f"k must be >= 1, got {k}")
        if not self._primed:
            self._prime_obs(self._views[0][0])  # the first obs: the batch's current one, as codes
        b, pol = self.batch, self.policy
        A = pol.towers[0][-1]
        cur = 0
        for _ in range(k):
            obs = self._views[cur][0]
            pol.act(obs=obs, deterministic=True, out=(self.greedy, None, None))
            select_device(self.greedy, A, self._eps, self.ctrl, self.seed, self.env_id_offset, self.actions)
            b.step(self.actions, io=self._ios[1 - cur])
            nxt, rew, te, tr = self._views[1 - cur]
            store_device(self.ring, self.geometry, obs, self.actions, nxt, rew, te, tr, b.terminal_obs, self.ctrl,
                         episode_return=b.episode_return, episode_length=b.episode_length, ep_count=self.ep_count,
                         ep_return_sum=self.ep_return_sum, ep_length_sum=self.ep_length_sum)
            cur = 1 - cur
        if cur:
            self._ios[0].copy_(self._ios[1])

    def sample(self, B):
        """A ReplayBatch of B transitions drawn uniformly with replacement from what is stored
        (ReplayBuffer.sample).  The batch's tensors belong to the collector: one set per B,
        allocated at the first sample(B) and overwritten by the next.  Before anything is
        stored the indices are (-1, -1) and everything else zero.  Current stream, no sync,
        graph-capturable after the first call of that size; a replay draws afresh."""
        B = check_batch_size(B)
        mb = self._batches.get(B)
        if mb is None:
            mb = self._batches[B] = ReplayBatch(self, B)
        sample_device(self.ring, self.ctrl, self.seed, mb.obs, mb.next_obs, mb.actions, mb.rewards, mb.dones, mb.indices)
        return mb

    def targets(self, mb, target_policy, gamma=0.99, out=None):
        """The TD targets f32 [B] of a ReplayBatch: reward + gamma * (1 - done) * max_a
        Q_target(next_obs), the target network evaluated by `target_policy.act_rows` on the
        next-obs codes.  Written to `out` (a contiguous float32 device tensor [B]) or to
        mb.targets.  Two kernels on the current stream; no sync, no allocation."""
        torch, b = self._torch, self.batch
        if not isinstance(mb, ReplayBatch) or mb._c is not self:
            raise ValueError("mb must be a ReplayBatch of this collector")
        if isinstance(target_policy, RecurrentPolicy) or not isinstance(target_policy, Policy) \
                or len(target_policy.towers) != 1:
            raise ValueError("target_policy must be a one-tower plantos_amd.Policy")
        if target_policy.batch is not b or target_policy.towers[0][-1] != self.policy.towers[0][-1]:
            raise ValueError("target_policy must be made for this batch with the Q-network's number of actions")
        B = mb.obs.shape[0]
        if out is None:
            out = mb.targets
        elif not C.on_device(out, b._dev_index, (torch.float32,), (B,)):
            raise ValueError(f"out must be a contiguous float32 tensor of shape {(B,)} on {b.device}")
        target_policy.act_rows(mb.next_obs, out=(mb._next_actions, mb._next_q, None))
        target_device(mb._next_q, mb.rewards, mb.dones, gamma, out)
        return out

    # ----------------------------------------------------------------- host twins
    def host_select(self, greedy, eps, steps, return_explored=False):
        """host_select with this collector's seed, env id offset and number of actions."""
        return host_select(greedy, self.policy.towers[0][-1], eps, steps, self.seed, self.env_id_offset, return_explored)

    def host_sample_indices(self, B, steps, draws):
        """host_sample_indices with this collector's n, K and seed."""
        return host_sample_indices(B, self.batch.num_envs, self.K, steps, draws, self.seed)

    @staticmethod
    def host_target(q_next, rewards, dones, gamma=0.99):
        return host_target(q_next, rewards, dones, gamma)

    def host_ring(self):
        """An empty HostRing of this collector's shape and geometry."""
        G, R, Cn = self.geometry
        return HostRing(self.batch.num_envs, self.K, G, Cn, R)

    @staticmethod
    def host_store(ring, obs, actions, next_obs, reward, terminated, truncated, terminal_obs, episode_return=None,
                   episode_length=None):
        """HostRing.add: the store's definition in numpy."""
        return ring.add(obs, actions, next_obs, reward, terminated, truncated, terminal_obs, episode_return,
                        episode_length)
