"""What the rollout collectors (rollout.py) and the replay collector (replay.py) share: the batch
behind a venv, the checks that tie a policy to it, the per-env episode accumulators and the first
obs of a collection.  Each collector keeps its own order of checks and its own messages."""
from .codes import encode_obs


def unwrap(batch_or_venv):
    """The PlantOSBatch of a PlantOSBatch or of a PlantOSVecEnv."""
    return getattr(batch_or_venv, "batch", batch_or_venv)


def check_policy_batch(policy, batch):
    if policy.batch is not batch:
        raise ValueError("the policy was made for another batch")


def check_autoreset(batch, who):
    if not batch.cfg.autoreset:
        raise ValueError(f"{who} a batch with autoreset=True")


class Collector:
    def _attach(self, batch, policy):
        """Bind a live batch and policy (a closed one raises) and allocate the per-env state:
        ep_count i32 [n], ep_return_sum f64 [n], ep_length_sum i32 [n], and the empty reset mask."""
        import torch
        self._torch = torch
        batch.handle  # a closed batch raises here
        policy._handle()
        self.batch, self.policy = batch, policy
        n, dev = batch.num_envs, batch.device
        self.ep_count = torch.zeros(n, dtype=torch.int32, device=dev)
        self.ep_return_sum = torch.zeros(n, dtype=torch.float64, device=dev)
        self.ep_length_sum = torch.zeros(n, dtype=torch.int32, device=dev)
        self._no_mask = torch.zeros(n, dtype=torch.uint8, device=dev)
        self._primed = False

    def _prime_obs(self, dst):
        """The batch's current obs into `dst` [n, D] (pe_reset with an empty mask writes every env's
        current obs and resets none): f32 as it is, encoded to byte codes on an ``obs_codes`` batch."""
        b = self.batch
        if not b.obs_codes:
            b.reset(mask=self._no_mask, obs=dst)
        else:
            cfg = b.cfg
            dst.copy_(encode_obs(b.reset(mask=self._no_mask), cfg.grid_size, cfg.lidar_channels, cfg.lidar_range))
        self._primed = True
