"""plantos_amd -- MI355X-native batched PlantOSEnv (GammaKing2000/RL-Env hot path).

Public surface:
  PlantOSBatch      N envs in HBM, device tensors in/out (C-ABI: include/plantos_batch.h)
  PlantOSVecEnv     Stable-Baselines3 VecEnv drop-in for DummyVecEnv (A2C_training.py:216-218)
  PlantOSVectorEnv  gymnasium-0.29 VectorEnv convention over the same batch
  Policy            batched MLP policy inference on the device: obs (codes or f32) -> actions
  RecurrentPolicy   the same for LSTM policies (sb3_contrib MlpLstmPolicy), state on the device
  RolloutCollector  on-policy rollouts on the device: rollout buffer, log-probs, time-limit
                    bootstrap and GAE (SB3's collect_rollouts); returns a Rollout
  RecurrentRolloutCollector  the same under a RecurrentPolicy (sb3_contrib's RecurrentPPO), with
                    snapshots of the LSTM state in the Rollout
  RolloutMinibatch  a shuffled minibatch of a Rollout, gathered on the device (SB3's
                    RolloutBuffer.get): Rollout.minibatches / env_minibatches / next_minibatch
  A2CLearner        SB3's A2C.train() on the device: loss, backward pass through both towers,
                    clip_grad_norm_ and the RMSpropTFLike step; the policy acts with the new weights
  ReplayCollector   DQN's collection on the device: epsilon-greedy exploration, the transition
                    ring, uniform minibatch sampling (a ReplayBatch) and TD targets
"""
from .batch import PlantOSBatch  # noqa: F401
from .learner import A2CLearner  # noqa: F401
from .policy import Policy, RecurrentPolicy  # noqa: F401
from .replay import ReplayBatch, ReplayCollector, linear_eps  # noqa: F401
from .rollout import (RecurrentRolloutCollector, Rollout, RolloutCollector, RolloutMinibatch,  # noqa: F401
                      host_adv_norm, host_minibatch_indices)
from .vec_env import PlantOSVecEnv, PlantOSVectorEnv  # noqa: F401

__all__ = ["A2CLearner", "PlantOSBatch", "PlantOSVecEnv", "PlantOSVectorEnv", "Policy", "RecurrentPolicy", "Rollout",
           "RolloutCollector", "RecurrentRolloutCollector", "ReplayBatch", "ReplayCollector", "linear_eps",
           "RolloutMinibatch", "host_minibatch_indices", "host_adv_norm"]
