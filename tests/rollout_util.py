"""Shared inputs of the rollout tests (test infra): seeded synthetic step outputs for the record
step and reward / value / start arrays for the GAE scan."""
import numpy as np

F32 = np.float32


def record_inputs(n, A, seed):
    rng = np.random.default_rng(seed)
    l = (rng.standard_normal((n, A)) * 3.0).astype(F32)
    a = rng.integers(0, A, n).astype(np.int32)
    r = rng.uniform(-10.0, 50.0, n).astype(F32)
    te = (np.arange(n) % 4 >= 2).astype(np.uint8)   # all four (terminated, truncated) pairs
    tr = (np.arange(n) % 2).astype(np.uint8)
    perm = rng.permutation(n)
    te, tr = te[perm], tr[perm]
    tv = (rng.uniform(1.0, 30.0, n) * rng.choice([-1.0, 1.0], n)).astype(F32)  # |g tv| >= 0.99: never absorbed
    er = rng.uniform(-200.0, 400.0, n)
    el = rng.integers(1, 1000, n).astype(np.int32)
    return l, a, r, te, tr, tv, er, el


def gae_inputs(T, n, density, seed):
    rng = np.random.default_rng(seed)
    rewards = rng.uniform(-10.0, 50.0, (T, n)).astype(F32)
    values = rng.uniform(-50.0, 150.0, (T, n)).astype(F32)
    last_values = rng.uniform(-50.0, 150.0, n).astype(F32)
    starts = (rng.random((T + 1, n)) < density).astype(np.uint8)
    return rewards, values, starts, last_values
