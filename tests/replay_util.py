"""Shared pieces of the replay tests (test infra): an independent numpy Philox4x32-10, the
domain words of the replay definition, and seeded synthetic step outputs for the store."""
import numpy as np

from plantos_amd.codes import CODE_POS, CODE_VIS, code_table

DOMAIN_EPS, DOMAIN_SAMPLE = 0x53504545, 0x504D4153
M32 = np.uint64(0xFFFFFFFF)


def philox4x32(c0, c1, c2, c3, key):
    """philox4x32-10 of counters (c0, c1, c2, c3) (scalars or arrays, broadcast) under the
    64-bit key (low word k0, high word k1): four uint64 arrays holding 32-bit words."""
    c = [np.asarray(v, np.uint64) & M32 for v in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = np.uint64(key & 0xFFFFFFFF), np.uint64((key >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & M32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c


def mulhi32(x, m):
    return (np.asarray(x, np.uint64) * np.uint64(m)) >> np.uint64(32)


def random_codes(rng, rows, geometry):
    """u8 [rows, D] of valid obs codes of geometry (grid_size, lidar_range, lidar_channels)."""
    G, R, C = geometry
    D = 5 * C + 27
    out = np.zeros((rows, D), np.uint8)
    lid = out[:, :5 * C].reshape(rows, C, 5)
    lid[..., 0] = rng.integers(0, R + 1, (rows, C))
    lid[..., 1:] = rng.integers(0, 2, (rows, C, 4)) * (R + 1)
    out[:, 5 * C:5 * C + 2] = CODE_POS + rng.integers(0, G, (rows, 2))
    out[:, 5 * C + 2:] = CODE_VIS + rng.integers(0, 11, (rows, 25))
    return out


def store_inputs(n, geometry, seed):
    """One step's store inputs (numpy): obs / next_obs codes, actions, reward, terminated /
    truncated cycling through all four combinations (over the envs, and for small n over
    consecutive seeds), terminal_obs f32 with real obs values in the rows of done envs and NaN
    in every other row, episode_return / episode_length."""
    G, R, C = geometry
    rng = np.random.default_rng(seed)
    combo = rng.permutation((np.arange(n) + seed) % 4)
    te, tr = (combo >> 1).astype(np.uint8), (combo & 1).astype(np.uint8)
    done = (te | tr) != 0
    term = code_table(G, R)[random_codes(rng, n, geometry)]
    term[~done] = np.nan
    return dict(obs=random_codes(rng, n, geometry), next_obs=random_codes(rng, n, geometry),
                actions=rng.integers(0, 5, n).astype(np.int32), reward=rng.uniform(-10.0, 50.0, n).astype(np.float32),
                terminated=te, truncated=tr, terminal_obs=np.ascontiguousarray(term, np.float32),
                episode_return=rng.uniform(-200.0, 400.0, n), episode_length=rng.integers(1, 1000, n).astype(np.int32))
