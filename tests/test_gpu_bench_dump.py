"""bench.py's plain run on the GPU: the headline window only (none of the --full objects in
the line) and --dump-outputs: the arrays it writes are what the last timed step returned,
checked against the same steps replayed in this process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, K, W, SEED = 300, 12, 3, 7  # 300 envs: several blocks, the last one partly filled


def test_plain_run_dumps_the_last_timed_step(tmp_path):
    import torch
    from plantos_amd import PlantOSBatch

    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--envs", str(N), "--steps", str(K),
                        "--warmup", str(W), "--seed", str(SEED), "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=120, env=env, cwd=REPO)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = lines[0]
    assert d["steps"] == K and d["warmup"] == W and d["value"] > 0 and d["unit"] == "env-steps/s"
    assert d["higher_is_better"] is True and d["dtype"] == "int32/f32"
    assert abs(d["value"] - N * K / (d["ms_per_step"] * 1e-3 * K)) <= 1e-6 * d["value"]
    for k in ("desync", "gather", "cpu_baseline"):
        assert k not in d
    assert "kernel_us_events" not in d["roofline"]

    # the same steps here: W warm-up steps on action rows 0..W-1, K timed steps on rows 0..K-1
    b = PlantOSBatch(N, grid_size=20, num_plants=10, num_obstacles=12, lidar_range=6, lidar_channels=16,
                     seed=SEED, device="cuda:0")
    act = torch.empty(N, dtype=torch.int32, device="cuda:0")
    for t in list(range(W)) + list(range(K)):
        b.synth_actions(SEED, t, out=act)
        obs, rew, te, tr = b.step(act)
    want = {"obs": obs, "reward": rew, "terminated": te, "truncated": tr}
    assert sorted(os.listdir(out)) == sorted(f"{k}.npy" for k in want)
    for name, t in want.items():
        got = np.load(out / f"{name}.npy")
        assert got.dtype == np.float32 and got.shape == tuple(t.shape)
        assert np.array_equal(got, t.to(torch.float32).cpu().numpy()), name
    assert np.count_nonzero(want["obs"].cpu().numpy()) > 0
    b.close()
