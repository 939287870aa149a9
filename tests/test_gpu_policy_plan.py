"""GPU check that policy creation follows its plan (csrc/pe_policy_plan.hpp) on the device's own
CU count: Policy and RecurrentPolicy at 64 envs and at 64 envs per CU get the env tile
pe_internal_policy_plan names, and one act() equals the host twin bit for bit.
"""
import pytest
import torch

from lstm_util import make_lstm_tensors
from policy_util import make_tensors
from test_gpu_policy import check_equal, np_

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
G7 = dict(grid_size=7, num_plants=3, num_obstacles=3, lidar_range=3, lidar_channels=12)
TOWERS, H = [[32, 5], [32, 1]], 32


@pytest.mark.parametrize("per_cu", [0, 64], ids=["n64", "n64xCUs"])
@pytest.mark.parametrize("recurrent", [False, True], ids=["mlp", "lstm"])
def test_create_follows_the_plan(recurrent, per_cu):
    from plantos_amd import PlantOSBatch, Policy, RecurrentPolicy
    from plantos_amd import _capi as C
    from plantos_amd.policy import ACTIVATIONS, _lstm_structs, _tower_structs
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = per_cu * cus or 64
    b = PlantOSBatch(n, seed=5, device=DEV, **G7)
    D = b.obs_dim
    obs = b.reset()
    if recurrent:
        tensors = make_lstm_tensors(D, H, TOWERS, 11)
        pol = RecurrentPolicy(b, H, TOWERS, seed=9).load(tensors)
    else:
        tensors = make_tensors(TOWERS, D, 11, "var")
        pol = Policy(b, TOWERS, seed=9).load(tensors)
    info = C.policy_plan(D, n, cus, _lstm_structs(H, 2) if recurrent else None, _tower_structs(TOWERS),
                         ACTIVATIONS["tanh"])
    assert pol.env_tile == info.env_tile == (64 if per_cu else 32)
    want = pol.host_forward(np_(obs))
    check_equal(pol.act(obs), want[0] if recurrent else want, f"recurrent={recurrent} n={n}")
    pol.close()
    b.close()
