"""The handle is the plan: what a created batch reports equals pe_internal_plan (csrc/pe_plan.hpp)
for the device's CU count, and a create that the plan rejects leaves the device usable."""
import numpy as np
import pytest
import torch

import rules_util as RU
from oracle_rollout import OracleVec
from plantos_amd import _capi as C

pytestmark = pytest.mark.gpu

CASES = [(g, 133, False) for g in RU.CFG] + [("g20", 4200, False), ("g20", 4200, True)]


@pytest.mark.parametrize("name,n,codes", CASES, ids=[f"{g}-n{n}{'-codes' if c else ''}" for g, n, c in CASES])
def test_handle_equals_plan(name, n, codes):
    b = RU.make_batch(RU.CFG[name], n, 31, 1000, 0.7, RU.PRESETS["default"], obs_codes=codes)
    try:
        cus = torch.cuda.get_device_properties(b.device).multi_processor_count
        info = C.plan(b.cfg, n, cus)
        got = (b.kernel_name, b.kernel_variant, b.prefetch_every, b.state_bytes)
        assert got == (info.kernel_name.decode(), info.variant, info.prefetch_every, info.state_bytes)
        assert b.kernel_name == RU.kernel_of(name, n, codes)
    finally:
        b.close()


def test_rejected_create_leaves_the_device_usable():
    with pytest.raises(ValueError) as e:
        RU.make_batch(RU.CFG["g21"], 133, 31, 1000, 0.7, RU.PRESETS["default"], obs_codes=True)
    assert str(e.value) == ("pe_create: obs_codes needs a byte-coded sector kernel (C=16/R=6 with G<=20, C=64/R=6, or "
                            "4<=C<=64 with 2<=R<=14 and no compile-time kernel)")
    cfg, n, seed = RU.CFG["g20"], 133, 2025
    b = RU.make_batch(cfg, n, seed, 1000, 0.7, RU.PRESETS["default"])
    try:
        ov = OracleVec(cfg, np.arange(n), seed)
        act = torch.empty(n, dtype=torch.int32, device="cuda:0")
        for t in range(10):
            b.synth_actions(seed, t, out=act)
            obs, rew, te, tr = b.step(act)
            o_obs, o_rew, o_te, o_tr, *_ = ov.step(act.cpu().numpy())
            assert np.array_equal(RU.np_(obs), o_obs), t
            assert np.array_equal(RU.np_(rew), o_rew.astype(np.float32)), t
            assert np.array_equal(RU.np_(te).astype(bool), o_te) and np.array_equal(RU.np_(tr).astype(bool), o_tr), t
    finally:
        b.close()
