"""GPU parity over the accepted geometry domain (tests/domain_cases.py): grid sides up to 128,
LIDAR ranges up to 64, 5 to 8 row words, more than 128 plants, the maze and the curriculum on the
kernel families that never ran them, G = 1..4 and C < 4 -- every case against the oracle twin bit
for bit: the state at creation, 40 steps with auto-resets in every one of them, a masked reset, a
load_maps and a set_state(visits) mid-run, the state, get_info and the curriculum records at the
end.  133 envs: two full 64-env workgroups and a ragged third.

The cases, with the step kernel, the row-word class, the reset path and the seconds one case took
on an MI355X (the oracle twin's host time included):

  G128P20O30R64C16-cur         pe_step_wave                               5-8  lane-hbm  0.79
  G8P3O3R64C16                 pe_step_wave                               5-8  lane-hbm  0.03
  G64P100O120R33C64            pe_step_wave                               5-8  lane-hbm  0.25
  G100P200O300R20C16           pe_step_wave                               5-8  lane-hbm  0.69
  G32P129O30R9C24-cur          pe_step_quad<runtime C,R>                  2    lane-hbm  0.09
  G20P150O12R6C16              pe_step_quad<C16,R6,1word,W8,E16>          1    lane-hbm  0.05
  G1P0O0R1C1                   pe_step_wave                               1    coop      0.11
  G1P0O0R2C4                   pe_step_quad<runtime C,R,1word>            1    coop      0.11
  G2P1O0R3C4                   pe_step_quad<runtime C,R,1word>            1    coop      0.03
  G3P2O0R2C8                   pe_step_quad<runtime C,R,1word>            1    coop      0.07
  G4P3O0R6C16                  pe_step_quad<C16,R6,1word,W8,E16>          1    coop      0.03
  G20P5O12R6C2                 pe_step_wave                               1    coop      0.03
  G30P10O12R7C120              pe_step_wave                               2    lane-hbm  0.04
  G128P100O120R6C64-codes      pe_step_quad<C64,R6,bytetile>              5-8  lane-hbm  0.35
  G128P20O30R9C24              pe_step_quad<runtime C,R>                  5-8  lane-hbm  0.17
  G128P20O30R9C24-codes        pe_step_quad<runtime C,R,bytetile>         5-8  lane-hbm  0.15
  G128P3O12R14C64-maze-codes   pe_step_quad<runtime C,R,bytetile>         5-8  lane-hbm  0.73
  G128P3O12R6C16-maze-cur      pe_step_quad<C16,R6>                       5-8  lane-hbm  0.80
  G128P3O12R4C16-maze          pe_step_quad<C16,R4>                       5-8  lane-hbm  0.72
  G128P3O12R2C10-maze          pe_step_quad<C10,R2>                       5-8  lane-hbm  0.73
  G100P3O12R14C32-maze-cur     pe_step_quad<runtime C,R>                  3-4  lane-hbm  0.46
  G100P3O12R6C16               pe_step_quad<C16,R6>                       3-4  lane-hbm  0.10
  G100P3O12R4C16               pe_step_quad<C16,R4>                       3-4  lane-hbm  0.10
  G100P3O12R2C10               pe_step_quad<C10,R2>                       3-4  lane-hbm  0.14
  G25P3O12R2C32-maze           pe_step_quad<runtime C,R>                  1    lane-lds  0.03
  G24P3O12R4C16-maze           pe_step_quad<C16,R4>                       1    lane-lds  0.03
  G128P3O12R64C100-maze        pe_step_wave                               5-8  lane-hbm  0.49
  G128P3O12R14C64-codes        pe_step_quad<runtime C,R,bytetile>         5-8  lane-hbm  0.15
  G64P3O12R32C64-maze-codes    pe_step_far<C64,R32,bytetile>              3-4  lane-hbm  0.21
  G64P129O12R32C64-codes       pe_step_far<C64,R32,bytetile>              3-4  lane-hbm  0.22
  G52P3O12R6C64-maze-codes     pe_step_quad<C64,R6,bytetile>              2    lane-hbm  0.11
  G25P3O12R6C16-maze           pe_step_quad<C16,R6>                       2    lane-lds  0.03
  G25P3O12R2C64-maze-codes     pe_step_quad<runtime C,R,bytetile>         1    lane-hbm  0.04
  G25P3O12R2C10-maze           pe_step_quad<C10,R2>                       1    lane-lds  0.03
  G20P3O12R6C64-maze-codes     pe_step_quad<C64,R6,bytetile>              1    lane-hbm  0.03
  G20P3O12R6C48-maze-codes     pe_step_quad<runtime C,R,1word,bytetile>   1    lane-hbm  0.03
  G20P3O12R4C16-maze           pe_step_quad<C16,R4,1word>                 1    lane-lds  0.03
  G20P3O12R2C10-maze           pe_step_quad<C10,R2,1word>                 1    lane-lds  0.03
"""
import pytest

import domain_cases as D

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("c", D.CASES, ids=D.case_id)
def test_domain_parity(c):
    D.conditions(c, D.run_case(c, gpu=True))
