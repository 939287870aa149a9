// pe_rollout_math.hpp -- the per-env arithmetic of the rollout definition
// (include/plantos_batch.h, "Rollout collection"), shared by the host twins
// (pe_rollout_host.cpp) and the kernels (pe_rollout.hip), so both execute the same
// operations in the same order: SB3 2.2.1's numpy arithmetic in f32, every product and sum
// rounded on its own (contraction is switched off inside each function), nothing
// re-associated.
#pragma once
#include "pe_policy_math.hpp"

namespace pe_pol {

// The stored reward of one env after a step: the step's reward, plus g * terminal_value
// where the episode was cut by the time limit only (SB3's TimeLimit.truncated) and a
// terminal value is given.
PE_HD float record_reward(float reward, uint8_t terminated, uint8_t truncated, const float* terminal_value, float g) {
#pragma clang fp contract(off)
  if (!terminal_value || !truncated || terminated) return reward;
  const float b = g * *terminal_value;  // the product rounded, then the sum
  return reward + b;
}

// One step of the reverse-time GAE scan: returns the new carried value `last` (the
// advantage of this step).  start_next: the episode-start flag of step t + 1; nv: the
// value of step t + 1 (last_values at t = T - 1).
PE_HD float gae_step(float reward, float value, float nv, uint8_t start_next, float g, float gl, float last) {
#pragma clang fp contract(off)
  const float nnt = 1.0f - (float)(start_next != 0);
  const float gv = g * nv;
  const float gvn = gv * nnt;
  const float rg = reward + gvn;
  const float delta = rg - value;
  const float gn = gl * nnt;
  const float c = gn * last;
  return delta + c;
}

PE_HD float gae_return(float adv, float value) {
#pragma clang fp contract(off)
  return adv + value;
}

// (float)gamma and (float)(gamma * gae_lambda), the product in f64, rounded once.
inline void gae_factors(double gamma, double gae_lambda, float* g, float* gl) {
  *g = (float)gamma;
  *gl = (float)(gamma * gae_lambda);
}

}  // namespace pe_pol
