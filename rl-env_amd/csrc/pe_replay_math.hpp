// pe_replay_math.hpp -- the per-element arithmetic of the replay definition
// (include/plantos_batch.h, "Replay collection"), shared by the host twins
// (pe_replay_host.cpp) and the kernels (pe_replay.hip), so both execute the same operations
// in the same order: integer Philox words, one f32 compare, and the TD target in f32 with
// every product and sum rounded on its own (contraction is switched off inside each
// function), nothing re-associated.
#pragma once
#include "pe_policy_math.hpp"

namespace pe_pol {

constexpr int kReplayCtrlSteps = 0, kReplayCtrlDraws = 1;  // u64 words of the control block

// floor(x * m / 2^32): uniform over [0, m) for a uniform 32-bit x.
PE_HD uint32_t mulhi32(uint32_t x, uint32_t m) { return (uint32_t)(((uint64_t)x * m) >> 32); }

// One Philox block of a 64-bit event counter (steps or draws), an index and a domain word:
// ctr = (low word of count, index, high word of count, domain).  The high word is 0 for the
// first 2^32 events, which is the (count, index, 0, domain) of the definition.
PE_HD U4 replay_words(uint64_t seed, uint64_t count, uint32_t index, uint32_t domain) {
  const U4 c = {(uint32_t)count, index, (uint32_t)(count >> 32), domain};
  return philox4x32(c, (uint32_t)seed, (uint32_t)(seed >> 32));
}

// Epsilon-greedy action of env `env_id` (global id) at step `steps`: explore iff u < eps,
// then uniform over all A actions.  *explored (may be null) receives the decision.
PE_HD int32_t replay_select(uint64_t seed, uint64_t steps, uint32_t env_id, int A, float eps, int32_t greedy,
                            uint8_t* explored) {
  const U4 o = replay_words(seed, steps, env_id, kDomainEps);
  const float u = (float)(o.x >> 8) * 5.9604644775390625e-08f;  // 2^-24: exact
  const bool ex = u < eps;
  if (explored) *explored = ex ? 1 : 0;
  return ex ? (int32_t)mulhi32(o.y, (uint32_t)A) : greedy;
}

// (slot, env) of sample j of draw number `draws`: uniform with replacement over filled * n.
PE_HD void replay_sample_index(uint64_t seed, uint64_t draws, uint32_t j, uint32_t filled, uint32_t n, int32_t* slot,
                               int32_t* env) {
  const U4 o = replay_words(seed, draws, j, kDomainSample);
  *slot = (int32_t)mulhi32(o.x, filled);
  *env = (int32_t)mulhi32(o.y, n);
}

// reward + (g * max_a q[a]) * (1 - done); the maximum is the first one in action order.
PE_HD float replay_target(const float* q, int A, float reward, uint8_t done, float g) {
#pragma clang fp contract(off)
  float m = q[0];  // the value at policy_argmax(q, A), without an indexed read
  for (int a = 1; a < A; ++a)
    if (q[a] > m) m = q[a];
  const float gm = g * m;
  const float nd = 1.0f - (float)(done != 0);
  const float b = gm * nd;
  return reward + b;
}

// The byte code of obs value x in column c of a row of D = 5C + 27 values
// (plantos_amd/codes.py encode_obs): LIDAR distance rint(x R); one-hot R + 1 / 0; position
// 96 + rint(x G); visit value 80 + rint(10 x); the products in f64, round-half-even.
PE_HD uint8_t replay_encode(float x, int c, int C5, int R, int G) {
  if (c < C5) {
    if (c % 5 == 0) return (uint8_t)(int)rint((double)x * (double)R);
    return x != 0.0f ? (uint8_t)(R + 1) : (uint8_t)0;
  }
  if (c < C5 + 2) return (uint8_t)(int)(96.0 + rint((double)x * (double)G));
  return (uint8_t)(int)(80.0 + rint((double)x * 10.0));
}

}  // namespace pe_pol
