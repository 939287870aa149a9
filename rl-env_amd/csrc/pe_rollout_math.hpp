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

// ---------------------------------------------------------------- rollout minibatches
// (csrc/pe_rollout_minibatch.h).  This project's definition of a shuffled epoch: numpy's
// `permutation` (SB3's RolloutBuffer.get) is not reproduced, in the spirit of the replay sampler.
//
// rollout_perm(seed, epoch, domain, M, i): a bijection of [0, M), 1 <= M <= 2^31 - 1, computed
// per index with no table.  A balanced Feistel network of kPermRounds rounds on 2w bits,
// w = max(1, ceil(ceil(log2 M) / 2)) <= 16, cycle-walked until the value is < M: the network
// permutes [0, 2^2w), 2^2w < 4M for M >= 2, so fewer than 4 walks are expected, and a walk ends
// because the cycle of i returns to i < M.  With x = L 2^w + R, round r maps (L, R) to
// (R, L ^ F_r(R)), F_r(R) = the low w bits of word x of the Philox4x32-10 block with
//   key     = (low word of seed, high word of seed)
//   counter = (low word of epoch, r 2^16 + R, high word of epoch, domain)
// which is replay_words' layout (count, index, count >> 32, domain) with the round number above
// the half being mixed.  Two domain words: row permutations (M = T n) and env permutations
// (M = n), distinct from every other kDomain* of the project.
constexpr uint32_t kDomainPermRows = 0x574F5250u;  // "PROW"
constexpr uint32_t kDomainPermEnvs = 0x564E4550u;  // "PENV"
constexpr int kPermRounds = 4;

// w of the definition above.
PE_HD int rollout_perm_bits(uint32_t M) {
  int b = 0;
  while (b < 31 && ((uint32_t)1 << b) < M) ++b;  // b = ceil(log2 M)
  const int w = (b + 1) / 2;
  return w < 1 ? 1 : w;
}

// One pass of the network over x < 2^2w (no cycle walk).
PE_HD uint32_t rollout_perm_pass(uint64_t seed, uint64_t epoch, uint32_t domain, int w, uint32_t x) {
  const uint32_t mask = ((uint32_t)1 << w) - 1u;
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  const uint32_t e0 = (uint32_t)epoch, e1 = (uint32_t)(epoch >> 32);
  uint32_t L = x >> w, R = x & mask;
  for (int r = 0; r < kPermRounds; ++r) {
    const U4 c = {e0, ((uint32_t)r << 16) | R, e1, domain};
    const uint32_t f = philox4x32(c, k0, k1).x & mask;
    const uint32_t nr = L ^ f;
    L = R;
    R = nr;
  }
  return (L << w) | R;
}

PE_HD uint32_t rollout_perm(uint64_t seed, uint64_t epoch, uint32_t domain, uint32_t M, uint32_t i) {
  const int w = rollout_perm_bits(M);
  uint32_t x = i;
  do {
    x = rollout_perm_pass(seed, epoch, domain, w, x);
  } while (x >= M);
  return x;
}

// Advantage normalisation of one minibatch (SB3's PPO.train): out = (a - mean) / (std + 1e-8f)
// over the N valid elements, std the unbiased standard deviation; N < 2 changes nothing.  The
// elements are a[t * ld + j], t < rows, j < count, numbered i = t * count + j, N = rows * count.
// The order, which does not depend on a grid size:
//   - element i belongs to chunk i / kNormChunk; inside a chunk, lane l = (i % kNormChunk) %
//     kNormLanes adds its elements in ascending i, in f64, starting from 0;
//   - the kNormLanes lane sums of a chunk are folded by the tree s[l] += s[l + h] for
//     h = kNormLanes / 2, .., 1 (all l < h at once); s[0] is the chunk's partial sum;
//   - the chunk partials are added in ascending chunk order, starting from 0.
// Pass 1 sums (double)a this way: mean = sum / N.  Pass 2 sums d * d, d = (double)a - mean,
// the same way: var = ss / (N - 1).  std = norm_sqrt_f32(var), the f32 nearest to sqrt(var) as
// defined below.  Then, in f32 with contraction off: out = (a - (float)mean) / (std + 1e-8f).
constexpr int kNormLanes = 256;
constexpr int kNormChunk = 4096;

// The f32 s >= 0 with mid(prev(s), s)^2 <= v < mid(s, next(s))^2, the midpoints and their
// squares exact in f64 (25 and 50 significant bits): sqrt(v) rounded to nearest, found from any
// starting guess, so host and device agree whatever their own sqrt rounds to.  v < 0 or NaN
// gives what (float)sqrt(v) gives.
PE_HD float norm_sqrt_f32(double v) {
  float s = (float)sqrt(v);
  if (!(v >= 0.0) || !(s < INFINITY)) return s;
  for (;;) {  // up while the midpoint above is still <= sqrt(v)
    const float up = bits_to_float(float_to_bits(s) + 1u);
    const double m = 0.5 * ((double)s + (double)up);
    if (!(up < INFINITY) || !(m * m <= v)) break;
    s = up;
  }
  while (s > 0.0f) {  // down while the midpoint below is > sqrt(v)
    const float dn = bits_to_float(float_to_bits(s) - 1u);
    const double m = 0.5 * ((double)s + (double)dn);
    if (!(m * m > v)) break;
    s = dn;
  }
  return s;
}

PE_HD double norm_square(float a, double mean) {
#pragma clang fp contract(off)
  const double d = (double)a - mean;
  return d * d;
}

PE_HD float norm_apply(float a, float mean, float std) {
#pragma clang fp contract(off)
  const float d = a - mean;
  const float s = std + 1e-8f;
  return d / s;
}

}  // namespace pe_pol
