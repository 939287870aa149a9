// pe_policy_math.hpp -- the scalar functions of the policy definition (include/plantos_batch.h,
// "Policy inference"), shared by the host twin (pe_policy_host.cpp) and the kernel
// (pe_policy.hip), so both execute the same operations in the same order.
//
// Everything here is built from operations that are correctly rounded and identical on the
// host and on gfx950: fmaf, f32 add / sub / mul / div, comparisons, integer and bit
// operations.  No libm / ocml transcendental, no a*b+c left to the compiler (every
// multiply-add is an explicit fmaf and contraction is switched off inside each function),
// no fast-math.  Subnormals are kept on both sides.
#pragma once
#include <stdint.h>
#include <string.h>

#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PE_HD __host__ __device__ inline
#else
#define PE_HD inline
#endif

namespace pe_pol {

constexpr uint32_t kDomainPolicy = 0x594C4F50u;  // Philox counter domain word of the action sampler
constexpr uint32_t kDomainEps = 0x53504545u;     // ... of epsilon-greedy exploration (pe_replay_select)
constexpr uint32_t kDomainSample = 0x504D4153u;  // ... of minibatch sampling (pe_replay_sample)

PE_HD float bits_to_float(uint32_t u) {
  float f;
  memcpy(&f, &u, 4);
  return f;
}
PE_HD uint32_t float_to_bits(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}

// exp(x) in f32 for x clamped to [-87, 88] (NaN passes through): n = round(x log2 e) by the
// 1.5 * 2^23 trick, r = x - n ln2 in two fmaf steps (ln2 split hi + lo), a degree-7 Taylor
// polynomial in fmaf, then one multiply by 2^n built from its bits.
PE_HD float pe_expf(float x) {
#pragma clang fp contract(off)
  if (x != x) return x;
  x = x < -87.0f ? -87.0f : (x > 88.0f ? 88.0f : x);
  const float magic = 12582912.0f;  // 1.5 * 2^23
  const float t = fmaf(x, 1.44269504088896341f, magic);
  const float nf = t - magic;
  float r = fmaf(nf, -0.693145751953125f, x);      // ln2 hi
  r = fmaf(nf, -1.42860682030941723e-06f, r);      // ln2 lo
  float p = 1.98412698412698413e-04f;              // 1/5040
  p = fmaf(p, r, 1.38888888888888894e-03f);        // 1/720
  p = fmaf(p, r, 8.33333333333333322e-03f);        // 1/120
  p = fmaf(p, r, 4.16666666666666644e-02f);        // 1/24
  p = fmaf(p, r, 1.66666666666666657e-01f);        // 1/6
  p = fmaf(p, r, 0.5f);
  p = fmaf(p, r, 1.0f);
  p = fmaf(p, r, 1.0f);
  const int32_t n = (int32_t)nf;                   // -126 .. 127: 2^n is a normal float
  return p * bits_to_float((uint32_t)(n + 127) << 23);
}

// tanh(x) in f32.  |x| < 0.55: x + x^3 P(x^2), P a degree-5 polynomial (a weighted minimax
// fit of (tanh(x)/x - 1)/x^2 on x^2 in [0, 0.3025]) in fmaf;
// 0.55 <= |x| <= 9.1: 1 - 2 / (exp(2|x|) + 1); above: 1 (tanh rounds to 1 from 9.02 on).
// The sign is copied from x's bit; NaN passes through; tanh(+-0) = +-0.
PE_HD float pe_tanhf(float x) {
#pragma clang fp contract(off)
  if (x != x) return x;
  const uint32_t sign = float_to_bits(x) & 0x80000000u;
  const float ax = bits_to_float(float_to_bits(x) & 0x7FFFFFFFu);
  float y;
  if (ax < 0.55f) {
    const float s = ax * ax;
    float p = 0.002398997312411666f;
    p = fmaf(p, s, -0.008416792377829552f);
    p = fmaf(p, s, 0.021783767268061638f);
    p = fmaf(p, s, -0.053959790617227554f);
    p = fmaf(p, s, 0.13333295285701752f);
    p = fmaf(p, s, -0.3333333134651184f);
    const float xs = ax * s;
    y = fmaf(xs, p, ax);
  } else if (ax <= 9.1f) {
    const float e = pe_expf(ax + ax);
    const float d = e + 1.0f;
    const float q = 2.0f / d;
    y = 1.0f - q;
  } else {
    y = 1.0f;
  }
  return bits_to_float(float_to_bits(y) | sign);
}

// log(x) in f32 (the log-probabilities of the rollout, pe_rollout_math.hpp).  x = 2^k m with m
// in [sqrt(1/2), sqrt(2)) taken from the bits; f = m - 1 (exact), s = f / (2 + f),
// log(m) = f - f^2/2 + s (f^2/2 + R(s^2)), R the even / odd split polynomial in s^2 with the
// coefficients Lg1 .. Lg4 of fdlibm's logf, in fmaf; the result is assembled as
// k ln2_hi - ((f^2/2 - (s (f^2/2 + R) + k ln2_lo)) - f), ln2 split hi + lo.
// Domain: positive normal floats.  Outside it: NaN passes through; +-0 -> -inf; x < 0
// (-inf included) -> the quiet NaN 0x7FC00000; +inf -> +inf; a positive subnormal is scaled
// by 2^23 (exact) first and gets its own logarithm.
PE_HD float pe_logf(float x) {
#pragma clang fp contract(off)
  if (x != x) return x;
  uint32_t ix = float_to_bits(x);
  if ((ix & 0x7FFFFFFFu) == 0u) return bits_to_float(0xFF800000u);
  if (ix & 0x80000000u) return bits_to_float(0x7FC00000u);
  if (ix == 0x7F800000u) return x;
  int32_t k = 0;
  if (ix < 0x00800000u) {
    ix = float_to_bits(x * 8388608.0f);  // 2^23: exact
    k = -23;
  }
  ix += 0x3F800000u - 0x3F3504F3u;
  k += (int32_t)(ix >> 23) - 127;
  ix = (ix & 0x007FFFFFu) + 0x3F3504F3u;
  const float f = bits_to_float(ix) - 1.0f;
  const float s = f / (2.0f + f);
  const float z = s * s;
  const float w = z * z;
  const float t1 = w * fmaf(w, 0.24279078841f, 0.40000972152f);    // Lg4, Lg2
  const float t2 = z * fmaf(w, 0.28498786688f, 0.66666662693f);    // Lg3, Lg1
  const float R = t2 + t1;
  const float hfsq = (0.5f * f) * f;
  const float dk = (float)k;
  const float lo = fmaf(s, hfsq + R, dk * 9.0580006145e-06f);      // ln2 lo
  return fmaf(dk, 6.9313812256e-01f, -((hfsq - lo) - f));          // ln2 hi: dk * hi is exact
}

PE_HD float pe_relu(float z) { return z > 0.0f ? z : 0.0f; }

// sigmoid(z) = 1/2 + 1/2 tanh(z / 2): no division of its own, results 0, 1 or in
// [2^-25, 1 - 2^-25] (never subnormal); NaN passes through.
PE_HD float pe_sigmoidf(float z) {
#pragma clang fp contract(off)
  return fmaf(0.5f, pe_tanhf(0.5f * z), 0.5f);
}

// The LSTM cell of the recurrent policy from its four gate pre-activations and the old cell
// state: c' = sigma(z_f) c + sigma(z_i) tanh(z_g) (the product rounded, then one fmaf),
// h' = sigma(z_o) tanh(c').
PE_HD void pe_lstm_cell(float zi, float zf, float zg, float zo, float c, float* h_new, float* c_new) {
#pragma clang fp contract(off)
  const float ig = pe_sigmoidf(zi) * pe_tanhf(zg);
  const float cn = fmaf(pe_sigmoidf(zf), c, ig);
  *c_new = cn;
  *h_new = pe_sigmoidf(zo) * pe_tanhf(cn);
}

// Philox4x32-10, the counter / key layout of the env's generator (pe_device.hpp,
// oracle/plantos_oracle.c); written with 64-bit products so host and device share it.
struct U4 {
  uint32_t x, y, z, w;
};
PE_HD U4 philox4x32(U4 c, uint32_t k0, uint32_t k1) {
  for (int i = 0; i < 10; ++i) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c.x, p1 = (uint64_t)0xCD9E8D57u * c.z;
    const U4 o = {(uint32_t)(p1 >> 32) ^ c.y ^ k0, (uint32_t)p1, (uint32_t)(p0 >> 32) ^ c.w ^ k1, (uint32_t)p0};
    c = o;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c;
}

// u in [0, 1) of env `env_id` (global id) at step t: 24 bits of one Philox block.
PE_HD float policy_uniform(uint64_t seed, uint32_t env_id, uint32_t t) {
  const U4 c = {t, env_id, 0u, kDomainPolicy};
  const U4 o = philox4x32(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  return (float)(o.x >> 8) * 5.9604644775390625e-08f;  // 2^-24: exact
}

// First index of the maximum (torch.argmax; a NaN never wins over an earlier entry).
PE_HD int policy_argmax(const float* l, int A) {
  int best = 0;
  for (int a = 1; a < A; ++a)
    if (l[a] > l[best]) best = a;
  return best;
}

// Categorical sample: p_a = pe_expf(l_a - max l), cumulative sums in action order in f32,
// the first a with u * S < cum_a, else A - 1.
PE_HD int policy_sample(const float* l, int A, float u) {
#pragma clang fp contract(off)
  float m = l[0];
  for (int a = 1; a < A; ++a) m = l[a] > m ? l[a] : m;
  float p[8];
  float S = 0.0f;
  for (int a = 0; a < A; ++a) {
    p[a] = pe_expf(l[a] - m);
    S = S + p[a];
  }
  const float us = u * S;
  float cum = 0.0f;
  for (int a = 0; a < A; ++a) {
    cum = cum + p[a];
    if (us < cum) return a;
  }
  return A - 1;
}

// log-probability of action a under the sampler's distribution: z_k = l_k - max l,
// S = the f32 sum of pe_expf(z_k) in action order (policy_sample's S, in [1, 8]),
// z_a - pe_logf(S).
PE_HD float policy_logprob(const float* l, int A, int a) {
#pragma clang fp contract(off)
  float m = l[0];
  for (int k = 1; k < A; ++k) m = l[k] > m ? l[k] : m;
  float S = 0.0f, za = 0.0f;
  for (int k = 0; k < A; ++k) {
    const float z = l[k] - m;
    S = S + pe_expf(z);
    za = k == a ? z : za;
  }
  return za - pe_logf(S);
}

}  // namespace pe_pol
