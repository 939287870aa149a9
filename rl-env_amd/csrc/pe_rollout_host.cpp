// pe_rollout_host.cpp -- the host twins of pe_rollout_record and pe_rollout_gae
// (include/plantos_batch.h, "Rollout collection") and of the rollout minibatches
// (pe_rollout_minibatch.h): the definitions executed literally on host arrays with the
// functions of pe_rollout_math.hpp, which the kernels (pe_rollout.hip) include too; and the
// argument rules both sides share.  Plain C++: no handle, no device.
#include <algorithm>
#include <string>

#include "../../include/plantos_batch.h"
#include "pe_rollout_math.hpp"
#include "pe_rollout_minibatch.h"

extern "C" int pe_internal_set_error(int code, const char* msg);

extern "C" int pe_internal_rollout_record_check(int32_t n, int32_t A, const void* logits, const void* actions,
                                                const void* reward, const void* terminated, const void* truncated,
                                                const void* log_prob, const void* reward_out, const void* start_next) {
  auto fail = [](const std::string& m) { return pe_internal_set_error(PE_ERR_ARG, m.c_str()); };
  if (n < 1) return fail("rollout record: n must be >= 1, got " + std::to_string(n));
  if (A < 2 || A > 8) return fail("rollout record: A must be in 2..8, got " + std::to_string(A));
  if (!logits || !actions || !reward || !terminated || !truncated)
    return fail("rollout record: null logits / actions / reward / terminated / truncated");
  if (!log_prob || !reward_out || !start_next) return fail("rollout record: null log_prob / reward_out / start_next");
  return PE_OK;
}

extern "C" int pe_internal_rollout_gae_check(int32_t T, int32_t n, int64_t reward_stride, int64_t value_stride,
                                             int64_t start_stride, int64_t out_stride, const void* rewards,
                                             const void* values, const void* starts, const void* last_values,
                                             const void* advantages, const void* returns) {
  auto fail = [](const std::string& m) { return pe_internal_set_error(PE_ERR_ARG, m.c_str()); };
  if (n < 1) return fail("rollout gae: n must be >= 1, got " + std::to_string(n));
  if (T < 1) return fail("rollout gae: T must be >= 1, got " + std::to_string(T));
  if (reward_stride < n || value_stride < n || start_stride < n || out_stride < n)
    return fail("rollout gae: every row stride must be >= n");
  if (!rewards || !values || !starts || !last_values) return fail("rollout gae: null rewards / values / starts / last_values");
  if (!advantages || !returns) return fail("rollout gae: null advantages / returns");
  return PE_OK;
}

using namespace pe_pol;

extern "C" {

int pe_logf_host(int32_t n, const float* x, float* y) {
  if (n < 0 || (n > 0 && (!x || !y))) return pe_internal_set_error(PE_ERR_ARG, "pe_logf_host: bad n or null argument");
  for (int i = 0; i < n; ++i) y[i] = pe_logf(x[i]);
  return PE_OK;
}

int pe_rollout_record_host(int32_t n, int32_t A, const float* logits, const int32_t* actions, const float* reward,
                           const uint8_t* terminated, const uint8_t* truncated, const float* terminal_value,
                           const double* episode_return, const int32_t* episode_length, double gamma, float* log_prob,
                           float* reward_out, uint8_t* start_next, int32_t* ep_count, double* ep_return_sum,
                           int32_t* ep_length_sum) {
  if (const int rc = pe_internal_rollout_record_check(n, A, logits, actions, reward, terminated, truncated, log_prob,
                                                      reward_out, start_next))
    return rc;
  const float g = (float)gamma;
  for (int e = 0; e < n; ++e) {
    const uint8_t te = terminated[e], tr = truncated[e];
    log_prob[e] = policy_logprob(logits + (size_t)e * A, A, actions[e]);
    reward_out[e] = record_reward(reward[e], te, tr, terminal_value ? terminal_value + e : nullptr, g);
    const bool done = (te | tr) != 0;
    start_next[e] = done ? 1 : 0;
    if (done) {
      if (ep_count) ep_count[e] += 1;
      if (ep_return_sum && episode_return) ep_return_sum[e] += episode_return[e];
      if (ep_length_sum && episode_length) ep_length_sum[e] += episode_length[e];
    }
  }
  return PE_OK;
}

int pe_rollout_gae_host(int32_t T, int32_t n, int64_t reward_stride, int64_t value_stride, int64_t start_stride,
                        int64_t out_stride, const float* rewards, const float* values, const uint8_t* starts,
                        const float* last_values, double gamma, double gae_lambda, float* advantages, float* returns) {
  if (const int rc = pe_internal_rollout_gae_check(T, n, reward_stride, value_stride, start_stride, out_stride, rewards,
                                                   values, starts, last_values, advantages, returns))
    return rc;
  float g, gl;
  gae_factors(gamma, gae_lambda, &g, &gl);
  for (int e = 0; e < n; ++e) {
    float last = 0.0f;
    for (int t = T - 1; t >= 0; --t) {
      const float nv = t == T - 1 ? last_values[e] : values[(int64_t)(t + 1) * value_stride + e];
      const float v = values[(int64_t)t * value_stride + e];
      last = gae_step(rewards[(int64_t)t * reward_stride + e], v, nv, starts[(int64_t)(t + 1) * start_stride + e], g, gl,
                      last);
      advantages[(int64_t)t * out_stride + e] = last;
      returns[(int64_t)t * out_stride + e] = gae_return(last, v);
    }
  }
  return PE_OK;
}

// ---------------------------------------------------------------- rollout minibatches
int pe_internal_rollout_minibatch_check(const pe_rollout_mb* a) {
  auto fail = [](const std::string& m) { return pe_internal_set_error(PE_ERR_ARG, ("rollout minibatch: " + m).c_str()); };
  if (!a) return fail("null argument block");
  if (a->mode != PE_MB_ROWS && a->mode != PE_MB_ENVS) return fail("mode must be PE_MB_ROWS or PE_MB_ENVS");
  if (a->T < 1 || a->n < 1 || a->D < 1) return fail("T, n and D must be >= 1");
  if (a->B < 1) return fail("the batch size must be >= 1, got " + std::to_string(a->B));
  const int64_t rows = (int64_t)a->T * a->n;
  if (rows > 2147483647LL) return fail("T * n must be <= 2^31 - 1, got " + std::to_string(rows));
  const int64_t M = a->mode == PE_MB_ROWS ? rows : (int64_t)a->n;
  const int64_t R = a->mode == PE_MB_ROWS ? (int64_t)a->B : (int64_t)a->T * a->B;
  if (R > 2147483647LL) return fail("T * B must be <= 2^31 - 1");
  const int64_t nmb = (M + a->B - 1) / a->B;
  if (!a->ctrl && a->k >= (uint64_t)nmb)
    return fail("k must be < ceil(M / B) = " + std::to_string(nmb) + ", got " + std::to_string(a->k));
  const int64_t row_bytes = (int64_t)a->n * a->D * (a->obs_f32 ? 4 : 1);
  if (!a->buf || ((uintptr_t)a->buf & 3) != 0) return fail("null or misaligned obs storage");
  if (a->obs_f32 && (a->stride & 3) != 0) return fail("the row stride of f32 storage must be a multiple of 4");
  if (((uintptr_t)a->out_obs & 15) != 0 || ((uintptr_t)a->out_codes & 3) != 0)
    return fail("out_obs must be 16-byte aligned and out_codes 4-byte aligned");
  if (a->T > 1 && a->stride < row_bytes) return fail("the obs row stride is shorter than a row");
  if (a->buf_bytes < (int64_t)(a->T - 1) * a->stride + row_bytes) return fail("buf_bytes does not cover T obs rows");
  if (!a->obs_f32 && !a->table) return fail("code storage needs the code table");
  if (a->obs_f32 && a->out_codes) return fail("f32 storage has no codes to return");
  if (!a->actions || !a->values || !a->log_probs || !a->advantages || !a->returns)
    return fail("null actions / values / log_probs / advantages / returns");
  if (a->s_actions < a->n || a->s_values < a->n || a->s_log_probs < a->n || a->s_advantages < a->n || a->s_returns < a->n)
    return fail("every row stride must be >= n");
  if (!a->indices || !a->out_obs || !a->out_actions || !a->out_values || !a->out_log_probs || !a->out_advantages ||
      !a->out_returns)
    return fail("null output");
  if (a->mode == PE_MB_ENVS && (!a->starts || !a->out_starts || a->s_starts < a->n))
    return fail("env mode needs starts (row stride >= n) and out_starts");
  if (a->n_states < 0 || a->n_states > PE_MB_MAX_STATES) return fail("n_states must be in 0..4");
  if (a->n_states > 0) {
    if (a->mode != PE_MB_ENVS) return fail("states are gathered in env mode only");
    if (a->H < 1) return fail("H must be >= 1 with states");
    for (int s = 0; s < a->n_states; ++s)
      if (!a->state_src[s] || !a->state_dst[s]) return fail("states requested but a state array is null");
  }
  return PE_OK;
}

int pe_internal_rollout_perm_host(int64_t M, uint64_t seed, uint64_t epoch, int32_t mode, int64_t first, int64_t count,
                                  int32_t* out) {
  auto fail = [](const std::string& m) { return pe_internal_set_error(PE_ERR_ARG, ("rollout perm: " + m).c_str()); };
  if (M < 1 || M > 2147483647LL) return fail("M must be in 1..2^31 - 1, got " + std::to_string(M));
  if (mode != PE_MB_ROWS && mode != PE_MB_ENVS) return fail("mode must be PE_MB_ROWS or PE_MB_ENVS");
  if (first < 0 || count < 0 || first > M - count) return fail("positions first .. first + count must lie in [0, M]");
  if (count > 0 && !out) return fail("null out");
  const uint32_t domain = mode == PE_MB_ROWS ? kDomainPermRows : kDomainPermEnvs;
  for (int64_t j = 0; j < count; ++j) out[j] = (int32_t)rollout_perm(seed, epoch, domain, (uint32_t)M, (uint32_t)(first + j));
  return PE_OK;
}

namespace {
// One pass of the normalisation's summation order (pe_rollout_math.hpp): of (double)a, or of
// norm_square(a, mean).
double norm_pass(int64_t N, int64_t count, int64_t ld, const float* a, bool square, double mean) {
  double total = 0.0;
  for (int64_t base = 0; base < N; base += kNormChunk) {
    const int64_t len = std::min<int64_t>(kNormChunk, N - base);
    double s[kNormLanes];
    for (int l = 0; l < kNormLanes; ++l) s[l] = 0.0;
    for (int64_t q = 0; q < len; ++q) {
      const int64_t i = base + q;
      const float v = a[(i / count) * ld + i % count];
      s[q % kNormLanes] += square ? norm_square(v, mean) : (double)v;
    }
    for (int h = kNormLanes / 2; h >= 1; h /= 2)
      for (int l = 0; l < h; ++l) s[l] += s[l + h];
    total += s[0];
  }
  return total;
}
}  // namespace

int pe_internal_rollout_adv_norm_host(int32_t rows, int32_t count, int64_t ld, const float* a, float* out) {
  auto fail = [](const std::string& m) { return pe_internal_set_error(PE_ERR_ARG, ("rollout adv norm: " + m).c_str()); };
  if (rows < 1 || count < 0 || ld < count) return fail("rows must be >= 1, count >= 0 and ld >= count");
  if (!a || !out) return fail("null a / out");
  const int64_t N = (int64_t)rows * count;
  if (N > 2147483647LL) return fail("rows * count must be <= 2^31 - 1");
  float mean = 0.0f, sd = 0.0f;
  if (N >= 2) {
    const double m = norm_pass(N, count, ld, a, false, 0.0) / (double)N;
    const double var = norm_pass(N, count, ld, a, true, m) / (double)(N - 1);
    mean = (float)m;
    sd = norm_sqrt_f32(var);
  }
  for (int64_t t = 0; t < rows; ++t)
    for (int64_t j = 0; j < count; ++j) {
      const float v = a[t * ld + j];
      out[t * ld + j] = N >= 2 ? norm_apply(v, mean, sd) : v;
    }
  return PE_OK;
}

}  // extern "C"
