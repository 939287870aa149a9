// pe_rollout_host.cpp -- the host twins of pe_rollout_record and pe_rollout_gae
// (include/plantos_batch.h, "Rollout collection"): the definitions executed literally on
// host arrays with the functions of pe_rollout_math.hpp, which the kernels (pe_rollout.hip)
// include too; and the argument rules both sides share.  Plain C++: no handle, no device.
#include <string>

#include "../../include/plantos_batch.h"
#include "pe_rollout_math.hpp"

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

}  // extern "C"
