// pe_rollout.hip -- the two kernels of on-policy rollout collection: pe_rollout_record (one
// env's log-prob, stored reward with the time-limit bootstrap, next episode-start flag and
// episode accumulators after a step) and pe_rollout_gae (the reverse-time GAE scan) of
// include/plantos_batch.h, "Rollout collection".  The arithmetic is pe_rollout_math.hpp's,
// shared with the host twins (pe_rollout_host.cpp).  Both work on caller-owned device
// arrays on the calling thread's current device: no handle, no allocation, no sync.
//
// Record: one thread per env, ~50 B per env; every array is read and written with
// consecutive lanes on consecutive elements (the A logits of a lane are A loads whose 64
// lanes together cover one contiguous 256 A-byte span).
//
// GAE: one thread per env, serial in t (the definition's rounding order is the scan order).
// The loads of step t -- reward, value, start flag -- do not depend on the carried value, so
// a window of kWin steps is loaded into registers while the previous window's dependent
// chain runs: between kWin and 2 kWin steps of loads (576 B per wave and step) are in
// flight per wave.  At 65536 envs a CU holds 4 one-wave workgroups, so that is 18 - 36 KiB
// in flight per CU against an HBM-miss latency of ~900 cycles.  A window reaching below
// t = 0 loads step 0 again (no guard on a load) and skips the stores; T need not be a
// multiple of kWin.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/plantos_batch.h"
#include "pe_rollout_math.hpp"

extern "C" int pe_internal_set_error(int code, const char* msg);
extern "C" int pe_internal_rollout_record_check(int32_t n, int32_t A, const void* logits, const void* actions,
                                                const void* reward, const void* terminated, const void* truncated,
                                                const void* log_prob, const void* reward_out, const void* start_next);
extern "C" int pe_internal_rollout_gae_check(int32_t T, int32_t n, int64_t reward_stride, int64_t value_stride,
                                             int64_t start_stride, int64_t out_stride, const void* rewards,
                                             const void* values, const void* starts, const void* last_values,
                                             const void* advantages, const void* returns);

namespace {
using namespace pe_pol;

constexpr int kRecThreads = 256;
constexpr int kGaeThreads = 64;
constexpr int kWin = 8;

struct RecArgs {
  int n, A;
  const float* logits;
  const int32_t* actions;
  const float* reward;
  const uint8_t* terminated;
  const uint8_t* truncated;
  const float* terminal_value;
  const double* episode_return;
  const int32_t* episode_length;
  float g;
  float* log_prob;
  float* reward_out;
  uint8_t* start_next;
  int32_t* ep_count;
  double* ep_return_sum;
  int32_t* ep_length_sum;
};

__global__ __launch_bounds__(kRecThreads) void pe_rollout_record_kernel(RecArgs a) {
  const int e = (int)(blockIdx.x * kRecThreads + threadIdx.x);
  if (e >= a.n) return;
  float l[8];
  const float* src = a.logits + (size_t)e * a.A;
#pragma unroll
  for (int k = 0; k < 8; ++k) l[k] = k < a.A ? src[k] : 0.0f;
  const uint8_t te = a.terminated[e], tr = a.truncated[e];
  const int act = a.actions[e];
  float lp;
  switch (a.A) {  // a constant A unrolls the loops over l: it stays in registers
    case 2: lp = policy_logprob(l, 2, act); break;
    case 3: lp = policy_logprob(l, 3, act); break;
    case 4: lp = policy_logprob(l, 4, act); break;
    case 5: lp = policy_logprob(l, 5, act); break;
    case 6: lp = policy_logprob(l, 6, act); break;
    case 7: lp = policy_logprob(l, 7, act); break;
    default: lp = policy_logprob(l, 8, act); break;
  }
  a.log_prob[e] = lp;
  a.reward_out[e] = record_reward(a.reward[e], te, tr, a.terminal_value ? a.terminal_value + e : nullptr, a.g);
  const bool done = (te | tr) != 0;
  a.start_next[e] = done ? 1 : 0;
  if (done) {
    if (a.ep_count) a.ep_count[e] += 1;
    if (a.ep_return_sum && a.episode_return) a.ep_return_sum[e] += a.episode_return[e];
    if (a.ep_length_sum && a.episode_length) a.ep_length_sum[e] += a.episode_length[e];
  }
}

struct GaeArgs {
  int T, n;
  int64_t sr, sv, ss, so;  // row strides in elements: rewards, values, starts, advantages / returns
  const float* rewards;
  const float* values;
  const uint8_t* starts;   // T + 1 rows; row 0 is not read
  const float* last_values;
  float g, gl;
  float* advantages;
  float* returns;
};

struct Win {
  float r[kWin], v[kWin];
  uint8_t s[kWin];
};

// Steps hi, hi - 1, .., hi - kWin + 1 of env e.  A step below 0 reads step 0 again (always
// in bounds, never used): the loads carry no guard, so nothing stands between them and the
// window they overlap with.
__device__ __forceinline__ void load_win(const GaeArgs& a, int e, int hi, Win& w) {
#pragma unroll
  for (int j = 0; j < kWin; ++j) {
    const int t = max(hi - j, 0);
    w.r[j] = a.rewards[(int64_t)t * a.sr + e];
    w.v[j] = a.values[(int64_t)t * a.sv + e];
    w.s[j] = a.starts[(int64_t)(t + 1) * a.ss + e];
  }
}

// The dependent chain over one loaded window; only the stores of steps >= 0 happen (past
// step 0 the carried values are no longer used).
__device__ __forceinline__ void scan_win(const GaeArgs& a, int e, int hi, const Win& w, float& nv, float& last) {
#pragma unroll
  for (int j = 0; j < kWin; ++j) {
    const int t = hi - j;
    last = gae_step(w.r[j], w.v[j], nv, w.s[j], a.g, a.gl, last);
    nv = w.v[j];
    if (t >= 0) {
      a.advantages[(int64_t)t * a.so + e] = last;
      a.returns[(int64_t)t * a.so + e] = gae_return(last, nv);
    }
  }
}

__global__ __launch_bounds__(kGaeThreads) void pe_rollout_gae_kernel(GaeArgs a) {
  const int e = (int)(blockIdx.x * kGaeThreads + threadIdx.x);
  if (e >= a.n) return;
  Win wa, wb;  // two windows by name, no copies: a copy would wait for the loads it moves
  float nv = a.last_values[e];
  float last = 0.0f;
  load_win(a, e, a.T - 1, wa);
  for (int hi = a.T - 1; hi >= 0; hi -= 2 * kWin) {
    load_win(a, e, hi - kWin, wb);  // the next window's loads are issued before this one's chain
    scan_win(a, e, hi, wa, nv, last);
    load_win(a, e, hi - 2 * kWin, wa);
    scan_win(a, e, hi - kWin, wb, nv, last);
  }
}

int launch_fail(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return PE_OK;
  return pe_internal_set_error(PE_ERR_DEVICE, (std::string(what) + ": " + hipGetErrorString(e)).c_str());
}

}  // namespace

extern "C" {

int pe_rollout_record(int32_t n, int32_t A, const float* logits, const int32_t* actions, const float* reward,
                      const uint8_t* terminated, const uint8_t* truncated, const float* terminal_value,
                      const double* episode_return, const int32_t* episode_length, double gamma, float* log_prob,
                      float* reward_out, uint8_t* start_next, int32_t* ep_count, double* ep_return_sum,
                      int32_t* ep_length_sum, void* stream) {
  if (const int rc = pe_internal_rollout_record_check(n, A, logits, actions, reward, terminated, truncated, log_prob,
                                                      reward_out, start_next))
    return rc;
  RecArgs a;
  a.n = n;
  a.A = A;
  a.logits = logits;
  a.actions = actions;
  a.reward = reward;
  a.terminated = terminated;
  a.truncated = truncated;
  a.terminal_value = terminal_value;
  a.episode_return = episode_return;
  a.episode_length = episode_length;
  a.g = (float)gamma;
  a.log_prob = log_prob;
  a.reward_out = reward_out;
  a.start_next = start_next;
  a.ep_count = ep_count;
  a.ep_return_sum = ep_return_sum;
  a.ep_length_sum = ep_length_sum;
  hipLaunchKernelGGL(pe_rollout_record_kernel, dim3((unsigned)((n + kRecThreads - 1) / kRecThreads)), dim3(kRecThreads), 0,
                     static_cast<hipStream_t>(stream), a);
  return launch_fail("pe_rollout_record");
}

int pe_rollout_gae(int32_t T, int32_t n, int64_t reward_stride, int64_t value_stride, int64_t start_stride,
                   int64_t out_stride, const float* rewards, const float* values, const uint8_t* starts,
                   const float* last_values, double gamma, double gae_lambda, float* advantages, float* returns,
                   void* stream) {
  if (const int rc = pe_internal_rollout_gae_check(T, n, reward_stride, value_stride, start_stride, out_stride, rewards,
                                                   values, starts, last_values, advantages, returns))
    return rc;
  GaeArgs a;
  a.T = T;
  a.n = n;
  a.sr = reward_stride;
  a.sv = value_stride;
  a.ss = start_stride;
  a.so = out_stride;
  a.rewards = rewards;
  a.values = values;
  a.starts = starts;
  a.last_values = last_values;
  gae_factors(gamma, gae_lambda, &a.g, &a.gl);
  a.advantages = advantages;
  a.returns = returns;
  hipLaunchKernelGGL(pe_rollout_gae_kernel, dim3((unsigned)((n + kGaeThreads - 1) / kGaeThreads)), dim3(kGaeThreads), 0,
                     static_cast<hipStream_t>(stream), a);
  return launch_fail("pe_rollout_gae");
}

}  // extern "C"
