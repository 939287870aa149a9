// pe_rollout.hip -- the kernels of on-policy rollout collection: pe_rollout_record (one
// env's log-prob, stored reward with the time-limit bootstrap, next episode-start flag and
// episode accumulators after a step) and pe_rollout_gae (the reverse-time GAE scan) of
// include/plantos_batch.h, "Rollout collection"; and the rollout minibatches of
// pe_rollout_minibatch.h (the permuted gather and the advantage normalisation, described where
// they stand).  The arithmetic is pe_rollout_math.hpp's, shared with the host twins
// (pe_rollout_host.cpp).  All work on caller-owned device arrays on the calling thread's
// current device: no handle, no allocation, no sync.
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
#include "pe_rollout_minibatch.h"

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

// ---------------------------------------------------------------- rollout minibatches
// pe_rollout_minibatch_kernel (pe_rollout_minibatch.h): a workgroup gathers a tile of kMbRows
// output rows (row mode: minibatch rows j; env mode: rows t * B + j of the time-major output).
// Its first kMbRows threads -- one wave -- walk the permutation to their source (t, env),
// gather the scalar fields and leave the byte offset of the source obs row in LDS; then all
// 256 threads sweep the tile's rows * D output floats, 4 consecutive ones per thread: one
// 16-byte store into the flat f32 output (a tile starts at float 64 q D of it, so every chunk
// is aligned; a chunk may span two output rows; the output's last partial chunk: scalar
// stores) and, where asked for, one dword store of the 4 codes.  The source side is irregular:
// rows are D bytes with D odd at arbitrary (t, env).  Where a thread's 4 codes lie in one
// source row it loads the aligned dword that holds the first and, unless that is all four,
// the next one, and shifts the pair into place: up to 3 bytes of a neighbouring env's row are
// touched, never a byte at or past buf + buf_bytes (the second dword is checked against it).
// Chunks that straddle two rows, hold a row past `count` or fail that check load byte by
// byte.  Codes are decoded through a 256-float LDS copy of the caller's table.  f32 storage:
// four dword loads per chunk.
constexpr int kMbThreads = 256;
constexpr int kMbRows = 64;

typedef float v4f __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(kMbThreads) void pe_rollout_minibatch_kernel(pe_rollout_mb a) {
  __shared__ int64_t src[kMbRows];  // byte offset in buf of the tile rows' obs; -1: a row past count
  __shared__ float ctab[256];
  const int tid = (int)threadIdx.x;
  const bool envs = a.mode == PE_MB_ENVS;
  const int64_t R = envs ? (int64_t)a.T * a.B : (int64_t)a.B;
  const int64_t q0 = (int64_t)blockIdx.x * kMbRows;
  const int rows = (int)min((int64_t)kMbRows, R - q0);
  uint64_t epoch = a.epoch, k = a.k;
  if (a.ctrl) {
    epoch = a.ctrl[0];
    k = a.ctrl[1];
  }
  const uint32_t M = envs ? (uint32_t)a.n : (uint32_t)a.T * (uint32_t)a.n;
  const uint64_t nmb = ((uint64_t)M + (uint32_t)a.B - 1) / (uint32_t)a.B;
  const uint64_t first = k < nmb ? k * (uint32_t)a.B : (uint64_t)M;  // < 2^31
  const int count = (int)min((uint64_t)a.B, (uint64_t)M - first);
  if (!a.obs_f32) ctab[tid] = a.table[tid];
  if (tid < rows) {
    const int64_t q = q0 + tid;
    const int tt = envs ? (int)(q / a.B) : 0;
    const int j = (int)(q - (int64_t)tt * a.B);
    int32_t idx = -1, act = 0;
    int64_t s = -1;
    float val = 0.0f, lp = 0.0f, adv = 0.0f, ret = 0.0f;
    uint8_t st = 0;
    if (j < count) {
      const uint32_t r = rollout_perm(a.seed, epoch, envs ? kDomainPermEnvs : kDomainPermRows, M,
                                      (uint32_t)first + (uint32_t)j);
      const int64_t t = envs ? tt : (int64_t)(r / (uint32_t)a.n);
      const int64_t e = envs ? (int64_t)r : (int64_t)(r % (uint32_t)a.n);
      idx = (int32_t)r;
      s = t * a.stride + e * a.D * (a.obs_f32 ? 4 : 1);
      act = a.actions[t * a.s_actions + e];
      val = a.values[t * a.s_values + e];
      lp = a.log_probs[t * a.s_log_probs + e];
      adv = a.advantages[t * a.s_advantages + e];
      ret = a.returns[t * a.s_returns + e];
      if (envs) st = a.starts[t * a.s_starts + e];
    }
    src[tid] = s;
    if (tt == 0) a.indices[j] = idx;
    a.out_actions[q] = act;
    a.out_values[q] = val;
    a.out_log_probs[q] = lp;
    a.out_advantages[q] = adv;
    a.out_returns[q] = ret;
    if (envs) a.out_starts[q] = st;
  }
  if (a.count && blockIdx.x == 0 && tid == 0) *a.count = count;
  __syncthreads();
  const int cnt = rows * a.D;         // the tile's output floats
  const int64_t ob = q0 * a.D;        // a multiple of 64: q0 is
  const uint8_t* buf = static_cast<const uint8_t*>(a.buf);
  for (int b = tid * 4; b < cnt; b += kMbThreads * 4) {
    const int kk = min(4, cnt - b);
    int r = b / a.D, c = b - r * a.D;
    float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    uint32_t cw = 0;
    if (a.obs_f32) {
      for (int q = 0; q < kk; ++q) {
        const int64_t s = src[r];
        if (s >= 0) v[q] = *reinterpret_cast<const float*>(buf + s + 4 * c);
        if (++c == a.D) {
          c = 0;
          ++r;  // read again only while b + q + 1 < cnt, i.e. r < rows
        }
      }
    } else {
      const int64_t s0 = src[r];
      const int64_t off0 = s0 + c;
      const int64_t al = off0 & ~(int64_t)3;
      const int sh = (int)(off0 & 3);
      if (kk == 4 && c + 4 <= a.D && s0 >= 0 && (sh == 0 || al + 8 <= a.buf_bytes)) {
        const uint32_t lo = *reinterpret_cast<const uint32_t*>(buf + al);
        cw = lo;
        if (sh != 0) {
          const uint32_t hi = *reinterpret_cast<const uint32_t*>(buf + al + 4);
          cw = (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * sh));
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = ctab[(cw >> (8 * q)) & 255u];
      } else {
        for (int q = 0; q < kk; ++q) {
          const int64_t s = src[r];
          if (s >= 0) {
            const uint32_t code = buf[s + c];
            cw |= code << (8 * q);
            v[q] = ctab[code];
          }
          if (++c == a.D) {
            c = 0;
            ++r;
          }
        }
      }
    }
    if (kk == 4) {
      v4f w;
      w.x = v[0];
      w.y = v[1];
      w.z = v[2];
      w.w = v[3];
      *reinterpret_cast<v4f*>(a.out_obs + ob + b) = w;
      if (a.out_codes) *reinterpret_cast<uint32_t*>(a.out_codes + ob + b) = cw;
    } else {
      for (int q = 0; q < kk; ++q) {
        a.out_obs[ob + b + q] = v[q];
        if (a.out_codes) a.out_codes[ob + b + q] = (uint8_t)(cw >> (8 * q));
      }
    }
  }
}

// Env mode's states: state_dst[s][j, :] = state_src[s][0, indices[j], :] (zeros where
// indices[j] = -1), one float per thread, blockIdx.y = s.  Runs behind the gather, which wrote
// `indices`.
__global__ __launch_bounds__(kMbThreads) void pe_rollout_state_kernel(pe_rollout_mb a) {
  const int64_t i = (int64_t)blockIdx.x * kMbThreads + threadIdx.x;
  if (i >= (int64_t)a.B * a.H) return;
  const float* sp = a.state_src[0];
  float* dp = a.state_dst[0];
#pragma unroll
  for (int s = 1; s < PE_MB_MAX_STATES; ++s)
    if ((int)blockIdx.y == s) {
      sp = a.state_src[s];
      dp = a.state_dst[s];
    }
  const int64_t j = i / a.H, c = i - j * a.H;
  const int32_t e = a.indices[j];
  dp[i] = e >= 0 ? sp[(int64_t)e * a.H + c] : 0.0f;
}

// ctrl = (epoch, next k) -> the minibatch after it.  One thread, behind every reader.
__global__ void pe_rollout_mb_advance_kernel(uint64_t* ctrl, uint64_t nmb) {
  const uint64_t k = ctrl[1] + 1;
  if (k >= nmb) {
    ctrl[0] += 1;
    ctrl[1] = 0;
  } else {
    ctrl[1] = k;
  }
}

// ---------------------------------------------------------------- advantage normalisation
// The order of pe_rollout_math.hpp.  Up to kNormChunk elements: one workgroup does both passes
// and the division.  More: three launches of one workgroup per chunk -- the chunks' sums, then
// their sums of squares, then the division -- with the chunk partials in `scratch`; thread 0
// of each workgroup adds the partials in ascending order, so every workgroup derives the same
// mean and std.  In place is safe: nothing is written before the last pass has read.
struct NormArgs {
  int rows, cap;
  int64_t ld;
  const int32_t* count_dev;
  const float* a;
  float* out;
  double* scratch;
  int nch_cap;
};

__device__ __forceinline__ int norm_count(const NormArgs& a) {
  const int c = a.count_dev ? *a.count_dev : a.cap;
  return min(max(c, 0), a.cap);
}

__device__ __forceinline__ int64_t norm_index(const NormArgs& a, int count, int64_t i) {
  if (a.rows == 1) return i;
  const int64_t t = i / count;
  return t * a.ld + (i - t * count);
}

constexpr int kNormPer = kNormChunk / kNormLanes;  // elements of a chunk per lane

// Lane l's elements of the chunk at `base`, all loads issued before any is used; v[u] is element
// base + l + u kNormLanes (left alone past the chunk's end).
__device__ __forceinline__ void norm_load(const NormArgs& a, int count, int64_t base, int64_t len, float (&v)[kNormPer]) {
#pragma unroll
  for (int u = 0; u < kNormPer; ++u) {
    const int64_t q = (int64_t)threadIdx.x + u * kNormLanes;
    v[u] = q < len ? a.a[norm_index(a, count, base + q)] : 0.0f;
  }
}

// out = norm_apply over the chunk at `base`.
__device__ __forceinline__ void norm_store(const NormArgs& a, int count, int64_t base, int64_t len, float mean, float sd) {
  float v[kNormPer];
  norm_load(a, count, base, len, v);
#pragma unroll
  for (int u = 0; u < kNormPer; ++u) {
    const int64_t q = (int64_t)threadIdx.x + u * kNormLanes;
    if (q < len) a.out[norm_index(a, count, base + q)] = norm_apply(v[u], mean, sd);
  }
}

// A chunk's partial sum, returned to every thread.  s: kNormLanes doubles of LDS.
__device__ double norm_chunk(const NormArgs& a, int64_t N, int count, int64_t base, bool square, double mean, double* s) {
  const int l = (int)threadIdx.x;
  const int64_t len = min((int64_t)kNormChunk, N - base);
  float v[kNormPer];
  norm_load(a, count, base, len, v);
  double acc = 0.0;
#pragma unroll
  for (int u = 0; u < kNormPer; ++u)
    if ((int64_t)l + u * kNormLanes < len) acc += square ? norm_square(v[u], mean) : (double)v[u];
  s[l] = acc;
  __syncthreads();
  for (int h = kNormLanes / 2; h >= 1; h /= 2) {
    if (l < h) s[l] += s[l + h];
    __syncthreads();
  }
  const double r = s[0];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(kNormLanes) void pe_rollout_adv_norm_kernel(NormArgs a) {
  __shared__ double s[kNormLanes];
  const int count = norm_count(a);
  const int64_t N = (int64_t)a.rows * count;
  const int l = (int)threadIdx.x;
  if (N < 2) {
    if (a.out != a.a)
      for (int64_t q = l; q < N; q += kNormLanes) a.out[norm_index(a, count, q)] = a.a[norm_index(a, count, q)];
    return;
  }
  double total = 0.0;
  total += norm_chunk(a, N, count, 0, false, 0.0, s);
  const double mean = total / (double)N;
  total = 0.0;
  total += norm_chunk(a, N, count, 0, true, mean, s);
  const double var = total / (double)(N - 1);
  const float mf = (float)mean, sd = norm_sqrt_f32(var);
  norm_store(a, count, 0, N, mf, sd);
}

// The chunk partials of `which` (0: sums, 1: sums of squares) added in ascending order by
// thread 0 and handed to every thread.
__device__ double norm_total(const NormArgs& a, int64_t N, int which, double* s) {
  if (threadIdx.x == 0) {
    const int nch = (int)((N + kNormChunk - 1) / kNormChunk);
    double t = 0.0;
    for (int c = 0; c < nch; ++c) t += a.scratch[(int64_t)which * a.nch_cap + c];
    s[0] = t;
  }
  __syncthreads();
  const double r = s[0];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(kNormLanes) void pe_rollout_adv_norm_part_kernel(NormArgs a, int pass) {
  __shared__ double s[kNormLanes];
  const int count = norm_count(a);
  const int64_t N = (int64_t)a.rows * count;
  const int64_t base = (int64_t)blockIdx.x * kNormChunk;
  if (N < 2 || base >= N) return;  // uniform over the workgroup
  double mean = 0.0;
  if (pass == 1) mean = norm_total(a, N, 0, s) / (double)N;
  const double p = norm_chunk(a, N, count, base, pass == 1, mean, s);
  if (threadIdx.x == 0) a.scratch[(int64_t)pass * a.nch_cap + blockIdx.x] = p;
}

__global__ __launch_bounds__(kNormLanes) void pe_rollout_adv_norm_apply_kernel(NormArgs a) {
  __shared__ double s[kNormLanes];
  const int count = norm_count(a);
  const int64_t N = (int64_t)a.rows * count;
  const int64_t base = (int64_t)blockIdx.x * kNormChunk;
  if (base >= N) return;
  const int64_t len = min((int64_t)kNormChunk, N - base);
  const int l = (int)threadIdx.x;
  if (N < 2) {
    if (a.out != a.a)
      for (int64_t q = l; q < len; q += kNormLanes) a.out[norm_index(a, count, base + q)] = a.a[norm_index(a, count, base + q)];
    return;
  }
  const double mean = norm_total(a, N, 0, s) / (double)N;
  const double var = norm_total(a, N, 1, s) / (double)(N - 1);
  const float mf = (float)mean, sd = norm_sqrt_f32(var);
  norm_store(a, count, base, len, mf, sd);
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

int pe_internal_rollout_minibatch(const pe_rollout_mb* a, void* stream) {
  if (const int rc = pe_internal_rollout_minibatch_check(a)) return rc;
  (void)hipGetLastError();
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool envs = a->mode == PE_MB_ENVS;
  const int64_t R = envs ? (int64_t)a->T * a->B : (int64_t)a->B;
  hipLaunchKernelGGL(pe_rollout_minibatch_kernel, dim3((unsigned)((R + kMbRows - 1) / kMbRows)), dim3(kMbThreads), 0, st, *a);
  if (const int rc = launch_fail("pe_rollout_minibatch")) return rc;
  if (a->n_states > 0) {
    const int64_t el = (int64_t)a->B * a->H;
    hipLaunchKernelGGL(pe_rollout_state_kernel, dim3((unsigned)((el + kMbThreads - 1) / kMbThreads), (unsigned)a->n_states),
                       dim3(kMbThreads), 0, st, *a);
    if (const int rc = launch_fail("pe_rollout_minibatch (states)")) return rc;
  }
  if (a->ctrl) {
    const int64_t M = envs ? (int64_t)a->n : (int64_t)a->T * a->n;
    hipLaunchKernelGGL(pe_rollout_mb_advance_kernel, dim3(1), dim3(1), 0, st, a->ctrl, (uint64_t)((M + a->B - 1) / a->B));
    return launch_fail("pe_rollout_minibatch (advance)");
  }
  return PE_OK;
}

int pe_internal_rollout_adv_norm(int32_t rows, int32_t count, int64_t ld, const int32_t* count_dev, const float* a,
                                 float* out, double* scratch, void* stream) {
  auto fail = [](const char* m) { return pe_internal_set_error(PE_ERR_ARG, m); };
  if (rows < 1 || count < 0 || ld < count) return fail("rollout adv norm: rows must be >= 1, count >= 0 and ld >= count");
  if (!a || !out) return fail("rollout adv norm: null a / out");
  const int64_t cap = (int64_t)rows * count;
  if (cap > 2147483647LL) return fail("rollout adv norm: rows * count must be <= 2^31 - 1");
  if (cap > kNormChunk && !scratch) return fail("rollout adv norm: more than 4096 elements need scratch");
  if (cap == 0) return PE_OK;
  (void)hipGetLastError();
  hipStream_t st = static_cast<hipStream_t>(stream);
  NormArgs n{rows, count, ld, count_dev, a, out, scratch, (int)((cap + kNormChunk - 1) / kNormChunk)};
  if (n.nch_cap == 1) {
    hipLaunchKernelGGL(pe_rollout_adv_norm_kernel, dim3(1), dim3(kNormLanes), 0, st, n);
    return launch_fail("pe_rollout_adv_norm");
  }
  for (int pass = 0; pass < 2; ++pass) {
    hipLaunchKernelGGL(pe_rollout_adv_norm_part_kernel, dim3((unsigned)n.nch_cap), dim3(kNormLanes), 0, st, n, pass);
    if (const int rc = launch_fail("pe_rollout_adv_norm (partial sums)")) return rc;
  }
  hipLaunchKernelGGL(pe_rollout_adv_norm_apply_kernel, dim3((unsigned)n.nch_cap), dim3(kNormLanes), 0, st, n);
  return launch_fail("pe_rollout_adv_norm (apply)");
}

}  // extern "C"
