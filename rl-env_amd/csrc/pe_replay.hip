// pe_replay.hip -- the kernels of DQN replay collection: pe_replay_select (epsilon-greedy over
// a forward's greedy actions), pe_replay_store (one step's n transitions into a ring slot,
// terminal obs encoded to byte codes), pe_replay_sample (a uniformly drawn minibatch gathered
// into dense outputs) and pe_replay_target (the TD target) of include/plantos_batch.h,
// "Replay collection".  The arithmetic is pe_replay_math.hpp's, shared with the host twins
// (pe_replay_host.cpp).  All work on caller-owned device arrays on the calling thread's
// current device: no handle, no allocation, no sync.
//
// Counters: steps and draws live in the caller's control block.  The store and sample kernels
// read their counter in every workgroup, so they never write it: a one-thread launch behind
// each of them adds 1 (stream order puts it after every reader, and before the next call's).
//
// Select, target: one thread per env / sample; consecutive lanes on consecutive elements.
//
// Store: the obs planes are byte arrays of n * D bytes per slot.  A thread moves 4 consecutive
// bytes of the slot's row: as one dword load and one dword store per plane when the row's
// byte offset slot * n * D is a multiple of 4 (always, if n * D is), else byte by byte.  The
// next-obs dword is patched byte by byte where its env is done: those bytes are encoded from
// the f32 terminal obs (at most two envs share a dword, D >= 32).  Rows of terminal_obs of
// envs that are not done are never addressed.  Thread e < n also writes env e's scalars.
//
// Sample: a workgroup gathers a tile of 16 samples.  Its first 16 threads draw the tile's
// (slot, env) pairs, write the scalars and leave the source row numbers in LDS; then all 256
// threads sweep the tile's 16 * D output bytes of each plane, 4 consecutive output bytes per
// thread.  The output side is what can be made regular: a tile starts at byte 16 j D of the
// dense output, a multiple of 16, so every thread's 4 bytes are one aligned dword store (the
// last partial dword of the whole output: byte stores).  The source side cannot: rows are D
// bytes with D odd at arbitrary (slot, env), so a row starts at any byte offset.  Where a
// thread's 4 bytes lie in one sampled row (all but one or two dwords per row) it loads the
// aligned dword that holds the first of them and, unless that is all four, the next one, and
// shifts the pair into place: the loads may touch up to 3 bytes of the neighbouring rows but
// never leave the plane (the second dword is checked against its end; the ring planes are
// 4-byte aligned).  The dwords that straddle two samples, and the one at the plane's end,
// are 4 byte loads, never addressed outside the sampled rows.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/plantos_batch.h"
#include "pe_replay_math.hpp"

extern "C" int pe_internal_set_error(int code, const char* msg);
extern "C" int pe_internal_replay_select_check(int32_t n, int32_t A, const void* greedy, const void* actions);
extern "C" int pe_internal_replay_store_check(int32_t n, int32_t K, int32_t G, int32_t R, int32_t C, const void* obs,
                                              const void* actions, const void* next_obs, const void* reward,
                                              const void* terminated, const void* truncated, const void* terminal_obs,
                                              const void* ring_obs, const void* ring_next_obs, const void* ring_actions,
                                              const void* ring_rewards, const void* ring_dones, const void* ctrl);
extern "C" int pe_internal_replay_sample_check(int32_t B, int32_t n, int32_t K, int32_t D, const void* ring_obs,
                                               const void* ring_next_obs, const void* ring_actions,
                                               const void* ring_rewards, const void* ring_dones, const void* ctrl,
                                               const void* obs, const void* next_obs, const void* actions,
                                               const void* rewards, const void* dones, const void* indices);
extern "C" int pe_internal_replay_target_check(int32_t B, int32_t A, const void* q_next, const void* rewards,
                                               const void* dones, const void* targets);

namespace {
using namespace pe_pol;

constexpr int kThreads = 256;
constexpr int kSampRows = 16;  // samples per workgroup of the gather

__global__ void pe_replay_advance_kernel(uint64_t* ctrl, int word) { ctrl[word] += 1; }

struct SelArgs {
  int n, A;
  const int32_t* greedy;
  const float* eps;
  const uint64_t* ctrl;
  uint64_t seed;
  uint32_t env_off;
  int32_t* actions;
  uint8_t* explored;
};

__global__ __launch_bounds__(kThreads) void pe_replay_select_kernel(SelArgs a) {
  const int e = (int)(blockIdx.x * kThreads + threadIdx.x);
  if (e >= a.n) return;
  const uint64_t steps = a.ctrl[kReplayCtrlSteps];
  const float eps = *a.eps;
  a.actions[e] = replay_select(a.seed, steps, a.env_off + (uint32_t)e, a.A, eps, a.greedy[e],
                               a.explored ? a.explored + e : nullptr);
}

struct StoreArgs {
  int n, K, D, C5, R, G;
  const uint8_t* obs;
  const int32_t* actions;
  const uint8_t* next_obs;
  const float* reward;
  const uint8_t* terminated;
  const uint8_t* truncated;
  const float* terminal_obs;
  const double* episode_return;
  const int32_t* episode_length;
  uint8_t* ring_obs;
  uint8_t* ring_next;
  int32_t* ring_actions;
  float* ring_rewards;
  uint8_t* ring_dones;
  int32_t* ep_count;
  double* ep_return_sum;
  int32_t* ep_length_sum;
  const uint64_t* ctrl;
};

__global__ __launch_bounds__(kThreads) void pe_replay_store_kernel(StoreArgs a) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const int64_t slot = (int64_t)(a.ctrl[kReplayCtrlSteps] % (uint64_t)a.K);
  if (i < a.n) {  // env i's scalars
    const int64_t o = slot * a.n + i;
    const uint8_t te = a.terminated[i], tr = a.truncated[i];
    a.ring_actions[o] = a.actions[i];
    a.ring_rewards[o] = a.reward[i];
    a.ring_dones[o] = te ? 1 : 0;
    if ((te | tr) != 0) {
      if (a.ep_count) a.ep_count[i] += 1;
      if (a.ep_return_sum && a.episode_return) a.ep_return_sum[i] += a.episode_return[i];
      if (a.ep_length_sum && a.episode_length) a.ep_length_sum[i] += a.episode_length[i];
    }
  }
  const int64_t nd = (int64_t)a.n * a.D;
  const int64_t b0 = i * 4;
  if (b0 >= nd) return;
  const int cnt = (int)min((int64_t)4, nd - b0);
  const int64_t rowb = slot * nd;
  const bool wide = cnt == 4 && (rowb & 3) == 0;
  uint32_t vo = 0, vn = 0;
  if (wide) {
    vo = *reinterpret_cast<const uint32_t*>(a.obs + b0);
    vn = *reinterpret_cast<const uint32_t*>(a.next_obs + b0);
  } else {
    for (int q = 0; q < cnt; ++q) {
      vo |= (uint32_t)a.obs[b0 + q] << (8 * q);
      vn |= (uint32_t)a.next_obs[b0 + q] << (8 * q);
    }
  }
  int64_t e = b0 / a.D;
  int c = (int)(b0 - e * a.D);
  bool done = (a.terminated[e] | a.truncated[e]) != 0;
  for (int q = 0; q < cnt; ++q) {
    if (done) {
      const uint32_t code = replay_encode(a.terminal_obs[e * a.D + c], c, a.C5, a.R, a.G);
      vn = (vn & ~(0xFFu << (8 * q))) | (code << (8 * q));
    }
    if (++c == a.D && q + 1 < cnt) {  // the next byte is the next env's first (e + 1 < n: b0 + q + 1 < nd)
      c = 0;
      ++e;
      done = (a.terminated[e] | a.truncated[e]) != 0;
    }
  }
  if (wide) {
    *reinterpret_cast<uint32_t*>(a.ring_obs + rowb + b0) = vo;
    *reinterpret_cast<uint32_t*>(a.ring_next + rowb + b0) = vn;
  } else {
    for (int q = 0; q < cnt; ++q) {
      a.ring_obs[rowb + b0 + q] = (uint8_t)(vo >> (8 * q));
      a.ring_next[rowb + b0 + q] = (uint8_t)(vn >> (8 * q));
    }
  }
}

struct SampArgs {
  int B, n, K, D;
  const uint8_t* ring_obs;
  const uint8_t* ring_next;
  const int32_t* ring_actions;
  const float* ring_rewards;
  const uint8_t* ring_dones;
  uint64_t seed;
  const uint64_t* ctrl;
  uint8_t* obs;
  uint8_t* next_obs;
  int32_t* actions;
  float* rewards;
  uint8_t* dones;
  int32_t* indices;
};

__global__ __launch_bounds__(kThreads) void pe_replay_sample_kernel(SampArgs a) {
  __shared__ int64_t src[kSampRows];  // slot * n + env of the tile's samples, -1: nothing stored
  const int tid = (int)threadIdx.x;
  const int j0 = (int)blockIdx.x * kSampRows;
  const int rows = min(kSampRows, a.B - j0);
  if (tid < rows) {
    const uint64_t steps = a.ctrl[kReplayCtrlSteps], draws = a.ctrl[kReplayCtrlDraws];
    const uint32_t filled = (uint32_t)(steps < (uint64_t)a.K ? steps : (uint64_t)a.K);
    const int j = j0 + tid;
    int32_t slot = -1, env = -1;
    int64_t s = -1;
    int32_t act = 0;
    float rew = 0.0f;
    uint8_t dn = 0;
    if (filled != 0) {
      replay_sample_index(a.seed, draws, (uint32_t)j, filled, (uint32_t)a.n, &slot, &env);
      s = (int64_t)slot * a.n + env;
      act = a.ring_actions[s];
      rew = a.ring_rewards[s];
      dn = a.ring_dones[s];
    }
    src[tid] = s;
    a.indices[2 * j] = slot;
    a.indices[2 * j + 1] = env;
    a.actions[j] = act;
    a.rewards[j] = rew;
    a.dones[j] = dn;
  }
  __syncthreads();
  const int cnt = rows * a.D;                 // the tile's bytes of each plane
  const int64_t ob = (int64_t)j0 * a.D;       // a multiple of 16: j0 is
  const int64_t plane = (int64_t)a.K * a.n * a.D;  // bytes of an obs plane
  for (int b = tid * 4; b < cnt; b += kThreads * 4) {
    const int k = min(4, cnt - b);
    int r = b / a.D, c = b - r * a.D;
    uint32_t vo = 0, vn = 0;
    const int64_t s0 = src[r];
    const int64_t off0 = s0 * a.D + c;
    const int64_t al = off0 & ~(int64_t)3;
    const int sh = (int)(off0 & 3);
    if (k == 4 && c + 4 <= a.D && s0 >= 0 && (sh == 0 || al + 8 <= plane)) {
      // the 4 bytes lie in one sampled row: the aligned dword(s) around them, shifted into place
      const uint32_t lo_o = *reinterpret_cast<const uint32_t*>(a.ring_obs + al);
      const uint32_t lo_n = *reinterpret_cast<const uint32_t*>(a.ring_next + al);
      if (sh == 0) {
        vo = lo_o;
        vn = lo_n;
      } else {
        const uint32_t hi_o = *reinterpret_cast<const uint32_t*>(a.ring_obs + al + 4);
        const uint32_t hi_n = *reinterpret_cast<const uint32_t*>(a.ring_next + al + 4);
        vo = (uint32_t)((((uint64_t)hi_o << 32) | lo_o) >> (8 * sh));
        vn = (uint32_t)((((uint64_t)hi_n << 32) | lo_n) >> (8 * sh));
      }
    } else {
      for (int q = 0; q < k; ++q) {
        const int64_t s = src[r];
        if (s >= 0) {
          const int64_t off = s * a.D + c;
          vo |= (uint32_t)a.ring_obs[off] << (8 * q);
          vn |= (uint32_t)a.ring_next[off] << (8 * q);
        }
        if (++c == a.D) {
          c = 0;
          ++r;  // read again only while b + q + 1 < cnt, i.e. r < rows
        }
      }
    }
    if (k == 4) {
      *reinterpret_cast<uint32_t*>(a.obs + ob + b) = vo;
      *reinterpret_cast<uint32_t*>(a.next_obs + ob + b) = vn;
    } else {
      for (int q = 0; q < k; ++q) {
        a.obs[ob + b + q] = (uint8_t)(vo >> (8 * q));
        a.next_obs[ob + b + q] = (uint8_t)(vn >> (8 * q));
      }
    }
  }
}

struct TgtArgs {
  int B, A;
  const float* q;
  const float* rewards;
  const uint8_t* dones;
  float g;
  float* targets;
};

__global__ __launch_bounds__(kThreads) void pe_replay_target_kernel(TgtArgs a) {
  const int j = (int)(blockIdx.x * kThreads + threadIdx.x);
  if (j >= a.B) return;
  float q[8];
  const float* src = a.q + (size_t)j * a.A;
#pragma unroll
  for (int k = 0; k < 8; ++k) q[k] = k < a.A ? src[k] : 0.0f;
  const float r = a.rewards[j];
  const uint8_t d = a.dones[j];
  float t;
  switch (a.A) {  // a constant A unrolls the loop over q: it stays in registers
    case 2: t = replay_target(q, 2, r, d, a.g); break;
    case 3: t = replay_target(q, 3, r, d, a.g); break;
    case 4: t = replay_target(q, 4, r, d, a.g); break;
    case 5: t = replay_target(q, 5, r, d, a.g); break;
    case 6: t = replay_target(q, 6, r, d, a.g); break;
    case 7: t = replay_target(q, 7, r, d, a.g); break;
    default: t = replay_target(q, 8, r, d, a.g); break;
  }
  a.targets[j] = t;
}

int launch_fail(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return PE_OK;
  return pe_internal_set_error(PE_ERR_DEVICE, (std::string(what) + ": " + hipGetErrorString(e)).c_str());
}

unsigned blocks_of(int64_t threads) { return (unsigned)((threads + kThreads - 1) / kThreads); }

}  // namespace

extern "C" {

int pe_replay_select(int32_t n, int32_t A, const int32_t* greedy, const float* eps, const uint64_t* ctrl,
                     uint64_t seed, uint32_t env_id_offset, int32_t* actions, uint8_t* explored, void* stream) {
  if (const int rc = pe_internal_replay_select_check(n, A, greedy, actions)) return rc;
  if (!eps || !ctrl) return pe_internal_set_error(PE_ERR_ARG, "replay select: null eps / ctrl");
  (void)hipGetLastError();
  const SelArgs a{n, A, greedy, eps, ctrl, seed, env_id_offset, actions, explored};
  hipLaunchKernelGGL(pe_replay_select_kernel, dim3(blocks_of(n)), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
  return launch_fail("pe_replay_select");
}

int pe_replay_store(int32_t n, int32_t K, int32_t grid_size, int32_t lidar_range, int32_t lidar_channels,
                    const uint8_t* obs, const int32_t* actions, const uint8_t* next_obs, const float* reward,
                    const uint8_t* terminated, const uint8_t* truncated, const float* terminal_obs,
                    const double* episode_return, const int32_t* episode_length, uint8_t* ring_obs,
                    uint8_t* ring_next_obs, int32_t* ring_actions, float* ring_rewards, uint8_t* ring_dones,
                    int32_t* ep_count, double* ep_return_sum, int32_t* ep_length_sum, uint64_t* ctrl, void* stream) {
  if (const int rc = pe_internal_replay_store_check(n, K, grid_size, lidar_range, lidar_channels, obs, actions, next_obs,
                                                    reward, terminated, truncated, terminal_obs, ring_obs, ring_next_obs,
                                                    ring_actions, ring_rewards, ring_dones, ctrl))
    return rc;
  (void)hipGetLastError();
  StoreArgs a;
  a.n = n;
  a.K = K;
  a.C5 = 5 * lidar_channels;
  a.D = a.C5 + 27;
  a.R = lidar_range;
  a.G = grid_size;
  a.obs = obs;
  a.actions = actions;
  a.next_obs = next_obs;
  a.reward = reward;
  a.terminated = terminated;
  a.truncated = truncated;
  a.terminal_obs = terminal_obs;
  a.episode_return = episode_return;
  a.episode_length = episode_length;
  a.ring_obs = ring_obs;
  a.ring_next = ring_next_obs;
  a.ring_actions = ring_actions;
  a.ring_rewards = ring_rewards;
  a.ring_dones = ring_dones;
  a.ep_count = ep_count;
  a.ep_return_sum = ep_return_sum;
  a.ep_length_sum = ep_length_sum;
  a.ctrl = ctrl;
  const int64_t quads = ((int64_t)n * a.D + 3) / 4;  // >= n: D >= 32
  hipLaunchKernelGGL(pe_replay_store_kernel, dim3(blocks_of(quads)), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                     a);
  if (const int rc = launch_fail("pe_replay_store")) return rc;
  hipLaunchKernelGGL(pe_replay_advance_kernel, dim3(1), dim3(1), 0, static_cast<hipStream_t>(stream), ctrl,
                     (int)kReplayCtrlSteps);
  return launch_fail("pe_replay_store (advance)");
}

int pe_replay_sample(int32_t B, int32_t n, int32_t K, int32_t D, const uint8_t* ring_obs,
                     const uint8_t* ring_next_obs, const int32_t* ring_actions, const float* ring_rewards,
                     const uint8_t* ring_dones, uint64_t seed, uint64_t* ctrl, uint8_t* obs, uint8_t* next_obs,
                     int32_t* actions, float* rewards, uint8_t* dones, int32_t* indices, void* stream) {
  if (const int rc = pe_internal_replay_sample_check(B, n, K, D, ring_obs, ring_next_obs, ring_actions, ring_rewards,
                                                     ring_dones, ctrl, obs, next_obs, actions, rewards, dones, indices))
    return rc;
  (void)hipGetLastError();
  const SampArgs a{B, n, K, D, ring_obs, ring_next_obs, ring_actions, ring_rewards, ring_dones, seed, ctrl,
                   obs, next_obs, actions, rewards, dones, indices};
  hipLaunchKernelGGL(pe_replay_sample_kernel, dim3((unsigned)((B + kSampRows - 1) / kSampRows)), dim3(kThreads), 0,
                     static_cast<hipStream_t>(stream), a);
  if (const int rc = launch_fail("pe_replay_sample")) return rc;
  hipLaunchKernelGGL(pe_replay_advance_kernel, dim3(1), dim3(1), 0, static_cast<hipStream_t>(stream), ctrl,
                     (int)kReplayCtrlDraws);
  return launch_fail("pe_replay_sample (advance)");
}

int pe_replay_target(int32_t B, int32_t A, const float* q_next, const float* rewards, const uint8_t* dones,
                     double gamma, float* targets, void* stream) {
  if (const int rc = pe_internal_replay_target_check(B, A, q_next, rewards, dones, targets)) return rc;
  (void)hipGetLastError();
  const TgtArgs a{B, A, q_next, rewards, dones, (float)gamma, targets};
  hipLaunchKernelGGL(pe_replay_target_kernel, dim3(blocks_of(B)), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
  return launch_fail("pe_replay_target");
}

}  // extern "C"
