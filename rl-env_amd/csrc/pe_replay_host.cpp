// pe_replay_host.cpp -- the host twins of pe_replay_select, pe_replay_sample's index draw and
// pe_replay_target (include/plantos_batch.h, "Replay collection"): the definitions executed
// literally on host arrays with the functions of pe_replay_math.hpp, which the kernels
// (pe_replay.hip) include too; and the argument rules both sides share.  Plain C++: no
// handle, no device.
#include <string>

#include "../../include/plantos_batch.h"
#include "pe_replay_math.hpp"

extern "C" int pe_internal_set_error(int code, const char* msg);

namespace {
int fail(const std::string& m) { return pe_internal_set_error(PE_ERR_ARG, m.c_str()); }
bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }
}  // namespace

extern "C" int pe_internal_replay_select_check(int32_t n, int32_t A, const void* greedy, const void* actions) {
  if (n < 1) return fail("replay select: n must be >= 1, got " + std::to_string(n));
  if (A < 2 || A > 8) return fail("replay select: A must be in 2..8, got " + std::to_string(A));
  if (!greedy || !actions) return fail("replay select: null greedy / actions");
  return PE_OK;
}

extern "C" int pe_internal_replay_store_check(int32_t n, int32_t K, int32_t G, int32_t R, int32_t C, const void* obs,
                                              const void* actions, const void* next_obs, const void* reward,
                                              const void* terminated, const void* truncated, const void* terminal_obs,
                                              const void* ring_obs, const void* ring_next_obs, const void* ring_actions,
                                              const void* ring_rewards, const void* ring_dones, const void* ctrl) {
  if (n < 1 || K < 1) return fail("replay store: n and K must be >= 1");
  if (G < 1 || G > 128 || R < 1 || R > 64 || C < 1 || 5 * (int64_t)C + 27 > 4096)
    return fail("replay store: grid_size 1..128, lidar_range 1..64, 5 * lidar_channels + 27 <= 4096");
  if (!obs || !actions || !next_obs || !reward || !terminated || !truncated || !terminal_obs)
    return fail("replay store: null step input");
  if (!ring_obs || !ring_next_obs || !ring_actions || !ring_rewards || !ring_dones || !ctrl)
    return fail("replay store: null ring plane / ctrl");
  if (!aligned4(obs) || !aligned4(next_obs) || !aligned4(ring_obs) || !aligned4(ring_next_obs))
    return fail("replay store: obs / next_obs and the ring's obs planes must be 4-byte aligned");
  return PE_OK;
}

extern "C" int pe_internal_replay_sample_check(int32_t B, int32_t n, int32_t K, int32_t D, const void* ring_obs,
                                               const void* ring_next_obs, const void* ring_actions,
                                               const void* ring_rewards, const void* ring_dones, const void* ctrl,
                                               const void* obs, const void* next_obs, const void* actions,
                                               const void* rewards, const void* dones, const void* indices) {
  if (B < 1 || n < 1 || K < 1) return fail("replay sample: B, n and K must be >= 1");
  if (D < 1 || D > 4096) return fail("replay sample: D must be in 1..4096, got " + std::to_string(D));
  if (!ring_obs || !ring_next_obs || !ring_actions || !ring_rewards || !ring_dones || !ctrl)
    return fail("replay sample: null ring plane / ctrl");
  if (!obs || !next_obs || !actions || !rewards || !dones || !indices) return fail("replay sample: null output");
  if (!aligned4(obs) || !aligned4(next_obs) || !aligned4(ring_obs) || !aligned4(ring_next_obs))
    return fail("replay sample: the obs / next_obs outputs and the ring's obs planes must be 4-byte aligned");
  return PE_OK;
}

extern "C" int pe_internal_replay_target_check(int32_t B, int32_t A, const void* q_next, const void* rewards,
                                               const void* dones, const void* targets) {
  if (B < 1) return fail("replay target: B must be >= 1, got " + std::to_string(B));
  if (A < 2 || A > 8) return fail("replay target: A must be in 2..8, got " + std::to_string(A));
  if (!q_next || !rewards || !dones || !targets) return fail("replay target: null argument");
  return PE_OK;
}

using namespace pe_pol;

extern "C" {

int pe_replay_select_host(int32_t n, int32_t A, const int32_t* greedy, float eps, uint64_t steps, uint64_t seed,
                          uint32_t env_id_offset, int32_t* actions, uint8_t* explored) {
  if (const int rc = pe_internal_replay_select_check(n, A, greedy, actions)) return rc;
  for (int e = 0; e < n; ++e)
    actions[e] = replay_select(seed, steps, env_id_offset + (uint32_t)e, A, eps, greedy[e], explored ? explored + e : nullptr);
  return PE_OK;
}

int pe_replay_sample_indices_host(int32_t B, int32_t n, int32_t K, uint64_t steps, uint64_t draws, uint64_t seed,
                                  int32_t* indices) {
  if (B < 1 || n < 1 || K < 1) return fail("replay sample: B, n and K must be >= 1");
  if (!indices) return fail("replay sample: null output");
  const uint32_t filled = (uint32_t)(steps < (uint64_t)K ? steps : (uint64_t)K);
  for (int j = 0; j < B; ++j) {
    if (filled == 0)
      indices[2 * j] = indices[2 * j + 1] = -1;
    else
      replay_sample_index(seed, draws, (uint32_t)j, filled, (uint32_t)n, indices + 2 * j, indices + 2 * j + 1);
  }
  return PE_OK;
}

int pe_replay_target_host(int32_t B, int32_t A, const float* q_next, const float* rewards, const uint8_t* dones,
                          double gamma, float* targets) {
  if (const int rc = pe_internal_replay_target_check(B, A, q_next, rewards, dones, targets)) return rc;
  const float g = (float)gamma;
  for (int j = 0; j < B; ++j) targets[j] = replay_target(q_next + (size_t)j * A, A, rewards[j], dones[j], g);
  return PE_OK;
}

}  // extern "C"
