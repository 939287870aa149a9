// pe_mcts_plan.hpp -- the device-free half of pe_mcts_create (pe_mcts.hip).
//
// make_mcts_plan() decides everything pe_mcts_create decides before its allocation -- the
// argument checks, the search kernel, its LDS and grid sizes and the layout of the handle's one
// device allocation -- as a pure function of (G, n envs, n_simulations, max_depth).  It makes no
// HIP call and includes no HIP header, so the choice can be examined without a GPU
// (pe_internal_mcts_plan, tests/test_mcts_plan_host.py).  pe_mcts keeps the plan:
// pe_mcts_kernel_name and pe_mcts_search read it and decide nothing again.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/plantos_batch.h"

extern "C" int pe_internal_set_error(int code, const char* msg);

namespace pe_mc {

// what the rule below shares with the kernels (pe_mcts_rng.hpp, pe_mcts_search.hpp)
constexpr int kRing = 32;        // buffered draws per lane (LDS ring)
constexpr int kRngStride = 628;  // mt[624], pos, saved mt[0], 2 pad (16-B rows)
constexpr int kNodeBytes = 32;   // sizeof(MNode)
constexpr size_t kMctsLdsMax = 64 * 1024;  // >= 2 workgroups per CU

// The arrays of a handle, in the order of the allocation.  Per env unless noted.
enum MctsArray : int {
  kCellw,  // u32 [G*G]           the clone: exact visit count | code | explored (both kernels)
  kUlog,   // uint2 [max_depth+4] undo log of a simulation (global kernel)
  kNodes,  // MNode [n_sims+1]    the tree
  kRng,    // u32 [kRngStride]    the np.random stream
  kLogt,   // f64 [n_sims+1]      log(k), once per handle
  kCellb,  // u8 [ggp]            the clone as LDS bytes (LDS kernel)
  kCsim,   // u32 [G*G]           exact counts of bumped saturated cells (LDS kernel)
  kCsg,    // u32 [G*G]           their stamps (LDS kernel)
  kMctsArrays
};

struct MctsPlan {
  bool use_lds;      // pe_mcts_search_lds_kernel; else pe_mcts_search_kernel
  int ldsp;          // LDS bytes of one lane's cells
  size_t lds;        // dynamic LDS bytes of a workgroup of the LDS kernel
  int ggp;           // global per-env byte stride of the clone bytes (G*G rounded up to 16)
  unsigned clone_blocks, search_blocks;  // grids: 256 cells, 64 envs per workgroup
  size_t off[kMctsArrays], size[kMctsArrays];  // 256-B aligned; size 0: the kernel reads no such array
  size_t total;
};

// Which search kernel a handle of grid side G runs.  The LDS kernel needs, per workgroup of 64
// lanes, each lane's cell bytes (G*G rounded up to whole dwords, one more dword when that count
// is even: odd dword stride between lanes) and its draw ring; it runs when G <= 64 and that fits
// kMctsLdsMax, else cells stay in global memory.  A handle allocates only its own kernel's arrays.
// PE_OK, or pe_mcts_create's error with pe_last_error() set.
inline int make_mcts_plan(int G, int n_envs, int32_t n_simulations, int32_t max_depth, MctsPlan* out) {
  if (n_simulations < 0 || n_simulations > 65534)
    return pe_internal_set_error(PE_ERR_ARG, "n_simulations must be in [0, 65534]");
  if (max_depth < 0 || max_depth > (1 << 20)) return pe_internal_set_error(PE_ERR_ARG, "max_depth must be in [0, 2^20]");
  if (G < 1 || n_envs < 0) return pe_internal_set_error(PE_ERR_ARG, "bad grid size or env count");
  MctsPlan p{};
  const size_t n = (size_t)n_envs, GG = (size_t)G * (size_t)G;
  p.ldsp = (int)((GG + 3) / 4 * 4);
  if ((p.ldsp / 4) % 2 == 0) p.ldsp += 4;  // odd dword stride between lanes
  p.lds = 64 * ((size_t)p.ldsp + 4 * (size_t)kRing);
  p.use_lds = G <= 64 && p.lds <= kMctsLdsMax;
  p.ggp = (int)((GG + 15) / 16 * 16);
  p.clone_blocks = (unsigned)((n * GG + 255) / 256);
  p.search_blocks = (unsigned)((n + 63) / 64);
  const size_t lds_only = p.use_lds ? 1 : 0;
  const size_t bytes[kMctsArrays] = {
      n * GG * 4,
      (1 - lds_only) * n * (size_t)(max_depth + 4) * 8,
      n * (size_t)(n_simulations + 1) * kNodeBytes,
      n * kRngStride * 4,
      (size_t)(n_simulations + 1) * 8,
      lds_only * n * (size_t)p.ggp,
      lds_only * n * GG * 4,
      lds_only * n * GG * 4,
  };
  for (int i = 0; i < kMctsArrays; ++i) {
    p.off[i] = p.total;
    p.size[i] = (bytes[i] + 255) / 256 * 256;
    p.total += p.size[i];
  }
  *out = p;
  return PE_OK;
}

}  // namespace pe_mc
