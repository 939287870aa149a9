// pe_mcts.hip -- batched MCTS search on MI355X (gfx950): one MCTS.search of the
// reference (mcts_custom_trainer.py:72-243) per env, all envs at once.
//
// One lane owns one env's search.  The search is sequential inside an env (every
// simulation reads the statistics the previous ones wrote), so the parallelism is
// across envs; everything a lane touches is its own:
//   cellw  u32 [N][G*G]        the sim env (_copy_env_state, :221-243): exact visit
//                              count (bits 0-28) | cell code << 29 | explored << 31
//   ulog   uint2 [N][D+4]      undo log of the current simulation: (cell, old word);
//                              replayed backwards instead of re-copying the state
//                              per simulation (a simulation touches <= D+2 cells)
//   nodes  MNode [N][S+1]      the tree: MCTSNode (:20-33) records, 32 B
//   rng    u32 [N][628]        the env's np.random stream (persistent across searches)
// The clone kernel rebuilds cellw from the live batch state (one thread per cell,
// coalesced) before every search; the search kernel reads nothing else of it.
// pe_mcts_plan.hpp chooses the search kernel and lays these arrays out (with the LDS
// kernel's cellb / csim / csg in place of ulog); the code is in pe_mcts_rng.hpp (the
// stream), pe_mcts_cells.hpp (the sim env, the clone kernel) and pe_mcts_search.hpp
// (the tree, the search kernels); this file is the handle and the C API.
//
// np.random stream (numpy legacy RandomState = MT19937).  Device form of a stream at
// position p: words [0,p) already hold the NEXT round's words, [p,624) this round's;
// the next output is temper(mt[p]).  A draw regenerates its own word (the twist done
// one word at a time, which is order-equivalent to numpy's block twist), so no lane
// ever stops for a 624-word twist.  Draws are generated ahead into a per-lane LDS ring
// (wave-uniform top-ups, all loads of a top-up in flight together); the unconsumed
// tail is rewound at the end, so the stream stops exactly at its first unconsumed draw.
// mt[625] keeps this round's mt[0] (overwritten at position 0) so the host can give
// the state back in numpy's own terms (pe_mcts_get_rng).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/plantos_batch.h"
#include "pe_device.hpp"
#include "pe_handle.hpp"
#include "pe_host.hpp"
#include "pe_mcts_plan.hpp"
#include "pe_mcts_rng.hpp"
#include "pe_mcts_cells.hpp"
#include "pe_mcts_search.hpp"

using namespace pe;

struct pe_mcts {
  pe_handle* h;
  int device;     // h->device, kept so that pe_mcts_destroy needs nothing of a handle destroyed before it
  MctsPlan plan;  // the kernel, its grids and LDS, the layout of mem
  void* mem;
  MctsArgs args;  // what create decides of a search's argument: the arrays, the strides, the budget
};

namespace {

#define MC_HIP(call)                                   \
  do {                                                 \
    hipError_t _e = (call);                            \
    if (_e != hipSuccess) return hip_fail(_e, #call);  \
  } while (0)

// np.random.seed(seeds[e]) for env e (HOST array of n, or null: base_seed + e) on stream s:
// the seed kernel's one launch site.  `what` names the API call in a launch error.
int seed_streams(pe_mcts* m, const uint32_t* seeds, uint32_t base_seed, hipStream_t s, const char* what) {
  const int n = m->h->n;
  uint32_t* dseeds = nullptr;
  if (seeds) {
    MC_HIP(hipMalloc(&dseeds, (size_t)n * 4));
    hipError_t e = hipMemcpy(dseeds, seeds, (size_t)n * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      (void)hipFree(dseeds);
      return hip_fail(e, "hipMemcpy");
    }
  }
  hipLaunchKernelGGL(pe_mcts_seed_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, m->args.rng, n, dseeds,
                     base_seed);
  hipError_t e = hipGetLastError();
  if (dseeds) {
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(dseeds);
  }
  return e == hipSuccess ? PE_OK : hip_fail(e, what);
}

// pe_mcts_set_rng's check of one numpy position
int check_pos(int32_t pos) { return pos < 0 || pos > kMtN ? fail(PE_ERR_ARG, "pos must be in [0, 624]") : PE_OK; }

}  // namespace

extern "C" {

int pe_internal_mcts_plan(int32_t G, int32_t n_envs, int32_t n_simulations, int32_t max_depth,
                          pe_mcts_plan_info* out) {
  if (!out) return fail(PE_ERR_ARG, "null argument");
  MctsPlan p;
  if (const int rc = make_mcts_plan(G, n_envs, n_simulations, max_depth, &p)) return rc;
  out->kernel = p.use_lds ? 1 : 0;
  out->ldsp = p.ldsp;
  out->ggp = p.ggp;
  out->lds_bytes = p.lds;
  out->clone_blocks = p.clone_blocks;
  out->search_blocks = p.search_blocks;
  for (int i = 0; i < kMctsArrays; ++i) {
    out->offset[i] = p.off[i];
    out->size[i] = p.size[i];
  }
  out->total = p.total;
  return PE_OK;
}

int pe_internal_mcts_rng_to_device_host(const uint32_t* key, int32_t pos, uint32_t* dev) {
  if (!key || !dev) return fail(PE_ERR_ARG, "null argument");
  if (const int rc = check_pos(pos)) return rc;
  np_to_device(key, pos, dev);
  return PE_OK;
}

int pe_internal_mcts_rng_from_device_host(const uint32_t* dev, uint32_t* key, int32_t* pos) {
  if (!dev || !key || !pos) return fail(PE_ERR_ARG, "null argument");
  if (dev[kMtN] >= (uint32_t)kMtN) return fail(PE_ERR_ARG, "device-form position must be in [0, 623]");
  device_to_np(dev, key, pos);
  return PE_OK;
}

int pe_mcts_kernel_name(pe_mcts* m, const char** name) {
  if (!m || !name) return fail(PE_ERR_ARG, "null argument");
  *name = m->plan.use_lds ? "pe_mcts_search_lds_kernel" : "pe_mcts_search_kernel";
  return PE_OK;
}

int pe_mcts_create(pe_handle* h, int32_t n_simulations, double c_param, int32_t max_depth, pe_mcts** out) {
  if (!h || !out) return fail(PE_ERR_ARG, "null argument");
  *out = nullptr;
  MctsPlan plan;
  if (const int rc = make_mcts_plan(h->g.G, h->n, n_simulations, max_depth, &plan)) return rc;
  DeviceGuard dg(h->device);
  if (dg.rc) return dg.rc;
  pe_mcts* m = new (std::nothrow) pe_mcts();
  if (!m) return fail(PE_ERR_NOMEM, "host allocation failed");
  hipError_t e = hipMalloc(&m->mem, plan.total);
  if (e != hipSuccess) {
    delete m;
    return fail(PE_ERR_NOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
  }
  m->h = h;
  m->device = h->device;
  m->plan = plan;
  // an array of size 0 is one the plan's kernel does not read: null
  auto at = [&](int i) -> void* { return plan.size[i] ? static_cast<char*>(m->mem) + plan.off[i] : nullptr; };
  MctsArgs& a = m->args;
  a.cellw = static_cast<uint32_t*>(at(kCellw));
  a.ulog = static_cast<uint2*>(at(kUlog));
  a.nodes = static_cast<MNode*>(at(kNodes));
  a.rng = static_cast<uint32_t*>(at(kRng));
  a.logt = static_cast<const double*>(at(kLogt));
  a.cellb = static_cast<uint8_t*>(at(kCellb));
  a.csim = static_cast<uint32_t*>(at(kCsim));
  a.csg = static_cast<uint32_t*>(at(kCsg));
  if (plan.use_lds) {
    a.ggp = plan.ggp;
    a.ldsp = plan.ldsp;
  }
  a.n_sims = n_simulations;
  a.max_depth = max_depth;
  a.c = c_param;
  std::vector<double> lt((size_t)n_simulations + 1);
  lt[0] = -INFINITY;
  for (int k = 1; k <= n_simulations; ++k) lt[k] = std::log((double)k);  // math.log(self.visits) (:56)
  int rc = PE_OK;
  e = hipMemcpy(at(kLogt), lt.data(), lt.size() * 8, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    rc = seed_streams(m, nullptr, 0u, 0, "pe_mcts_create");  // np.random.seed(e) until pe_mcts_seed
    if (rc == PE_OK) e = hipDeviceSynchronize();
  }
  if (e != hipSuccess) rc = hip_fail(e, "pe_mcts_create");
  if (rc != PE_OK) {
    (void)hipFree(m->mem);
    delete m;
    return rc;
  }
  *out = m;
  return PE_OK;
}

int pe_mcts_destroy(pe_mcts* m) {
  if (!m) return PE_OK;
  DeviceGuard dg(m->device);  // not m->h->device: the env handle may be gone already
  hipError_t e = hipFree(m->mem);
  delete m;
  return e == hipSuccess ? PE_OK : hip_fail(e, "hipFree");
}

int pe_mcts_seed(pe_mcts* m, const uint32_t* seeds, uint32_t base_seed, void* stream) {
  if (!m) return fail(PE_ERR_ARG, "null handle");
  DeviceGuard dg(m->h->device);
  if (dg.rc) return dg.rc;
  return seed_streams(m, seeds, base_seed, static_cast<hipStream_t>(stream), "pe_mcts_seed");
}

int pe_mcts_set_rng(pe_mcts* m, const uint32_t* key, const int32_t* pos) {
  if (!m || !key || !pos) return fail(PE_ERR_ARG, "null argument");
  const int n = m->h->n;
  std::vector<uint32_t> dev((size_t)n * kRngStride);
  for (int e = 0; e < n; ++e) {
    if (const int rc = check_pos(pos[e])) return rc;
    np_to_device(key + (size_t)e * kMtN, pos[e], dev.data() + (size_t)e * kRngStride);
  }
  DeviceGuard dg(m->h->device);
  if (dg.rc) return dg.rc;
  MC_HIP(hipDeviceSynchronize());
  MC_HIP(hipMemcpy(m->args.rng, dev.data(), dev.size() * 4, hipMemcpyHostToDevice));
  return PE_OK;
}

int pe_mcts_get_rng(pe_mcts* m, uint32_t* key, int32_t* pos) {
  if (!m || !key || !pos) return fail(PE_ERR_ARG, "null argument");
  const int n = m->h->n;
  std::vector<uint32_t> dev((size_t)n * kRngStride);
  DeviceGuard dg(m->h->device);
  if (dg.rc) return dg.rc;
  MC_HIP(hipDeviceSynchronize());
  MC_HIP(hipMemcpy(dev.data(), m->args.rng, dev.size() * 4, hipMemcpyDeviceToHost));
  for (int e = 0; e < n; ++e) device_to_np(dev.data() + (size_t)e * kRngStride, key + (size_t)e * kMtN, pos + e);
  return PE_OK;
}

int pe_mcts_search(pe_mcts* m, const uint8_t* mask, int32_t* actions, int32_t* root_order, int32_t* root_visits,
                   double* root_value, void* stream) {
  if (!m || !actions) return fail(PE_ERR_ARG, "null argument");
  pe_handle* h = m->h;
  DeviceGuard dg(h->device);
  if (dg.rc) return dg.rc;
  MctsArgs a = m->args;
  a.st = h->st;
  a.g = h->g;
  a.rl = h->rl;
  a.n = h->n;
  a.mask = mask;
  a.actions = actions;
  a.rorder = root_order;
  a.rvisits = root_visits;
  a.rvalue = root_value;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const MctsPlan& p = m->plan;
  if (p.clone_blocks > 0) {
    // the steps' deferred visit-overflow writes first: the clone reads the exact counts
    if (const int fr = pe_internal_flush_vx(h, s)) return fr;
    hipLaunchKernelGGL(pe_mcts_clone_kernel, dim3(p.clone_blocks), dim3(256), 0, s, a);
    if (p.use_lds)
      hipLaunchKernelGGL(pe_mcts_search_lds_kernel, dim3(p.search_blocks), dim3(64), p.lds, s, a);
    else
      hipLaunchKernelGGL(pe_mcts_search_kernel, dim3(p.search_blocks), dim3(64), 0, s, a);
  }
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? PE_OK : hip_fail(e, "pe_mcts_search");
}

#ifdef PE_MCTS_PROF
int pe_mcts_debug_prof(uint64_t* host, int64_t count) {
  if (count > (int64_t)(1 << 20) * 4) count = (int64_t)(1 << 20) * 4;
  hipError_t e = hipMemcpyFromSymbol(host, HIP_SYMBOL(g_mcts_prof), (size_t)count * 8);
  return e == hipSuccess ? PE_OK : hip_fail(e, "hipMemcpyFromSymbol");
}
#endif

}  // extern "C"
