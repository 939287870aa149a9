// plantos_batch.hip -- MI355X (gfx950) batched PlantOSEnv step/reset + C-ABI.
//
// One lane owns one env (no cross-env writes, so no atomics on state).  The fused
// step kernel does, per env: action decode, move/collide or water, visit/explored
// update, f64 reward (cast once), terminated/truncated, optional auto-reset, LIDAR
// ray-march, position, 5x5 visit slice; each lane assembles its obs row in LDS and
// the workgroup streams the contiguous [BLOCK x D] obs tile to HBM with 16-byte
// stores.  C-ABI: include/plantos_batch.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "../../include/plantos_batch.h"
#include "lidar_tables.inc"
#include "pe_device.hpp"
#include "pe_fast.hpp"
#include "pe_coop.hpp"
#include "pe_quad.hpp"

using namespace pe;

namespace {

#include "pe_step_args.hpp"      // StepArgs, kBlock, kTabFloats
#include "pe_obs.hpp"            // build_obs_*, load_tables*
#include "pe_tile.hpp"           // store_tile*, the write-through 16-B store
#include "pe_step_fast.hpp"      // pe_step_fast<C, R, ONEWORD>
#include "pe_stamps.hpp"         // PE_STAMP* (diagnostic builds only)
#include "pe_quad_done.hpp"      // the sector kernels' LDS layout and auto-reset slow path
#include "pe_step_quad.hpp"      // pe_step_quad<C, R, ...>
#include "pe_far.hpp"  // pe_step_far<C, R>: the sector kernel of long LIDAR ranges (R > 14)
#include "pe_step_wave.hpp"      // pe_step_wave<MAXW, ALN>, wave_done
#include "pe_reset_kernels.hpp"  // reset, prefetch, load-maps kernels
#include "pe_state_kernels.hpp"  // info / get / set / flush / synth kernels

}  // namespace

#include "pe_expand_codes.hpp"  // pe_expand_codes_kernel (external linkage)

// ====================================================================== host side
#include "pe_host.hpp"  // fail / hip_fail / DeviceGuard

namespace {

thread_local std::string g_err;

#define PE_HIP(call)                                   \
  do {                                                 \
    hipError_t _e = (call);                            \
    if (_e != hipSuccess) return hip_fail(_e, #call);  \
  } while (0)

StepArgs base_args(const pe_handle* h) {
  StepArgs a;
  std::memset(&a, 0, sizeof(a));
  a.st = h->st;
  a.g = h->g;
  a.rl = h->rl;
  a.n = h->n;
  a.autoreset = h->cfg.autoreset;
  a.stagger = h->stagger;
  a.coop_max_done = h->coop_max_done;
  a.pf = h->pf;
  return a;
}

}  // namespace

// make_plan(): geometry, kernel selection, allocation layouts and the host tables -- no HIP call
#include "pe_plan.hpp"

namespace {

int launch_step(const pe_handle* h, const StepArgs& a, hipStream_t s) {
  const StepKernel& k = h->k;
  dim3 grid((unsigned)((h->n + k.epb - 1) / k.epb)), block(64 * k.waves);
  size_t lds = step_lds_bytes(h->g, k);
  switch (k.family) {
    case StepFamily::far:
      if (h->lds_floor > lds) lds = h->lds_floor;  // diagnostics: caps workgroups per CU
      hipLaunchKernelGGL((pe_step_far<64, 32>), grid, block, lds, s, a);
      break;
    case StepFamily::quad:
      if (h->lds_floor > lds) lds = h->lds_floor;  // diagnostics: caps workgroups per CU
      // the row of PE_QUAD_KERNELS that is the handle's kernel
#define PE_ROW(KC, KR, OW, NW, BT, EPB)                                                                      \
  else if (k.C == KC && k.R == KR && k.oneword == OW && k.waves == NW && k.bytetile == BT && k.epb == EPB)   \
    hipLaunchKernelGGL((pe_step_quad<KC, KR, OW, NW, BT, EPB>), grid, block, lds, s, a);
      if (false) {
      }
      PE_QUAD_KERNELS(PE_ROW)
      else return fail(PE_ERR_ARG, "internal: no such sector kernel");
#undef PE_ROW
      break;
    case StepFamily::fast:
      if (k.C == 16 && k.oneword)
        hipLaunchKernelGGL((pe_step_fast<16, 6, true>), grid, block, lds, s, a);
      else if (k.C == 16)
        hipLaunchKernelGGL((pe_step_fast<16, 6, false>), grid, block, lds, s, a);
      else
        hipLaunchKernelGGL((pe_step_fast<64, 6, false>), grid, block, lds, s, a);
      break;
    case StepFamily::wave: {  // pe_step_wave: one wave per env
      const bool aln = wave_aligned(h->g);
      if (h->g.WPR == 1) {
        if (aln)
          hipLaunchKernelGGL((pe_step_wave<1, true>), grid, block, lds, s, a);
        else
          hipLaunchKernelGGL((pe_step_wave<1, false>), grid, block, lds, s, a);
      } else {
        if (aln)
          hipLaunchKernelGGL((pe_step_wave<kCoopWPR, true>), grid, block, lds, s, a);
        else
          hipLaunchKernelGGL((pe_step_wave<kCoopWPR, false>), grid, block, lds, s, a);
      }
      break;
    }
  }
  PE_HIP(hipGetLastError());
  return PE_OK;
}

// The prefetch launches (pe_prefetch_kernel): queue mode on one resident grid
// (h->pf_blocks: every workgroup the chip holds at once; a steady-state batch of K
// steps' resets, ~65 K envs at 65536 envs, is about one map per wave), all mode
// with one wave per env.
int launch_prefetch(const pe_handle* h, hipStream_t s, int all) {
  StepArgs a = base_args(h);
  const unsigned nb = (unsigned)((h->n + 3) / 4);
  dim3 grid(all ? nb : std::min(nb, (unsigned)h->pf_blocks)), block(256);
  if (!all) {
    hipLaunchKernelGGL(pe_pf_compact_kernel, dim3((unsigned)((h->n + 255) / 256)), dim3(256), 0, s, h->pf, h->n);
    PE_HIP(hipGetLastError());
  }
  const size_t lds = coop_lds_bytes(h->g);
  if (h->g.WPR == 1) {
    if (h->k.bytetile)
      hipLaunchKernelGGL((pe_prefetch_kernel<1, true>), grid, block, lds, s, a, all);
    else
      hipLaunchKernelGGL((pe_prefetch_kernel<1, false>), grid, block, lds, s, a, all);
  } else {
    if (h->k.bytetile)
      hipLaunchKernelGGL((pe_prefetch_kernel<kCoopWPR, true>), grid, block, lds, s, a, all);
    else
      hipLaunchKernelGGL((pe_prefetch_kernel<kCoopWPR, false>), grid, block, lds, s, a, all);
  }
  PE_HIP(hipGetLastError());
  return PE_OK;
}

int launch_reset(const pe_handle* h, const StepArgs& a, hipStream_t s) {
  if (h->coop_max_done > 0) {  // the cooperative reset applies (pe_coop.hpp coop_reset_ok)
    dim3 cgrid((unsigned)((h->n + 3) / 4)), cblock(256);
    const size_t clds = coop_lds_bytes(h->g);
    if (h->g.WPR == 1)
      hipLaunchKernelGGL(pe_reset_coop_kernel<1>, cgrid, cblock, clds, s, a);
    else
      hipLaunchKernelGGL(pe_reset_coop_kernel<kCoopWPR>, cgrid, cblock, clds, s, a);
    PE_HIP(hipGetLastError());
    return PE_OK;
  }
  dim3 grid((unsigned)((h->n + kBlock - 1) / kBlock)), block(kBlock);
  size_t lds = lds_bytes(h->g);
  hipLaunchKernelGGL(pe_reset_kernel, grid, block, lds, s, a);
  PE_HIP(hipGetLastError());
  return PE_OK;
}

// Everything a handle owns, freed, with its device bound by the caller: pe_destroy, and the
// owner of a handle that pe_create does not finish.
int free_handle(pe_handle* h) {
  int rc = PE_OK;
  if (h->mem) {
    hipError_t e = hipFree(h->mem);
    if (e != hipSuccess) rc = hip_fail(e, "hipFree");
  }
  if (h->cur_mem) (void)hipFree(h->cur_mem);
  if (h->pf_mem) (void)hipFree(h->pf_mem);
  pe_internal_render_free(h);
  delete h;
  return rc;
}
struct HandleDeleter {
  void operator()(pe_handle* h) const { (void)free_handle(h); }
};

// make_plan() with this build's knobs; a rejection recorded for pe_last_error()
int plan_for(const pe_config& c, int n_envs, int num_cus, Plan& p) {
#ifdef PE_DEBUG_KNOBS
  const Knobs kb = knobs_from_env();
#else
  const Knobs kb;
#endif
  const PlanError e = make_plan(c, n_envs, num_cus, kb, p);
  return e.code == PE_OK ? PE_OK : fail(e.code, e.msg);
}

}  // namespace

extern "C" {

void pe_default_config(pe_config* c, int32_t G, int32_t P, int32_t O, int32_t R, int32_t C) {
  std::memset(c, 0, sizeof(*c));
  c->abi_version = PE_ABI_VERSION;
  c->grid_size = G;
  c->num_plants = P;
  c->num_obstacles = O;
  c->lidar_range = R;
  c->lidar_channels = C;
  c->max_steps = 1000;             // plantos_env.py:120
  c->autoreset = 1;                // DummyVecEnv semantics
  c->thirsty_plant_prob = 0.7;     // plantos_env.py:26
  c->r_goal = 20;                  // plantos_env.py:76-83
  c->r_mistake = -10;
  c->r_invalid = -5;
  c->r_water_empty = -5;
  c->r_step = -0.1;
  c->r_exploration = 10;
  c->r_revisit = -1;
  c->r_complete = 50;
  c->seed = 0;
  c->env_id_offset = 0;
  c->coop_max_done = -1;           // the library's choice per geometry
  c->prefetch_every = -1;
}

int32_t pe_obs_dim(const pe_config* c) { return c->lidar_channels * 5 + 2 + 25; }

const char* pe_last_error(void) { return g_err.c_str(); }

int pe_internal_set_error(int code, const char* msg) {
  g_err = msg;
  return code;
}

int pe_internal_plan(const pe_config* c, int32_t n_envs, int32_t num_cus, pe_plan_info* out) {
  if (!c || !out) return fail(PE_ERR_ARG, "null argument");
  Plan p;
  if (const int rc = plan_for(*c, n_envs, num_cus, p)) return rc;
  std::memset(out, 0, sizeof(*out));
  out->variant = kernel_variant(p.k);
  std::memcpy(out->kernel_name, p.kname, sizeof(out->kernel_name));
  out->tile_codes = p.k.bytetile ? 1 : 0;
  out->stagger = p.stagger;
  out->quad_epb = p.k.epb;
  out->quad_waves = p.k.waves;
  out->coop_max_done = p.coop_max_done;
  out->prefetch_every = p.pf_every;
  out->state_bytes = p.mem.bytes;
  out->prefetch_bytes = p.pf.bytes;
  return PE_OK;
}

// Plan (pe_plan.hpp: every argument check and every choice, no device), bind the device,
// allocate, build and upload the tables, reset, publish.  A return before the last line leaves
// what was allocated to `owner`.
int pe_create(const pe_config* c, int32_t device, int32_t n_envs, pe_handle** out) {
  if (!c || !out) return fail(PE_ERR_ARG, "null argument");
  *out = nullptr;
  // (the CU count is the plan's one input from the device: read before it, so that a rejected
  // config never binds a device)
  int ndev = 0;
  const bool have_dev = hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0;
  const bool dev_ok = have_dev && device >= 0 && device < ndev;
  hipDeviceProp_t prop;
  std::memset(&prop, 0, sizeof(prop));
  if (dev_ok) PE_HIP(hipGetDeviceProperties(&prop, device));
  Plan p;
  if (const int rc = plan_for(*c, n_envs, prop.multiProcessorCount, p)) return rc;
  if (!have_dev) return fail(PE_ERR_DEVICE, "no HIP device available (no CPU fallback)");
  if (!dev_ok) return fail(PE_ERR_ARG, "bad device index");
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(PE_ERR_DEVICE, std::string("built for gfx950, device is ") + prop.gcnArchName);
  DeviceGuard dg(device);  // (also drops a stale error of an earlier call)
  if (dg.rc) return dg.rc;

  std::unique_ptr<pe_handle, HandleDeleter> owner(new (std::nothrow) pe_handle());
  pe_handle* h = owner.get();
  if (!h) return fail(PE_ERR_NOMEM, "host allocation failed");
  h->device = device;
  h->n = n_envs;
  h->cfg = *c;
  h->g = p.g;
  h->rl = p.rl;
  h->k = p.k;
  h->obs_codes = p.obs_codes;
  std::memcpy(h->kname, p.kname, sizeof(h->kname));
  h->lds_floor = p.lds_floor;
  h->stagger = p.stagger;
  h->num_cus = prop.multiProcessorCount;
  h->coop_max_done = p.coop_max_done;
  h->pf_every = p.pf_every;
  h->bytes = p.mem.bytes;

  const StateLayout& m = p.mem;
  hipError_t me = hipMalloc(&h->mem, m.bytes);
  if (me != hipSuccess) return fail(PE_ERR_NOMEM, std::string("hipMalloc: ") + hipGetErrorString(me));
  char* base = static_cast<char*>(h->mem);
  h->st.tab = reinterpret_cast<const Tables*>(base + m.tab);
  h->st.ldx = reinterpret_cast<const signed char*>(base + m.ldx);
  h->st.ldy = reinterpret_cast<const signed char*>(base + m.ldy);
  h->st.ldxy = reinterpret_cast<const int16_t*>(base + m.ldxy);
  h->st.err_bits = reinterpret_cast<uint32_t*>(base + m.err);
  h->st.scal = reinterpret_cast<uint4*>(base + m.scal);
  h->st.ep_ret = reinterpret_cast<double*>(base + m.ret);
  h->st.grid = reinterpret_cast<uint64_t*>(base + m.grid);
  h->st.vis = reinterpret_cast<uint32_t*>(base + m.vis);
  h->st.vx = reinterpret_cast<uint32_t*>(base + m.vx);
  h->st.vpend = reinterpret_cast<uint32_t*>(base + m.vpend);
  h->st.expl = reinterpret_cast<uint32_t*>(base + m.expl);
  if (p.pf_every > 0) {
    const PrefetchLayout& f = p.pf;
    if (hipMalloc(&h->pf_mem, f.bytes) != hipSuccess || hipMemset(h->pf_mem, 0, f.bytes) != hipSuccess)
      return fail(PE_ERR_NOMEM, "prefetch buffers: hipMalloc failed");
    char* pb = static_cast<char*>(h->pf_mem);
    h->pf.scal = reinterpret_cast<uint4*>(pb + f.scal);
    h->pf.grid = reinterpret_cast<uint64_t*>(pb + f.grid);
    h->pf.obs = reinterpret_cast<float*>(pb + f.obs);
    h->pf.ostride = f.ostride;
    h->pf.queue = reinterpret_cast<uint32_t*>(pb + f.queue);
    h->pf.qn = reinterpret_cast<uint32_t*>(pb + f.qn);
    h->pf.flag = reinterpret_cast<uint8_t*>(pb + f.flag);
    // the queue-mode prefetch grid: every workgroup the chip holds at once (launch_prefetch)
    int per_cu = 0;
    hipError_t oe = h->g.WPR == 1
        ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, pe_prefetch_kernel<1, false>, 256, coop_lds_bytes(h->g))
        : hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, pe_prefetch_kernel<kCoopWPR, false>, 256,
                                                       coop_lds_bytes(h->g));
    if (oe != hipSuccess || per_cu < 1) per_cu = 1;
    h->pf_blocks = per_cu * prop.multiProcessorCount;
  }

  const Tables tab = make_tables(h->g);
  const std::vector<uint8_t> ldxy = ray_table(p.ray_tab, h->g.C, h->g.R, p.ldx, p.ldy);
  if (ldxy.size() != ray_table_bytes(p.ray_tab, h->g.C, h->g.R)) return fail(PE_ERR_ARG, "internal: ray table size");
  if (hipMemset(h->mem, 0, m.bytes) != hipSuccess ||
      hipMemcpy(base + m.tab, &tab, sizeof(Tables), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(base + m.ldx, p.ldx.data(), p.ldx.size(), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(base + m.ldy, p.ldy.data(), p.ldy.size(), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(base + m.ldxy, ldxy.data(), ldxy.size(), hipMemcpyHostToDevice) != hipSuccess)
    return fail(PE_ERR_DEVICE, "initial upload failed");
  // every env starts reset (episode 0), like DummyVecEnv.reset() before the first step
  if (const int rc = launch_reset(h, base_args(h), nullptr)) return rc;
  if (h->pf_every > 0)
    if (const int rc = launch_prefetch(h, nullptr, 1)) return rc;
  hipError_t se = hipDeviceSynchronize();
  if (se != hipSuccess) return hip_fail(se, "initial reset");
  *out = owner.release();
  return PE_OK;
}

int pe_destroy(pe_handle* h) {
  if (!h) return PE_OK;
  DeviceGuard dg(h);
  const int rc = free_handle(h);
  return dg.rc ? dg.rc : rc;
}

int pe_curriculum_enable(pe_handle* h, double initial_threshold, double max_threshold, double threshold_increment,
                         int32_t max_episodes_per_maze, int32_t terminate_on_threshold, void* stream) {
  if (!h) return fail(PE_ERR_ARG, "null handle");
  if (max_episodes_per_maze < 1) return fail(PE_ERR_ARG, "max_episodes_per_maze must be >= 1");
  DeviceGuard dg(h);
  if (dg.rc) return dg.rc;
  if (!h->cur_mem) {
    hipError_t me = hipMalloc(&h->cur_mem, sizeof(CurRec) * (size_t)h->n);
    if (me != hipSuccess) {
      h->cur_mem = nullptr;
      return fail(PE_ERR_NOMEM, std::string("hipMalloc: ") + hipGetErrorString(me));
    }
  }
  // A2C_training.py:41-54 / trainingCode.py:29-42: counters 0, maze_completed False,
  // persistent None -- written on the caller's stream, after its queued steps
  hipLaunchKernelGGL(pe_cur_init_kernel, dim3((h->n + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream),
                     static_cast<CurRec*>(h->cur_mem), h->n, initial_threshold);
  PE_HIP(hipGetLastError());
  h->st.cur = static_cast<CurRec*>(h->cur_mem);
  h->rl.cur_max = max_threshold;
  h->rl.cur_inc = threshold_increment;
  h->rl.cur_max_eps = max_episodes_per_maze;
  h->rl.cur_term = terminate_on_threshold ? 1 : 0;
  return PE_OK;
}

int pe_curriculum_disable(pe_handle* h) {
  if (!h) return fail(PE_ERR_ARG, "null handle");
  h->st.cur = nullptr;
  return PE_OK;
}

int pe_curriculum_get(pe_handle* h, double* threshold, int32_t* counters, void* stream) {
  if (!h || !h->st.cur) return fail(PE_ERR_ARG, "curriculum not enabled");
  DeviceGuard dg(h);
  if (dg.rc) return dg.rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t pitch = sizeof(CurRec);
  if (threshold)
    PE_HIP(hipMemcpy2DAsync(threshold, sizeof(double), h->st.cur, pitch, sizeof(double), (size_t)h->n,
                            hipMemcpyDeviceToDevice, s));
  if (counters)
    PE_HIP(hipMemcpy2DAsync(counters, 4 * sizeof(int32_t), reinterpret_cast<char*>(h->st.cur) + 8, pitch,
                            4 * sizeof(int32_t), (size_t)h->n, hipMemcpyDeviceToDevice, s));
  return PE_OK;
}

int pe_seed(pe_handle* h, uint64_t seed, int32_t reset_episode_counters, void* stream) {
  if (!h) return fail(PE_ERR_ARG, "null handle");
  DeviceGuard dg(h);
  if (dg.rc) return dg.rc;
  // on the caller's stream: a step or prefetch kernel queued before this call must
  // finish before the records and counters are cleared (a prefetch still running
  // could otherwise publish an old-seed record after the clear)
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (h->pf.scal && seed != h->rl.seed)  // every prefetched map belongs to the old seed
    PE_HIP(hipMemsetAsync(h->pf.scal, 0, sizeof(uint4) * (size_t)h->n, s));
  h->rl.seed = seed;
  h->cfg.seed = seed;
  if (reset_episode_counters) {
    // the episode counters to 0, the visit rows of envs at an odd episode moved along
    // (they live in the counter's slot, pe_device.hpp vis_env)
    StepArgs a = base_args(h);
    hipLaunchKernelGGL(pe_zero_episodes_kernel, dim3((unsigned)((h->n + 255) / 256)), dim3(256), 0, s, a);
    PE_HIP(hipGetLastError());
  }
  return PE_OK;
}

// The steps' deferred overflow writes applied (pe_vx_flush_kernel), before a call that
// reads the exact visit counts (state export, the MCTS clone) or replaces them (set
// state, resets: reset_env's map scratch is the overflow array).
int flush_vx(const pe_handle* h, hipStream_t s) {
  hipLaunchKernelGGL(pe_vx_flush_kernel, dim3((unsigned)((h->n + 255) / 256)), dim3(256), 0, s, base_args(h));
  PE_HIP(hipGetLastError());
  return PE_OK;
}

extern "C" int pe_internal_flush_vx(const pe_handle* h, void* stream) {
  return flush_vx(h, static_cast<hipStream_t>(stream));
}

int pe_reset(pe_handle* h, const uint8_t* mask, float* obs, void* stream) {
  if (!h) return fail(PE_ERR_ARG, "null handle");
  DeviceGuard dg(h);
  if (dg.rc) return dg.rc;
  StepArgs a = base_args(h);
  a.mask = mask;
  a.obs = obs;
  if (const int fr = flush_vx(h, static_cast<hipStream_t>(stream))) return fr;
  const int rc = launch_reset(h, a, static_cast<hipStream_t>(stream));
  if (rc != PE_OK || h->pf_every <= 0) return rc;
  return launch_prefetch(h, static_cast<hipStream_t>(stream), 1);  // the new episodes' next maps
}

// pe_step / pe_step_codes after their argument checks: the step (obs as f32 or as byte codes, the
// other one NULL), then every pf_every-th call the prefetch of the envs reset since the last one
static int step_common(pe_handle* h, const void* actions, int32_t action_bytes, float* obs, uint8_t* obs_codes,
                       float* reward, uint8_t* terminated, uint8_t* truncated, float* terminal_obs, double* ep_ret,
                       int32_t* ep_len, int32_t* terminal_info, void* stream) {
  if (action_bytes != 4 && action_bytes != 8) return fail(PE_ERR_ARG, "action_bytes must be 4 or 8");
  DeviceGuard dg(h);
  if (dg.rc) return dg.rc;
  StepArgs a = base_args(h);
  a.act_bytes = action_bytes;
  a.actions = actions;
  a.obs = obs;
  a.obs_codes = obs_codes;
  a.reward = reward;
  a.term = terminated;
  a.trunc = truncated;
  a.tobs = terminal_obs;
  a.ep_ret_out = ep_ret;
  a.ep_len_out = ep_len;
  a.tinfo = terminal_info;
  const int rc = launch_step(h, a, static_cast<hipStream_t>(stream));
  if (rc != PE_OK || h->pf_every <= 0 || ++h->pf_count < h->pf_every) return rc;
  h->pf_count = 0;
  return launch_prefetch(h, static_cast<hipStream_t>(stream), 0);  // maps for the envs reset since the last one
}

int pe_step(pe_handle* h, const void* actions, int32_t action_bytes, float* obs, float* reward, uint8_t* terminated,
            uint8_t* truncated, float* terminal_obs, double* ep_ret, int32_t* ep_len, int32_t* terminal_info,
            void* stream) {
  if (!h || !actions || !obs || !reward || !terminated || !truncated) return fail(PE_ERR_ARG, "null argument");
  return step_common(h, actions, action_bytes, obs, nullptr, reward, terminated, truncated, terminal_obs, ep_ret, ep_len,
                     terminal_info, stream);
}

int pe_step_codes(pe_handle* h, const void* actions, int32_t action_bytes, uint8_t* obs_codes, float* reward,
                  uint8_t* terminated, uint8_t* truncated, float* terminal_obs, double* ep_ret, int32_t* ep_len,
                  int32_t* terminal_info, void* stream) {
  if (!h || !actions || !obs_codes || !reward || !terminated || !truncated) return fail(PE_ERR_ARG, "null argument");
  if (!h->obs_codes) return fail(PE_ERR_ARG, "pe_step_codes needs a handle created with obs_codes = 1");
  return step_common(h, actions, action_bytes, nullptr, obs_codes, reward, terminated, truncated, terminal_obs, ep_ret,
                     ep_len, terminal_info, stream);
}

int pe_obs_code_table(const pe_handle* h, float* table) {
  if (!h || !table) return fail(PE_ERR_ARG, "null argument");
  // obs_code_pick's table on the host tables: the same f32 quotients pe_create uploads
  const int R = h->g.R, G = h->g.G;
  for (int c = 0; c < 256; ++c) {
    float v = 0.0f;
    if (c <= R) v = (float)((double)c / (double)R);
    else if (c == R + 1) v = 1.0f;
    else if (c >= kCodeVis && c < kCodeVis + 16) v = (float)((double)(c - kCodeVis < 10 ? c - kCodeVis : 10) / 10.0);
    else if (c >= kCodePos && c < kCodePos + G) v = (float)((double)(c - kCodePos) / (double)G);
    table[c] = v;
  }
  return PE_OK;
}

int pe_expand_obs_codes(const pe_handle* h, int32_t blocks, int32_t rows, const uint8_t* src, int64_t src_stride,
                        float* obs, float* reward, uint8_t* terminated, uint8_t* truncated, void* stream) {
  if (!h || !src || !obs) return fail(PE_ERR_ARG, "null argument");
  if (blocks < 1 || blocks > 65535 || rows < 1) return fail(PE_ERR_ARG, "blocks must be 1..65535, rows >= 1");
  const int64_t need = (((int64_t)rows * h->g.D + 15) & ~(int64_t)15) + 6 * (int64_t)rows;
  if (blocks > 1 && (src_stride < need || (src_stride & 15))) return fail(PE_ERR_ARG, "src_stride too small or not a multiple of 16");
  if ((reinterpret_cast<uintptr_t>(src) & 15u) || (reinterpret_cast<uintptr_t>(obs) & 15u))
    return fail(PE_ERR_ARG, "src and obs must be 16-B aligned");
  DeviceGuard dg(h);
  if (dg.rc) return dg.rc;
  const int64_t groups = ((int64_t)rows * h->g.D + 3) / 4;
  // kExpandPer groups per thread; the per-env outputs need a thread per env
  const int64_t gx = std::max((groups + 256 * kExpandPer - 1) / (256 * kExpandPer), ((int64_t)rows + 255) / 256);
  dim3 grid((unsigned)gx, (unsigned)blocks), block(256);
  hipLaunchKernelGGL(pe_expand_codes_kernel, grid, block, 0, static_cast<hipStream_t>(stream), h->st.tab, h->g.R,
                     h->g.G, h->g.D, rows, src, src_stride, obs, reward, terminated, truncated);
  PE_HIP(hipGetLastError());
  return PE_OK;
}

int pe_get_info(pe_handle* h, int32_t* info, void* stream) {
  if (!h || !info) return fail(PE_ERR_ARG, "null argument");
  DeviceGuard dg(h);
  if (dg.rc) return dg.rc;
  StepArgs a = base_args(h);
  hipLaunchKernelGGL(pe_info_kernel, dim3((h->n + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), a, info);
  PE_HIP(hipGetLastError());
  return PE_OK;
}

int pe_get_state(pe_handle* h, uint8_t* cells, int32_t* visits, int8_t* explored, int32_t* scalars, void* stream) {
  if (!h) return fail(PE_ERR_ARG, "null handle");
  DeviceGuard dg(h);
  if (dg.rc) return dg.rc;
  StepArgs a = base_args(h);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (visits)
    if (const int fr = flush_vx(h, s)) return fr;
  if (cells || visits || explored) {
    int64_t total = (int64_t)h->n * h->g.GG;
    hipLaunchKernelGGL(pe_get_cells_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a, cells, visits,
                       explored);
    PE_HIP(hipGetLastError());
  }
  if (scalars) {
    hipLaunchKernelGGL(pe_get_scal_kernel, dim3((h->n + 255) / 256), dim3(256), 0, s, a, scalars);
    PE_HIP(hipGetLastError());
  }
  return PE_OK;
}

int pe_set_state(pe_handle* h, const uint8_t* cells, const int32_t* visits, const int8_t* explored,
                 const int32_t* scalars, void* stream) {
  if (!h) return fail(PE_ERR_ARG, "null handle");
  DeviceGuard dg(h);
  if (dg.rc) return dg.rc;
  StepArgs a = base_args(h);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (const int fr = flush_vx(h, s)) return fr;
  hipLaunchKernelGGL(pe_set_env_kernel, dim3((h->n + 127) / 128), dim3(128), 0, s, a, cells, visits, explored, scalars);
  PE_HIP(hipGetLastError());
  return PE_OK;
}

int pe_load_maps(pe_handle* h, int32_t k, const int32_t* env_index, const uint8_t* cells, const int32_t* rover,
                 float* obs_k, void* stream) {
  if (!h || (k > 0 && (!env_index || !cells || !rover))) return fail(PE_ERR_ARG, "null argument");
  if (k <= 0) return PE_OK;
  DeviceGuard dg(h);
  if (dg.rc) return dg.rc;
  StepArgs a = base_args(h);
  a.obs = obs_k;
  if (const int fr = flush_vx(h, static_cast<hipStream_t>(stream))) return fr;
  hipLaunchKernelGGL(pe_load_maps_kernel, dim3((k + kBlock - 1) / kBlock), dim3(kBlock), lds_bytes(h->g),
                     static_cast<hipStream_t>(stream), a, k, env_index, cells, rover);
  PE_HIP(hipGetLastError());
  return PE_OK;
}

int pe_synth_actions(pe_handle* h, uint64_t seed, uint32_t t, int32_t* actions, void* stream) {
  if (!h || !actions) return fail(PE_ERR_ARG, "null argument");
  DeviceGuard dg(h);
  if (dg.rc) return dg.rc;
  hipLaunchKernelGGL(pe_synth_kernel, dim3((h->n + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), h->n,
                     seed, h->rl.env_off, t, actions);
  PE_HIP(hipGetLastError());
  return PE_OK;
}

int pe_poll_errors(pe_handle* h, int32_t* bits, void* stream) {
  if (!h || !bits) return fail(PE_ERR_ARG, "null argument");
  DeviceGuard dg(h);
  if (dg.rc) return dg.rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  uint32_t v = 0;
  PE_HIP(hipMemcpyAsync(&v, h->st.err_bits, sizeof(v), hipMemcpyDeviceToHost, s));
  PE_HIP(hipMemsetAsync(h->st.err_bits, 0, sizeof(uint32_t), s));
  PE_HIP(hipStreamSynchronize(s));
  *bits = (int32_t)((v >> 2) & 7u);
  return PE_OK;
}

#ifdef PE_STAMPS
int pe_debug_dstamps(uint64_t* host, int64_t count) {
  if (count > 16384 * 8) count = 16384 * 8;
  PE_HIP(hipDeviceSynchronize());
  PE_HIP(hipMemcpyFromSymbol(host, HIP_SYMBOL(g_dstamps), (size_t)count * 8, 0, hipMemcpyDeviceToHost));
  return PE_OK;
}
#endif
#if defined(PE_STAMPS) || defined(PE_STAMPS_RESET)
int pe_debug_stamps(uint64_t* host, int64_t count) {
  if (count > 16384 * 8) count = 16384 * 8;
  PE_HIP(hipDeviceSynchronize());
  PE_HIP(hipMemcpyFromSymbol(host, HIP_SYMBOL(g_stamps), (size_t)count * 8, 0, hipMemcpyDeviceToHost));
  return PE_OK;
}
#endif

int32_t pe_num_envs(const pe_handle* h) { return h ? h->n : 0; }
int32_t pe_kernel_variant(const pe_handle* h) { return h ? kernel_variant(h->k) : -1; }
const char* pe_kernel_name(const pe_handle* h) { return h ? h->kname : ""; }
int32_t pe_prefetch_every(const pe_handle* h) { return h ? h->pf_every : 0; }
uint64_t pe_state_bytes(const pe_handle* h) { return h ? (uint64_t)h->bytes : 0; }

}  // extern "C"
