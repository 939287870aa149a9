// pe_handle.hpp -- the handle behind the opaque pe_handle* of include/plantos_batch.h
// (shared by the translation units of libplantos_hip.so; not part of the ABI).
#pragma once
#include "../../include/plantos_batch.h"
#include "pe_device.hpp"

namespace pe {
// A handle's step kernel, by what it is.  pe_plan.hpp chooses it; the launch, its LDS size, its
// name, the ray-table format and pe_kernel_variant() all read this one choice.
enum class StepFamily : int {
  wave,  // pe_step_wave: one wave per env, any geometry
  fast,  // pe_step_fast<C, R, ONEWORD>: one lane per env (A/B measurement, debug builds only)
  quad,  // pe_step_quad<C, R, ONEWORD, NW, BT, EPB>: the sector kernel
  far    // pe_step_far<C, R>: the sector kernel of long LIDAR ranges
};
struct StepKernel {
  StepFamily family;
  int C, R;       // the compile-time LIDAR table (lidar_tables.inc); 0, 0: rays from the runtime table
  bool oneword;   // the whole padded grid row in one u64 and 16-B visit rows
  bool bytetile;  // the obs tile holds byte codes (pe_step_quad<..., BT>); so do the prefetched records' obs rows
  int epb;        // envs per workgroup (the sector kernel: 64; 16 / 32 for small batches, C16R6 one-word)
  int waves;      // waves per workgroup (the sector kernel: 4; 8 with 16-env workgroups up to 4096 envs)
};
}  // namespace pe

struct pe_handle {
  int device;
  int n;
  pe_config cfg;
  pe::Geo g;
  pe::Rules rl;
  pe::State st;
  void* mem;
  size_t bytes;
  pe::StepKernel k;
  int obs_codes;     // pe_config.obs_codes: pe_step_codes allowed (implies k.bytetile)
  char kname[64];    // the step kernel's name (pe_kernel_name)
  void* cur_mem;     // CurriculumWrapper records (pe_curriculum_enable), or NULL
  size_t lds_floor;  // minimum dynamic LDS per step workgroup (PE_LDS_FLOOR, debug builds only)
  int stagger;       // sector-kernel start delay per block quarter (byte-tile kernels; PE_STAGGER in debug builds)
  int num_cus;       // the device's CUs
  int coop_max_done; // wave-cooperative auto-resets up to this many done envs per block (pe_coop.hpp;
                     // pe_config.coop_max_done)
  pe::Prefetch pf;   // prefetched resets (pf.scal == NULL: off)
  void* pf_mem;
  int pf_every;      // steps between queue-mode prefetch launches (pe_config.prefetch_every)
  int pf_count;      // steps since the last one
  int pf_blocks;     // queue-mode prefetch grid: workgroups resident at once
  void* render_cache;  // pe_render's per-cell_size device tables (pe_render.hip), or NULL
};

// pe_internal_set_error (plantos_batch.hip): records pe_last_error() for this thread.
extern "C" int pe_internal_set_error(int code, const char* msg);
// pe_internal_flush_vx (plantos_batch.hip): the steps' deferred visit-overflow writes applied
// on `stream` (before anything reads the exact visit counts, e.g. the MCTS clone).
extern "C" int pe_internal_flush_vx(const pe_handle* h, void* stream);
// pe_internal_plan (plantos_batch.hip): what pe_create would decide for (config, n_envs) on a
// device of num_cus CUs, before it touches a device (pe_plan.hpp) -- no HIP call.  On rejection
// pe_create's error code, with pe_last_error() set.
struct pe_plan_info {
  int32_t variant;       // pe_kernel_variant()
  char kernel_name[64];  // pe_kernel_name()
  int32_t tile_codes, stagger, quad_epb, quad_waves, coop_max_done, prefetch_every;
  uint64_t state_bytes;     // pe_state_bytes(): the main allocation
  uint64_t prefetch_bytes;  // the prefetched resets' allocation (0: none)
};
extern "C" int pe_internal_plan(const pe_config* c, int32_t n_envs, int32_t num_cus, pe_plan_info* out);
// pe_internal_policy_plan (pe_policy.hip): what pe_policy_create (lstms null) or
// pe_policy_create_lstm would decide for obs rows of D values, before they touch a device
// (pe_policy_plan.hpp) -- no HIP call.  On rejection their error code, with pe_last_error() set.
struct pe_policy_plan_info {
  int32_t env_tile;        // pe_policy_env_tile()
  uint64_t lds_bytes;      // a forward workgroup's dynamic LDS
  uint64_t packed_floats;  // the packed weights
  uint64_t state_floats;   // one (tower, h or c) LSTM state image; 0: feed-forward
};
extern "C" int pe_internal_policy_plan(int32_t D, int32_t n_envs, int32_t num_cus, int32_t n_towers,
                                       const pe_policy_lstm* lstms, const pe_policy_tower* shapes, int32_t activation,
                                       int32_t env_tile, pe_policy_plan_info* out);
// ... for a precision (pe_policy_create_prec; PE_PREC_F32 answers as pe_internal_policy_plan;
// lstms with another precision is PE_ERR_ARG).
extern "C" int pe_internal_policy_plan_prec(int32_t D, int32_t n_envs, int32_t num_cus, int32_t n_towers,
                                            const pe_policy_lstm* lstms, const pe_policy_tower* shapes,
                                            int32_t activation, int32_t env_tile, int32_t precision,
                                            pe_policy_plan_info* out);
// pe_internal_mcts_plan (pe_mcts.hip): what pe_mcts_create would decide for a handle of grid side
// G and n_envs envs, before it touches a device (pe_mcts_plan.hpp) -- no HIP call.  On rejection
// pe_mcts_create's error code, with pe_last_error() set.
struct pe_mcts_plan_info {
  int32_t kernel;      // 1: pe_mcts_search_lds_kernel, 0: pe_mcts_search_kernel
  int32_t ldsp, ggp;   // LDS / global per-env byte strides of the clone bytes
  uint32_t clone_blocks, search_blocks;
  uint64_t lds_bytes;  // dynamic LDS of a workgroup of the LDS kernel (whichever kernel runs)
  // cellw, ulog, nodes, rng, logt, cellb, csim, csg: bytes from the start of the handle's one
  // allocation; size 0: not allocated (the kernel reads no such array)
  uint64_t offset[8], size[8];
  uint64_t total;
};
extern "C" int pe_internal_mcts_plan(int32_t G, int32_t n_envs, int32_t n_simulations, int32_t max_depth,
                                     pe_mcts_plan_info* out);
// One np.random stream between numpy's (key u32[624], pos in [0, 624]) and the device form
// (u32[628], pe_mcts_rng.hpp), as pe_mcts_set_rng / pe_mcts_get_rng convert it.  Host arrays; no device.
extern "C" int pe_internal_mcts_rng_to_device_host(const uint32_t* key, int32_t pos, uint32_t* dev);
extern "C" int pe_internal_mcts_rng_from_device_host(const uint32_t* dev, uint32_t* key, int32_t* pos);
// pe_internal_render_free (pe_render.hip): frees the handle's render tables (pe_destroy).
extern "C" void pe_internal_render_free(pe_handle* h);
