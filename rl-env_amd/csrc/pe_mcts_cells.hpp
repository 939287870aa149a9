// pe_mcts_cells.hpp -- the sim env of a search (a part of pe_mcts.hip): the kernels' argument,
// the cell word of the clone, the sim cells in global memory (GCells) and in LDS (LCells), one
// PlantOSEnv.step on them (sim_step) and the clone kernel.
#pragma once
#include <hip/hip_runtime.h>

#include "pe_device.hpp"

namespace {

using namespace pe;

constexpr uint32_t kVisMask = 0x1FFFFFFFu;
constexpr int kCodeShift = 29;
constexpr uint32_t kCodeMask = 3u << kCodeShift;
constexpr uint32_t kExpl = 1u << 31;
constexpr uint32_t kOffMap = (uint32_t)OBST << kCodeShift;  // off-map neighbour == obstacle (:193-195)

struct MNode;  // pe_mcts_search.hpp

// The argument of the clone and search kernels.  pe_mcts_create fills what the plan and the
// handle decide once; pe_mcts_search copies that and sets the env state, the mask and the outputs.
struct MctsArgs {
  State st;
  Geo g;
  Rules rl;
  int n;
  uint32_t* cellw;
  uint8_t* cellb;   // [N][ggp] clone bytes (LDS path)
  uint32_t* csim;   // [N][G*G] (LDS path)
  uint32_t* csg;    // [N][G*G] (LDS path)
  int ggp, ldsp;    // global / LDS per-env byte strides of the clone bytes
  uint2* ulog;
  MNode* nodes;
  uint32_t* rng;
  int n_sims, max_depth;
  double c;
  const double* logt;  // logt[k] = log(k) from the host's libm (CPython's math.log)
  const uint8_t* mask;
  int32_t* actions;
  int32_t* rorder;
  int32_t* rvisits;
  double* rvalue;
};

struct Sim {
  int x, y, step, expl;
  bool cur_expl, bonus;
};

// What one sim step reads: the rover's N, E, S, W neighbours (plantos_env.py:186)
// and its own cell (index 4).  Off-map neighbours read as obstacles (:193-195).
struct Nbr {
  uint32_t code[5], vis[5];  // cell code, exact visit count
  uint32_t expl;             // bit q: explored_map > 0
};

__device__ __forceinline__ uint32_t sel5(const uint32_t w[5], int k) {
  uint32_t v = 0;
#pragma unroll
  for (int j = 0; j < 5; ++j) v |= w[j] & (0u - (uint32_t)(j == k));
  return v;
}

__device__ __forceinline__ int nbr_cell(int c, int G, int q) {
  return q == 0 ? c - G : (q == 1 ? c + 1 : (q == 2 ? c + G : (q == 3 ? c - 1 : c)));
}

__device__ __forceinline__ bool nbr_on_map(const Sim& s, int G, int q) {
  return q == 0 ? s.x > 0 : (q == 1 ? s.y + 1 < G : (q == 2 ? s.x + 1 < G : (q == 3 ? s.y > 0 : true)));
}

// Sim cells in global memory (any G): u32 words, exact visits; undo log of
// (cell, old word).
struct GCells {
  uint32_t* cw;
  uint2* lg;
  int nlog, G, c;
  uint32_t w[5];
  __device__ void load(const Sim& s, Nbr& nb) {
    c = s.x * G + s.y;
    nb.expl = 0;
#pragma unroll
    for (int q = 0; q < 5; ++q) {  // all five loads issued together (off-map: read own cell, replace)
      const bool on = nbr_on_map(s, G, q);
      const uint32_t r = cw[on ? nbr_cell(c, G, q) : c];
      w[q] = on ? r : kOffMap;
      nb.code[q] = (w[q] & kCodeMask) >> kCodeShift;
      nb.vis[q] = w[q] & kVisMask;
      nb.expl |= (w[q] & kExpl) ? 1u << q : 0u;
    }
  }
  // visit_counts[new] += 1, explored_map[new] = 2, explored_map[old] = 1 (:198-203)
  __device__ void move(int q, bool set_old) {
    if (set_old) {
      lg[nlog++] = make_uint2((uint32_t)c, w[4]);
      cw[c] = w[4] | kExpl;
    }
    const int nc = nbr_cell(c, G, q);
    const uint32_t nw = sel5(w, q);
    lg[nlog++] = make_uint2((uint32_t)nc, nw);
    cw[nc] = (nw | kExpl) + 1u;
  }
  __device__ void water() {  // thirsty -> hydrated (fork :237-240)
    lg[nlog++] = make_uint2((uint32_t)c, w[4]);
    cw[c] = (w[4] & ~kCodeMask) | ((uint32_t)HYD << kCodeShift);
  }
  __device__ void undo() {
    for (int k = nlog - 1; k >= 0; --k) {
      const uint2 u = lg[k];
      cw[u.x] = u.y;
    }
    nlog = 0;
  }
};

// Sim cells in LDS (G <= 64): one byte per cell = visits min(v,31) (bits 0-4) |
// explored << 5 | code << 6.  A field of 31 means "31 or more": the exact count is
// the clone's word (cellw) or, once this simulation has bumped the cell, csim
// (valid where csg holds the simulation's stamp).  Undo = copy the clone's pristine
// bytes (cellb, global, 16-B loads) back over the lane's LDS cells.  cb is 4-B aligned.
constexpr uint32_t kLSat = 31u, kLExpl = 32u;
constexpr int kLCodeShift = 6;

__device__ __forceinline__ uint32_t sat_byte(uint32_t w) {
  const uint32_t v = w & kVisMask;
  return (v < kLSat ? v : kLSat) | ((w & kExpl) ? kLExpl : 0u) | (((w & kCodeMask) >> kCodeShift) << kLCodeShift);
}

struct LCells {
  uint8_t* cb;            // this lane's cells (LDS)
  const uint4* pristine;  // this lane's clone bytes (global)
  const uint32_t* cw;     // exact clone words (global)
  uint32_t* csim;         // exact sim counts of bumped saturated cells (global)
  uint32_t* csg;          // their stamps
  int G, c, nchunk, ldsw; // nchunk = pristine 16-B chunks, ldsw = LDS dwords per lane
  uint32_t stamp;
  uint32_t b[5];
  __device__ uint32_t exact(int i) const { return csg[i] == stamp ? csim[i] : (cw[i] & kVisMask); }
  __device__ void load(const Sim& s, Nbr& nb) {
    c = s.x * G + s.y;
    nb.expl = 0;
    uint32_t sat = 0;
#pragma unroll
    for (int q = 0; q < 5; ++q) {  // all five LDS reads issued together (off-map: read own cell, replace)
      const bool on = nbr_on_map(s, G, q);
      const uint32_t r = cb[on ? nbr_cell(c, G, q) : c];
      b[q] = on ? r : ((uint32_t)OBST << kLCodeShift);
    }
#pragma unroll
    for (int q = 0; q < 5; ++q) {
      nb.code[q] = b[q] >> kLCodeShift;
      nb.vis[q] = b[q] & kLSat;
      sat |= nb.vis[q] == kLSat ? 1u << q : 0u;
      nb.expl |= (b[q] & kLExpl) ? 1u << q : 0u;
    }
    if (sat) {  // rare: counts of 31 or more come from global memory
#pragma unroll
      for (int q = 0; q < 5; ++q)
        if (sat & (1u << q)) nb.vis[q] = exact(nbr_cell(c, G, q));
    }
  }
  __device__ void move(int q, bool set_old) {
    if (set_old) cb[c] = (uint8_t)(b[4] | kLExpl);
    const int nc = nbr_cell(c, G, q);
    const uint32_t nb_ = sel5(b, q);
    const uint32_t f = nb_ & kLSat;
    uint32_t nv = nb_ | kLExpl;
    if (f + 1u < kLSat) {
      nv += 1u;
    } else {
      const uint32_t x = f < kLSat ? kLSat : exact(nc) + 1u;
      nv |= kLSat;
      csim[nc] = x;
      csg[nc] = stamp;
    }
    cb[nc] = (uint8_t)nv;
  }
  __device__ void water() {
    cb[c] = (uint8_t)((b[4] & ~(3u << kLCodeShift)) | ((uint32_t)HYD << kLCodeShift));
  }
  __device__ void undo() {
    uint32_t* d = reinterpret_cast<uint32_t*>(cb);
#pragma unroll 8
    for (int k = 0; k < nchunk; ++k) {  // LDS stores never alias the loads
      const uint4 v = pristine[k];
      if (4 * k + 0 < ldsw) d[4 * k + 0] = v.x;
      if (4 * k + 1 < ldsw) d[4 * k + 1] = v.y;
      if (4 * k + 2 < ldsw) d[4 * k + 2] = v.z;
      if (4 * k + 3 < ldsw) d[4 * k + 3] = v.w;
    }
    ++stamp;
  }
};

// PlantOSEnv.step on the sim env (plantos_env.py:160-183; watering of the fork,
// plantos_env_new.py:236-245).  Only what MCTS reads is produced: reward,
// terminated, truncated (the observation and info dict are never used by the search).
template <class CS>
__device__ double sim_step(const Rules& rl, CS& cs, Sim& s, int total, int act, const Nbr& nb, bool& te, bool& tr) {
  s.step += 1;                                                   // :162
  double r = rl.r_step;                                          // :164
  if (act < 4) {
    if (sel5(nb.code, act) != (uint32_t)OBST) {                 // in bounds, not an obstacle (:193-195)
      const bool never = sel5(nb.vis, act) == 0u;                // :197
      const bool new_unexpl = ((nb.expl >> act) & 1u) == 0u;
      cs.move(act, !s.cur_expl);                                 // :198-203
      s.expl += (s.cur_expl ? 0 : 1) + (new_unexpl ? 1 : 0);
      s.x += act == 0 ? -1 : (act == 2 ? 1 : 0);
      s.y += act == 1 ? 1 : (act == 3 ? -1 : 0);
      s.cur_expl = true;
      r += never ? rl.r_exploration : rl.r_revisit;              // :204-207
    } else {
      r += rl.r_invalid;                                         // :208-211
    }
  } else {
    const uint32_t code = nb.code[4];
    if (code == (uint32_t)THIRSTY) {                             // fork :237-240
      cs.water();
      r += rl.r_goal;
    } else if (code == (uint32_t)HYD) {
      r += rl.r_mistake;                                         // fork :241-242
    } else {
      r += rl.r_water_empty;                                     // :221-222
    }
  }
  // exploration_percentage = explored / total * 100 >= 100 (:320-331, 176, 244-246)
  // holds exactly when explored >= total: for e < t the f64 quotient is at most
  // 1 - 2^-53 and its product with 100 rounds below 100
  const bool full = s.expl >= total;
  te = full;
  tr = s.step >= rl.max_steps;                                   // :177
  if (full && !s.bonus) {                                        // :179-181
    r += rl.r_complete;
    s.bonus = true;
  }
  return r;
}

// _copy_env_state (:221-243): the live env -> the lane's sim cells, one thread per cell.
__global__ void pe_mcts_clone_kernel(MctsArgs a) {
  const Geo& g = a.g;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)a.n * g.GG) return;
  const int64_t e = t / g.GG;
  if (a.mask && !a.mask[e]) return;
  const int c = (int)(t - e * g.GG);
  const int row = c / g.G, col = c - row * g.G;
  const Scal s = unpack(a.st.scal[e]);
  const uint32_t code = (uint32_t)grid_code(a.st, g, e, row, col + g.R);
  const uint32_t v = (uint32_t)visit_exact(a.st, g, e, s.episode, row, col);
  bool ex;
  if (s.flags & F_EXPL_BITMAP)
    ex = (a.st.expl[e * g.estride + (c >> 5)] >> (c & 31)) & 1u;
  else
    ex = v > 0u;  // explored_map > 0 <=> visit > 0 (derived mode)
  const uint32_t w = (v & kVisMask) | (code << kCodeShift) | (ex ? kExpl : 0u);
  a.cellw[e * (int64_t)g.GG + c] = w;
  if (a.cellb) {
    a.cellb[e * (int64_t)a.ggp + c] = (uint8_t)sat_byte(w);
    a.csg[e * (int64_t)g.GG + c] = 0u;
  }
}

}  // namespace
