// pe_learner_plan.hpp -- the device-free half of a learner's creation (pe_learner.hip):
// make_learner_plan() lays out the master parameters, the workspace, the weight-gradient
// problems and their grid, and the chunk counts as a pure function of (towers, D, max_rows, CU
// count, env_tile asked).  No HIP call and no HIP header (pe_internal_learner_plan,
// tests/test_learner_host.py).
#pragma once
#include <algorithm>

#include "pe_learner.h"
#include "pe_learner_math.hpp"
#include "pe_policy_plan.hpp"

namespace pe_pol {

constexpr int kMaxGridY = 65535;  // HIP's limit on a grid's y dimension
constexpr int kWgradTiles = 4;  // 32-wide input tiles of one weight-gradient wave: one dZ load feeds 4 MFMAs
constexpr int kWgradRows = 2;   // 32-neuron tiles of it: one input load feeds 2

// One weight-gradient problem: dW[N][K] and db[N] of a layer, from dZ [rows][ldz] and the layer's
// input [rows][lda] in the workspace.  Column K of the problem is the bias (input 1).
struct WgradLayer {
  uint64_t ws_in, ws_dz;  // float offsets into the workspace
  int lda, ldz, N, K;
  uint32_t off_w, off_b;  // float offsets into the flat parameters
  int KG;                 // groups of kWgradTiles k tiles
  int first_group;        // this layer's first workgroup of a chunk's grid
};

struct LearnerPlan {
  PolicyPlan pol;
  int max_rows;
  uint32_t poff_w[2][4], poff_b[2][4];  // flat parameter offsets of (tower, layer)
  uint32_t off_wt[2][4];                // transposed packed weights of hidden layer l >= 1
  uint64_t n_params, n_packed_t;
  uint64_t ws_x, ws_act[2][3], ws_dz[2][3], ws_g, ws_gv, ws_terms, ws_floats;
  int n_layers;
  WgradLayer L[8];
  int wgrad_groups, max_chunks, sum_chunks;
};

inline int make_learner_plan(int D, int max_rows, int num_cus, int32_t n_towers, const pe_policy_tower* shapes,
                             int32_t activation, int32_t env_tile, LearnerPlan* out) {
  if (n_towers != 2)
    return pe_internal_set_error(PE_ERR_ARG, "the A2C learner needs a two-tower policy (pi and vf)");
  if (max_rows < 1) return pe_internal_set_error(PE_ERR_ARG, "max_rows must be >= 1");
  if (D < 1) return pe_internal_set_error(PE_ERR_ARG, "obs length must be >= 1");
  // the row chunks are the weight-gradient grid's y dimension
  if (((int64_t)max_rows + kGradChunk - 1) / kGradChunk > kMaxGridY)
    return pe_internal_set_error(PE_ERR_ARG, "max_rows is more than 65535 gradient chunks (65535 * kGradChunk rows)");
  LearnerPlan p{};
  if (const int rc = make_policy_plan(D, max_rows, num_cus, n_towers, nullptr, shapes, activation, env_tile, false, &p.pol))
    return rc;
  p.max_rows = max_rows;
  const uint64_t R = (uint64_t)max_rows;
  uint64_t po = 0, pt = 0, ws = 0;
  p.ws_x = ws;
  ws += R * D;
  for (int i = 0; i < 2; ++i) {
    const Tower& t = p.pol.tw[i];
    for (int l = 0; l <= t.n_hidden; ++l) {
      const Layer& Ly = t.l[l];
      p.poff_w[i][l] = (uint32_t)po;
      po += (uint64_t)Ly.N * Ly.K;
      p.poff_b[i][l] = (uint32_t)po;
      po += (uint64_t)Ly.N;
      if (l >= 1 && l < t.n_hidden) {
        p.off_wt[i][l] = (uint32_t)pt;
        pt += (uint64_t)Ly.N * Ly.K;
      }
      if (l < t.n_hidden) {
        p.ws_act[i][l] = ws;
        ws += R * Ly.N;
        p.ws_dz[i][l] = ws;
        ws += R * Ly.N;
      }
    }
  }
  const int A = p.pol.tw[0].n_out;
  p.ws_g = ws;
  ws += R * A;
  p.ws_gv = ws;
  ws += R;
  p.ws_terms = ws;
  ws += 3 * R;
  p.ws_floats = ws;
  p.n_params = po;
  p.n_packed_t = pt;
  int groups = 0;
  for (int i = 0; i < 2; ++i) {
    const Tower& t = p.pol.tw[i];
    for (int l = 0; l <= t.n_hidden; ++l) {
      const Layer& Ly = t.l[l];
      WgradLayer& W = p.L[p.n_layers++];
      const bool head = l == t.n_hidden;
      W.ws_in = l == 0 ? p.ws_x : p.ws_act[i][l - 1];
      W.lda = Ly.K;
      W.ws_dz = head ? (i == 0 ? p.ws_g : p.ws_gv) : p.ws_dz[i][l];
      W.ldz = Ly.N;
      W.N = Ly.N;
      W.K = Ly.K;
      W.off_w = p.poff_w[i][l];
      W.off_b = p.poff_b[i][l];
      const int KT = (Ly.K + 1 + 31) / 32;
      W.KG = (KT + kWgradTiles - 1) / kWgradTiles;
      W.first_group = groups;
      groups += ((Ly.N + 31) / 32 + kWgradRows - 1) / kWgradRows * W.KG;
    }
  }
  p.wgrad_groups = groups;
  p.max_chunks = (max_rows + kGradChunk - 1) / kGradChunk;
  const uint64_t longer = std::max<uint64_t>(R, p.n_params);
  p.sum_chunks = (int)((longer + kNormChunk - 1) / kNormChunk);
  *out = p;
  return PE_OK;
}

inline pe_learner_plan_info learner_plan_info(const LearnerPlan& p) {
  pe_learner_plan_info o{};
  o.env_tile = p.pol.env_tile;
  o.n_layers = p.n_layers;
  o.grad_chunk = kGradChunk;
  o.max_chunks = p.max_chunks;
  o.wgrad_groups = p.wgrad_groups;
  o.sum_chunks = p.sum_chunks;
  o.lds_bytes = p.pol.lds;
  o.n_params = p.n_params;
  o.ws_floats = p.ws_floats;
  o.partial_floats = (uint64_t)p.max_chunks * p.n_params;
  o.sums_doubles = 4 * (uint64_t)p.sum_chunks;
  o.packed_floats = p.pol.n_packed;
  o.packed_t_floats = p.n_packed_t ? p.n_packed_t : 4;
  return o;
}

}  // namespace pe_pol
