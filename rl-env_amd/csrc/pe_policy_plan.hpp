// pe_policy_plan.hpp -- the device-free half of policy creation (pe_policy.hip, pe_policy_lstm.hip).
//
// make_policy_plan() decides everything pe_policy_create / pe_policy_create_lstm decide before
// their first allocation -- the shape checks, the layer tables and the packed buffer's layout,
// the LDS images' size, the envs per workgroup and the LSTM state's size -- as a pure function
// of (obs length, batch size, CU count, shapes, activation, env_tile asked).  It makes no HIP
// call and includes no HIP header, so the choice can be examined without a GPU
// (pe_internal_policy_plan, tests/test_policy_plan_host.py).  make_policy_plan_prec() is the plan
// of a feed-forward policy of a precision: make_policy_plan() itself for PE_PREC_F32, the bf16
// layouts at the end of this file for PE_PREC_BF16 (pe_internal_policy_plan_prec,
// tests/test_policy_bf16_host.py).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "../../include/plantos_batch.h"

extern "C" int pe_internal_set_error(int code, const char* msg);
// the shape rules (pe_policy_host.cpp); with_ptrs: the tensors must be there
extern "C" int pe_internal_policy_check(int32_t n_towers, const pe_policy_tower* tw, int32_t activation,
                                        int with_ptrs);
extern "C" int pe_internal_policy_lstm_check(int32_t n_towers, const pe_policy_lstm* ls, int with_ptrs);

namespace pe_pol {

constexpr int kMaxLds = 160 * 1024;  // LDS per workgroup (gfx950)
constexpr int kHeadRows = 9;         // tower 0's <= 8 outputs + the value

struct Layer {
  int K, Kp, N;            // inputs, inputs padded to a multiple of 8 (hidden layers), outputs
  uint32_t off_w, off_b;   // float offsets into the packed buffer
};
struct Tower {
  int n_hidden, n_out;
  Layer l[4];  // hidden layers, then the head
};

struct PolicyPlan {
  int n_towers, act;
  int D, SD, Kp0, HB;      // obs length, D | 1 staging pitch, D padded to 8, rows of a hidden buffer
  int H;                   // LSTM hidden size; 0: feed-forward
  int precision;           // PE_PREC_F32 / PE_PREC_BF16 (feed-forward only)
  int env_tile;            // envs per workgroup: 32 or 64
  Tower tw[2];
  uint32_t off_lw[2];      // packed gate weights of tower i: [unit tile][k group][gate][lane][4]
  uint32_t off_lb[2];      // bias_ih + bias_hh of tower i: [4H]
  size_t n_packed;         // floats of the packed weights (the code table follows them)
  size_t lds;              // dynamic LDS of a forward workgroup, bytes
  size_t n_state;          // floats of one (tower, h or c) state image: tiles * H * env_tile
};

// The forward kernels' LDS: the code table, the head rows, xT [Kp0][E] and two buffers [HB][E].
inline size_t lds_bytes(int E, int Kp0, int HB) {
  return sizeof(float) * ((size_t)256 + (size_t)E * (kHeadRows + Kp0 + 2 * HB));
}

// Fills p's layer tables of `n_towers` towers whose first layer reads K0 inputs, packed from
// float offset `off` on; returns the end offset and the widest hidden layer.
inline size_t layout_towers(PolicyPlan* p, int n_towers, const pe_policy_tower* shapes, int K0, size_t off, int* hmax) {
  *hmax = 0;
  for (int i = 0; i < n_towers; ++i) {
    Tower& t = p->tw[i];
    t.n_hidden = shapes[i].n_hidden;
    t.n_out = shapes[i].n_out;
    int K = K0;
    for (int l = 0; l <= t.n_hidden; ++l) {
      Layer& L = t.l[l];
      const bool head = l == t.n_hidden;
      L.K = K;
      L.Kp = head ? K : (K + 7) & ~7;
      L.N = head ? t.n_out : shapes[i].hidden[l];
      L.off_w = (uint32_t)off;
      off += (size_t)L.N * L.Kp;
      L.off_b = (uint32_t)off;
      off += ((size_t)L.N + 3) & ~(size_t)3;  // every offset stays a multiple of 16 B
      if (!head) *hmax = *hmax > L.N ? *hmax : L.N;
      K = L.N;
    }
  }
  return off;
}

// The plan of a policy over obs rows of D values for n_envs envs on a device of num_cus CUs;
// lstms: null for a feed-forward policy.  PE_OK, or the error of the create call with
// pe_last_error() set.
inline int make_policy_plan(int D, int n_envs, int num_cus, int32_t n_towers, const pe_policy_lstm* lstms,
                            const pe_policy_tower* shapes, int32_t activation, int32_t env_tile, bool recurrent,
                            PolicyPlan* out) {
  if (const int rc = pe_internal_policy_check(n_towers, shapes, activation, 0)) return rc;
  if (recurrent)
    if (const int rc = pe_internal_policy_lstm_check(n_towers, lstms, 0)) return rc;
  if (env_tile != 0 && env_tile != 32 && env_tile != 64)
    return pe_internal_set_error(PE_ERR_ARG, "env_tile must be 0, 32 or 64");
  PolicyPlan p{};
  p.n_towers = n_towers;
  p.act = activation;
  p.D = D;
  p.SD = D | 1;
  p.Kp0 = (D + 7) & ~7;
  p.H = recurrent ? lstms[0].hidden : 0;
  size_t off = 0;
  for (int i = 0; i < n_towers && recurrent; ++i) {  // the gates' K = Kp0 + H chain, then the MLP
    p.off_lw[i] = (uint32_t)off;
    off += (size_t)4 * p.H * (p.Kp0 + p.H);
    p.off_lb[i] = (uint32_t)off;
    off += (size_t)4 * p.H;
  }
  int hmax = 0;
  p.n_packed = layout_towers(&p, n_towers, shapes, recurrent ? p.H : D, off, &hmax);
  p.HB = std::max(std::max(hmax, p.H), p.SD);  // a hidden buffer first holds the staging image [E][SD]
  const bool fits64 = lds_bytes(64, p.Kp0, p.HB) <= (size_t)kMaxLds;
  const bool fits32 = lds_bytes(32, p.Kp0, p.HB) <= (size_t)kMaxLds;
  // the library's choice: 64 envs per workgroup once that still gives every CU a workgroup
  // (each workgroup streams the whole net), else 32
  if (env_tile == 0) env_tile = (fits64 && (int64_t)n_envs >= 64 * (int64_t)std::max(num_cus, 1)) ? 64 : 32;
  if (!(env_tile == 64 ? fits64 : fits32))
    return pe_internal_set_error(
        PE_ERR_ARG,
        recurrent ? "the env tile's obs, h and activation images do not fit 160 KiB of LDS "
                    "(obs length / lstm hidden size / layer widths / env_tile; a hidden size of 512 needs env_tile 32)"
                  : "the env tile's activations do not fit 160 KiB of LDS (obs length / layer widths / env_tile)");
  p.env_tile = env_tile;
  p.lds = lds_bytes(env_tile, p.Kp0, p.HB);
  p.n_state = ((size_t)n_envs + env_tile - 1) / env_tile * p.H * env_tile;
  *out = p;
  return PE_OK;
}

// ---------------------------------------------------------------- bf16 (PE_PREC_BF16)
// A bf16 policy's packed buffer is still counted in floats.  A hidden layer's weights are bf16
// in [neuron tile of 32][k step of 16][lane][8] -- lane l holds W[tile*32 + (l & 31)]
// [step*16 + 8 (l >> 5) + 0..7], the A operand of one v_mfma_f32_32x32x16_bf16 as one 16-byte
// load -- so N * Kp / 2 floats with K padded to Kp, a multiple of 16.  Biases and head weights
// are f32 in the f32 plan's layout.
inline size_t layout_towers_bf16(PolicyPlan* p, int n_towers, const pe_policy_tower* shapes, int K0, int* hmax) {
  size_t off = 0;
  *hmax = 0;
  for (int i = 0; i < n_towers; ++i) {
    Tower& t = p->tw[i];
    t.n_hidden = shapes[i].n_hidden;
    t.n_out = shapes[i].n_out;
    int K = K0;
    for (int l = 0; l <= t.n_hidden; ++l) {
      Layer& L = t.l[l];
      const bool head = l == t.n_hidden;
      L.K = K;
      L.Kp = head ? K : (K + 15) & ~15;
      L.N = head ? t.n_out : shapes[i].hidden[l];
      L.off_w = (uint32_t)off;
      off += head ? (size_t)L.N * L.Kp : (size_t)L.N * L.Kp / 2;
      off = (off + 3) & ~(size_t)3;  // every offset stays a multiple of 16 B
      L.off_b = (uint32_t)off;
      off += ((size_t)L.N + 3) & ~(size_t)3;
      if (!head) *hmax = *hmax > L.N ? *hmax : L.N;
      K = L.N;
    }
  }
  return off;
}

// The bf16 forward kernels' LDS: the f32 code table and head rows, then three bf16 images in
// [k group of 8][env][8] (a lane's B operand is one ds_read_b128): the obs x [Kp0 / 8] and two
// activation images [HB / 8].  The obs go from global memory straight into x (a thread converts
// the 8 values of one (env, k group)), so there is no staging image.
inline size_t lds_bytes_bf16(int E, int Kp0, int HB) {
  return sizeof(float) * ((size_t)256 + (size_t)E * kHeadRows) + 2 * (size_t)E * ((size_t)Kp0 + 2 * (size_t)HB);
}

// make_policy_plan for a feed-forward policy of `precision`; PE_PREC_F32 is make_policy_plan.
inline int make_policy_plan_prec(int D, int n_envs, int num_cus, int32_t n_towers, const pe_policy_tower* shapes,
                                 int32_t activation, int32_t env_tile, int32_t precision, PolicyPlan* out) {
  if (precision == PE_PREC_F32)
    return make_policy_plan(D, n_envs, num_cus, n_towers, nullptr, shapes, activation, env_tile, false, out);
  if (precision != PE_PREC_BF16) return pe_internal_set_error(PE_ERR_ARG, "precision must be PE_PREC_F32 or PE_PREC_BF16");
  if (const int rc = pe_internal_policy_check(n_towers, shapes, activation, 0)) return rc;
  if (env_tile != 0 && env_tile != 32 && env_tile != 64)
    return pe_internal_set_error(PE_ERR_ARG, "env_tile must be 0, 32 or 64");
  PolicyPlan p{};
  p.n_towers = n_towers;
  p.act = activation;
  p.D = D;
  p.SD = D;  // no staging image
  p.Kp0 = (D + 15) & ~15;
  p.precision = PE_PREC_BF16;
  int hmax = 0;
  p.n_packed = layout_towers_bf16(&p, n_towers, shapes, D, &hmax);
  p.HB = hmax;
  const bool fits64 = lds_bytes_bf16(64, p.Kp0, p.HB) <= (size_t)kMaxLds;
  const bool fits32 = lds_bytes_bf16(32, p.Kp0, p.HB) <= (size_t)kMaxLds;
  // the f32 plan's rule: 64 envs per workgroup once that still gives every CU a workgroup
  if (env_tile == 0) env_tile = (fits64 && (int64_t)n_envs >= 64 * (int64_t)std::max(num_cus, 1)) ? 64 : 32;
  if (!(env_tile == 64 ? fits64 : fits32))
    return pe_internal_set_error(
        PE_ERR_ARG, "the env tile's bf16 obs and activation images do not fit 160 KiB of LDS (obs length / layer widths / env_tile)");
  p.env_tile = env_tile;
  p.lds = lds_bytes_bf16(env_tile, p.Kp0, p.HB);
  *out = p;
  return PE_OK;
}

}  // namespace pe_pol
