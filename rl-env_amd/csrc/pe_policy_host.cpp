// pe_policy_host.cpp -- the host twins of pe_policy_forward and pe_policy_forward_lstm
// (include/plantos_batch.h, "Policy inference" and "Recurrent policy inference"): the
// definitions executed literally, one fmaf chain per pre-activation in ascending k,
// pe_tanhf / pe_sigmoidf / pe_expf / the sampler from the header the kernels include too.
// pe_policy_forward_host_bf16 is the twin of a PE_PREC_BF16 policy ("Reduced-precision policy
// inference"): operands rounded to bf16, hidden sums in f64 rounded to f32 once, the f32 head chain.
// Plain C++: no handle, no device.
#include <cstring>
#include <string>
#include <vector>

#include "../../include/plantos_batch.h"
#include "pe_policy_math.hpp"

extern "C" int pe_internal_set_error(int code, const char* msg);

// Shape rules of a policy (shared with pe_policy.hip); with_ptrs: the tensors must be there.
extern "C" int pe_internal_policy_check(int32_t n_towers, const pe_policy_tower* tw, int32_t activation,
                                        int with_ptrs) {
  auto fail = [](const std::string& m) { return pe_internal_set_error(PE_ERR_ARG, m.c_str()); };
  if (!tw) return fail("null towers");
  if (n_towers < 1 || n_towers > 2) return fail("a policy has 1 or 2 towers");
  if (activation != PE_ACT_TANH && activation != PE_ACT_RELU) return fail("activation must be PE_ACT_TANH or PE_ACT_RELU");
  for (int i = 0; i < n_towers; ++i) {
    const pe_policy_tower& t = tw[i];
    if (t.n_hidden < 1 || t.n_hidden > 3) return fail("a tower has 1..3 hidden layers");
    for (int l = 0; l < t.n_hidden; ++l)
      if (t.hidden[l] < 32 || t.hidden[l] > 512 || (t.hidden[l] & 31))
        return fail("hidden widths must be multiples of 32 in 32..512");
    if (i == 0 && (t.n_out < 2 || t.n_out > 8)) return fail("tower 0's head must have 2..8 outputs");
    if (i == 1 && t.n_out != 1) return fail("tower 1's head must have 1 output");
    if (with_ptrs)
      for (int l = 0; l <= t.n_hidden; ++l)
        if (!t.weight[l] || !t.bias[l]) return fail("null weight or bias tensor");
  }
  return PE_OK;
}

// Shape rules of the LSTMs of a recurrent policy (shared with pe_policy_lstm.hip).
extern "C" int pe_internal_policy_lstm_check(int32_t n_towers, const pe_policy_lstm* ls, int with_ptrs) {
  auto fail = [](const std::string& m) { return pe_internal_set_error(PE_ERR_ARG, m.c_str()); };
  if (!ls) return fail("null lstms");
  if (n_towers < 1 || n_towers > 2) return fail("a policy has 1 or 2 towers");
  for (int i = 0; i < n_towers; ++i) {
    const int H = ls[i].hidden;
    if (H > 512)
      return fail("lstm hidden size " + std::to_string(H) + " > 512: the h tile no longer fits LDS beside the obs "
                  "tile; that needs a K-streamed GEMM kernel, which this library does not have");
    if (H < 32 || (H & 31)) return fail("lstm hidden size must be a multiple of 32 in 32..512");
    if (H != ls[0].hidden) return fail("both towers' LSTMs must have the same hidden size");
    if (with_ptrs && (!ls[i].weight_ih || !ls[i].weight_hh || !ls[i].bias_ih || !ls[i].bias_hh))
      return fail("null lstm tensor");
  }
  return PE_OK;
}

namespace {
using namespace pe_pol;

// One pre-activation: the fmaf chain of the definition.  HW: the caller is compiled for the
// CPU's fused multiply-add, which gives the bits of libm's fmaf (both round once).
template <bool HW>
__attribute__((always_inline)) inline float chain(const float* w, const float* x, int K, float acc) {
  for (int k = 0; k < K; ++k) acc = HW ? __builtin_fmaf(w[k], x[k], acc) : std::fmaf(w[k], x[k], acc);
  return acc;
}

// One tower on one obs row: out[0..n_out).
template <bool HW>
__attribute__((always_inline)) inline void tower_body(const pe_policy_tower& t, int D, int activation, const float* x,
                                                      float* out) {
  float a[512], b[512];
  const float* in = x;
  int K = D;
  float* cur = a;
  for (int l = 0; l <= t.n_hidden; ++l) {
    const bool head = l == t.n_hidden;
    const int N = head ? t.n_out : t.hidden[l];
    float* dst = head ? out : cur;
    int j = 0;
    for (; j + 4 <= N; j += 4) {  // four neurons' chains side by side (each still one chain in k order)
      const float* w = t.weight[l] + (size_t)j * K;
      float acc[4] = {t.bias[l][j], t.bias[l][j + 1], t.bias[l][j + 2], t.bias[l][j + 3]};
      for (int k = 0; k < K; ++k)
        for (int q = 0; q < 4; ++q)
          acc[q] = HW ? __builtin_fmaf(w[(size_t)q * K + k], in[k], acc[q]) : std::fmaf(w[(size_t)q * K + k], in[k], acc[q]);
      for (int q = 0; q < 4; ++q)
        dst[j + q] = head ? acc[q] : (activation == PE_ACT_TANH ? pe_tanhf(acc[q]) : pe_relu(acc[q]));
    }
    for (; j < N; ++j) {
      const float acc = chain<HW>(t.weight[l] + (size_t)j * K, in, K, t.bias[l][j]);
      dst[j] = head ? acc : (activation == PE_ACT_TANH ? pe_tanhf(acc) : pe_relu(acc));
    }
    in = dst;
    K = N;
    cur = cur == a ? b : a;
  }
}

#if defined(__x86_64__) && !defined(__HIP_DEVICE_COMPILE__)
__attribute__((target("fma"))) void tower_forward_hw(const pe_policy_tower& t, int D, int activation, const float* x,
                                                     float* out) {
  tower_body<true>(t, D, activation, x, out);
}
bool have_hw_fma() { return __builtin_cpu_supports("fma"); }
#else
void tower_forward_hw(const pe_policy_tower& t, int D, int activation, const float* x, float* out) {
  tower_body<false>(t, D, activation, x, out);
}
bool have_hw_fma() { return false; }
#endif

void tower_forward(const pe_policy_tower& t, int D, int activation, const float* x, float* out) {
  static const bool hw = have_hw_fma();
  if (hw)
    tower_forward_hw(t, D, activation, x, out);
  else
    tower_body<false>(t, D, activation, x, out);
}

// One LSTM step of one env: (h, c) f32[H] are replaced; `start` reads them as +0.  Two units'
// four gates run side by side (each still one chain: bias sum, x in k order, h in k order).
template <bool HW>
__attribute__((always_inline)) inline void lstm_body(const pe_policy_lstm& L, int D, const float* x, bool start,
                                                     float* h, float* c) {
#pragma clang fp contract(off)
  const int H = L.hidden;
  float h_old[512];
  for (int k = 0; k < H; ++k) h_old[k] = start ? 0.0f : h[k];
  for (int j = 0; j < H; j += 2) {
    float acc[8];
    const float *wi[8], *wh[8];
    for (int q = 0; q < 8; ++q) {
      const size_t row = (size_t)(q & 3) * H + j + (q >> 2);
      acc[q] = L.bias_ih[row] + L.bias_hh[row];
      wi[q] = L.weight_ih + row * D;
      wh[q] = L.weight_hh + row * H;
    }
    for (int k = 0; k < D; ++k)
      for (int q = 0; q < 8; ++q) acc[q] = HW ? __builtin_fmaf(wi[q][k], x[k], acc[q]) : std::fmaf(wi[q][k], x[k], acc[q]);
    for (int k = 0; k < H; ++k)
      for (int q = 0; q < 8; ++q)
        acc[q] = HW ? __builtin_fmaf(wh[q][k], h_old[k], acc[q]) : std::fmaf(wh[q][k], h_old[k], acc[q]);
    for (int u = 0; u < 2; ++u)
      pe_lstm_cell(acc[4 * u], acc[4 * u + 1], acc[4 * u + 2], acc[4 * u + 3], start ? 0.0f : c[j + u], &h[j + u],
                   &c[j + u]);
  }
}

#if defined(__x86_64__) && !defined(__HIP_DEVICE_COMPILE__)
__attribute__((target("fma"))) void lstm_step_hw(const pe_policy_lstm& L, int D, const float* x, bool start, float* h,
                                                 float* c) {
  lstm_body<true>(L, D, x, start, h, c);
}
#else
void lstm_step_hw(const pe_policy_lstm& L, int D, const float* x, bool start, float* h, float* c) {
  lstm_body<false>(L, D, x, start, h, c);
}
#endif

void lstm_step(const pe_policy_lstm& L, int D, const float* x, bool start, float* h, float* c) {
  static const bool hw = have_hw_fma();
  if (hw)
    lstm_step_hw(L, D, x, start, h, c);
  else
    lstm_body<false>(L, D, x, start, h, c);
}

// x rounded to bf16, to nearest even, as an f32 (what v_cvt_pk_bf16_f32 gives; NaN stays NaN).
inline float bf16_round(float x) {
  uint32_t u = float_to_bits(x);
  if ((u & 0x7FFFFFFFu) > 0x7F800000u) return bits_to_float(u | 0x00400000u);
  u += 0x7FFFu + ((u >> 16) & 1u);
  return bits_to_float(u & 0xFFFF0000u);
}

// One tower of a PE_PREC_BF16 policy on one obs row xb (already bf16-valued); wb[l]: the
// hidden layers' weights, bf16-valued.  A hidden pre-activation is the f64 sum rounded to f32
// once; the head is tower_body's fmaf chain.
void tower_forward_bf16(const pe_policy_tower& t, const std::vector<float>* wb, int D, int activation, const float* xb,
                        float* out) {
  float a[512], b[512];
  const float* in = xb;
  int K = D;
  float* cur = a;
  for (int l = 0; l < t.n_hidden; ++l) {
    const int N = t.hidden[l];
    for (int j = 0; j < N; ++j) {
      const float* w = wb[l].data() + (size_t)j * K;
      double s = (double)t.bias[l][j];
      for (int k = 0; k < K; ++k) s += (double)w[k] * (double)in[k];
      const float z = (float)s;
      cur[j] = bf16_round(activation == PE_ACT_TANH ? pe_tanhf(z) : pe_relu(z));
    }
    in = cur;
    K = N;
    cur = cur == a ? b : a;
  }
  const int l = t.n_hidden;
  for (int j = 0; j < t.n_out; ++j) out[j] = chain<false>(t.weight[l] + (size_t)j * K, in, K, t.bias[l][j]);
}

}  // namespace

extern "C" {

int pe_policy_forward_host_bf16(int32_t n, int32_t D, int32_t n_towers, const pe_policy_tower* towers,
                                int32_t activation, const float* obs, int32_t mode, uint64_t seed,
                                uint32_t env_id_offset, uint32_t t, int32_t* actions, float* head0, float* head1) {
  if (const int rc = pe_internal_policy_check(n_towers, towers, activation, 1)) return rc;
  if (n < 0 || D < 1 || !obs || !actions) return pe_internal_set_error(PE_ERR_ARG, "bad n / D or null obs / actions");
  if (mode != PE_POLICY_ARGMAX && mode != PE_POLICY_SAMPLE)
    return pe_internal_set_error(PE_ERR_ARG, "mode must be PE_POLICY_ARGMAX or PE_POLICY_SAMPLE");
  if (head1 && n_towers < 2) return pe_internal_set_error(PE_ERR_ARG, "head1 needs a second tower");
  std::vector<float> wb[2][3];
  for (int i = 0; i < n_towers; ++i) {
    int K = D;
    for (int l = 0; l < towers[i].n_hidden; ++l) {
      const size_t cnt = (size_t)towers[i].hidden[l] * K;
      wb[i][l].resize(cnt);
      for (size_t q = 0; q < cnt; ++q) wb[i][l][q] = bf16_round(towers[i].weight[l][q]);
      K = towers[i].hidden[l];
    }
  }
  const int A = towers[0].n_out;
  std::vector<float> xb(D);
  for (int e = 0; e < n; ++e) {
    for (int k = 0; k < D; ++k) xb[k] = bf16_round(obs[(size_t)e * D + k]);
    float l[8], v;
    tower_forward_bf16(towers[0], wb[0], D, activation, xb.data(), l);
    if (n_towers == 2) {
      tower_forward_bf16(towers[1], wb[1], D, activation, xb.data(), &v);
      if (head1) head1[e] = v;
    }
    if (head0) std::memcpy(head0 + (size_t)e * A, l, sizeof(float) * A);
    actions[e] = mode == PE_POLICY_ARGMAX ? policy_argmax(l, A)
                                          : policy_sample(l, A, policy_uniform(seed, env_id_offset + (uint32_t)e, t));
  }
  return PE_OK;
}

int pe_policy_forward_host(int32_t n, int32_t D, int32_t n_towers, const pe_policy_tower* towers,
                           int32_t activation, const float* obs, int32_t mode, uint64_t seed,
                           uint32_t env_id_offset, uint32_t t, int32_t* actions, float* head0, float* head1) {
  if (const int rc = pe_internal_policy_check(n_towers, towers, activation, 1)) return rc;
  if (n < 0 || D < 1 || !obs || !actions) return pe_internal_set_error(PE_ERR_ARG, "bad n / D or null obs / actions");
  if (mode != PE_POLICY_ARGMAX && mode != PE_POLICY_SAMPLE)
    return pe_internal_set_error(PE_ERR_ARG, "mode must be PE_POLICY_ARGMAX or PE_POLICY_SAMPLE");
  if (head1 && n_towers < 2) return pe_internal_set_error(PE_ERR_ARG, "head1 needs a second tower");
  const int A = towers[0].n_out;
  for (int e = 0; e < n; ++e) {
    const float* x = obs + (size_t)e * D;
    float l[8], v;
    tower_forward(towers[0], D, activation, x, l);
    if (n_towers == 2) {
      tower_forward(towers[1], D, activation, x, &v);
      if (head1) head1[e] = v;
    }
    if (head0) std::memcpy(head0 + (size_t)e * A, l, sizeof(float) * A);
    actions[e] = mode == PE_POLICY_ARGMAX ? policy_argmax(l, A)
                                          : policy_sample(l, A, policy_uniform(seed, env_id_offset + (uint32_t)e, t));
  }
  return PE_OK;
}

int pe_policy_lstm_forward_host(int32_t n, int32_t D, int32_t n_towers, const pe_policy_lstm* lstms,
                                const pe_policy_tower* towers, int32_t activation, const float* obs,
                                const uint8_t* start, float* h_state, float* c_state, int32_t mode, uint64_t seed,
                                uint32_t env_id_offset, uint32_t t, int32_t* actions, float* head0, float* head1) {
  if (const int rc = pe_internal_policy_check(n_towers, towers, activation, 1)) return rc;
  if (const int rc = pe_internal_policy_lstm_check(n_towers, lstms, 1)) return rc;
  if (n < 0 || D < 1 || !obs || !actions || !h_state || !c_state)
    return pe_internal_set_error(PE_ERR_ARG, "bad n / D or null obs / actions / state");
  if (mode != PE_POLICY_ARGMAX && mode != PE_POLICY_SAMPLE)
    return pe_internal_set_error(PE_ERR_ARG, "mode must be PE_POLICY_ARGMAX or PE_POLICY_SAMPLE");
  if (head1 && n_towers < 2) return pe_internal_set_error(PE_ERR_ARG, "head1 needs a second tower");
  const int A = towers[0].n_out, H = lstms[0].hidden;
  for (int e = 0; e < n; ++e) {
    const float* x = obs + (size_t)e * D;
    const bool st = start && start[e];
    float l[8], v;
    for (int ti = 0; ti < n_towers; ++ti) {
      float* h = h_state + ((size_t)ti * n + e) * H;
      float* c = c_state + ((size_t)ti * n + e) * H;
      lstm_step(lstms[ti], D, x, st, h, c);
      tower_forward(towers[ti], H, activation, h, ti == 0 ? l : &v);
    }
    if (n_towers == 2 && head1) head1[e] = v;
    if (head0) std::memcpy(head0 + (size_t)e * A, l, sizeof(float) * A);
    actions[e] = mode == PE_POLICY_ARGMAX ? policy_argmax(l, A)
                                          : policy_sample(l, A, policy_uniform(seed, env_id_offset + (uint32_t)e, t));
  }
  return PE_OK;
}

int pe_policy_math_host(int32_t which, int32_t n, const float* x, float* y) {
  if (n < 0 || (n > 0 && (!x || !y)) || which < 0 || which > 2)
    return pe_internal_set_error(PE_ERR_ARG, "which must be 0 (pe_tanhf), 1 (pe_expf) or 2 (pe_sigmoidf); null argument");
  for (int i = 0; i < n; ++i) y[i] = which == 0 ? pe_tanhf(x[i]) : (which == 1 ? pe_expf(x[i]) : pe_sigmoidf(x[i]));
  return PE_OK;
}

}  // extern "C"
