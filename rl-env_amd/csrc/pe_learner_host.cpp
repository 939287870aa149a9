// pe_learner_host.cpp -- the host twin of the A2C learner (pe_internal_learner_update_host): the
// definition of pe_learner_math.hpp executed literally, one chain per sum in the order written
// there, and the device-free plan (pe_internal_learner_plan).  Plain C++: no handle, no device.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "pe_learner.h"
#include "pe_learner_math.hpp"
#include "pe_learner_plan.hpp"

namespace {
using namespace pe_pol;

// The f64 sum of term(i), i < N, in the chunk order of pe_rollout_math.hpp.
template <class F>
double chunk_sum(int64_t N, F term) {
  double total = 0.0;
  for (int64_t base = 0; base < N; base += kNormChunk) {
    const int64_t len = std::min<int64_t>(kNormChunk, N - base);
    double s[kNormLanes];
    for (int l = 0; l < kNormLanes; ++l) s[l] = 0.0;
    for (int64_t q = 0; q < len; ++q) s[q % kNormLanes] += term(base + q);
    for (int h = kNormLanes / 2; h >= 1; h /= 2)
      for (int l = 0; l < h; ++l) s[l] += s[l + h];
    total += s[0];
  }
  return total;
}

struct Args {
  int rows, D, act, apply;
  const pe_policy_tower* tw;
  const float* obs;
  const int32_t* actions;
  const float* adv;
  const float* ret;
  LearnerHyper h;
  float* sq;
  float* grads;
  float* out;
};

// HW: the caller is compiled for the CPU's fused multiply-add, which gives libm fmaf's bits.
#define PE_FMA(a, b, c) (HW ? __builtin_fmaf((a), (b), (c)) : std::fmaf((a), (b), (c)))

template <bool HW>
__attribute__((always_inline)) inline void update_body(const Args& a) {
#pragma clang fp contract(off)
  const int B = a.rows, D = a.D, A = a.tw[0].n_out;
  const float Bf = (float)B;
  std::vector<float> acts[2][3], dzs[2][3], G((size_t)B * A), GV(B), tpol(B), tval(B), tent(B);
  int width[2][4];  // outputs of (tower, layer)
  for (int i = 0; i < 2; ++i)
    for (int l = 0; l <= a.tw[i].n_hidden; ++l) {
      width[i][l] = l == a.tw[i].n_hidden ? a.tw[i].n_out : a.tw[i].hidden[l];
      if (l < a.tw[i].n_hidden) {
        acts[i][l].resize((size_t)B * width[i][l]);
        dzs[i][l].resize((size_t)B * width[i][l]);
      }
    }

  // forward, head gradients, backward data: row by row
  std::vector<float> dA(512);
  for (int r = 0; r < B; ++r) {
    float head[2][8];
    for (int i = 0; i < 2; ++i) {
      const pe_policy_tower& t = a.tw[i];
      const float* in = a.obs + (size_t)r * D;
      int K = D;
      for (int l = 0; l <= t.n_hidden; ++l) {
        const bool last = l == t.n_hidden;
        const int N = width[i][l];
        float* dst = last ? head[i] : acts[i][l].data() + (size_t)r * N;
        for (int j = 0; j < N; ++j) {
          const float* w = t.weight[l] + (size_t)j * K;
          float acc = t.bias[l][j];
          for (int k = 0; k < K; ++k) acc = PE_FMA(w[k], in[k], acc);
          dst[j] = last ? acc : (a.act == PE_ACT_TANH ? pe_tanhf(acc) : pe_relu(acc));
        }
        in = dst;
        K = N;
      }
    }
    learner_row(head[0], A, a.actions[r], a.adv[r], a.h.ent_coef, Bf, G.data() + (size_t)r * A, &tpol[r], &tent[r]);
    learner_value(head[1][0], a.ret[r], a.h.two_vf, Bf, &GV[r], &tval[r]);
    for (int i = 0; i < 2; ++i) {
      const pe_policy_tower& t = a.tw[i];
      const float* dz = i == 0 ? G.data() + (size_t)r * A : &GV[r];
      for (int l = t.n_hidden; l >= 1; --l) {  // dZ_l -> dZ_{l-1}
        const int N = width[i][l], K = width[i][l - 1];
        for (int k = 0; k < K; ++k) dA[k] = 0.0f;
        for (int j = 0; j < N; ++j) {  // every dA[k] is one chain over ascending j
          const float* w = t.weight[l] + (size_t)j * K;
          const float d = dz[j];
          for (int k = 0; k < K; ++k) dA[k] = PE_FMA(w[k], d, dA[k]);
        }
        const float* act = acts[i][l - 1].data() + (size_t)r * K;
        float* o = dzs[i][l - 1].data() + (size_t)r * K;
        for (int k = 0; k < K; ++k) o[k] = dA[k] * act_deriv(act[k], a.act);
        dz = o;
      }
    }
  }

  // parameter gradients: a chain per chunk of kGradChunk rows, the partials in f64
  size_t off = 0;
  std::vector<float> part;
  std::vector<double> sum;
  for (int i = 0; i < 2; ++i) {
    const pe_policy_tower& t = a.tw[i];
    for (int l = 0; l <= t.n_hidden; ++l) {
      const int N = width[i][l], K = l == 0 ? D : width[i][l - 1];
      const float* in = l == 0 ? a.obs : acts[i][l - 1].data();
      const float* dz = l == t.n_hidden ? (i == 0 ? G.data() : GV.data()) : dzs[i][l].data();
      const size_t cnt = (size_t)N * K + N;  // weight, then bias
      sum.assign(cnt, 0.0);
      for (int c0 = 0; c0 < B; c0 += kGradChunk) {
        part.assign(cnt, 0.0f);
        const int c1 = std::min(B, c0 + kGradChunk);
        for (int r = c0; r < c1; ++r) {
          const float* x = in + (size_t)r * K;
          for (int j = 0; j < N; ++j) {
            const float d = dz[(size_t)r * N + j];
            float* pw = part.data() + (size_t)j * K;
            for (int k = 0; k < K; ++k) pw[k] = PE_FMA(d, x[k], pw[k]);
            float* pb = part.data() + (size_t)N * K + j;
            *pb = PE_FMA(d, 1.0f, *pb);
          }
        }
        for (size_t q = 0; q < cnt; ++q) sum[q] += (double)part[q];
      }
      for (size_t q = 0; q < cnt; ++q) a.grads[off + q] = (float)sum[q];
      off += cnt;
    }
  }
  const int64_t P = (int64_t)off;

  const double s_pol = chunk_sum(B, [&](int64_t q) { return (double)tpol[q]; });
  const double s_val = chunk_sum(B, [&](int64_t q) { return (double)tval[q]; });
  const double s_ent = chunk_sum(B, [&](int64_t q) { return (double)tent[q]; });
  const double ss = chunk_sum(P, [&](int64_t q) { return grad_square(a.grads[q]); });
  learner_scalars(s_pol, s_val, s_ent, ss, B, a.h, a.out);
  if (!a.apply) return;

  const float coef = a.out[kOutClipCoef];
  off = 0;
  for (int i = 0; i < 2; ++i) {
    const pe_policy_tower& t = a.tw[i];
    for (int l = 0; l <= t.n_hidden; ++l) {
      const int N = width[i][l], K = l == 0 ? D : width[i][l - 1];
      float* w = const_cast<float*>(t.weight[l]);
      float* b = const_cast<float*>(t.bias[l]);
      for (size_t q = 0; q < (size_t)N * K; ++q) rms_step(a.grads[off + q], coef, a.h, &w[q], &a.sq[off + q]);
      off += (size_t)N * K;
      for (int q = 0; q < N; ++q) rms_step(a.grads[off + q], coef, a.h, &b[q], &a.sq[off + q]);
      off += N;
    }
  }
}

#if defined(__x86_64__) && !defined(__HIP_DEVICE_COMPILE__)
__attribute__((target("avx2,fma"))) void update_hw(const Args& a) { update_body<true>(a); }
bool have_hw_fma() { return __builtin_cpu_supports("fma") && __builtin_cpu_supports("avx2"); }
#else
void update_hw(const Args& a) { update_body<false>(a); }
bool have_hw_fma() { return false; }
#endif

}  // namespace

extern "C" int pe_internal_set_error(int code, const char* msg);
extern "C" int pe_internal_policy_check(int32_t n_towers, const pe_policy_tower* tw, int32_t activation, int with_ptrs);

extern "C" {

int pe_internal_learner_plan(int32_t D, int32_t max_rows, int32_t num_cus, int32_t n_towers,
                             const pe_policy_tower* shapes, int32_t activation, int32_t env_tile,
                             pe_learner_plan_info* out) {
  if (!out) return pe_internal_set_error(PE_ERR_ARG, "null argument");
  LearnerPlan plan;
  if (const int rc = make_learner_plan(D, max_rows, num_cus, n_towers, shapes, activation, env_tile, &plan)) return rc;
  *out = learner_plan_info(plan);
  return PE_OK;
}

int pe_internal_learner_update_host(int32_t rows, int32_t D, int32_t n_towers, const pe_policy_tower* towers,
                                    int32_t activation, const float* obs, const int32_t* actions,
                                    const float* advantages, const float* returns, double learning_rate,
                                    double ent_coef, double vf_coef, double max_grad_norm, double alpha,
                                    double rms_prop_eps, int32_t apply, float* square_avg, float* grads, float* out) {
  if (const int rc = pe_internal_policy_check(n_towers, towers, activation, 1)) return rc;
  if (n_towers != 2) return pe_internal_set_error(PE_ERR_ARG, "the A2C learner needs a two-tower policy (pi and vf)");
  if (rows < 1 || D < 1) return pe_internal_set_error(PE_ERR_ARG, "rows and D must be >= 1");
  if (!obs || !actions || !advantages || !returns || !grads || !out || (apply && !square_avg))
    return pe_internal_set_error(PE_ERR_ARG, "null argument");
  Args a{rows, D, activation, apply, towers, obs, actions, advantages, returns,
         learner_hyper(learning_rate, ent_coef, vf_coef, max_grad_norm, alpha, rms_prop_eps), square_avg, grads, out};
  for (int q = 0; q < kOutWords; ++q) out[q] = 0.0f;
  static const bool hw = have_hw_fma();
  if (hw)
    update_hw(a);
  else
    update_body<false>(a);
  return PE_OK;
}

}  // extern "C"
