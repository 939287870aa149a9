// pe_learner_math.hpp -- the definition of the A2C learner (plantos_amd.A2CLearner): SB3's
// A2C.train() for a two-tower f32 policy -- evaluate_actions, the loss, the backward pass through
// both MLP towers, clip_grad_norm_ and one RMSpropTFLike step.  The host twin
// (pe_learner_host.cpp) and the kernels (pe_learner.hip) include this header; the twin executes
// it literally.  Every operation is one that is correctly rounded and identical on the host and
// on gfx950 (pe_policy_math.hpp): fmaf, f32 add / sub / mul / div / sqrt, f64 add / mul / div,
// comparisons; contraction is off inside every function.
//
// Inputs.  B >= 1 rows: obs [B, D] (f32, or u8 codes decoded through the batch's 256-entry
// table), actions i32 [B], advantages and returns f32 [B]; the policy's parameters in torch
// layout (weight [N, K] row-major, bias [N]), tower 0 = pi (head of A = 2..8 logits), tower 1 =
// vf (head of 1 value); the hyper-parameters ent_coef, vf_coef, max_grad_norm, learning_rate,
// alpha, rms_prop_eps, each given as a double and rounded to f32 once (1 - alpha: the f64
// difference rounded once; 2 vf_coef: the f32 product, exact).
//
// Forward.  pe_policy_forward_host's chains (pe_policy_math.hpp): per layer and neuron one fmaf
// chain from the bias over ascending k, a = pe_tanhf(z) or pe_relu(z); the heads are the same
// chain without an activation: logits l[A] and the value v.  Every hidden activation is kept.
//
// Row quantities (learner_row, learner_value).  With m = max l, z_k = l_k - m, S = the f32 sum
// of pe_expf(z_k) in action order, logS = pe_logf(S):
//   logp = z_a - logS (= policy_logprob(l, A, a)), p_k = pe_expf(z_k) / S, lp_k = z_k - logS,
//   H = -(the fmaf chain from 0 of p_k lp_k in action order);
//   row terms t_pol = adv * logp, t_val = (ret - v)^2, t_ent = H;
//   g_k = ((-adv) (d_ka - p_k) + (ent_coef p_k) (lp_k + H)) / (float)B, every product and sum
//         rounded on its own, in this order;
//   g_v = ((2 vf_coef) (v - ret)) / (float)B.
// g is dZ of tower 0's head, g_v of tower 1's.
//
// Loss.  The three row sums are taken in f64 over the rows in the chunk order of the advantage
// normalisation (pe_rollout_math.hpp: kNormChunk, kNormLanes, the lane tree, chunks ascending).
// policy_loss = (float)(-(sum t_pol / B)), value_loss = (float)(sum t_val / B), entropy_loss =
// (float)(-(sum t_ent / B)), loss = (policy_loss + ent_coef * entropy_loss) + vf_coef *
// value_loss in f32 (loss_total).
//
// Backward data.  For a layer l with dZ_l known, dA_{l-1}[k] = the fmaf chain from +0 over
// ascending j of W_l[j][k] dZ_l[j]; dZ_{l-1}[k] = dA_{l-1}[k] * act_deriv(a_{l-1}[k]) (one f32
// product; tanh: fmaf(-a, a, 1), relu: a > 0 ? 1 : 0).  No gradient is taken to the obs.
//
// Parameter gradients.  dW_l[j][k] = sum over rows of dZ_l[j] a_{l-1}[k] (a_{-1} = the obs) and
// db_l[j] = sum over rows of dZ_l[j] * 1.0f, both as two-level sums: rows are cut into chunks of
// kGradChunk consecutive rows; a chunk's partial is one f32 fmaf chain from +0 over its rows in
// ascending order; the partials are added in ascending chunk order in f64, starting from 0, and
// rounded to f32 once.  kGradChunk is part of this definition: it does not depend on the device,
// its CU count or any tile choice, which change speed and never results.
//
// Clip.  The gradients form one flat vector in the order tower, layer, weight (row-major) then
// bias -- the order of the master parameters.  ss = the f64 sum of (double)g * (double)g over
// that vector in the same kNormChunk order as the loss sums; norm = norm_sqrt_f32(ss), the f32
// nearest to sqrt(ss) (pe_rollout_math.hpp); coef = min(1, max_grad_norm / (norm + 1e-6f))
// (clip_coef; torch's clip_grad_norm_).  Every gradient is multiplied by coef.
//
// Optimizer.  SB3's RMSpropTFLike, momentum 0, not centred, square_avg starting at ones
// (rms_step): gc = g * coef, sq' = fmaf(1 - alpha, gc * gc, alpha * sq), p' = fmaf(-lr, gc /
// sqrtf(sq' + eps), p): epsilon inside the root.
#pragma once
#include "../../include/plantos_batch.h"
#include "pe_rollout_math.hpp"

namespace pe_pol {

constexpr int kGradChunk = 256;  // rows per level-one chain of a parameter gradient

// The six f32 outputs of an update, in this order.
enum { kOutPolicyLoss = 0, kOutValueLoss, kOutEntropyLoss, kOutLoss, kOutGradNorm, kOutClipCoef, kOutWords = 8 };

struct LearnerHyper {
  float ent_coef, vf_coef, two_vf, max_grad_norm, lr, alpha, one_minus_alpha, eps;
};

inline LearnerHyper learner_hyper(double lr, double ent_coef, double vf_coef, double max_grad_norm, double alpha,
                                  double eps) {
  LearnerHyper h;
  h.ent_coef = (float)ent_coef;
  h.vf_coef = (float)vf_coef;
  h.two_vf = 2.0f * h.vf_coef;
  h.max_grad_norm = (float)max_grad_norm;
  h.lr = (float)lr;
  h.alpha = (float)alpha;
  h.one_minus_alpha = (float)(1.0 - alpha);
  h.eps = (float)eps;
  return h;
}

// Tower 0's head of one row: g[0..A) = dZ of the logits, *t_pol = adv * logp, *t_ent = H.
PE_HD void learner_row(const float* l, int A, int a, float adv, float ent_coef, float Bf, float* g, float* t_pol,
                       float* t_ent) {
#pragma clang fp contract(off)
  float m = l[0];
  for (int k = 1; k < A; ++k) m = l[k] > m ? l[k] : m;
  float z[8], e[8];
  float S = 0.0f;
  for (int k = 0; k < A; ++k) {
    z[k] = l[k] - m;
    e[k] = pe_expf(z[k]);
    S = S + e[k];
  }
  const float logS = pe_logf(S);
  float p[8], lp[8];
  float acc = 0.0f, za = 0.0f;
  for (int k = 0; k < A; ++k) {
    p[k] = e[k] / S;
    lp[k] = z[k] - logS;
    acc = fmaf(p[k], lp[k], acc);
    za = k == a ? z[k] : za;
  }
  const float H = -acc;
  const float logp = za - logS;
  const float nadv = -adv;
  for (int k = 0; k < A; ++k) {
    const float d = (k == a ? 1.0f : 0.0f) - p[k];
    const float t1 = nadv * d;
    const float s = lp[k] + H;
    const float t2 = ent_coef * p[k];
    const float t3 = t2 * s;
    const float sum = t1 + t3;
    g[k] = sum / Bf;
  }
  *t_pol = adv * logp;
  *t_ent = H;
}

// Tower 1's head of one row: *g_v = dZ of the value, *t_val = (ret - v)^2.
PE_HD void learner_value(float v, float ret, float two_vf, float Bf, float* g_v, float* t_val) {
#pragma clang fp contract(off)
  const float d = v - ret;
  const float t = two_vf * d;
  *g_v = t / Bf;
  const float r = ret - v;
  *t_val = r * r;
}

// act'(z) from the stored activation a = act(z).
PE_HD float act_deriv(float a, int act) {
#pragma clang fp contract(off)
  return act == PE_ACT_TANH ? fmaf(-a, a, 1.0f) : (a > 0.0f ? 1.0f : 0.0f);
}

PE_HD float loss_total(float policy_loss, float value_loss, float entropy_loss, float ent_coef, float vf_coef) {
#pragma clang fp contract(off)
  const float e = ent_coef * entropy_loss;
  const float u = policy_loss + e;
  const float w = vf_coef * value_loss;
  return u + w;
}

// The loss scalars, the gradient norm and the clip coefficient from the four f64 sums.
PE_HD void learner_scalars(double s_pol, double s_val, double s_ent, double ss, int B, const LearnerHyper& h,
                           float* out) {
#pragma clang fp contract(off)
  const double n = (double)B;
  out[kOutPolicyLoss] = (float)(-(s_pol / n));
  out[kOutValueLoss] = (float)(s_val / n);
  out[kOutEntropyLoss] = (float)(-(s_ent / n));
  out[kOutLoss] = loss_total(out[kOutPolicyLoss], out[kOutValueLoss], out[kOutEntropyLoss], h.ent_coef, h.vf_coef);
  const float norm = norm_sqrt_f32(ss);
  out[kOutGradNorm] = norm;
  const float d = norm + 1e-6f;
  const float c = h.max_grad_norm / d;
  out[kOutClipCoef] = c < 1.0f ? c : 1.0f;  // a NaN norm gives 1
}

PE_HD double grad_square(float g) {
#pragma clang fp contract(off)
  return (double)g * (double)g;
}

// One parameter's clip and RMSpropTFLike step.
PE_HD void rms_step(float g, float coef, const LearnerHyper& h, float* p, float* sq) {
#pragma clang fp contract(off)
  const float gc = g * coef;
  const float g2 = gc * gc;
  const float as = h.alpha * *sq;
  const float s = fmaf(h.one_minus_alpha, g2, as);
  *sq = s;
  const float r = sqrtf(s + h.eps);
  const float q = gc / r;
  *p = fmaf(-h.lr, q, *p);
}

}  // namespace pe_pol
