// pe_learner.hip -- the A2C learner on the device (pe_learner.h; the definition is
// pe_learner_math.hpp, the host twin pe_learner_host.cpp).  One update is these launches on the
// caller's stream:
//   1  pe_learner_fwd_bwd_kernel, one workgroup of 8 waves per tile of E = 32 or 64 rows: the
//      policy's forward (stage_obs / hidden_layer / head_layer of pe_policy_impl.hpp, on
//      v_mfma_f32_32x32x2_f32) with every hidden activation also written row-major to the
//      workspace; per row the head gradients and the three loss terms (VALU); then the backward
//      data layers: the last hidden layer's dA from the <= 8 head rows as VALU chains, the
//      layers below on the same MFMA from a transposed packed copy of the weights (C starts at
//      +0, k-steps ascending j: the definition's chain), dZ = dA * act' applied in the MFMA
//      epilogue in place of the stored activation, and each dZ written row-major;
//   2  pe_learner_wgrad_kernel, a split-K GEMM over (2 32-neuron tiles x group of 4 32-wide input
//      tiles) x (chunk of kGradChunk rows): one wave per workgroup, both operands read straight
//      from the row-major workspace (a lane's A value is dZ[row + lane / 32][j0 + lane % 32], its
//      B values a[row + lane / 32][k0 + lane % 32]: ascending rows = ascending k-steps = the
//      chain), the bias as one more input column of ones; chunk partials go to HBM;
//   3  pe_learner_combine_kernel (the f64 sum of the partials of every parameter),
//      pe_learner_sums_kernel (kNormChunk partial sums of the three loss terms and of g^2) and
//      pe_learner_final_kernel (the scalars, the clip coefficient, the update counter);
//   4  pe_learner_rms_kernel (clip + RMSpropTFLike per parameter) and the repack of the new
//      parameters for this learner's kernels and into the policy (pe_policy_load's kernel).
// Nothing past row rows - 1 of an input or of a workspace array is read or written.
#include <string>

#include "pe_policy_impl.hpp"  // (first: hip_runtime.h before the shared math headers)

#include "pe_learner.h"
#include "pe_learner_math.hpp"
#include "pe_learner_plan.hpp"

struct pe_learner {
  pe_pol::LearnerPlan plan;
  pe_policy* pol;
  pe_learner_bufs b;
};

namespace {

struct LearnArgs {
  const float* packed;
  const float* packed_t;
  const float* tab;
  const void* obs;
  int obs_is_codes;
  int n, D, SD, Kp0, HB, act, max_rows;
  const int32_t* actions;
  const float* adv;
  const float* ret;
  float ent_coef, two_vf, Bf;
  float* ws;
  uint64_t ws_x, ws_act[2][3], ws_dz[2][3], ws_g, ws_gv, ws_terms;
  uint32_t off_wt[2][4];
  Tower tw[2];
};

// The LDS image buf [H][E] of the tile's rows -> g [rows][H] row-major (g: row e0's).
template <int E>
__device__ __forceinline__ void store_rows(const float* buf, int H, float* g, int rows) {
  for (int idx = threadIdx.x; idx < rows * H; idx += kThreads) {
    const int row = idx / H, j = idx - row * H;
    g[idx] = buf[j * E + row];
  }
}

// out[j][e] = (sum_k WT[j][k] in[k][e]) * act'(out[j][e]): hidden_layer with C = +0 and the
// derivative of the activation stored in `out` as the epilogue.
template <int ET>
__device__ __forceinline__ void backward_layer(const float* __restrict__ wp, const float* in, float* out, int KG,
                                               int NT, int act) {
#pragma clang fp contract(off)
  constexpr int E = 32 * ET;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, col = lane & 31, half = lane >> 5;
  for (int jt = wave; jt < NT; jt += kWaves) {
    f32x16 acc[ET];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
#pragma unroll
      for (int et = 0; et < ET; ++et) acc[et][r] = 0.0f;
    }
    const float4* w4 = reinterpret_cast<const float4*>(wp) + (size_t)jt * KG * 64 + lane;
    const float* xin = in + half * E + col;
    float4 w = w4[0];
    for (int kg = 0; kg < KG; ++kg) {
      const float4 wn = w4[(size_t)min(kg + 1, KG - 1) * 64];
      const float* x = xin + kg * 8 * E;
      const float wq[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
      for (int q = 0; q < 4; ++q) {
#pragma unroll
        for (int et = 0; et < ET; ++et)
          acc[et] = __builtin_amdgcn_mfma_f32_32x32x2f32(wq[q], x[q * 2 * E + et * 32], acc[et], 0, 0, 0);
      }
      w = wn;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int j = jt * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
#pragma unroll
      for (int et = 0; et < ET; ++et) {
        float* o = out + j * E + et * 32 + col;
        *o = acc[et][r] * act_deriv(*o, act);
      }
    }
  }
}

template <int ET>
__global__ __launch_bounds__(kThreads) void pe_learner_fwd_bwd_kernel(LearnArgs a) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int E = 32 * ET;
  float* tab = lds;                    // the forward kernel's images
  float* hd = tab + 256;               // [kHeadRows][E]: logits / value, then their gradients
  float* xT = hd + kHeadRows * E;      // [Kp0][E]
  float* h0 = xT + a.Kp0 * E;          // [HB][E] (first the staging image [E][SD])
  float* h1 = h0 + a.HB * E;           // [HB][E]
  const int tid = threadIdx.x;
  const int64_t e0 = (int64_t)blockIdx.x * E;
  const int rows = (int)min((int64_t)E, (int64_t)a.n - e0);
  const int64_t R = a.max_rows;

  stage_obs<E>(a.obs, a.obs_is_codes, a.tab, tab, h0, xT, e0, rows, a.D, a.SD, a.Kp0);
  {  // the obs rows as f32, for layer 0's weight gradient (h0 still holds the staging image)
    float* X = a.ws + a.ws_x + e0 * a.D;
    for (int i = tid; i < rows * a.D; i += kThreads) {
      const int row = i / a.D;
      X[i] = h0[row * a.SD + (i - row * a.D)];
    }
  }
  __syncthreads();

  for (int ti = 0; ti < 2; ++ti) {
    const Tower& tw = a.tw[ti];
    const int nh = tw.n_hidden;
    float* cur = xT;
    for (int l = 0; l < nh; ++l) {
      const Layer& L = tw.l[l];
      float* out = (l & 1) ? h1 : h0;
      hidden_layer<ET, float>(a.packed + L.off_w, a.packed + L.off_b, cur, out, L.Kp >> 3, L.N >> 5, a.act);
      __syncthreads();
      store_rows<E>(out, L.N, a.ws + a.ws_act[ti][l] + e0 * L.N, rows);
      cur = out;
    }
    const Layer& LH = tw.l[nh];
    head_layer<E>(a.packed, LH, tw.n_out, ti, cur, hd);
    __syncthreads();

    // the head's gradient per row, into the head rows it was read from
    if (tid < E) {
      if (tid < rows) {
        const int64_t e = e0 + tid;
        if (ti == 0) {
          const int A = tw.n_out;
          float l[8], g[8], t_pol, t_ent;
          for (int k = 0; k < A; ++k) l[k] = hd[k * E + tid];
          learner_row(l, A, a.actions[e], a.adv[e], a.ent_coef, a.Bf, g, &t_pol, &t_ent);
          for (int k = 0; k < A; ++k) {
            hd[k * E + tid] = g[k];
            a.ws[a.ws_g + e * A + k] = g[k];
          }
          a.ws[a.ws_terms + e] = t_pol;
          a.ws[a.ws_terms + 2 * R + e] = t_ent;
        } else {
          float g_v, t_val;
          learner_value(hd[(kHeadRows - 1) * E + tid], a.ret[e], a.two_vf, a.Bf, &g_v, &t_val);
          hd[(kHeadRows - 1) * E + tid] = g_v;
          a.ws[a.ws_gv + e] = g_v;
          a.ws[a.ws_terms + R + e] = t_val;
        }
      } else {  // a row past the end contributes nothing
        for (int k = 0; k < kHeadRows; ++k) hd[k * E + tid] = 0.0f;
      }
    }
    __syncthreads();

    // backward data, last hidden layer: dA from the head rows (VALU chains over ascending j)
    {
      const int K = LH.K, no = tw.n_out;
      const float* w = a.packed + LH.off_w;
      for (int idx = tid; idx < K * E; idx += kThreads) {
        const int k = idx / E, e = idx - k * E;
        float acc = 0.0f;
        for (int j = 0; j < no; ++j) acc = fmaf(w[j * K + k], hd[(ti == 0 ? j : kHeadRows - 1) * E + e], acc);
        cur[idx] = acc * act_deriv(cur[idx], a.act);
      }
      __syncthreads();
      store_rows<E>(cur, K, a.ws + a.ws_dz[ti][nh - 1] + e0 * K, rows);
    }
    // ... and the layers below on the MFMA: dZ_l (cur) -> dZ_{l-1} (the other buffer, which
    // holds a_{l-1} unless a_{l+1} has overwritten it: then it is read back from the workspace)
    for (int l = nh - 1; l >= 1; --l) {
      const Layer& L = tw.l[l];  // K = width of layer l - 1, N = width of layer l
      float* other = cur == h0 ? h1 : h0;
      if (l + 1 <= nh - 1) {
        __syncthreads();  // the stores of dZ_{l+1} have read `other`
        const float* src = a.ws + a.ws_act[ti][l - 1] + e0 * L.K;
        for (int idx = tid; idx < E * L.K; idx += kThreads) {
          const int row = idx / L.K, j = idx - row * L.K;
          other[j * E + row] = row < rows ? src[idx] : 0.0f;
        }
        __syncthreads();
      }
      backward_layer<ET>(a.packed_t + a.off_wt[ti][l], cur, other, L.N >> 3, L.K >> 5, a.act);
      __syncthreads();
      store_rows<E>(other, L.K, a.ws + a.ws_dz[ti][l - 1] + e0 * L.K, rows);
      cur = other;
    }
    __syncthreads();  // the next tower overwrites h0 / h1 and the head rows
  }
}

// ---------------------------------------------------------------- weight gradients
struct WgradArgs {
  const float* ws;
  float* partials;
  uint64_t n_params;
  int rows, n_layers;
  WgradLayer L[8];
};

__global__ __launch_bounds__(64) void pe_learner_wgrad_kernel(WgradArgs a) {
  const int lane = threadIdx.x, col = lane & 31, half = lane >> 5;
  const int g = blockIdx.x, chunk = blockIdx.y;
  int li = 0;
  for (int q = 1; q < a.n_layers; ++q) li = g >= a.L[q].first_group ? q : li;
  const WgradLayer& L = a.L[li];
  const int lg = g - L.first_group, jg = lg / L.KG, kq = lg - jg * L.KG;
  const int N = L.N, K = L.K;
  const int KT = (K + 1 + 31) >> 5, NT = (N + 31) >> 5;
  const int nt = min(kWgradTiles, KT - kq * kWgradTiles);  // wave-uniform
  const int nj = min(kWgradRows, NT - jg * kWgradRows);    // wave-uniform
  const float* dz = a.ws + L.ws_dz;
  const float* in = a.ws + L.ws_in;
  int jj[kWgradRows], kk[kWgradTiles];
#pragma unroll
  for (int u = 0; u < kWgradRows; ++u) jj[u] = (jg * kWgradRows + u) * 32 + col;
#pragma unroll
  for (int t = 0; t < kWgradTiles; ++t) kk[t] = (kq * kWgradTiles + t) * 32 + col;
  f32x16 acc[kWgradRows][kWgradTiles];
#pragma unroll
  for (int u = 0; u < kWgradRows; ++u)
#pragma unroll
    for (int t = 0; t < kWgradTiles; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[u][t][r] = 0.0f;
  const int c0 = chunk * kGradChunk, c1 = min(a.rows, c0 + kGradChunk);
  for (int r0 = c0; r0 < c1; r0 += 2) {
    const int r = r0 + half;
    const bool rv = r < c1;  // an odd chunk's last k-step: zeros
    float av[kWgradRows], bv[kWgradTiles];
#pragma unroll
    for (int u = 0; u < kWgradRows; ++u) av[u] = (rv && u < nj && jj[u] < N) ? dz[(size_t)r * L.ldz + jj[u]] : 0.0f;
#pragma unroll
    for (int t = 0; t < kWgradTiles; ++t) {
      bv[t] = 0.0f;
      if (rv && t < nt) bv[t] = kk[t] < K ? in[(size_t)r * L.lda + kk[t]] : (kk[t] == K ? 1.0f : 0.0f);
    }
#pragma unroll
    for (int u = 0; u < kWgradRows; ++u) {
      if (u < nj) {
#pragma unroll
        for (int t = 0; t < kWgradTiles; ++t)
          if (t < nt) acc[u][t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], bv[t], acc[u][t], 0, 0, 0);
      }
    }
  }
  float* part = a.partials + (size_t)chunk * a.n_params;
#pragma unroll
  for (int u = 0; u < kWgradRows; ++u) {
    if (u < nj) {
#pragma unroll
      for (int t = 0; t < kWgradTiles; ++t) {
        if (t < nt) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int j = (jg * kWgradRows + u) * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
            if (j < N) {
              if (kk[t] < K)
                part[L.off_w + (size_t)j * K + kk[t]] = acc[u][t][r];
              else if (kk[t] == K)
                part[L.off_b + j] = acc[u][t][r];
            }
          }
        }
      }
    }
  }
}

// grads[p] = the f64 sum of p's chunk partials in ascending chunk order, rounded once.
__global__ __launch_bounds__(256) void pe_learner_combine_kernel(const float* partials, float* grads, uint64_t P,
                                                                 int nch) {
  const uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (p >= P) return;
  double s = 0.0;
  for (int c = 0; c < nch; ++c) s += (double)partials[(size_t)c * P + p];
  grads[p] = (float)s;
}

struct SumArgs {
  const float* terms;  // [3][max_rows]
  const float* grads;
  double* sums;        // [4][sum_chunks]
  float* out;
  int64_t* n_updates;
  int64_t max_rows, rows, P;
  int sum_chunks;
  LearnerHyper h;
};

// Chunk blockIdx.x of quantity blockIdx.y (the three row terms, g^2) in the order of
// pe_rollout_math.hpp: lane l adds its elements in ascending order, then the tree.
__global__ __launch_bounds__(kNormLanes) void pe_learner_sums_kernel(SumArgs a) {
  __shared__ double s[kNormLanes];
  const int q = blockIdx.y, l = threadIdx.x;
  const int64_t N = q < 3 ? a.rows : a.P;
  const int64_t base = (int64_t)blockIdx.x * kNormChunk;
  if (base >= N) return;  // uniform
  const int64_t len = min((int64_t)kNormChunk, N - base);
  const float* src = q < 3 ? a.terms + q * a.max_rows : a.grads;
  double acc = 0.0;
  for (int u = 0; u < kNormChunk / kNormLanes; ++u) {
    const int64_t i = (int64_t)l + u * kNormLanes;
    if (i < len) {
      const float v = src[base + i];
      acc += q < 3 ? (double)v : grad_square(v);
    }
  }
  s[l] = acc;
  __syncthreads();
  for (int h = kNormLanes / 2; h >= 1; h /= 2) {
    if (l < h) s[l] += s[l + h];
    __syncthreads();
  }
  if (l == 0) a.sums[(size_t)q * a.sum_chunks + blockIdx.x] = s[0];
}

__global__ __launch_bounds__(64) void pe_learner_final_kernel(SumArgs a) {
  if (threadIdx.x != 0) return;
  double t[4];
  for (int q = 0; q < 4; ++q) {
    const int64_t N = q < 3 ? a.rows : a.P;
    const int nch = (int)((N + kNormChunk - 1) / kNormChunk);
    double s = 0.0;
    for (int c = 0; c < nch; ++c) s += a.sums[(size_t)q * a.sum_chunks + c];
    t[q] = s;
  }
  learner_scalars(t[0], t[1], t[2], t[3], (int)a.rows, a.h, a.out);
  *a.n_updates += 1;
}

__global__ __launch_bounds__(256) void pe_learner_rms_kernel(const float* grads, const float* out, float* params,
                                                             float* sq, uint64_t P, LearnerHyper h) {
  const uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (p >= P) return;
  float w = params[p], s = sq[p];
  rms_step(grads[p], out[kOutClipCoef], h, &w, &s);
  params[p] = w;
  sq[p] = s;
}

// The transposed packed weights of the backward-data layers: hidden_layer's format of W^T
// (rows = the layer's inputs k < K, summed index = its neurons j < N; both multiples of 32).
struct PackTLayer {
  const float* w;
  int N, K;
  uint32_t off, n_w;
};
struct PackTArgs {
  float* packed;
  PackTLayer l[4];
};
__global__ __launch_bounds__(256) void pe_learner_pack_t_kernel(PackTArgs a) {
  const PackTLayer& L = a.l[blockIdx.y];
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= L.n_w) return;
  const uint32_t q = i & 3u, lane = (i >> 2) & 63u, blk = i >> 8, KG = (uint32_t)L.N >> 3;
  const uint32_t kg = blk % KG, jt = blk / KG;
  const uint32_t row = jt * 32u + (lane & 31u), k = kg * 8u + q * 2u + (lane >> 5);  // W^T[row][k] = W[k][row]
  a.packed[L.off + i] = L.w[(size_t)k * L.K + row];
}

const TileKernel kFwdBwd(pe_learner_fwd_bwd_kernel<1>, pe_learner_fwd_bwd_kernel<2>);

int launched(const char* what) {
  const hipError_t le = hipGetLastError();
  return le == hipSuccess ? PE_OK : hip_fail(le, what);
}

// The master parameters as a pe_policy_tower array (device pointers into bufs->params).
void master_towers(const pe_learner* l, pe_policy_tower* tw) {
  for (int i = 0; i < 2; ++i) {
    const Tower& t = l->plan.pol.tw[i];
    tw[i] = pe_policy_tower{};
    tw[i].n_hidden = t.n_hidden;
    tw[i].n_out = t.n_out;
    for (int q = 0; q <= t.n_hidden; ++q) {
      if (q < t.n_hidden) tw[i].hidden[q] = t.l[q].N;
      tw[i].weight[q] = l->b.params + l->plan.poff_w[i][q];
      tw[i].bias[q] = l->b.params + l->plan.poff_b[i][q];
    }
  }
}

}  // namespace

extern "C" {

int pe_internal_learner_create(pe_policy* policy, int32_t max_rows, const pe_learner_bufs* bufs, pe_learner** out) {
  if (!policy || !bufs || !out) return fail(PE_ERR_ARG, "null argument");
  if (policy->H) return fail(PE_ERR_ARG, "the A2C learner does not train a recurrent policy");
  if (policy->precision != PE_PREC_F32) return fail(PE_ERR_ARG, "the A2C learner trains f32 policies only (not bf16)");
  if (policy->n_towers != 2) return fail(PE_ERR_ARG, "the A2C learner needs a two-tower policy (pi and vf)");
  if (!bufs->params || !bufs->grads || !bufs->square_avg || !bufs->out || !bufs->n_updates || !bufs->ws ||
      !bufs->partials || !bufs->sums || !bufs->packed || !bufs->packed_t)
    return fail(PE_ERR_ARG, "null buffer");
  pe_policy_tower shapes[2] = {};
  for (int i = 0; i < 2; ++i) {
    shapes[i].n_hidden = policy->tw[i].n_hidden;
    shapes[i].n_out = policy->tw[i].n_out;
    for (int q = 0; q < policy->tw[i].n_hidden; ++q) shapes[i].hidden[q] = policy->tw[i].l[q].N;
  }
  LearnerPlan plan;
  if (const int rc = make_learner_plan(policy->D, max_rows, policy->h->num_cus, 2, shapes, policy->act,
                                       policy->env_tile, &plan))
    return rc;
  if (plan.pol.n_packed != policy->n_packed || plan.pol.lds != policy->lds)
    return fail(PE_ERR_ARG, "the learner's plan differs from the policy's");
  DeviceGuard dg(policy->h);
  if (dg.rc) return dg.rc;
  const hipError_t e =
      hipFuncSetAttribute(kFwdBwd.of(plan.pol), hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.pol.lds);
  if (e != hipSuccess) return hip_fail(e, "pe_internal_learner_create");
  pe_learner* l = new (std::nothrow) pe_learner{plan, policy, *bufs};
  if (!l) return fail(PE_ERR_NOMEM, "host allocation failed");
  *out = l;
  return PE_OK;
}

int pe_internal_learner_destroy(pe_learner* l) {
  delete l;
  return PE_OK;
}

int pe_internal_learner_repack(pe_learner* l, void* stream) {
  if (!l) return fail(PE_ERR_ARG, "null argument");
  pe_policy_tower tw[2];
  master_towers(l, tw);
  PackArgs a;
  int nl = 0;
  uint32_t most = 0;
  if (const int rc = pack_towers(l->pol, tw, &a, &nl, &most)) return rc;
  DeviceGuard dg(l->pol->h);
  if (dg.rc) return dg.rc;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(pe_policy_pack_kernel, dim3((most + 255) / 256, (unsigned)nl), dim3(256), 0, st, a);  // the policy's
  a.packed = l->b.packed;
  hipLaunchKernelGGL(pe_policy_pack_kernel, dim3((most + 255) / 256, (unsigned)nl), dim3(256), 0, st, a);
  PackTArgs pt{};
  pt.packed = l->b.packed_t;
  int nt = 0;
  uint32_t most_t = 0;
  for (int i = 0; i < 2; ++i)
    for (int q = 1; q < l->plan.pol.tw[i].n_hidden; ++q) {
      const Layer& L = l->plan.pol.tw[i].l[q];
      pt.l[nt++] = PackTLayer{tw[i].weight[q], L.N, L.K, l->plan.off_wt[i][q], (uint32_t)(L.N * L.K)};
      most_t = most_t > (uint32_t)(L.N * L.K) ? most_t : (uint32_t)(L.N * L.K);
    }
  if (nt) hipLaunchKernelGGL(pe_learner_pack_t_kernel, dim3((most_t + 255) / 256, (unsigned)nt), dim3(256), 0, st, pt);
  return launched("pe_internal_learner_repack");
}

int pe_internal_learner_update(pe_learner* l, int32_t rows, const void* obs, int32_t obs_is_codes,
                               const int32_t* actions, const float* advantages, const float* returns,
                               double learning_rate, double ent_coef, double vf_coef, double max_grad_norm,
                               double alpha, double rms_prop_eps, void* stream) {
  if (!l || !obs || !actions || !advantages || !returns) return fail(PE_ERR_ARG, "null argument");
  const LearnerPlan& P = l->plan;
  if (rows < 1 || rows > P.max_rows)
    return fail(PE_ERR_ARG, "rows must be in 1.." + std::to_string(P.max_rows) + " (max_rows), got " + std::to_string(rows));
  if (obs_is_codes != 0 && obs_is_codes != 1) return fail(PE_ERR_ARG, "obs_is_codes must be 0 or 1");
  if (obs_is_codes && !l->pol->h->obs_codes) return fail(PE_ERR_ARG, "obs_is_codes = 1 needs a handle created with obs_codes");
  const LearnerHyper h = learner_hyper(learning_rate, ent_coef, vf_coef, max_grad_norm, alpha, rms_prop_eps);
  const hipStream_t st = static_cast<hipStream_t>(stream);

  LearnArgs a{};
  a.packed = l->b.packed;
  a.packed_t = l->b.packed_t;
  a.tab = l->pol->mem + l->pol->n_packed;
  a.obs = obs;
  a.obs_is_codes = obs_is_codes;
  a.n = rows;
  a.D = P.pol.D;
  a.SD = P.pol.SD;
  a.Kp0 = P.pol.Kp0;
  a.HB = P.pol.HB;
  a.act = P.pol.act;
  a.max_rows = P.max_rows;
  a.actions = actions;
  a.adv = advantages;
  a.ret = returns;
  a.ent_coef = h.ent_coef;
  a.two_vf = h.two_vf;
  a.Bf = (float)rows;
  a.ws = l->b.ws;
  a.ws_x = P.ws_x;
  a.ws_g = P.ws_g;
  a.ws_gv = P.ws_gv;
  a.ws_terms = P.ws_terms;
  for (int i = 0; i < 2; ++i) {
    a.tw[i] = P.pol.tw[i];
    for (int q = 0; q < 3; ++q) {
      a.ws_act[i][q] = P.ws_act[i][q];
      a.ws_dz[i][q] = P.ws_dz[i][q];
    }
    for (int q = 0; q < 4; ++q) a.off_wt[i][q] = P.off_wt[i][q];
  }
  if (const int rc = kFwdBwd.launch(l->pol, rows, stream, "pe_internal_learner_update", a)) return rc;

  DeviceGuard dg(l->pol->h);
  if (dg.rc) return dg.rc;
  const int nch = (rows + kGradChunk - 1) / kGradChunk;
  WgradArgs w{};
  w.ws = l->b.ws;
  w.partials = l->b.partials;
  w.n_params = P.n_params;
  w.rows = rows;
  w.n_layers = P.n_layers;
  for (int q = 0; q < P.n_layers; ++q) w.L[q] = P.L[q];
  hipLaunchKernelGGL(pe_learner_wgrad_kernel, dim3((unsigned)P.wgrad_groups, (unsigned)nch), dim3(64), 0, st, w);
  const unsigned pb = (unsigned)((P.n_params + 255) / 256);
  hipLaunchKernelGGL(pe_learner_combine_kernel, dim3(pb), dim3(256), 0, st, l->b.partials, l->b.grads, P.n_params, nch);
  SumArgs s{l->b.ws + P.ws_terms, l->b.grads, l->b.sums, l->b.out, l->b.n_updates, P.max_rows, rows,
            (int64_t)P.n_params, P.sum_chunks, h};
  const int64_t longer = rows > (int64_t)P.n_params ? rows : (int64_t)P.n_params;
  hipLaunchKernelGGL(pe_learner_sums_kernel, dim3((unsigned)((longer + kNormChunk - 1) / kNormChunk), 4),
                     dim3(kNormLanes), 0, st, s);
  hipLaunchKernelGGL(pe_learner_final_kernel, dim3(1), dim3(64), 0, st, s);
  hipLaunchKernelGGL(pe_learner_rms_kernel, dim3(pb), dim3(256), 0, st, l->b.grads, l->b.out, l->b.params,
                     l->b.square_avg, P.n_params, h);
  if (const int rc = launched("pe_internal_learner_update")) return rc;
  return pe_internal_learner_repack(l, stream);
}

}  // extern "C"
