// pe_policy_bf16.hip -- the PE_PREC_BF16 side of the MLP policy (include/plantos_batch.h,
// "Reduced-precision policy inference"): what pe_policy_create_prec / _load / _forward /
// _forward_rows / _value run for a bf16 policy.  pe_policy.hip keeps the entry points and their
// argument checks and calls the pe_internal_policy_bf16_* functions below; the f32 kernels are
// not part of this translation unit.  The plan is pe_policy_plan.hpp's make_policy_plan_prec,
// the host twin pe_policy_forward_host_bf16 (pe_policy_host.cpp).
//
// One fused kernel per forward, one workgroup of 8 waves per tile of E = 32 or 64 envs:
//   0  a thread converts the 8 obs values of one (env, k group of 8) -- byte codes through the
//      256-entry code table in LDS, or f32 -- to bf16 and writes them as one 16-byte LDS store
//      into the obs image x [k group][env][8]; rows of envs past n and k >= D are zero;
//   1  every hidden layer runs on v_mfma_f32_32x32x16_bf16: A = the weights (row = neuron; one
//      16-byte global load per lane and k step of 16 from the packed buffer), B = the activations
//      (column = env; one ds_read_b128 per lane and k step), C starts as the bias.  A wave owns
//      32-neuron tiles (x all env tiles).  The activation is applied to the f32 accumulators,
//      the result rounded to bf16 and written into the other of two images [k group][env][8]:
//      registers 4g..4g+3 of a lane are 4 consecutive neurons, one 8-byte LDS store;
//   2  the heads are pe_policy.hip's VALU fmaf chains in k order over the last image, its bf16
//      values widened to f32;
//   3  act_and_store of pe_policy_impl.hpp.
// No static LDS, no scratch.  Nothing past row n - 1 of obs or of an output is read or written.
#include <string>

#include "pe_policy_impl.hpp"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

struct BfArgs {
  const float* packed;
  const float* tab;  // f32[256] code table
  const void* obs;
  int obs_is_codes;
  int n, D, Kp0, HB;  // Kp0 = D padded to 16, HB = rows of an activation image
  int n_towers, act, mode;
  uint64_t seed;
  uint32_t env_off, t;
  int32_t* actions;
  float* head0;
  float* head1;
  Tower tw[2];
};

// Packed hidden weights: bf16 [neuron tile jt][k step ks][lane][q], element = W[jt*32 + (lane & 31)]
// [ks*16 + 8 (lane >> 5) + q] rounded to nearest even (0 for k >= K).  Head weights and all
// biases are copied as f32.
__global__ __launch_bounds__(256) void pe_policy_bf16_pack_kernel(PackArgs a) {
  const PackLayer& L = a.l[blockIdx.y];
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < L.n_w) {
    if (L.head) {
      a.packed[L.off_w + i] = L.w[i];
    } else {
      const uint32_t q = i & 7u, lane = (i >> 3) & 63u, blk = i >> 9, KS = (uint32_t)L.Kp >> 4;
      const uint32_t ks = blk % KS, jt = blk / KS;
      const uint32_t j = jt * 32u + (lane & 31u), k = ks * 16u + 8u * (lane >> 5) + q;
      const float v = k < (uint32_t)L.K ? L.w[(size_t)j * L.K + k] : 0.0f;
      reinterpret_cast<__bf16*>(a.packed + L.off_w)[i] = (__bf16)v;
    }
  } else if (i < L.n_w + (uint32_t)L.N) {
    a.packed[L.off_b + (i - L.n_w)] = L.b[i - L.n_w];
  }
}

// The tile's obs rows -> x [k group][env][8] in bf16: k >= D and rows of envs past `rows` zero.
// Ends with a barrier.
template <int E>
__device__ __forceinline__ void stage_obs_bf16(const void* obs, int obs_is_codes, const float* tab_g, float* tab,
                                               bf16x8* x, int64_t e0, int rows, int D, int Kp0) {
  const int tid = threadIdx.x;
  if (obs_is_codes) {
    if (tid < 256) tab[tid] = tab_g[tid];
    __syncthreads();
  }
  const int KG = Kp0 >> 3;
  for (int idx = tid; idx < KG * E; idx += kThreads) {
    const int e = idx / KG, kg = idx - e * KG;  // consecutive lanes read consecutive memory
    bf16x8 v;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int k = kg * 8 + q;
      float f = 0.0f;
      if (e < rows && k < D) {
        const int64_t at = (e0 + e) * D + k;
        f = obs_is_codes ? tab[static_cast<const uint8_t*>(obs)[at]] : static_cast<const float*>(obs)[at];
      }
      v[q] = (__bf16)f;
    }
    x[kg * E + e] = v;
  }
  __syncthreads();
}

// out[j][e] = bf16(act(b_j + sum_k W[j][k] in[k][e])) for the tile's E = 32 * ET envs; in / out
// are LDS images [k group of 8][E][8]; KS k steps of 16, NT neuron tiles of 32.
template <int ET>
__device__ __forceinline__ void hidden_layer_bf16(const float* __restrict__ wp, const float* __restrict__ bias,
                                                  const bf16x8* in, bf16x8* out, int KS, int NT, int act) {
  constexpr int E = 32 * ET;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, col = lane & 31, half = lane >> 5;
  for (int jt = wave; jt < NT; jt += kWaves) {
    f32x16 acc[ET];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float b = bias[jt * 32 + (r & 3) + 8 * (r >> 2) + 4 * half];
#pragma unroll
      for (int et = 0; et < ET; ++et) acc[et][r] = b;
    }
    const bf16x8* w8 = reinterpret_cast<const bf16x8*>(wp) + (size_t)jt * KS * 64 + lane;
    const bf16x8* xin = in + half * E + col;  // k group 2 ks + half of step ks
    bf16x8 w = w8[0];
    for (int ks = 0; ks < KS; ++ks) {
      const bf16x8 wn = w8[(size_t)min(ks + 1, KS - 1) * 64];  // the next step's, in flight over the MFMAs
      const bf16x8* x = xin + ks * 2 * E;
#pragma unroll
      for (int et = 0; et < ET; ++et) acc[et] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w, x[et * 32], acc[et], 0, 0, 0);
      w = wn;
    }
    // registers 4g..4g+3: neurons jt*32 + 8g + 4 half + 0..3 = elements 4 half.. of k group jt*4 + g
#pragma unroll
    for (int g = 0; g < 4; ++g) {
#pragma unroll
      for (int et = 0; et < ET; ++et) {
        bf16x4 v;
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = (__bf16)activate(acc[et][4 * g + q], act);
        reinterpret_cast<bf16x4*>(out + (jt * 4 + g) * E + et * 32 + col)[half] = v;
      }
    }
  }
}

// head_layer of pe_policy_impl.hpp over a bf16 image `in` [K / 8][E][8]: the same fmaf chain in
// k order, each activation widened to f32.
template <int E>
__device__ __forceinline__ void head_layer_bf16(const float* packed, const Layer& H, int n_out, int ti,
                                                const bf16x8* in, float* hd) {
  for (int idx = threadIdx.x; idx < n_out * E; idx += kThreads) {
    const int o = idx / E, e = idx - o * E;
    const float* w = packed + H.off_w + (size_t)o * H.K;
    float acc = packed[H.off_b + o];
    for (int kg = 0; kg < (H.K >> 3); ++kg) {
      const bf16x8 v = in[kg * E + e];
#pragma unroll
      for (int q = 0; q < 8; ++q) acc = fmaf(w[kg * 8 + q], (float)v[q], acc);
    }
    hd[(ti == 0 ? o : kHeadRows - 1) * E + e] = acc;
  }
}

// Tower ti of the policy from x into its head row(s) of hd.  Ends with a barrier.
template <int ET>
__device__ __forceinline__ void tower_bf16(const BfArgs& a, int ti, const bf16x8* x, bf16x8* h0, bf16x8* h1, float* hd) {
  constexpr int E = 32 * ET;
  const Tower& tw = a.tw[ti];
  const bf16x8* in = x;
  for (int l = 0; l < tw.n_hidden; ++l) {
    const Layer& L = tw.l[l];
    bf16x8* out = (l & 1) ? h1 : h0;
    hidden_layer_bf16<ET>(a.packed + L.off_w, a.packed + L.off_b, in, out, L.Kp >> 4, L.N >> 5, a.act);
    __syncthreads();
    in = out;
  }
  head_layer_bf16<E>(a.packed, tw.l[tw.n_hidden], tw.n_out, ti, in, hd);
  __syncthreads();  // the next tower overwrites h0 / h1; the epilogue reads hd
}

template <int ET>
__global__ __launch_bounds__(kThreads) void pe_policy_bf16_forward_kernel(BfArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int E = 32 * ET;
  float* tab = lds;                                          // [256]
  float* hd = tab + 256;                                     // [kHeadRows][E]
  bf16x8* x = reinterpret_cast<bf16x8*>(hd + kHeadRows * E);  // [Kp0 / 8][E]
  bf16x8* h0 = x + (a.Kp0 >> 3) * E;                         // [HB / 8][E]
  bf16x8* h1 = h0 + (a.HB >> 3) * E;                         // [HB / 8][E]
  const int64_t e0 = (int64_t)blockIdx.x * E;
  const int rows = (int)min((int64_t)E, (int64_t)a.n - e0);

  stage_obs_bf16<E>(a.obs, a.obs_is_codes, a.tab, tab, x, e0, rows, a.D, a.Kp0);
  for (int ti = 0; ti < a.n_towers; ++ti) tower_bf16<ET>(a, ti, x, h0, h1, hd);
  act_and_store<E>(hd, a.tw[0].n_out, rows, e0, a.mode, a.seed, a.env_off, a.t, a.actions, a.head0, a.head1);
}

// pe_policy_value for a bf16 policy: tower 1 alone and values[e] of the selected envs; a
// workgroup none of whose envs is selected returns before it reads obs.
template <int ET>
__global__ __launch_bounds__(kThreads) void pe_policy_bf16_value_kernel(BfArgs a, ValueSel s) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int E = 32 * ET;
  float* tab = lds;  // the forward kernel's images
  float* hd = tab + 256;
  bf16x8* x = reinterpret_cast<bf16x8*>(hd + kHeadRows * E);
  bf16x8* h0 = x + (a.Kp0 >> 3) * E;
  bf16x8* h1 = h0 + (a.HB >> 3) * E;
  const int64_t e0 = (int64_t)blockIdx.x * E;
  const int rows = (int)min((int64_t)E, (int64_t)a.n - e0);

  const bool sel = selected(s, e0, rows);
  if (!block_any(sel, hd)) return;  // uniform: every thread of the workgroup leaves, before any other barrier

  stage_obs_bf16<E>(a.obs, a.obs_is_codes, a.tab, tab, x, e0, rows, a.D, a.Kp0);
  tower_bf16<ET>(a, 1, x, h0, h1, hd);
  store_values<E>(hd, sel, e0, s.values);
}

// ---------------------------------------------------------------- host side
const TileKernel kForward(pe_policy_bf16_forward_kernel<1>, pe_policy_bf16_forward_kernel<2>);
const TileKernel kValue(pe_policy_bf16_value_kernel<1>, pe_policy_bf16_value_kernel<2>);

// What every launch of p reads; the sampler and output fields are left zero.
BfArgs bf_args(const pe_policy* p, const void* obs, int32_t obs_is_codes) {
  BfArgs a{};
  a.packed = p->mem;
  a.tab = p->mem + p->n_packed;
  a.obs = obs;
  a.obs_is_codes = obs_is_codes;
  a.n = p->h->n;
  a.D = p->D;
  a.Kp0 = p->Kp0;
  a.HB = p->HB;
  a.n_towers = p->n_towers;
  a.act = p->act;
  a.env_off = p->h->cfg.env_id_offset;
  a.tw[0] = p->tw[0];
  a.tw[1] = p->tw[p->n_towers - 1];
  return a;
}

}  // namespace

// The calls of pe_policy.hip for a PE_PREC_BF16 policy; the arguments are checked there.
extern "C" {

int pe_internal_policy_bf16_create(pe_handle* h, const PolicyPlan* plan, pe_policy** out) {
  return create_policy(h, *plan, {kForward.of(*plan), plan->n_towers == 2 ? kValue.of(*plan) : nullptr},
                       "pe_policy_create_prec", out);
}

int pe_internal_policy_bf16_load(pe_policy* p, const pe_policy_tower* towers, void* stream) {
  PackArgs a;
  int nl = 0;
  uint32_t most = 0;
  if (const int rc = pack_towers(p, towers, &a, &nl, &most)) return rc;
  DeviceGuard dg(p->h);
  if (dg.rc) return dg.rc;
  hipLaunchKernelGGL(pe_policy_bf16_pack_kernel, dim3((most + 255) / 256, (unsigned)nl), dim3(256), 0,
                     static_cast<hipStream_t>(stream), a);
  const hipError_t le = hipGetLastError();
  return le == hipSuccess ? PE_OK : hip_fail(le, "pe_policy_load");
}

int pe_internal_policy_bf16_forward(pe_policy* p, int32_t rows, const void* obs, int32_t obs_is_codes, int32_t mode,
                                    uint64_t seed, uint32_t t, int32_t* actions, float* head0, float* head1,
                                    void* stream, const char* what) {
  BfArgs a = bf_args(p, obs, obs_is_codes);
  a.n = rows;  // the kernel bounds its last tile, its loads and its stores by a.n
  a.mode = mode;
  a.seed = seed;
  a.t = t;
  a.actions = actions;
  a.head0 = head0;
  a.head1 = head1;
  return kForward.launch(p, rows, stream, what, a);
}

int pe_internal_policy_bf16_value(pe_policy* p, const void* obs, int32_t obs_is_codes, const uint8_t* want,
                                  const uint8_t* unless, float* values, void* stream) {
  const BfArgs a = bf_args(p, obs, obs_is_codes);
  return kValue.launch(p, a.n, stream, "pe_policy_value", a, ValueSel{want, unless, values});
}

}  // extern "C"
