// pe_policy_impl.hpp -- what the two policy translation units share (pe_policy.hip: the
// feed-forward policy; pe_policy_lstm.hip: the recurrent one): the pe_policy object, the MFMA
// hidden layer, the weight packing kernel and the host side's one create, launch and argument
// check.  What a policy is made of is decided in pe_policy_plan.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <initializer_list>
#include <memory>
#include <new>
#include <string>

#include "../../include/plantos_batch.h"
#include "pe_host.hpp"
#include "pe_policy_math.hpp"
#include "pe_policy_plan.hpp"

namespace pe_pol {

constexpr int kThreads = 512, kWaves = kThreads / 64;

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct PackLayer {
  const float* w;
  const float* b;
  int K, Kp, N, head;
  uint32_t off_w, off_b, n_w;  // n_w: packed weight floats
};
struct PackArgs {
  float* packed;
  PackLayer l[8];
};

}  // namespace pe_pol

// A policy is its plan (pe_policy_plan.hpp), the handle whose obs it reads and two allocations.
struct pe_policy : pe_pol::PolicyPlan {
  pe_handle* h;
  float* mem;    // packed weights, then the code table
  float* state;  // recurrent policies only: [tower][h, c][env tile][H][env_tile]
};

namespace {
using namespace pe_pol;

// Packed hidden weights: [neuron tile jt][k group kg][lane][q], element = W[jt*32 + (lane & 31)]
// [kg*8 + q*2 + (lane >> 5)] (0 for k >= K): float4 q = 0..3 of a lane are its A operands of
// four consecutive 32x32x2 k-steps.  Head weights and all biases keep their layout.
__global__ __launch_bounds__(256) void pe_policy_pack_kernel(PackArgs a) {
  const PackLayer& L = a.l[blockIdx.y];
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < L.n_w) {
    float v;
    if (L.head) {
      v = L.w[i];
    } else {
      const uint32_t q = i & 3u, lane = (i >> 2) & 63u, blk = i >> 8, KG = (uint32_t)L.Kp >> 3;
      const uint32_t kg = blk % KG, jt = blk / KG;
      const uint32_t j = jt * 32u + (lane & 31u), k = kg * 8u + q * 2u + (lane >> 5);
      v = k < (uint32_t)L.K ? L.w[(size_t)j * L.K + k] : 0.0f;
    }
    a.packed[L.off_w + i] = v;
  } else if (i < L.n_w + (uint32_t)L.N) {
    a.packed[L.off_b + (i - L.n_w)] = L.b[i - L.n_w];
  }
}

__device__ __forceinline__ float activate(float z, int act) { return act == PE_ACT_TANH ? pe_tanhf(z) : pe_relu(z); }

// out[j][e] = act(b_j + sum_k W[j][k] in[k][e]) for the tile's E = 32 * ET envs; in / out are
// LDS images [k][E] / [j][E].  T is the operand type (only float is defined and built).
template <int ET, typename T>
__device__ __forceinline__ void hidden_layer(const T* __restrict__ wp, const float* __restrict__ bias,
                                             const T* in, T* out, int KG, int NT, int act) {
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
    const float4* w4 = reinterpret_cast<const float4*>(wp) + (size_t)jt * KG * 64 + lane;
    const T* xin = in + half * E + col;
    float4 w = w4[0];
    for (int kg = 0; kg < KG; ++kg) {
      const float4 wn = w4[(size_t)min(kg + 1, KG - 1) * 64];  // the next group's, in flight over the MFMAs
      const T* x = xin + kg * 8 * E;
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
      for (int et = 0; et < ET; ++et) out[j * E + et * 32 + col] = activate(acc[et][r], act);
    }
  }
}

// The tile's obs rows -> the staging image [env][SD] (LDS, `stage`) -> xT[k][env], k padded
// with zeros to Kp0, rows of envs past n zero.  Ends with a barrier.
template <int E>
__device__ __forceinline__ void stage_obs(const void* obs, int obs_is_codes, const float* tab_g, float* tab,
                                          float* stage, float* xT, int64_t e0, int rows, int D, int SD, int Kp0) {
  const int tid = threadIdx.x;
  const int count = rows * D;
  if (obs_is_codes) {
    if (tid < 256) tab[tid] = tab_g[tid];
    __syncthreads();
    const uint8_t* src = static_cast<const uint8_t*>(obs) + e0 * D;
    for (int i = tid; i < count; i += kThreads) {
      const int row = i / D;
      stage[row * SD + (i - row * D)] = tab[src[i]];
    }
  } else {
    const float* src = static_cast<const float*>(obs) + e0 * D;
    for (int i = tid; i < count; i += kThreads) {
      const int row = i / D;
      stage[row * SD + (i - row * D)] = src[i];
    }
  }
  __syncthreads();
  for (int idx = tid; idx < Kp0 * E; idx += kThreads) {
    const int k = idx / E, e = idx - k * E;
    xT[idx] = (k < D && e < rows) ? stage[e * SD + k] : 0.0f;
  }
  __syncthreads();
}

// Head of a tower (<= 8 + 1 outputs): VALU fmaf chains, one (env, output) per lane, over the
// last hidden buffer `in` [K][E]; row `o` of tower 0 / the last row of tower 1 in hd.
template <int E>
__device__ __forceinline__ void head_layer(const float* packed, const Layer& H, int n_out, int ti, const float* in,
                                           float* hd) {
  for (int idx = threadIdx.x; idx < n_out * E; idx += kThreads) {
    const int o = idx / E, e = idx - o * E;
    const float* w = packed + H.off_w + (size_t)o * H.K;
    float acc = packed[H.off_b + o];
    for (int k = 0; k < H.K; ++k) acc = fmaf(w[k], in[k * E + e], acc);
    hd[(ti == 0 ? o : kHeadRows - 1) * E + e] = acc;
  }
}

// Action + outputs of env e0 + tid from the head rows in hd.
template <int E>
__device__ __forceinline__ void act_and_store(const float* hd, int A, int rows, int64_t e0, int mode, uint64_t seed,
                                              uint32_t env_off, uint32_t t, int32_t* actions, float* head0,
                                              float* head1) {
  const int tid = threadIdx.x;
  if (tid < rows) {
    const int64_t e = e0 + tid;
    float l[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) l[q] = q < A ? hd[q * E + tid] : 0.0f;
    int act;
    if (mode == PE_POLICY_ARGMAX)
      act = policy_argmax(l, A);
    else
      act = policy_sample(l, A, policy_uniform(seed, env_off + (uint32_t)e, t));
    actions[e] = act;
    if (head0) {
#pragma unroll
      for (int q = 0; q < 8; ++q)
        if (q < A) head0[e * A + q] = l[q];
    }
    if (head1) head1[e] = hd[(kHeadRows - 1) * E + tid];
  }
}

// ---------------------------------------------------------------- value-only forwards
// What pe_policy_value / pe_policy_value_lstm add to a forward's arguments.
struct ValueSel {
  const uint8_t* want;    // u8[n] or null: null selects every env
  const uint8_t* unless;  // u8[n] or null: a non-zero flag deselects the env
  float* values;          // f32[n]: written for selected envs only
};

// Whether this thread's env of the tile (e0 + threadIdx.x, for the first `rows` threads) is selected.
__device__ __forceinline__ bool selected(const ValueSel& s, int64_t e0, int rows) {
  const int tid = threadIdx.x;
  if (tid >= rows) return false;
  const int64_t e = e0 + tid;
  return (!s.want || s.want[e] != 0) && !(s.unless && s.unless[e] != 0);
}

// Whether `mine` holds for any thread of the workgroup: the same answer in every thread.  Every
// thread of the workgroup must call it (two barriers); `word` is an LDS word that nobody writes
// before the workgroup's next barrier after the call.
__device__ __forceinline__ bool block_any(bool mine, float* word) {
  int* w = reinterpret_cast<int*>(word);
  if (threadIdx.x == 0) *w = 0;
  __syncthreads();
  if (mine) *w = 1;
  __syncthreads();
  return __builtin_amdgcn_readfirstlane(*w) != 0;
}

// values[e] of the tile's selected envs from tower 1's head row in hd.
template <int E>
__device__ __forceinline__ void store_values(const float* hd, bool sel, int64_t e0, float* values) {
  if (sel) values[e0 + threadIdx.x] = hd[(kHeadRows - 1) * E + threadIdx.x];
}

// ---------------------------------------------------------------- host side
// Frees p and what it owns (the policy's device bound); the first error.
inline hipError_t free_policy(pe_policy* p) {
  hipError_t e = hipFree(p->mem);
  if (p->state) {
    const hipError_t es = hipFree(p->state);
    if (e == hipSuccess) e = es;
  }
  delete p;
  return e;
}
struct PolicyDeleter {
  void operator()(pe_policy* p) const { (void)free_policy(p); }
};

// The two instantiations of a forward kernel, for tiles of 32 and of 64 envs.
template <class... A>
struct TileKernel {
  void (*k32)(A...);
  void (*k64)(A...);
  TileKernel(void (*a)(A...), void (*b)(A...)) : k32(a), k64(b) {}
  const void* of(const PolicyPlan& p) const { return reinterpret_cast<const void*>(p.env_tile == 64 ? k64 : k32); }
  // p's instantiation over `rows` obs rows on `stream`; PE_OK or the launch error, named `what`
  int launch(const pe_policy* p, int64_t rows, void* stream, const char* what, const A&... args) const {
    DeviceGuard dg(p->h);
    if (dg.rc) return dg.rc;
    const int E = p->env_tile;
    hipLaunchKernelGGL(E == 64 ? k64 : k32, dim3((unsigned)((rows + E - 1) / E)), dim3(kThreads), p->lds,
                       static_cast<hipStream_t>(stream), args...);
    const hipError_t le = hipGetLastError();
    return le == hipSuccess ? PE_OK : hip_fail(le, what);
  }
};

// The policy of `plan` over h's envs: the allocations zeroed, the code table uploaded and the
// dynamic-LDS limit of `kernels` (TileKernel::of; null entries skipped) raised to the plan's.
// Every exit before the last frees what was made.
inline int create_policy(pe_handle* h, const PolicyPlan& plan, std::initializer_list<const void*> kernels,
                         const char* what, pe_policy** out) {
  DeviceGuard dg(h);
  if (dg.rc) return dg.rc;
  std::unique_ptr<pe_policy, PolicyDeleter> p(new (std::nothrow) pe_policy{plan, h, nullptr, nullptr});
  if (!p) return fail(PE_ERR_NOMEM, "host allocation failed");
  const size_t bytes = (p->n_packed + 256) * sizeof(float);
  const size_t state_bytes = (size_t)2 * p->n_towers * p->n_state * sizeof(float);
  hipError_t e = hipMalloc(&p->mem, bytes);
  if (e == hipSuccess && state_bytes) e = hipMalloc(&p->state, state_bytes);
  if (e != hipSuccess) return fail(PE_ERR_NOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
  float table[256];
  pe_obs_code_table(h, table);
  e = hipMemset(p->mem, 0, bytes);
  if (e == hipSuccess && state_bytes) e = hipMemset(p->state, 0, state_bytes);
  if (e == hipSuccess) e = hipMemcpy(p->mem + p->n_packed, table, sizeof(table), hipMemcpyHostToDevice);
  for (const void* k : kernels)
    if (e == hipSuccess && k) e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p->lds);
  if (e != hipSuccess) return hip_fail(e, what);
  *out = p.release();
  return PE_OK;
}

// The argument checks the forwards share.  wrong_kind: the error of a policy of the other kind
// (want_recurrent says which this entry point evaluates); out: the output that must be there.
inline int check_forward(const pe_policy* p, bool want_recurrent, const void* obs, const void* out,
                         int32_t obs_is_codes, int32_t mode, const float* head1, const char* wrong_kind) {
  if (!p || !obs || !out) return fail(PE_ERR_ARG, "null argument");
  if ((p->H != 0) != want_recurrent) return fail(PE_ERR_ARG, wrong_kind);
  if (obs_is_codes != 0 && obs_is_codes != 1) return fail(PE_ERR_ARG, "obs_is_codes must be 0 or 1");
  if (obs_is_codes && !p->h->obs_codes) return fail(PE_ERR_ARG, "obs_is_codes = 1 needs a handle created with obs_codes");
  if (mode != PE_POLICY_ARGMAX && mode != PE_POLICY_SAMPLE)
    return fail(PE_ERR_ARG, "mode must be PE_POLICY_ARGMAX or PE_POLICY_SAMPLE");
  if (head1 && p->n_towers < 2) return fail(PE_ERR_ARG, "head1 needs a second tower");
  return PE_OK;
}

// The pack arguments of p's MLP layers from the caller's device tensors; PE_OK or PE_ERR_ARG.
inline int pack_towers(const pe_policy* p, const pe_policy_tower* towers, PackArgs* a, int* nl, uint32_t* most) {
  a->packed = p->mem;
  *nl = 0;
  *most = 0;
  for (int i = 0; i < p->n_towers; ++i) {
    const Tower& t = p->tw[i];
    if (towers[i].n_hidden != t.n_hidden || towers[i].n_out != t.n_out)
      return fail(PE_ERR_ARG, "tower shape differs from pe_policy_create's");
    for (int l = 0; l <= t.n_hidden; ++l) {
      if (l < t.n_hidden && towers[i].hidden[l] != t.l[l].N)
        return fail(PE_ERR_ARG, "tower shape differs from pe_policy_create's");
      if (!towers[i].weight[l] || !towers[i].bias[l]) return fail(PE_ERR_ARG, "null weight or bias tensor");
      PackLayer& L = a->l[(*nl)++];
      L.w = towers[i].weight[l];
      L.b = towers[i].bias[l];
      L.K = t.l[l].K;
      L.Kp = t.l[l].Kp;
      L.N = t.l[l].N;
      L.head = l == t.n_hidden;
      L.off_w = t.l[l].off_w;
      L.off_b = t.l[l].off_b;
      L.n_w = (uint32_t)(L.N * L.Kp);
      *most = *most > L.n_w + (uint32_t)L.N ? *most : L.n_w + (uint32_t)L.N;
    }
  }
  return PE_OK;
}

}  // namespace
