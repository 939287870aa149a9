// pe_policy.hip -- batched MLP policy inference from the obs of a handle's envs to their
// next actions: pe_policy_create / _load / _forward / _destroy of include/plantos_batch.h
// (the definition of the outputs heads that header's "Policy inference" block; the host
// twin is pe_policy_host.cpp and shares pe_policy_math.hpp with this file).
//
// One fused kernel per forward, one workgroup of 8 waves per tile of E = 32 or 64 envs:
//   0  the tile's obs rows (contiguous in memory: E * D values) are read with coalesced
//      loads -- byte codes go through the 256-entry code table in LDS -- into a staging
//      image [env][D | 1] in LDS, then transposed to xT[k][env] (k padded with zeros to a
//      multiple of 8, rows of envs past n zero);
//   1  every hidden layer runs on v_mfma_f32_32x32x2_f32: A = the weights (row = neuron),
//      B = the activations (column = env), C starts as the bias, and the k-steps are
//      issued in ascending k into ONE accumulator per output -- on gfx950 that is bit for
//      bit the fmaf chain of the definition.  A wave owns 32-neuron tiles (x all env
//      tiles); its weights come from the packed buffer, where the 8 k of a neuron tile
//      that a wave's next four MFMAs need are one 16-B load per lane (1 KiB per wave,
//      contiguous); the activation function is applied to the accumulators and the
//      result written to the other of two LDS buffers [neuron][env];
//   2  the heads (<= 8 + 1 outputs) are VALU fmaf chains, one (env, output) per lane, over
//      the last hidden buffer -- the same chain, with too few outputs to fill a 32-wide
//      MFMA tile;
//   3  argmax or the categorical sample per env, then the only global stores: actions and,
//      where asked for, the head outputs.
// Activations never leave LDS / registers.  Nothing past row n - 1 of obs or of an
// output is read or written.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <string>

#include "../../include/plantos_batch.h"
#include "pe_handle.hpp"
#include "pe_policy_math.hpp"

extern "C" int pe_internal_policy_check(int32_t n_towers, const pe_policy_tower* tw, int32_t activation,
                                        int with_ptrs);

namespace {
using namespace pe_pol;

constexpr int kThreads = 512, kWaves = kThreads / 64;
constexpr int kMaxLds = 160 * 1024;
constexpr int kHeadRows = 9;  // tower 0's <= 8 outputs + the value

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct Layer {
  int K, Kp, N;            // inputs, inputs padded to a multiple of 8 (hidden layers), outputs
  uint32_t off_w, off_b;   // float offsets into the packed buffer
};
struct Tower {
  int n_hidden, n_out;
  Layer l[4];  // hidden layers, then the head
};

struct FwdArgs {
  const float* packed;
  const float* tab;   // f32[256] code table
  const void* obs;
  int obs_is_codes;
  int n, D, SD, Kp0, HB;  // SD = D | 1 staging pitch, Kp0 = D padded to 8, HB = rows of a hidden buffer
  int n_towers, act, mode;
  uint64_t seed;
  uint32_t env_off, t;
  int32_t* actions;
  float* head0;
  float* head1;
  Tower tw[2];
};

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

template <int ET>
__global__ __launch_bounds__(kThreads) void pe_policy_forward_kernel(FwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int E = 32 * ET;
  float* tab = lds;                    // [256]
  float* hd = tab + 256;               // [kHeadRows][E]
  float* xT = hd + kHeadRows * E;      // [Kp0][E]
  float* h0 = xT + a.Kp0 * E;          // [HB][E] (first the staging image [E][SD])
  float* h1 = h0 + a.HB * E;           // [HB][E]
  const int tid = threadIdx.x;
  const int64_t e0 = (int64_t)blockIdx.x * E;
  const int rows = (int)min((int64_t)E, (int64_t)a.n - e0);
  const int D = a.D, SD = a.SD;

  // 0: obs tile -> staging -> xT
  const int count = rows * D;
  if (a.obs_is_codes) {
    if (tid < 256) tab[tid] = a.tab[tid];
    __syncthreads();
    const uint8_t* src = static_cast<const uint8_t*>(a.obs) + e0 * D;
    for (int i = tid; i < count; i += kThreads) {
      const int row = i / D;
      h0[row * SD + (i - row * D)] = tab[src[i]];
    }
  } else {
    const float* src = static_cast<const float*>(a.obs) + e0 * D;
    for (int i = tid; i < count; i += kThreads) {
      const int row = i / D;
      h0[row * SD + (i - row * D)] = src[i];
    }
  }
  __syncthreads();
  for (int idx = tid; idx < a.Kp0 * E; idx += kThreads) {
    const int k = idx / E, e = idx - k * E;
    xT[idx] = (k < D && e < rows) ? h0[e * SD + k] : 0.0f;
  }
  __syncthreads();

  // 1 + 2: towers
  for (int ti = 0; ti < a.n_towers; ++ti) {
    const Tower& tw = a.tw[ti];
    const float* in = xT;
    for (int l = 0; l < tw.n_hidden; ++l) {
      const Layer& L = tw.l[l];
      float* out = (l & 1) ? h1 : h0;
      hidden_layer<ET, float>(a.packed + L.off_w, a.packed + L.off_b, in, out, L.Kp >> 3, L.N >> 5, a.act);
      __syncthreads();
      in = out;
    }
    const Layer& H = tw.l[tw.n_hidden];
    for (int idx = tid; idx < tw.n_out * E; idx += kThreads) {
      const int o = idx / E, e = idx - o * E;
      const float* w = a.packed + H.off_w + (size_t)o * H.K;
      float acc = a.packed[H.off_b + o];
      for (int k = 0; k < H.K; ++k) acc = fmaf(w[k], in[k * E + e], acc);
      hd[(ti == 0 ? o : kHeadRows - 1) * E + e] = acc;
    }
    __syncthreads();  // the next tower overwrites h0 / h1; the epilogue reads hd
  }

  // 3: action + outputs
  if (tid < rows) {
    const int A = a.tw[0].n_out;
    const int64_t e = e0 + tid;
    float l[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) l[q] = q < A ? hd[q * E + tid] : 0.0f;
    int act;
    if (a.mode == PE_POLICY_ARGMAX)
      act = policy_argmax(l, A);
    else
      act = policy_sample(l, A, policy_uniform(a.seed, a.env_off + (uint32_t)e, a.t));
    a.actions[e] = act;
    if (a.head0) {
#pragma unroll
      for (int q = 0; q < 8; ++q)
        if (q < A) a.head0[e * A + q] = l[q];
    }
    if (a.head1) a.head1[e] = hd[(kHeadRows - 1) * E + tid];
  }
}

// ---------------------------------------------------------------- host side
int fail(int code, const std::string& msg) { return pe_internal_set_error(code, msg.c_str()); }

int hip_fail(hipError_t e, const char* what) {
  return fail(PE_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
}

struct DevBind {
  int prev = -1;
  hipError_t err = hipSuccess;
  explicit DevBind(int dev) {
    (void)hipGetLastError();  // drop a stale error of an earlier call (launch checks below)
    int cur = -1;
    err = hipGetDevice(&cur);
    if (err == hipSuccess && cur != dev) {
      err = hipSetDevice(dev);
      if (err == hipSuccess) prev = cur;
    }
  }
  ~DevBind() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

size_t lds_bytes(int E, int Kp0, int HB) { return sizeof(float) * ((size_t)256 + (size_t)E * (kHeadRows + Kp0 + 2 * HB)); }

}  // namespace

struct pe_policy {
  pe_handle* h;
  int n_towers, act, env_tile;
  int D, SD, Kp0, HB;
  Tower tw[2];
  float* mem;        // packed weights, then the code table
  size_t n_packed;   // floats
  size_t lds;
};

extern "C" {

int pe_policy_create(pe_handle* h, int32_t n_towers, const pe_policy_tower* shapes, int32_t activation,
                     int32_t env_tile, pe_policy** out) {
  if (!h || !out) return fail(PE_ERR_ARG, "null argument");
  if (const int rc = pe_internal_policy_check(n_towers, shapes, activation, 0)) return rc;
  if (env_tile != 0 && env_tile != 32 && env_tile != 64) return fail(PE_ERR_ARG, "env_tile must be 0, 32 or 64");
  pe_policy* p = new (std::nothrow) pe_policy();
  if (!p) return fail(PE_ERR_NOMEM, "host allocation failed");
  p->h = h;
  p->n_towers = n_towers;
  p->act = activation;
  p->D = h->g.D;
  p->SD = p->D | 1;
  p->Kp0 = (p->D + 7) & ~7;
  int hmax = 0;
  size_t off = 0;
  for (int i = 0; i < n_towers; ++i) {
    Tower& t = p->tw[i];
    t.n_hidden = shapes[i].n_hidden;
    t.n_out = shapes[i].n_out;
    int K = p->D;
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
      if (!head) hmax = std::max(hmax, L.N);
      K = L.N;
    }
  }
  p->n_packed = off;
  p->HB = std::max(hmax, p->SD);
  const bool fits64 = lds_bytes(64, p->Kp0, p->HB) <= (size_t)kMaxLds;
  const bool fits32 = lds_bytes(32, p->Kp0, p->HB) <= (size_t)kMaxLds;
  // the library's choice: 64 envs per workgroup once that still gives every CU a workgroup
  // (each workgroup streams the whole net), else 32
  if (env_tile == 0) env_tile = (fits64 && (int64_t)h->n >= 64 * (int64_t)std::max(h->num_cus, 1)) ? 64 : 32;
  if (!(env_tile == 64 ? fits64 : fits32)) {
    delete p;
    return fail(PE_ERR_ARG, "the env tile's activations do not fit 160 KiB of LDS (obs length / layer widths / env_tile)");
  }
  p->env_tile = env_tile;
  p->lds = lds_bytes(env_tile, p->Kp0, p->HB);
  DevBind db(h->device);
  if (db.err != hipSuccess) {
    delete p;
    return hip_fail(db.err, "hipSetDevice");
  }
  const size_t bytes = (p->n_packed + 256) * sizeof(float);
  hipError_t e = hipMalloc(&p->mem, bytes);
  if (e != hipSuccess) {
    delete p;
    return fail(PE_ERR_NOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
  }
  float table[256];
  pe_obs_code_table(h, table);
  e = hipMemset(p->mem, 0, bytes);
  if (e == hipSuccess) e = hipMemcpy(p->mem + p->n_packed, table, sizeof(table), hipMemcpyHostToDevice);
  if (e == hipSuccess)
    e = env_tile == 64 ? hipFuncSetAttribute(reinterpret_cast<const void*>(&pe_policy_forward_kernel<2>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)p->lds)
                       : hipFuncSetAttribute(reinterpret_cast<const void*>(&pe_policy_forward_kernel<1>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)p->lds);
  if (e != hipSuccess) {
    (void)hipFree(p->mem);
    delete p;
    return hip_fail(e, "pe_policy_create");
  }
  *out = p;
  return PE_OK;
}

int pe_policy_destroy(pe_policy* p) {
  if (!p) return PE_OK;
  DevBind db(p->h->device);
  const hipError_t e = hipFree(p->mem);
  delete p;
  return e == hipSuccess ? PE_OK : hip_fail(e, "hipFree");
}

int32_t pe_policy_env_tile(const pe_policy* p) { return p ? p->env_tile : 0; }

int pe_policy_load(pe_policy* p, const pe_policy_tower* towers, void* stream) {
  if (!p || !towers) return fail(PE_ERR_ARG, "null argument");
  PackArgs a;
  a.packed = p->mem;
  int nl = 0;
  uint32_t most = 0;
  for (int i = 0; i < p->n_towers; ++i) {
    const Tower& t = p->tw[i];
    if (towers[i].n_hidden != t.n_hidden || towers[i].n_out != t.n_out)
      return fail(PE_ERR_ARG, "tower shape differs from pe_policy_create's");
    for (int l = 0; l <= t.n_hidden; ++l) {
      if (l < t.n_hidden && towers[i].hidden[l] != t.l[l].N)
        return fail(PE_ERR_ARG, "tower shape differs from pe_policy_create's");
      if (!towers[i].weight[l] || !towers[i].bias[l]) return fail(PE_ERR_ARG, "null weight or bias tensor");
      PackLayer& L = a.l[nl++];
      L.w = towers[i].weight[l];
      L.b = towers[i].bias[l];
      L.K = t.l[l].K;
      L.Kp = t.l[l].Kp;
      L.N = t.l[l].N;
      L.head = l == t.n_hidden;
      L.off_w = t.l[l].off_w;
      L.off_b = t.l[l].off_b;
      L.n_w = (uint32_t)(L.N * L.Kp);
      most = std::max(most, L.n_w + (uint32_t)L.N);
    }
  }
  DevBind db(p->h->device);
  if (db.err != hipSuccess) return hip_fail(db.err, "hipSetDevice");
  hipLaunchKernelGGL(pe_policy_pack_kernel, dim3((most + 255) / 256, (unsigned)nl), dim3(256), 0,
                     static_cast<hipStream_t>(stream), a);
  const hipError_t le = hipGetLastError();
  return le == hipSuccess ? PE_OK : hip_fail(le, "pe_policy_load");
}

int pe_policy_forward(pe_policy* p, const void* obs, int32_t obs_is_codes, int32_t mode, uint64_t seed,
                      uint32_t t, int32_t* actions, float* head0, float* head1, void* stream) {
  if (!p || !obs || !actions) return fail(PE_ERR_ARG, "null argument");
  if (obs_is_codes != 0 && obs_is_codes != 1) return fail(PE_ERR_ARG, "obs_is_codes must be 0 or 1");
  if (obs_is_codes && !p->h->obs_codes) return fail(PE_ERR_ARG, "obs_is_codes = 1 needs a handle created with obs_codes");
  if (mode != PE_POLICY_ARGMAX && mode != PE_POLICY_SAMPLE)
    return fail(PE_ERR_ARG, "mode must be PE_POLICY_ARGMAX or PE_POLICY_SAMPLE");
  if (head1 && p->n_towers < 2) return fail(PE_ERR_ARG, "head1 needs a second tower");
  FwdArgs a;
  a.packed = p->mem;
  a.tab = p->mem + p->n_packed;
  a.obs = obs;
  a.obs_is_codes = obs_is_codes;
  a.n = p->h->n;
  a.D = p->D;
  a.SD = p->SD;
  a.Kp0 = p->Kp0;
  a.HB = p->HB;
  a.n_towers = p->n_towers;
  a.act = p->act;
  a.mode = mode;
  a.seed = seed;
  a.env_off = p->h->cfg.env_id_offset;
  a.t = t;
  a.actions = actions;
  a.head0 = head0;
  a.head1 = head1;
  a.tw[0] = p->tw[0];
  a.tw[1] = p->tw[p->n_towers - 1];
  DevBind db(p->h->device);
  if (db.err != hipSuccess) return hip_fail(db.err, "hipSetDevice");
  const int E = p->env_tile;
  const dim3 grid((unsigned)((a.n + E - 1) / E)), block(kThreads);
  if (E == 64)
    hipLaunchKernelGGL(pe_policy_forward_kernel<2>, grid, block, p->lds, static_cast<hipStream_t>(stream), a);
  else
    hipLaunchKernelGGL(pe_policy_forward_kernel<1>, grid, block, p->lds, static_cast<hipStream_t>(stream), a);
  const hipError_t le = hipGetLastError();
  return le == hipSuccess ? PE_OK : hip_fail(le, "pe_policy_forward");
}

}  // extern "C"
