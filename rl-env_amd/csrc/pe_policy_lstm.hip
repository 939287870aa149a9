// pe_policy_lstm.hip -- batched recurrent policy inference (sb3_contrib's MlpLstmPolicy with
// one LSTM layer per tower): pe_policy_create_lstm / _load_lstm / _forward_lstm / _value_lstm and the
// state calls of include/plantos_batch.h ("Recurrent policy inference" there is the definition;
// the host twin is pe_policy_host.cpp).
//
// One fused kernel per forward, one workgroup of 8 waves per tile of E = 32 or 64 envs, as
// the feed-forward kernel of pe_policy.hip, whose stages 0, 2 and 3 it shares:
//   0  obs tile -> staging -> xT[k][env] (k padded to Kp0);
//   L  per tower: the tile's h is copied from the state in HBM into hT[k][env], which lies
//      right behind xT, so the gates' K = Kp0 + H chain reads ONE LDS image; rows of envs
//      that start an episode are zeroed on the way.  A wave owns 32-unit tiles and carries
//      four accumulator tiles (i, f, g, o) per env tile on v_mfma_f32_32x32x2_f32: C starts
//      as bias_ih + bias_hh, the k-steps run in ascending k (x rows, then h rows) -- bit for
//      bit the definition's fmaf chain.  The same lane and register index holds the same
//      (unit, env) in all four, so the cell runs in registers: the lane reads c from HBM,
//      writes c' and h' back (each workgroup touches its own envs' state only, and its h
//      was copied to LDS before the first write: the update is in place) and h' into the
//      LDS image hN[unit][env].  No gate goes through LDS;
//   1  the tower's MLP reads hN and alternates between hT and hN (both dead by then);
//   2  heads; 3  argmax / sample and the stores.
// The state is kept in the kernel's own order, [tower][h, c][env tile][unit][env in tile]:
// the tile's image is contiguous, and the lanes' c / h accesses are 128-B rows.
#include <algorithm>
#include <string>

#include "pe_policy_impl.hpp"

namespace {

struct LstmArgs {
  const float* packed;
  const float* tab;   // f32[256] code table
  const void* obs;
  const uint8_t* start_a;
  const uint8_t* start_b;
  float* state;
  size_t n_state;
  int obs_is_codes;
  int n, D, SD, Kp0, HB, H;
  int n_towers, act, mode;
  uint64_t seed;
  uint32_t env_off, t;
  uint32_t off_lw[2], off_lb[2];
  int32_t* actions;
  float* head0;
  float* head1;
  Tower tw[2];
};

struct LstmPackArgs {
  float* packed;
  const float* w_ih[2];
  const float* w_hh[2];
  const float* b_ih[2];
  const float* b_hh[2];
  uint32_t off_lw[2], off_lb[2];
  int D, Kp0, H;
};

// Packed gate weights of tower blockIdx.y: [unit tile jt][k group kg][gate][lane][q], element =
// W[gate*H + jt*32 + (lane & 31)][k], k = kg*8 + q*2 + (lane >> 5) of the concatenated chain:
// k < D: weight_ih[.][k]; D <= k < Kp0: 0; else weight_hh[.][k - Kp0].  Bias: b_ih + b_hh.
__global__ __launch_bounds__(256) void pe_policy_lstm_pack_kernel(LstmPackArgs a) {
#pragma clang fp contract(off)
  const int ti = blockIdx.y;
  const uint32_t KG = (uint32_t)(a.Kp0 + a.H) >> 3, H = (uint32_t)a.H;
  const uint32_t n_w = 4u * H * KG * 8u;
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < n_w) {
    const uint32_t q = i & 3u, lane = (i >> 2) & 63u, gate = (i >> 8) & 3u, blk = i >> 10;
    const uint32_t kg = blk % KG, jt = blk / KG;
    const uint32_t row = gate * H + jt * 32u + (lane & 31u), k = kg * 8u + q * 2u + (lane >> 5);
    float v = 0.0f;
    if (k < (uint32_t)a.D)
      v = a.w_ih[ti][(size_t)row * a.D + k];
    else if (k >= (uint32_t)a.Kp0)
      v = a.w_hh[ti][(size_t)row * H + (k - (uint32_t)a.Kp0)];
    a.packed[a.off_lw[ti] + i] = v;
  } else if (i < n_w + 4u * H) {
    const uint32_t j = i - n_w;
    a.packed[a.off_lb[ti] + j] = a.b_ih[ti][j] + a.b_hh[ti][j];
  }
}

// The LSTM of one tower for the tile: gates over the LDS image xh [Kp0 + H][E], cell in
// registers, h' to hN [H][E] and, with c', to the tile's state images hs / cs [H][E] in HBM.
// STORE = false (the value-only forward) reads the state and leaves it as it is.
template <int ET, bool STORE>
__device__ __forceinline__ void lstm_layer(const float* __restrict__ wp, const float* __restrict__ bias,
                                           const float* xh, float* hN, float* hs, float* cs, int KG, int H,
                                           const bool (&started)[ET], const bool (&live)[ET]) {
  constexpr int E = 32 * ET;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, col = lane & 31, half = lane >> 5;
  const int NT = H >> 5;
  for (int jt = wave; jt < NT; jt += kWaves) {
    f32x16 acc[4][ET];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float b = bias[g * H + jt * 32 + (r & 3) + 8 * (r >> 2) + 4 * half];
#pragma unroll
        for (int et = 0; et < ET; ++et) acc[g][et][r] = b;
      }
    }
    const float4* w4 = reinterpret_cast<const float4*>(wp) + (size_t)jt * KG * 256 + lane;
    const float* xin = xh + half * E + col;
    float4 w[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) w[g] = w4[g * 64];
    for (int kg = 0; kg < KG; ++kg) {
      float4 wn[4];  // the next group's, in flight over the MFMAs
      const float4* wnext = w4 + (size_t)min(kg + 1, KG - 1) * 256;
#pragma unroll
      for (int g = 0; g < 4; ++g) wn[g] = wnext[g * 64];
      const float* x = xin + kg * 8 * E;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float xv[ET];
#pragma unroll
        for (int et = 0; et < ET; ++et) xv[et] = x[q * 2 * E + et * 32];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const float wq = q == 0 ? w[g].x : (q == 1 ? w[g].y : (q == 2 ? w[g].z : w[g].w));
#pragma unroll
          for (int et = 0; et < ET; ++et)
            acc[g][et] = __builtin_amdgcn_mfma_f32_32x32x2f32(wq, xv[et], acc[g][et], 0, 0, 0);
        }
      }
#pragma unroll
      for (int g = 0; g < 4; ++g) w[g] = wn[g];
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int j = jt * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
#pragma unroll
      for (int et = 0; et < ET; ++et) {
        const int idx = j * E + et * 32 + col;
        const float c_old = (started[et] || !live[et]) ? 0.0f : cs[idx];
        float hn, cn;
        pe_lstm_cell(acc[0][et][r], acc[1][et][r], acc[2][et][r], acc[3][et][r], c_old, &hn, &cn);
        hN[idx] = hn;
        if constexpr (STORE) {
          if (live[et]) {
            cs[idx] = cn;
            hs[idx] = hn;
          }
        }
      }
    }
  }
}

template <int ET>
__global__ __launch_bounds__(kThreads) void pe_policy_lstm_forward_kernel(LstmArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int E = 32 * ET;
  float* tab = lds;                    // [256]
  float* hd = tab + 256;               // [kHeadRows][E]
  float* xT = hd + kHeadRows * E;      // [Kp0][E]
  float* hT = xT + a.Kp0 * E;          // [HB][E]: the tower's old h, rows [0, H) (xT | hT is one image)
  float* hN = hT + a.HB * E;           // [HB][E]: first the staging image [E][SD], then the new h
  const int tid = threadIdx.x;
  const int64_t e0 = (int64_t)blockIdx.x * E;
  const int rows = (int)min((int64_t)E, (int64_t)a.n - e0);
  const int H = a.H;

  // episode starts of the envs this thread meets: as a loader (env tid % E) and as an MFMA lane
  const int le = tid & (E - 1);
  bool l_start = false;
  if (le < rows) l_start = (a.start_a && a.start_a[e0 + le]) | (a.start_b && a.start_b[e0 + le]);
  bool started[ET], live[ET];
#pragma unroll
  for (int et = 0; et < ET; ++et) {
    const int e = et * 32 + (tid & 31);
    live[et] = e < rows;
    started[et] = live[et] && ((a.start_a && a.start_a[e0 + e]) | (a.start_b && a.start_b[e0 + e]));
  }

  // 0: obs tile -> staging -> xT
  stage_obs<E>(a.obs, a.obs_is_codes, a.tab, tab, hN, xT, e0, rows, a.D, a.SD, a.Kp0);

  const size_t tile_off = (size_t)blockIdx.x * H * E;
  for (int ti = 0; ti < a.n_towers; ++ti) {
    const Tower& tw = a.tw[ti];
    float* hs = a.state + (size_t)(2 * ti) * a.n_state + tile_off;
    float* cs = hs + a.n_state;
    // L: old h -> hT (zero where the env starts or lies past n), gates, cell
    for (int idx = tid; idx < H * E; idx += kThreads) hT[idx] = (l_start || le >= rows) ? 0.0f : hs[idx];
    __syncthreads();
    lstm_layer<ET, true>(a.packed + a.off_lw[ti], a.packed + a.off_lb[ti], xT, hN, hs, cs, (a.Kp0 + H) >> 3, H, started,
                         live);
    __syncthreads();
    // 1 + 2: the tower's MLP and head
    const float* in = hN;
    for (int l = 0; l < tw.n_hidden; ++l) {
      const Layer& L = tw.l[l];
      float* out = (l & 1) ? hN : hT;
      hidden_layer<ET, float>(a.packed + L.off_w, a.packed + L.off_b, in, out, L.Kp >> 3, L.N >> 5, a.act);
      __syncthreads();
      in = out;
    }
    head_layer<E>(a.packed, tw.l[tw.n_hidden], tw.n_out, ti, in, hd);
    __syncthreads();  // the next tower overwrites hT / hN; the epilogue reads hd
  }

  // 3: action + outputs
  act_and_store<E>(hd, a.tw[0].n_out, rows, e0, a.mode, a.seed, a.env_off, a.t, a.actions, a.head0, a.head1);
}

// pe_policy_value_lstm: the forward kernel cut down to tower 1, from the state as it is --
// read, never written -- and values[e] of the selected envs.  A workgroup none of whose envs
// is selected returns before it reads obs.  A kernel of its own, so that the forward kernel's
// code stays as it was; the stages are the same calls.
template <int ET>
__global__ __launch_bounds__(kThreads) void pe_policy_lstm_value_kernel(LstmArgs a, ValueSel s) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int E = 32 * ET;
  float* tab = lds;                    // the forward kernel's images
  float* hd = tab + 256;
  float* xT = hd + kHeadRows * E;
  float* hT = xT + a.Kp0 * E;
  float* hN = hT + a.HB * E;
  const int tid = threadIdx.x;
  const int64_t e0 = (int64_t)blockIdx.x * E;
  const int rows = (int)min((int64_t)E, (int64_t)a.n - e0);
  const int H = a.H;

  const bool sel = selected(s, e0, rows);
  if (!block_any(sel, hd)) return;  // uniform: every thread of the workgroup leaves, before any other barrier

  const int le = tid & (E - 1);
  bool l_start = false;
  if (le < rows) l_start = (a.start_a && a.start_a[e0 + le]) | (a.start_b && a.start_b[e0 + le]);
  bool started[ET], live[ET];
#pragma unroll
  for (int et = 0; et < ET; ++et) {
    const int e = et * 32 + (tid & 31);
    live[et] = e < rows;
    started[et] = live[et] && ((a.start_a && a.start_a[e0 + e]) | (a.start_b && a.start_b[e0 + e]));
  }

  stage_obs<E>(a.obs, a.obs_is_codes, a.tab, tab, hN, xT, e0, rows, a.D, a.SD, a.Kp0);

  const Tower& tw = a.tw[1];
  float* hs = a.state + (size_t)2 * a.n_state + (size_t)blockIdx.x * H * E;  // tower 1's h image, then its c
  float* cs = hs + a.n_state;
  for (int idx = tid; idx < H * E; idx += kThreads) hT[idx] = (l_start || le >= rows) ? 0.0f : hs[idx];
  __syncthreads();
  lstm_layer<ET, false>(a.packed + a.off_lw[1], a.packed + a.off_lb[1], xT, hN, hs, cs, (a.Kp0 + H) >> 3, H, started,
                        live);
  __syncthreads();
  const float* in = hN;
  for (int l = 0; l < tw.n_hidden; ++l) {
    const Layer& L = tw.l[l];
    float* out = (l & 1) ? hN : hT;
    hidden_layer<ET, float>(a.packed + L.off_w, a.packed + L.off_b, in, out, L.Kp >> 3, L.N >> 5, a.act);
    __syncthreads();
    in = out;
  }
  head_layer<E>(a.packed, tw.l[tw.n_hidden], tw.n_out, 1, in, hd);
  __syncthreads();
  store_values<E>(hd, sel, e0, s.values);
}

// state image [tile][H][E] <-> the caller's [n][H]
__global__ __launch_bounds__(256) void pe_policy_lstm_state_kernel(float* img, float* user, int n, int H, int E,
                                                                   int to_user) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)n * H) return;
  const int e = (int)(i / H), k = (int)(i - (int64_t)e * H);
  const size_t s = ((size_t)(e / E) * H + k) * E + (e % E);
  if (to_user)
    user[i] = img[s];
  else
    img[s] = user[i];
}

const TileKernel kForward(pe_policy_lstm_forward_kernel<1>, pe_policy_lstm_forward_kernel<2>);
const TileKernel kValue(pe_policy_lstm_value_kernel<1>, pe_policy_lstm_value_kernel<2>);

// What every launch of p reads; the sampler and output fields are left zero.
LstmArgs lstm_args(const pe_policy* p, const void* obs, int32_t obs_is_codes, const uint8_t* start_a,
                   const uint8_t* start_b) {
  LstmArgs a{};
  a.packed = p->mem;
  a.tab = p->mem + p->n_packed;
  a.obs = obs;
  a.start_a = start_a;
  a.start_b = start_b;
  a.state = p->state;
  a.n_state = p->n_state;
  a.obs_is_codes = obs_is_codes;
  a.n = p->h->n;
  a.D = p->D;
  a.SD = p->SD;
  a.Kp0 = p->Kp0;
  a.HB = p->HB;
  a.H = p->H;
  a.n_towers = p->n_towers;
  a.act = p->act;
  a.env_off = p->h->cfg.env_id_offset;
  for (int i = 0; i < 2; ++i) {
    const int s = std::min(i, p->n_towers - 1);
    a.off_lw[i] = p->off_lw[s];
    a.off_lb[i] = p->off_lb[s];
    a.tw[i] = p->tw[s];
  }
  return a;
}

int state_copy(pe_policy* p, int tower, float* h, float* c, void* stream, int to_user, const char* what) {
  if (!p) return fail(PE_ERR_ARG, "null policy");
  if (!p->H) return fail(PE_ERR_ARG, "not a recurrent policy");
  if (tower < 0 || tower >= p->n_towers) return fail(PE_ERR_ARG, "no such tower");
  DeviceGuard dg(p->h);
  if (dg.rc) return dg.rc;
  const int n = p->h->n;
  const unsigned blocks = (unsigned)(((int64_t)n * p->H + 255) / 256);
  float* user[2] = {h, c};
  for (int w = 0; w < 2; ++w)
    if (user[w])
      hipLaunchKernelGGL(pe_policy_lstm_state_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream),
                         p->state + (size_t)(2 * tower + w) * p->n_state, user[w], n, p->H, p->env_tile, to_user);
  const hipError_t le = hipGetLastError();
  return le == hipSuccess ? PE_OK : hip_fail(le, what);
}

}  // namespace

extern "C" {

int pe_policy_create_lstm(pe_handle* h, int32_t n_towers, const pe_policy_lstm* lstms, const pe_policy_tower* shapes,
                          int32_t activation, int32_t env_tile, pe_policy** out) {
  if (!h || !out) return fail(PE_ERR_ARG, "null argument");
  PolicyPlan plan;
  if (const int rc = make_policy_plan(h->g.D, h->n, h->num_cus, n_towers, lstms, shapes, activation, env_tile, true,
                                      &plan))
    return rc;
  return create_policy(h, plan, {kForward.of(plan), n_towers == 2 ? kValue.of(plan) : nullptr}, "pe_policy_create_lstm",
                       out);
}

int pe_policy_load_lstm(pe_policy* p, const pe_policy_lstm* lstms, const pe_policy_tower* towers, void* stream) {
  if (!p || !lstms || !towers) return fail(PE_ERR_ARG, "null argument");
  if (!p->H) return fail(PE_ERR_ARG, "a feed-forward policy is loaded with pe_policy_load");
  if (const int rc = pe_internal_policy_lstm_check(p->n_towers, lstms, 1)) return rc;
  if (lstms[0].hidden != p->H) return fail(PE_ERR_ARG, "lstm hidden size differs from pe_policy_create_lstm's");
  PackArgs a;
  int nl = 0;
  uint32_t most = 0;
  if (const int rc = pack_towers(p, towers, &a, &nl, &most)) return rc;
  LstmPackArgs la;
  la.packed = p->mem;
  for (int i = 0; i < 2; ++i) {
    const int s = std::min(i, p->n_towers - 1);
    la.w_ih[i] = lstms[s].weight_ih;
    la.w_hh[i] = lstms[s].weight_hh;
    la.b_ih[i] = lstms[s].bias_ih;
    la.b_hh[i] = lstms[s].bias_hh;
    la.off_lw[i] = p->off_lw[s];
    la.off_lb[i] = p->off_lb[s];
  }
  la.D = p->D;
  la.Kp0 = p->Kp0;
  la.H = p->H;
  DeviceGuard dg(p->h);
  if (dg.rc) return dg.rc;
  const uint32_t n_l = (uint32_t)(4 * p->H * (p->Kp0 + p->H) + 4 * p->H);
  hipLaunchKernelGGL(pe_policy_lstm_pack_kernel, dim3((n_l + 255) / 256, (unsigned)p->n_towers), dim3(256), 0,
                     static_cast<hipStream_t>(stream), la);
  hipLaunchKernelGGL(pe_policy_pack_kernel, dim3((most + 255) / 256, (unsigned)nl), dim3(256), 0,
                     static_cast<hipStream_t>(stream), a);
  const hipError_t le = hipGetLastError();
  return le == hipSuccess ? PE_OK : hip_fail(le, "pe_policy_load_lstm");
}

int pe_policy_forward_lstm(pe_policy* p, const void* obs, int32_t obs_is_codes, const uint8_t* start_a,
                           const uint8_t* start_b, int32_t mode, uint64_t seed, uint32_t t, int32_t* actions,
                           float* head0, float* head1, void* stream) {
  if (const int rc = check_forward(p, true, obs, actions, obs_is_codes, mode, head1,
                                   "a feed-forward policy runs with pe_policy_forward"))
    return rc;
  LstmArgs a = lstm_args(p, obs, obs_is_codes, start_a, start_b);
  a.mode = mode;
  a.seed = seed;
  a.t = t;
  a.actions = actions;
  a.head0 = head0;
  a.head1 = head1;
  return kForward.launch(p, a.n, stream, "pe_policy_forward_lstm", a);
}

int pe_policy_value_lstm(pe_policy* p, const void* obs, int32_t obs_is_codes, const uint8_t* start_a,
                         const uint8_t* start_b, const uint8_t* want, const uint8_t* unless, float* values,
                         void* stream) {
  if (const int rc = check_forward(p, true, obs, values, obs_is_codes, PE_POLICY_ARGMAX, nullptr,
                                   "a feed-forward policy runs with pe_policy_value"))
    return rc;
  if (p->n_towers < 2) return fail(PE_ERR_ARG, "values need a second tower");
  const LstmArgs a = lstm_args(p, obs, obs_is_codes, start_a, start_b);
  return kValue.launch(p, a.n, stream, "pe_policy_value_lstm", a, ValueSel{want, unless, values});
}

int pe_policy_lstm_reset_state(pe_policy* p, void* stream) {
  if (!p) return fail(PE_ERR_ARG, "null policy");
  if (!p->H) return fail(PE_ERR_ARG, "not a recurrent policy");
  DeviceGuard dg(p->h);
  if (dg.rc) return dg.rc;
  const hipError_t e = hipMemsetAsync(p->state, 0, (size_t)2 * p->n_towers * p->n_state * sizeof(float),
                                      static_cast<hipStream_t>(stream));
  return e == hipSuccess ? PE_OK : hip_fail(e, "pe_policy_lstm_reset_state");
}

int pe_policy_lstm_get_state(pe_policy* p, int32_t tower, float* h, float* c, void* stream) {
  return state_copy(p, tower, h, c, stream, 1, "pe_policy_lstm_get_state");
}

int pe_policy_lstm_set_state(pe_policy* p, int32_t tower, const float* h, const float* c, void* stream) {
  return state_copy(p, tower, const_cast<float*>(h), const_cast<float*>(c), stream, 0, "pe_policy_lstm_set_state");
}

}  // extern "C"
