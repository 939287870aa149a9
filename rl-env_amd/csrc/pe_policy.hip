// pe_policy.hip -- batched MLP policy inference from the obs of a handle's envs to their
// next actions: pe_policy_create / _load / _forward / _forward_rows / _value / _destroy of
// include/plantos_batch.h (the definition of the outputs heads that header's "Policy inference" block; the host
// twin is pe_policy_host.cpp and shares pe_policy_math.hpp with this file; the pieces the
// recurrent policy of pe_policy_lstm.hip uses too are in pe_policy_impl.hpp).
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
#include <string>

#include "pe_policy_impl.hpp"

namespace {

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

template <int ET>
__global__ __launch_bounds__(kThreads) void pe_policy_forward_kernel(FwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int E = 32 * ET;
  float* tab = lds;                    // [256]
  float* hd = tab + 256;               // [kHeadRows][E]
  float* xT = hd + kHeadRows * E;      // [Kp0][E]
  float* h0 = xT + a.Kp0 * E;          // [HB][E] (first the staging image [E][SD])
  float* h1 = h0 + a.HB * E;           // [HB][E]
  const int64_t e0 = (int64_t)blockIdx.x * E;
  const int rows = (int)min((int64_t)E, (int64_t)a.n - e0);

  // 0: obs tile -> staging -> xT
  stage_obs<E>(a.obs, a.obs_is_codes, a.tab, tab, h0, xT, e0, rows, a.D, a.SD, a.Kp0);

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
    head_layer<E>(a.packed, tw.l[tw.n_hidden], tw.n_out, ti, in, hd);
    __syncthreads();  // the next tower overwrites h0 / h1; the epilogue reads hd
  }

  // 3: action + outputs
  act_and_store<E>(hd, a.tw[0].n_out, rows, e0, a.mode, a.seed, a.env_off, a.t, a.actions, a.head0, a.head1);
}

// pe_policy_value: the forward kernel cut down to tower 1 and values[e] of the selected envs.
// A workgroup none of whose envs is selected returns before it reads obs.  A kernel of its
// own, so that the forward kernel's code stays as it was; the stages are the same calls.
template <int ET>
__global__ __launch_bounds__(kThreads) void pe_policy_value_kernel(FwdArgs a, ValueSel s) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int E = 32 * ET;
  float* tab = lds;                    // the forward kernel's images
  float* hd = tab + 256;
  float* xT = hd + kHeadRows * E;
  float* h0 = xT + a.Kp0 * E;
  float* h1 = h0 + a.HB * E;
  const int64_t e0 = (int64_t)blockIdx.x * E;
  const int rows = (int)min((int64_t)E, (int64_t)a.n - e0);

  const bool sel = selected(s, e0, rows);
  if (!block_any(sel, hd)) return;  // uniform: every thread of the workgroup leaves, before any other barrier

  stage_obs<E>(a.obs, a.obs_is_codes, a.tab, tab, h0, xT, e0, rows, a.D, a.SD, a.Kp0);
  const Tower& tw = a.tw[1];
  const float* in = xT;
  for (int l = 0; l < tw.n_hidden; ++l) {
    const Layer& L = tw.l[l];
    float* out = (l & 1) ? h1 : h0;
    hidden_layer<ET, float>(a.packed + L.off_w, a.packed + L.off_b, in, out, L.Kp >> 3, L.N >> 5, a.act);
    __syncthreads();
    in = out;
  }
  head_layer<E>(a.packed, tw.l[tw.n_hidden], tw.n_out, 1, in, hd);
  __syncthreads();
  store_values<E>(hd, sel, e0, s.values);
}

// ---------------------------------------------------------------- host side
const TileKernel kForward(pe_policy_forward_kernel<1>, pe_policy_forward_kernel<2>);
const TileKernel kValue(pe_policy_value_kernel<1>, pe_policy_value_kernel<2>);

// What every launch of p reads; the sampler and output fields are left zero.
FwdArgs fwd_args(const pe_policy* p, const void* obs, int32_t obs_is_codes) {
  FwdArgs a{};
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
  a.env_off = p->h->cfg.env_id_offset;
  a.tw[0] = p->tw[0];
  a.tw[1] = p->tw[p->n_towers - 1];
  return a;
}

}  // namespace

// The PE_PREC_BF16 side (pe_policy_bf16.hip); the arguments are checked here.
extern "C" {
int pe_internal_policy_bf16_create(pe_handle* h, const PolicyPlan* plan, pe_policy** out);
int pe_internal_policy_bf16_load(pe_policy* p, const pe_policy_tower* towers, void* stream);
int pe_internal_policy_bf16_forward(pe_policy* p, int32_t rows, const void* obs, int32_t obs_is_codes, int32_t mode,
                                    uint64_t seed, uint32_t t, int32_t* actions, float* head0, float* head1,
                                    void* stream, const char* what);
int pe_internal_policy_bf16_value(pe_policy* p, const void* obs, int32_t obs_is_codes, const uint8_t* want,
                                  const uint8_t* unless, float* values, void* stream);
}

extern "C" {

int pe_internal_policy_plan(int32_t D, int32_t n_envs, int32_t num_cus, int32_t n_towers, const pe_policy_lstm* lstms,
                            const pe_policy_tower* shapes, int32_t activation, int32_t env_tile,
                            pe_policy_plan_info* out) {
  if (!out) return fail(PE_ERR_ARG, "null argument");
  PolicyPlan plan;
  if (const int rc = make_policy_plan(D, n_envs, num_cus, n_towers, lstms, shapes, activation, env_tile, lstms != nullptr,
                                      &plan))
    return rc;
  *out = {plan.env_tile, (uint64_t)plan.lds, (uint64_t)plan.n_packed, (uint64_t)plan.n_state};
  return PE_OK;
}

int pe_internal_policy_plan_prec(int32_t D, int32_t n_envs, int32_t num_cus, int32_t n_towers,
                                 const pe_policy_lstm* lstms, const pe_policy_tower* shapes, int32_t activation,
                                 int32_t env_tile, int32_t precision, pe_policy_plan_info* out) {
  if (!out) return fail(PE_ERR_ARG, "null argument");
  if (lstms) {
    if (precision != PE_PREC_F32) return fail(PE_ERR_ARG, "a recurrent policy has no reduced precision");
    return pe_internal_policy_plan(D, n_envs, num_cus, n_towers, lstms, shapes, activation, env_tile, out);
  }
  PolicyPlan plan;
  if (const int rc = make_policy_plan_prec(D, n_envs, num_cus, n_towers, shapes, activation, env_tile, precision, &plan))
    return rc;
  *out = {plan.env_tile, (uint64_t)plan.lds, (uint64_t)plan.n_packed, (uint64_t)plan.n_state};
  return PE_OK;
}

int pe_policy_create_prec(pe_handle* h, int32_t n_towers, const pe_policy_tower* shapes, int32_t activation,
                          int32_t env_tile, int32_t precision, pe_policy** out) {
  if (!h || !out) return fail(PE_ERR_ARG, "null argument");
  PolicyPlan plan;
  if (const int rc = make_policy_plan_prec(h->g.D, h->n, h->num_cus, n_towers, shapes, activation, env_tile, precision,
                                           &plan))
    return rc;
  if (plan.precision == PE_PREC_BF16) return pe_internal_policy_bf16_create(h, &plan, out);
  return create_policy(h, plan, {kForward.of(plan), n_towers == 2 ? kValue.of(plan) : nullptr}, "pe_policy_create", out);
}

int pe_policy_create(pe_handle* h, int32_t n_towers, const pe_policy_tower* shapes, int32_t activation,
                     int32_t env_tile, pe_policy** out) {
  return pe_policy_create_prec(h, n_towers, shapes, activation, env_tile, PE_PREC_F32, out);
}

int32_t pe_policy_precision(const pe_policy* p) { return p ? p->precision : -1; }

int pe_policy_destroy(pe_policy* p) {
  if (!p) return PE_OK;
  DeviceGuard dg(p->h);
  const hipError_t e = free_policy(p);
  return e == hipSuccess ? PE_OK : hip_fail(e, "hipFree");
}

int32_t pe_policy_env_tile(const pe_policy* p) { return p ? p->env_tile : 0; }

int pe_policy_load(pe_policy* p, const pe_policy_tower* towers, void* stream) {
  if (!p || !towers) return fail(PE_ERR_ARG, "null argument");
  if (p->H) return fail(PE_ERR_ARG, "a recurrent policy is loaded with pe_policy_load_lstm");
  if (p->precision == PE_PREC_BF16) return pe_internal_policy_bf16_load(p, towers, stream);
  PackArgs a;
  int nl = 0;
  uint32_t most = 0;
  if (const int rc = pack_towers(p, towers, &a, &nl, &most)) return rc;
  DeviceGuard dg(p->h);
  if (dg.rc) return dg.rc;
  hipLaunchKernelGGL(pe_policy_pack_kernel, dim3((most + 255) / 256, (unsigned)nl), dim3(256), 0,
                     static_cast<hipStream_t>(stream), a);
  const hipError_t le = hipGetLastError();
  return le == hipSuccess ? PE_OK : hip_fail(le, "pe_policy_load");
}

int pe_policy_forward(pe_policy* p, const void* obs, int32_t obs_is_codes, int32_t mode, uint64_t seed,
                      uint32_t t, int32_t* actions, float* head0, float* head1, void* stream) {
  if (const int rc = check_forward(p, false, obs, actions, obs_is_codes, mode, head1,
                                   "a recurrent policy runs with pe_policy_forward_lstm"))
    return rc;
  if (p->precision == PE_PREC_BF16)
    return pe_internal_policy_bf16_forward(p, p->h->n, obs, obs_is_codes, mode, seed, t, actions, head0, head1, stream,
                                           "pe_policy_forward");
  FwdArgs a = fwd_args(p, obs, obs_is_codes);
  a.mode = mode;
  a.seed = seed;
  a.t = t;
  a.actions = actions;
  a.head0 = head0;
  a.head1 = head1;
  return kForward.launch(p, a.n, stream, "pe_policy_forward", a);
}

int pe_policy_forward_rows(pe_policy* p, int32_t rows, const void* obs, int32_t obs_is_codes, int32_t* actions,
                           float* head0, float* head1, void* stream) {
  if (const int rc = check_forward(p, false, obs, actions, obs_is_codes, PE_POLICY_ARGMAX, head1,
                                   "pe_policy_forward_rows does not evaluate a recurrent policy"))
    return rc;
  if (rows < 1) return fail(PE_ERR_ARG, "rows must be >= 1, got " + std::to_string(rows));
  if (p->precision == PE_PREC_BF16)
    return pe_internal_policy_bf16_forward(p, rows, obs, obs_is_codes, PE_POLICY_ARGMAX, 0, 0, actions, head0, head1,
                                           stream, "pe_policy_forward_rows");
  FwdArgs a = fwd_args(p, obs, obs_is_codes);
  a.n = rows;  // the kernel bounds its last tile, its loads and its stores by a.n
  a.mode = PE_POLICY_ARGMAX;
  a.actions = actions;
  a.head0 = head0;
  a.head1 = head1;
  return kForward.launch(p, rows, stream, "pe_policy_forward_rows", a);
}

int pe_policy_value(pe_policy* p, const void* obs, int32_t obs_is_codes, const uint8_t* want, const uint8_t* unless,
                    float* values, void* stream) {
  if (const int rc = check_forward(p, false, obs, values, obs_is_codes, PE_POLICY_ARGMAX, nullptr,
                                   "a recurrent policy runs with pe_policy_value_lstm"))
    return rc;
  if (p->n_towers < 2) return fail(PE_ERR_ARG, "values need a second tower");
  if (p->precision == PE_PREC_BF16) return pe_internal_policy_bf16_value(p, obs, obs_is_codes, want, unless, values, stream);
  const FwdArgs a = fwd_args(p, obs, obs_is_codes);
  return kValue.launch(p, a.n, stream, "pe_policy_value", a, ValueSel{want, unless, values});
}

}  // extern "C"
