/* pe_learner.h -- the A2C learner on the device: the private entry points behind
 * plantos_amd.A2CLearner.  NOT part of the C-ABI of include/plantos_batch.h (PE_ABI_VERSION does
 * not move): like pe_internal_plan they are exported under pe_internal_* names and bound through
 * plantos_amd._capi.INTERNAL_SIGNATURES.  What an update computes is written out in
 * pe_learner_math.hpp; pe_internal_learner_update_host is that definition executed on the host.
 *
 * A learner owns no memory: its caller allocates what pe_internal_learner_plan asks for and hands
 * the device pointers over in a pe_learner_bufs, once.  After that an update launches kernels on
 * the caller's stream and nothing else: no sync, no allocation, the update counter on the device. */
#ifndef PE_LEARNER_H
#define PE_LEARNER_H
#include <stdint.h>

#include "../../include/plantos_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pe_learner pe_learner;

/* What a learner of a two-tower f32 policy over obs rows of D values and at most max_rows rows
 * per update is made of (pe_learner_plan.hpp): no HIP call. */
typedef struct pe_learner_plan_info {
  int32_t env_tile;         /* rows per workgroup of the forward + backward-data kernel: 32 or 64 */
  int32_t n_layers;         /* weight-gradient problems: every layer of both towers */
  int32_t grad_chunk;       /* kGradChunk */
  int32_t max_chunks;       /* ceil(max_rows / kGradChunk) */
  int32_t wgrad_groups;     /* workgroups of the weight-gradient kernel per chunk */
  int32_t sum_chunks;       /* kNormChunk chunks of the longer of (rows, parameters) */
  uint64_t lds_bytes;       /* dynamic LDS of a forward + backward-data workgroup */
  uint64_t n_params;        /* floats of the master parameters (= gradients = square_avg) */
  uint64_t ws_floats;       /* the workspace: obs, activations, dZ, head gradients, row terms */
  uint64_t partial_floats;  /* the chunk partials: max_chunks * n_params */
  uint64_t sums_doubles;    /* 4 * sum_chunks */
  uint64_t packed_floats;   /* the forward's packed weights (pe_policy_plan_info.packed_floats) */
  uint64_t packed_t_floats; /* the transposed packed weights of the backward-data layers */
} pe_learner_plan_info;

int pe_internal_learner_plan(int32_t D, int32_t max_rows, int32_t num_cus, int32_t n_towers,
                             const pe_policy_tower* shapes, int32_t activation, int32_t env_tile,
                             pe_learner_plan_info* out);

/* Device buffers of the sizes the plan gives, all 16-byte aligned. */
typedef struct pe_learner_bufs {
  float* params;      /* [n_params]: tower, layer, weight [N, K] then bias [N] */
  float* grads;       /* [n_params]: the gradients before the clip */
  float* square_avg;  /* [n_params] */
  float* out;         /* [8]: policy_loss, value_loss, entropy_loss, loss, grad_norm, clip_coef */
  int64_t* n_updates; /* [1] */
  float* ws;
  float* partials;
  double* sums;
  float* packed;
  float* packed_t;
} pe_learner_bufs;

/* A learner of `policy` (two towers, f32, feed-forward; its env_tile and code table are used).
 * PE_ERR_ARG otherwise, or for max_rows < 1 or a null buffer. */
int pe_internal_learner_create(pe_policy* policy, int32_t max_rows, const pe_learner_bufs* bufs, pe_learner** out);
int pe_internal_learner_destroy(pe_learner* l);

/* Repacks bufs->params for the learner's kernels and into the policy (pe_policy_load's kernel). */
int pe_internal_learner_repack(pe_learner* l, void* stream);

/* One update over `rows` <= max_rows rows (PE_ERR_ARG beyond): obs u8 codes or f32 [rows, D]. */
int pe_internal_learner_update(pe_learner* l, int32_t rows, const void* obs, int32_t obs_is_codes,
                               const int32_t* actions, const float* advantages, const float* returns,
                               double learning_rate, double ent_coef, double vf_coef, double max_grad_norm,
                               double alpha, double rms_prop_eps, void* stream);

/* The host twin: towers' tensors (host, torch layout) and square_avg [n_params] are updated in
 * place; grads [n_params] and out [8] are written.  apply = 0: gradients and scalars only. */
int pe_internal_learner_update_host(int32_t rows, int32_t D, int32_t n_towers, const pe_policy_tower* towers,
                                    int32_t activation, const float* obs, const int32_t* actions,
                                    const float* advantages, const float* returns, double learning_rate,
                                    double ent_coef, double vf_coef, double max_grad_norm, double alpha,
                                    double rms_prop_eps, int32_t apply, float* square_avg, float* grads, float* out);

#ifdef __cplusplus
}
#endif
#endif
