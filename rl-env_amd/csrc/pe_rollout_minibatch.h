/* pe_rollout_minibatch.h -- rollout minibatches on the device: the private entry points behind
 * plantos_amd.Rollout.minibatches / env_minibatches / next_minibatch.  NOT part of the C-ABI of
 * include/plantos_batch.h (PE_ABI_VERSION does not move): like pe_internal_plan they are
 * exported with default visibility under pe_internal_* names and bound through
 * plantos_amd._capi.INTERNAL_SIGNATURES.  The definition (the keyed permutation, its Philox
 * counter layout, the normalisation's summation order) is written out in pe_rollout_math.hpp.
 *
 * A minibatch is gathered out of a rollout's own storage: obs row t at buf + t * stride, env
 * e's obs at byte e * D (codes, u8) or 4 * e * D (f32) of it, and five [T, n] fields (plus the
 * episode-start flags in env mode), each with its own row stride in elements.
 *
 * Row mode (PE_MB_ROWS): minibatch k of epoch `epoch` holds positions p = k B + j, j < count =
 * min(B, M - k B), M = T n; position p takes row r = rollout_perm(seed, epoch, rows, M, p),
 * t = r / n, env = r % n.  Outputs [B, ..]: indices[j] = r, obs[j, :] f32 (table[code] on code
 * storage, a copy on f32 storage), optionally the codes themselves, and the five fields at
 * (t, env).  Rows j >= count are written as zeros with indices[j] = -1.
 *
 * Env mode (PE_MB_ENVS): positions run over the n envs, B envs per minibatch:
 * env_j = rollout_perm(seed, epoch, envs, n, k B + j).  Outputs are time-major [T, B, ..]: the
 * same quantities at (t, env_j) plus starts[t, j]; indices[j] = env_j ([B]); and, for each of
 * the n_states state arrays given (f32 [>= 1, n, H]: row 0 is read), state_dst[s][j, :] =
 * state_src[s][0, env_j, :].  Whole sequences of length T: sb3_contrib's split-and-pad sampler
 * is not reproduced.
 *
 * (epoch, k) come by value, or from `ctrl` (device u64[2] = (epoch, next k)) when it is given;
 * then a one-thread kernel behind the gather advances it: k + 1, or (epoch + 1, 0) after the
 * epoch's last minibatch.  `count` (device i32, may be null) receives count.  Everything is
 * launched on `stream`: no sync, no allocation.  PE_ERR_ARG (nothing launched): B < 1, by-value
 * k >= ceil(M / B), T n > 2^31 - 1, a null required pointer, a row stride below n, n_states
 * outside 0..4 or with a null array or H < 1, states in row mode. */
#ifndef PE_ROLLOUT_MINIBATCH_H
#define PE_ROLLOUT_MINIBATCH_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PE_MB_ROWS 0
#define PE_MB_ENVS 1
#define PE_MB_MAX_STATES 4

typedef struct pe_rollout_mb {
  int32_t mode;      /* PE_MB_ROWS / PE_MB_ENVS */
  int32_t T, n, D;   /* the rollout: steps, envs, obs length */
  int32_t B;         /* rows (row mode) or envs (env mode) per minibatch */
  int32_t obs_f32;   /* obs storage: 0 = byte codes, 1 = f32 */
  int32_t n_states;  /* env mode: state arrays to gather, 0..PE_MB_MAX_STATES */
  int32_t H;         /* their row length */
  uint64_t seed, epoch, k; /* epoch, k: ignored when ctrl is given */
  /* the rollout's storage (device) */
  const void* buf;   /* 4-byte aligned */
  int64_t stride;    /* bytes between obs rows */
  int64_t buf_bytes; /* readable bytes at buf (>= (T - 1) * stride + the obs of one row) */
  const float* table; /* f32[256], the value of every code; code storage only */
  const int32_t* actions;
  const float* values;
  const float* log_probs;
  const float* advantages;
  const float* returns;
  const uint8_t* starts; /* env mode */
  int64_t s_actions, s_values, s_log_probs, s_advantages, s_returns, s_starts; /* row strides, elements */
  const float* state_src[PE_MB_MAX_STATES];
  /* control (device, may be null) */
  uint64_t* ctrl;
  int32_t* count;
  /* outputs (device, contiguous); R = B in row mode, T * B in env mode */
  int32_t* indices;       /* [B] */
  float* out_obs;         /* [R, D] */
  uint8_t* out_codes;     /* [R, D], code storage only; may be null */
  int32_t* out_actions;   /* [R] */
  float* out_values;
  float* out_log_probs;
  float* out_advantages;
  float* out_returns;
  uint8_t* out_starts;    /* [R], env mode */
  float* state_dst[PE_MB_MAX_STATES]; /* [B, H] */
} pe_rollout_mb;

/* The argument rules alone (no device): PE_OK or PE_ERR_ARG with pe_last_error set. */
int pe_internal_rollout_minibatch_check(const pe_rollout_mb* a);
int pe_internal_rollout_minibatch(const pe_rollout_mb* a, void* stream);

/* out[j] = rollout_perm(seed, epoch, domain word of `mode`, M, first + j), j < count (host). */
int pe_internal_rollout_perm_host(int64_t M, uint64_t seed, uint64_t epoch, int32_t mode, int64_t first,
                                  int64_t count, int32_t* out);

/* Advantage normalisation over a[t * ld + j], t < rows, j < count (pe_rollout_math.hpp), into
 * out (the same layout; may be a).  Device: count is *count_dev when that is given (device
 * i32; then `count` is its upper bound, which sizes the launch), else `count`.  scratch:
 * device f64[2 * ceil(rows * count / 4096)], needed when rows * count > 4096.  Fewer than 2
 * elements: out = a. */
int pe_internal_rollout_adv_norm(int32_t rows, int32_t count, int64_t ld, const int32_t* count_dev, const float* a,
                                 float* out, double* scratch, void* stream);
int pe_internal_rollout_adv_norm_host(int32_t rows, int32_t count, int64_t ld, const float* a, float* out);

#ifdef __cplusplus
}
#endif
#endif
