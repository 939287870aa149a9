// pe_expand_codes.hpp -- pe_expand_codes_kernel, the expansion of packed byte-coded obs blocks to
// floats (pe_expand_obs_codes).  Not in the anonymous namespace: include after it closes.
// (needs pe_coop.hpp's obs_code_loads / obs_code_pick and pe_tile.hpp)
#pragma once

// pe_expand_obs_codes: blocks x rows packed code buffers (codes u8 [rows, D] | reward
// f32 | terminated | truncated, block b at src + b * stride) -> contiguous f32 obs
// (+ the other outputs).  Grid: (x: 16-B output chunks, y: block); one u32 of 4 codes
// per thread through the LDS code table, one 16-B store.
constexpr int kExpandPer = 4;  // 4-code groups per thread (the table build amortized over them)
__global__ __launch_bounds__(256) void pe_expand_codes_kernel(const Tables* tab, int R, int G, int D, int rows,
                                                              const uint8_t* src, int64_t stride, float* obs,
                                                              float* rew, uint8_t* te, uint8_t* tr) {
  __shared__ float ctab[256];
  const CodeLd cld = obs_code_loads(tab, R, G, (int)threadIdx.x);  // (with the code loads: one round trip)
  const int b = blockIdx.y;
  const uint8_t* sb = src + (int64_t)b * stride;
  const int64_t nc = (int64_t)rows * D;  // codes per block
  float* ob = obs + (int64_t)b * nc;
  // a workgroup expands 256 * kExpandPer consecutive 4-code groups; thread t the groups
  // g0 + t + 256 j (each load and each 16-B store instruction contiguous over the wave),
  // every code word loaded before the table barrier
  const int64_t g0 = (int64_t)blockIdx.x * 256 * kExpandPer + threadIdx.x;
  if ((nc & 3) == 0) {
    uint32_t c[kExpandPer];
#pragma unroll
    for (int j = 0; j < kExpandPer; ++j) {
      const int64_t k = g0 + 256 * j;
      c[j] = 4 * k < nc ? *reinterpret_cast<const uint32_t*>(sb + 4 * k) : 0u;
    }
    ctab[threadIdx.x] = obs_code_pick(cld, R, G, (int)threadIdx.x);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kExpandPer; ++j) {
      const int64_t k = g0 + 256 * j;
      if (4 * k < nc) {
        typedef float v4f __attribute__((ext_vector_type(4)));
        v4f v;
        v.x = ctab[c[j] & 255u];
        v.y = ctab[(c[j] >> 8) & 255u];
        v.z = ctab[(c[j] >> 16) & 255u];
        v.w = ctab[c[j] >> 24];
        // the expanded obs stream write-through, as the step kernels' tile stores (expansion
        // 7.85 -> 5.93 us, gather leg 20.45 -> 19.4)
        store16_wt(ob + 4 * k, v);
      }
    }
  } else {
    ctab[threadIdx.x] = obs_code_pick(cld, R, G, (int)threadIdx.x);
    __syncthreads();
    for (int j = 0; j < kExpandPer; ++j) {
      const int64_t k = g0 + 256 * j;
      for (int64_t i = 4 * k; i < 4 * k + 4 && i < nc; ++i) ob[i] = ctab[sb[i]];
    }
  }
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;  // the per-env outputs below
  // the per-env outputs: one env per thread of the first ceil(rows / 256) workgroups
  if (k < rows) {
    const int64_t ro = (nc + 15) & ~(int64_t)15;
    const int64_t o = (int64_t)b * rows + k;
    if (rew) rew[o] = reinterpret_cast<const float*>(sb + ro)[k];
    if (te) te[o] = sb[ro + 4 * (int64_t)rows + k];
    if (tr) tr[o] = sb[ro + 5 * (int64_t)rows + k];
  }
}
