// pe_tile.hpp -- the obs tile stores of the step kernels: f32 rows, byte codes expanded through
// the LDS code table, byte codes as they are; and the write-through 16-B store they are made of.
// (a fragment of plantos_batch.hip's anonymous namespace; include after pe_step_args.hpp)
#pragma once

// One 16-B store of the obs stream.  The stream (28 MB per step at the headline batch) is written
// with sc1 (write-through; the line is dropped from the XCD's L2) so it does not evict the envs'
// state from L2 / the Infinity Cache: plain stores 12.8 us, nt 11.4, sc1 11.1 us per step
// (profiles/r1i_store_policy.json).  Inline asm: the compiler does not count these stores in
// vmcnt, so the reset path waits for them explicitly (s_waitcnt vmcnt(0)) before it reads what
// they wrote.  s_nop 1: a 128-bit store reads its data VGPRs after issue; nothing inside the asm
// pads that hazard for hipcc's next write of them.  V4: a 16-B vector type.
template <typename V4>
__device__ __forceinline__ void store16_wt(void* dst, const V4& v) {
  static_assert(sizeof(V4) == 16, "one dwordx4");
  asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(dst), "v"(v) : "memory");
}

// Stream the block's [valid x D] obs tile (LDS rows of stride DS) to HBM.
// t0 / nt: this thread's index among the nt storing threads (default: the block).
// obs tile store: 16-B chunks per thread read from LDS ahead of their stores (f32 20x20: 3 same, 9 slower)
constexpr int kTileBatch = 1;
constexpr int kTileBatchCodes = 4;  // the same for the byte-coded tile (64x64: 25.6 -> 23.0 us; 2: 23.2, 6: 23.6)
__device__ __forceinline__ void store_tile(const float* rows, float* dst, int valid, int D, int DS,
                                           int t0 = -1, int nt = 0) {
  const int total = valid * D;
  const int tid = t0 < 0 ? (int)threadIdx.x : t0;
  const int nth = t0 < 0 ? (int)blockDim.x : nt;
  if (DS == D) {
    if ((reinterpret_cast<uintptr_t>(dst) & 15u) == 0) {
      const int n4 = total >> 2;
      float4* d4 = reinterpret_cast<float4*>(dst);
      typedef float v4f __attribute__((ext_vector_type(4)));
      const v4f* sv = reinterpret_cast<const v4f*>(rows);
      // kTileBatch chunks per thread read from LDS before their stores are issued:
      // the asm's memory clobber keeps a later LDS read below an earlier store, so
      // one chunk at a time would wait out an LDS round trip per store
      constexpr int TB = kTileBatch;
      for (int k0 = tid; k0 < n4; k0 += TB * nth) {
        v4f v[TB];
#pragma unroll
        for (int b = 0; b < TB; ++b)
          if (k0 + b * nth < n4) v[b] = sv[k0 + b * nth];
#pragma unroll
        for (int b = 0; b < TB; ++b)
          if (k0 + b * nth < n4) store16_wt(d4 + k0 + b * nth, v[b]);
      }
      for (int k = (n4 << 2) + tid; k < total; k += nth) dst[k] = rows[k];
    } else {
      for (int k = tid; k < total; k += nth) dst[k] = rows[k];
    }
  } else {
    for (int k = tid; k < total; k += nth) {
      int r = k / D, c = k - r * D;
      dst[k] = rows[r * DS + c];
    }
  }
}

// Stream the block's byte-coded [valid x D] obs tile (contiguous codes, pe_coop.hpp
// ObsW<uint8_t>) to HBM as floats: 4 codes per thread and step expanded through the
// LDS code table ctab[256] into one 16-B store (same store policy as store_tile).
__device__ __forceinline__ void store_tile_codes(const uint8_t* codes, const float* ctab, float* dst, int valid, int D,
                                                 int t0, int nt) {
  const int total = valid * D;
  if ((reinterpret_cast<uintptr_t>(dst) & 15u) == 0) {
    const int n4 = total >> 2;
    const uint32_t* c4 = reinterpret_cast<const uint32_t*>(codes);
    typedef float v4f __attribute__((ext_vector_type(4)));
    v4f* d4 = reinterpret_cast<v4f*>(dst);
    constexpr int TB = kTileBatchCodes;  // chunks per thread expanded before their stores (see store_tile)
    for (int k0 = t0; k0 < n4; k0 += TB * nt) {
      uint32_t c[TB];
#pragma unroll
      for (int b = 0; b < TB; ++b) c[b] = k0 + b * nt < n4 ? c4[k0 + b * nt] : 0u;
      v4f v[TB];
#pragma unroll
      for (int b = 0; b < TB; ++b) {
        v[b].x = ctab[c[b] & 255u];
        v[b].y = ctab[(c[b] >> 8) & 255u];
        v[b].z = ctab[(c[b] >> 16) & 255u];
        v[b].w = ctab[c[b] >> 24];
      }
#pragma unroll
      for (int b = 0; b < TB; ++b)
        if (k0 + b * nt < n4) store16_wt(d4 + k0 + b * nt, v[b]);
    }
    for (int k = (n4 << 2) + t0; k < total; k += nt) dst[k] = ctab[codes[k]];
  } else {
    for (int k = t0; k < total; k += nt) dst[k] = ctab[codes[k]];
  }
}

// The byte-coded tile as it is (pe_step_codes): [valid x D] codes, 16-B sc1 stores
// where the destination allows, bytes for the rest.
__device__ __forceinline__ void store_tile_bytes(const uint8_t* codes, uint8_t* dst, int valid, int D, int t0,
                                                 int nt) {
  const int total = valid * D;
  int head = 0;
  if ((reinterpret_cast<uintptr_t>(dst) & 15u) == 0) {
    const int n16 = total >> 4;
    typedef uint32_t v4u __attribute__((ext_vector_type(4)));
    const v4u* sv = reinterpret_cast<const v4u*>(codes);
    v4u* d4 = reinterpret_cast<v4u*>(dst);
    for (int k = t0; k < n16; k += nt) {
      store16_wt(d4 + k, sv[k]);
    }
    head = n16 << 4;
  }
  for (int k = head + t0; k < total; k += nt) dst[k] = codes[k];
}
