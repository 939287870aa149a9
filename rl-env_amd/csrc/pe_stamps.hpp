// pe_stamps.hpp -- the diagnostic phase stamps of the sector kernel and its reset path: the
// PE_STAMP / PE_DSTAMP / PE_RSTAMP macros and the device arrays they write.  Empty statements in
// the product build; tools/stamps.py builds separate libraries with -DPE_STAMPS / -DPE_STAMPS_RESET.
// (a fragment of plantos_batch.hip's anonymous namespace; needs none of the unit's other headers)
#pragma once

// Diagnostic phase stamps (tools/stamps.py builds a SEPARATE library with
// -DPE_STAMPS): lane 0 of every wave of the sector kernel records s_memrealtime
// (100 MHz) at 8 points; pe_debug_stamps() copies them out.  Not in the product build.
#if defined(PE_STAMPS) || defined(PE_STAMPS_RESET)
__device__ uint64_t g_stamps[16384 * 8];
#define PE_STAMP_RAW(k)                                                                     \
  do {                                                                                      \
    uint64_t _t;                                                                            \
    __builtin_amdgcn_sched_barrier(0);                                                      \
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(_t)::"memory");        \
    __builtin_amdgcn_sched_barrier(0);                                                      \
    const int _w = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);                     \
    if ((threadIdx.x & 63) == 0 && _w < 16384) g_stamps[_w * 8 + (k)] = _t;                \
  } while (0)
#endif
#ifdef PE_STAMPS
#define PE_STAMP(k) PE_STAMP_RAW(k)
// done-path stamps of the wave running a block's auto-reset (per block)
__device__ uint64_t g_dstamps[16384 * 8];
#define PE_DSTAMP(k)                                                                        \
  do {                                                                                      \
    uint64_t _t;                                                                            \
    __builtin_amdgcn_sched_barrier(0);                                                      \
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(_t)::"memory");        \
    __builtin_amdgcn_sched_barrier(0);                                                      \
    if ((threadIdx.x & 63) == 0 && blockIdx.x < 16384) g_dstamps[blockIdx.x * 8 + (k)] = _t; \
  } while (0)
#else
#define PE_DSTAMP(k) \
  do {               \
  } while (0)
#define PE_STAMP(k) \
  do {              \
  } while (0)
#endif
#ifdef PE_STAMPS_RESET
#define PE_RSTAMP(k) PE_STAMP_RAW(k)
// where the wave runs: HW_ID (wave slot [3:0], SIMD [5:4], CU [11:8], SH [12], SE [15:13]) | XCC_ID << 32
#define PE_RSTAMP_HWID(k)                                                                   \
  do {                                                                                      \
    uint32_t _h, _x;                                                                        \
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(_h));                       \
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(_x));                      \
    const int _w = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);                     \
    if ((threadIdx.x & 63) == 0 && _w < 16384) g_stamps[_w * 8 + (k)] = (uint64_t)_h | ((uint64_t)_x << 32); \
  } while (0)
#else
#define PE_RSTAMP_HWID(k) \
  do {                    \
  } while (0)
#define PE_RSTAMP(k) \
  do {               \
  } while (0)
#endif
