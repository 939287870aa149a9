// pe_mcts_rng.hpp -- an env's np.random stream (numpy legacy RandomState = MT19937) in the MCTS
// search (a part of pe_mcts.hip; pe_mcts.hip's file comment describes the device form).  First
// the half that is plain C++ -- the twist of one word and the conversions between numpy's
// (key, pos) and the device form, which a host compiler takes as they are
// (tools/mcts_host_check.cpp) -- then, for hipcc, the device half: NpStream and the seed kernel.
#pragma once
#include <cstdint>
#include <cstring>

#include "pe_mcts_plan.hpp"

#ifdef __HIPCC__
#define PE_MC_HD __host__ __device__ __forceinline__
#else
#define PE_MC_HD inline
#endif

namespace {

using namespace pe_mc;

constexpr int kMtN = 624, kMtM = 397;
constexpr uint32_t kUpper = 0x80000000u, kLower = 0x7fffffffu, kMag = 0x9908b0dfu;

PE_MC_HD uint32_t twist(uint32_t cur, uint32_t nxt, uint32_t far) {
  const uint32_t y = (cur & kUpper) | (nxt & kLower);
  return far ^ (y >> 1) ^ ((y & 1u) ? kMag : 0u);
}

// stream position i in [0, 2 * 624) -> [0, 624).  The host conversions use it; the device code
// below keeps its wrap spelled out at each site, because the compiler orders the same
// compare-and-select differently once it comes out of a function.
PE_MC_HD int mt_wrap(int i) { return i - (i >= kMtN ? kMtN : 0); }

// numpy (key, pos) -> device form (host; see pe_mcts.hip's file comment)
inline void np_to_device(const uint32_t* key, int pos, uint32_t* out) {
  std::memcpy(out, key, kMtN * sizeof(uint32_t));
  out[kMtN + 1] = key[0];
  out[kMtN + 2] = out[kMtN + 3] = 0;
  const int upto = pos >= kMtN ? kMtN : pos;
  for (int i = 0; i < upto; ++i) out[i] = twist(out[i], out[mt_wrap(i + 1)], out[mt_wrap(i + kMtM)]);
  out[kMtN] = (uint32_t)(pos >= kMtN ? 0 : pos);
}

// device form -> numpy (key, pos): undo the twist of the words below pos.
inline void device_to_np(const uint32_t* dev, uint32_t* key, int32_t* pos) {
  const int p = (int)dev[kMtN];
  std::memcpy(key, dev, kMtN * sizeof(uint32_t));
  *pos = p;
  if (p == 0) return;  // a fresh round: (twisted words, pos 0) is numpy's own form too
  // y_i from new[i] = far_i ^ (y_i >> 1) ^ (y_i & 1 ? MAG : 0)
  auto far_of = [&](int i) -> uint32_t { return (i + kMtM < kMtN ? key : dev)[mt_wrap(i + kMtM)]; };
  auto y_of = [&](int i) -> uint32_t {
    uint32_t t = dev[i] ^ far_of(i);
    const uint32_t b = t >> 31;
    if (b) t ^= kMag;
    return (t << 1) | b;
  };
  for (int j = p - 1; j >= 1; --j) key[j] = (y_of(j) & kUpper) | (y_of(j - 1) & kLower);
  key[0] = dev[kMtN + 1];
}

}  // namespace

#ifdef __HIPCC__
namespace {

__device__ __forceinline__ uint32_t temper(uint32_t y) {
  y ^= y >> 11;
  y ^= (y << 7) & 0x9d2c5680u;
  y ^= (y << 15) & 0xefc60000u;
  y ^= y >> 18;
  return y;
}

__device__ __forceinline__ uint32_t untemper(uint32_t y) {
  y ^= y >> 18;
  y ^= (y << 15) & 0xefc60000u;
  uint32_t t = y;
#pragma unroll
  for (int i = 0; i < 4; ++i) t = y ^ ((t << 7) & 0x9d2c5680u);
  y = t;
  return y ^ (y >> 11) ^ (y >> 22);
}

constexpr int kTop = 16;   // draws per top-up: one 16-aligned block of stream positions
constexpr int kLow = 8;    // the wave tops up when any lane has fewer left (> draws of one step, typically)
static_assert(kMtN % kTop == 0 && kRngStride % 4 == 0, "16-aligned blocks never straddle the wrap");

// One env's np.random stream, device form (see pe_mcts.hip's file comment).  Draws are
// generated ahead into an LDS ring, one 16-aligned block of stream positions per
// top-up: the block's words, its successors and its "far" words (+397) come in as
// 16-B loads and the next-round words go out as 16-B stores.  Top-ups are
// wave-uniform (top_up_if_low), so a wave pays one memory round trip for all its
// lanes.  Until the position is 16-aligned (a stream left mid-block by a previous
// search) draws come one at a time (gen_direct).  close() rewinds the
// generated-but-unconsumed tail (raw word = untemper(output)), so the stored stream
// stops exactly at the first unconsumed draw.  The ring is [slot][lane] interleaved
// (a top-up's 64 lanes write one slot row: no bank conflicts).
struct NpStream {
  uint32_t* mt;
  uint32_t* ring;      // &ring_base[lane]; slot k at ring[k * 64]
  int p;               // position of the next draw to generate
  uint32_t cur;        // mt[p] (the current-round word at p)
  int head, cnt;       // ring read slot, draws buffered
  uint32_t saved_prev; // mt[625] before the last generation of position 0
#ifdef PE_MCTS_PROF  // diagnostics build: shader-clock cycles spent in top-ups
  uint64_t topups = 0;
#define PE_MP_TOPUP(call)                                  \
  do {                                                     \
    const uint64_t t0 = __builtin_amdgcn_s_memtime();      \
    call;                                                  \
    topups += __builtin_amdgcn_s_memtime() - t0;           \
  } while (0)
#else
#define PE_MP_TOPUP(call) call
#endif

  __device__ void open(uint32_t* m, uint32_t* r) {
    mt = m;
    ring = r;
    p = (int)m[kMtN];
    cur = m[p];
    head = 0;
    cnt = 0;
    saved_prev = m[kMtN + 1];
  }
  __device__ void top_up() {  // positions p .. p+15 (p % 16 == 0, cnt <= kRing - kTop)
    const uint4* m4 = reinterpret_cast<const uint4*>(mt);
    uint32_t nx[kTop], far[kTop];
    // successors p+1 .. p+16: the block itself shifted by one, plus the next block's first word
    const uint4 b0 = m4[p / 4], b1 = m4[p / 4 + 1], b2 = m4[p / 4 + 2], b3 = m4[p / 4 + 3];
    int pn = p + kTop;
    pn -= pn >= kMtN ? kMtN : 0;
    const uint32_t w16 = mt[pn];
    // far words p+397 .. p+412 lie in the 4-word chunks starting at p+396, +400, ..., +412
    uint4 f[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      int q = p + 396 + 4 * k;
      q -= q >= kMtN ? kMtN : 0;
      q -= q >= kMtN ? kMtN : 0;
      f[k] = m4[q / 4];
    }
    const uint32_t blk[16] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w,
                              b2.x, b2.y, b2.z, b2.w, b3.x, b3.y, b3.z, b3.w};
    const uint32_t fw[20] = {f[0].x, f[0].y, f[0].z, f[0].w, f[1].x, f[1].y, f[1].z, f[1].w,
                             f[2].x, f[2].y, f[2].z, f[2].w, f[3].x, f[3].y, f[3].z, f[3].w,
                             f[4].x, f[4].y, f[4].z, f[4].w};
#pragma unroll
    for (int k = 0; k < kTop; ++k) {
      nx[k] = k + 1 < kTop ? blk[k + 1] : w16;
      far[k] = fw[k + 1];
    }
    if (p == 0) {  // this round's mt[0], kept for pe_mcts_get_rng
      saved_prev = mt[kMtN + 1];
      mt[kMtN + 1] = cur;
    }
    uint32_t nw[kTop];
    const int slot0 = (head + cnt) & (kRing - 1);
#pragma unroll
    for (int k = 0; k < kTop; ++k) {
      nw[k] = twist(cur, nx[k], far[k]);
      ring[((slot0 + k) & (kRing - 1)) * 64] = temper(cur);
      cur = nx[k];
    }
    uint4* o4 = reinterpret_cast<uint4*>(mt) + p / 4;
    o4[0] = make_uint4(nw[0], nw[1], nw[2], nw[3]);
    o4[1] = make_uint4(nw[4], nw[5], nw[6], nw[7]);
    o4[2] = make_uint4(nw[8], nw[9], nw[10], nw[11]);
    o4[3] = make_uint4(nw[12], nw[13], nw[14], nw[15]);
    p = pn;
    cnt += kTop;
  }
  __device__ void top_up_if_low() {
    if (__any(cnt < kLow) && cnt <= kRing - kTop && (p & (kTop - 1)) == 0) PE_MP_TOPUP(top_up());
  }
  // one draw straight from the stream (ring empty: before the first aligned block,
  // or a long rejection streak)
  __device__ uint32_t gen_direct() {
    int i1 = p + 1, i2 = p + kMtM;
    i1 -= i1 >= kMtN ? kMtN : 0;
    i2 -= i2 >= kMtN ? kMtN : 0;
    const uint32_t nxt = mt[i1], far = mt[i2];
    if (p == 0) {
      saved_prev = mt[kMtN + 1];
      mt[kMtN + 1] = cur;
    }
    mt[p] = twist(cur, nxt, far);
    const uint32_t v = temper(cur);
    cur = nxt;
    p = i1;
    return v;
  }
  __device__ uint32_t next() {
    if (cnt == 0) return gen_direct();
    const uint32_t v = ring[head * 64];
    head = (head + 1) & (kRing - 1);
    --cnt;
    return v;
  }
  // two draws: both ring reads issued before any branch (the ring is rarely short)
  __device__ void next2(uint32_t& a, uint32_t& b) {
    const uint32_t r0 = ring[head * 64], r1 = ring[((head + 1) & (kRing - 1)) * 64];
    if (cnt >= 2) {
      a = r0;
      b = r1;
      head = (head + 2) & (kRing - 1);
      cnt -= 2;
    } else {
      a = next();
      b = next();
    }
  }
  __device__ void close() {
    int q = p - cnt;
    q += q < 0 ? kMtN : 0;
    for (int j = 0; j < cnt; ++j) {  // rewind the unconsumed tail
      int pos = q + j;
      pos -= pos >= kMtN ? kMtN : 0;
      mt[pos] = untemper(ring[((head + j) & (kRing - 1)) * 64]);
      if (pos == 0) mt[kMtN + 1] = saved_prev;
    }
    mt[kMtN] = (uint32_t)q;
  }
  // np.random.random() < 0.7, decided on the 53 bits of its two draws: random() =
  // ((a >> 5) * 2^26 + (b >> 6)) / 2^53 = N / 2^53 exactly and the double 0.7 is
  // 6305039478318694 / 2^53, so the comparison is N < that.
  __device__ bool random_lt_07() {
    uint32_t a, b;
    next2(a, b);
    const uint64_t nbits = ((uint64_t)(a >> 5) << 26) | (uint64_t)(b >> 6);
    return nbits < 6305039478318694ull;
  }
  // np.random.randint(n): masked rejection on 32-bit draws, no draw for n == 1
  __device__ int randint(int n) {
    const uint32_t rng = (uint32_t)(n - 1);
    if (rng == 0) return 0;
    uint32_t mask = rng;
    mask |= mask >> 1;
    mask |= mask >> 2;
    mask |= mask >> 4;
    mask |= mask >> 8;
    mask |= mask >> 16;
    uint32_t v;
    while ((v = (next() & mask)) > rng) {
    }
    return (int)v;
  }
};

// np.random.seed(seed) (init_genrand, pos 624) then the pending block twist, giving
// the device form at position 0.  One thread per env.
__global__ void pe_mcts_seed_kernel(uint32_t* rng, int n, const uint32_t* seeds, uint32_t base) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  uint32_t* mt = rng + e * (int64_t)kRngStride;
  uint32_t v = seeds ? seeds[e] : base + (uint32_t)e;
  mt[0] = v;
  for (int i = 1; i < kMtN; ++i) {
    v = 1812433253u * (v ^ (v >> 30)) + (uint32_t)i;
    mt[i] = v;
  }
  uint32_t first = mt[0];
  uint32_t cur = first;
  for (int i = 0; i < kMtN; ++i) {
    const uint32_t nxt = i + 1 < kMtN ? mt[i + 1] : mt[0];
    const uint32_t far = mt[i + kMtM < kMtN ? i + kMtM : i + kMtM - kMtN];
    mt[i] = twist(cur, nxt, far);
    cur = nxt;
  }
  mt[kMtN] = 0;
  mt[kMtN + 1] = first;
  mt[kMtN + 2] = 0;
  mt[kMtN + 3] = 0;
}

}  // namespace
#endif  // __HIPCC__
