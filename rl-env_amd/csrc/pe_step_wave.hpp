// pe_step_wave.hpp -- the wave-per-env step kernel of every geometry without a sector kernel:
// its LDS sizes (wave_*), the rover-aligned window's tables, wave_done and pe_step_wave.
// (a fragment of plantos_batch.hip's anonymous namespace; include after pe_coop.hpp and pe_obs.hpp)
#pragma once

// ---------------------------------------------------------------- pe_step_wave
// The fused step for every geometry without a compile-time sector kernel (any
// G <= 128, C <= 120, R <= 64; e.g. SURVEY §8(d)'s 64x64 / 64 rays / R=32 stress
// variant): ONE WAVE PER ENV.  The rover's window -- grid rows x-R-1 .. x+R+1
// clipped to the map, one contiguous 16-B-aligned span of the env's block, and
// visit rows x-3 .. x+3 -- is staged into the wave's LDS region with coalesced
// loads in one round after the scalars; the transition and commit are wave-uniform
// (scalar loads of the env's scalars / action / return); lane i marches ray i
// (i+64, ... for C > 64) over LDS (plantos_env.py:260-292), lanes 0..26 build the
// position and the 5x5 visit slice, and the obs row goes out through LDS as
// contiguous stores.  A done env's auto-reset is the wave-cooperative one of the
// sector kernel (prefetched record or in-place map generation, pe_coop.hpp) where
// coop_reset_ok; otherwise lane 0 runs the serial reset (reset_env).
// Per-wave LDS: the window words (max(min(G,2R+3)*WPR + 2, G*WPR) u64: also the
// cooperative reset's scratch), 7 visit rows of NW u32, the D-float obs row.
__host__ __device__ constexpr int wave_win_words(int G, int R, int WPR) {
  return ((((G < 2 * R + 3 ? G : 2 * R + 3) * WPR + 2) > G * WPR ? ((G < 2 * R + 3 ? G : 2 * R + 3) * WPR + 2)
                                                                  : G * WPR) + 1) & ~1;
}
__host__ __device__ constexpr int wave_lds_floats(int G, int R, int WPR, int NW, int D) {
  return 2 * wave_win_words(G, R, WPR) + ((7 * NW + 3) & ~3) + ((D + 3) & ~3);
}
// The workgroup's shared header: the obs tables (Tables' first kTabPads floats: dist,
// pos, vis) and the LIDAR offsets as int16 (dx & 0xFF | dy << 8) [C][RP], RP = R
// rounded up to 8 (one 16-B LDS read per 8 probes of a ray).
// (the rover-aligned kernels' entries are 3 B: a u16 LDS byte offset [C][RP], then a u8
// bit shift [C][RP]; rounded up to 16 B)
__host__ __device__ constexpr int wave_hdr_floats(int C, int R, bool aln) {
  return kTabPads + (aln ? ((C * ((R + 7) & ~7) * 3 + 15) & ~15) / 4 : C * ((R + 7) & ~7) / 2);
}
constexpr int kWaveEnvs = 8;  // envs (waves) per workgroup
// Rover-aligned window (ALN): after the transition the post-move rows xp-R .. xp+R
// are re-staged over the raw window, each shifted so that cell yp+dy+R of the
// padded row sits at bit 2(dy+R) of NWA = ceil((4R+2)/32) words, rows off the map
// filled with OBST.  A probe (dx, dy) is then word (dx+R)*NWA + (2(dy+R))>>5,
// shift (2(dy+R))&31 -- constants per (ray, probe) held in the LDS offset table
// (11-bit word | 5-bit shift << 11), no bounds check and no position arithmetic per
// probe.  Used when the aligned rows fit the raw region and kAlnSlots words per lane.
constexpr int kAlnSlots = 8;
__host__ __device__ constexpr int wave_aln_words(int R) { return (2 * R + 1) * ((4 * R + 33) >> 5); }
__host__ __device__ constexpr bool wave_aln_ok(int G, int R, int WPR) {
  return wave_aln_words(R) <= 64 * kAlnSlots && wave_aln_words(R) <= 2 * wave_win_words(G, R, WPR);
}
// one packed (dx & 0xFF | dy << 8) offset -> the aligned window's (word | shift << 11)
__host__ __device__ __forceinline__ uint32_t aln_entry(uint32_t v, int R, int NWA) {
  const int dx = (int)(int8_t)(v & 0xFFu), dy = (int)(int8_t)((v >> 8) & 0xFFu);
  const int cb = 2 * (dy + R);
  return (uint32_t)((dx + R) * NWA + (cb >> 5)) | ((uint32_t)(cb & 31) << 11);
}

// The wave kernel's done path (terminal obs / info, auto-reset), called by the
// wave of a done env with all lanes active.
template <int MAXW>
__device__ __attribute__((noinline)) void wave_done(const StepArgs& a, int64_t e, Scal s, int wfix, float* row,
                                                    uint64_t* win, const float* tdist, const float* tpos,
                                                    const float* tvis, int lane) {
  const Geo& g = a.g;
  const Rules& rl = a.rl;
  const State& st = a.st;
  const Tables* tab = st.tab;
  const int D = g.D;
  if (a.tobs)
    for (int k = lane; k < D; k += 64) a.tobs[e * D + k] = row[k];
  if (!a.autoreset) {
    if (a.tinfo && lane == 0) write_info(st, g, tab, e, s, a.tinfo + e * PE_NINFO);
  } else if (a.coop_max_done > 0) {  // coop_reset_ok geometry (pe_create)
    constexpr int KD = 6;            // D <= 347 (C <= 64): the record's obs row after its check
    PfLoad<MAXW, KD> pl;
    if (a.pf.scal) coop_load_prefetched<MAXW, KD>(a.pf, g, e, pl, lane);  // in flight from here on
    bool keep = false;
    if (st.cur && lane == 0) keep = curriculum_on_reset(st.cur, e, rl);  // A2C_training.py:56-95
    keep = __builtin_amdgcn_readfirstlane((int)keep) != 0;
    // with the curriculum the commit stored this env's rows: they land before the
    // info reads them and the reset rewrites them
    if (st.cur) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (a.tinfo) coop_write_info<MAXW>(st, g, e, s, a.tinfo + e * PE_NINFO, lane, wfix);
    Row4<MAXW> rw;
    Scal ns;
    asm volatile("" ::: "memory");  // terminal obs read out of the row before the fresh one goes in
    if (a.pf.scal && coop_take_prefetched<MAXW, KD>(a.pf, g, e, s.episode, pl, rw, ns, row, lane)) {
      ns = coop_apply_reset<MAXW>(st, g, e, ns, keep, rw, lane, nullptr, true);
    } else {
      ns = coop_reset_env<MAXW>(st, g, rl, e, s.episode, keep, rw, lane, win);
      coop_fresh_obs<MAXW>(g, rw, ns, row, tdist, tpos, tvis, st.ldx, st.ldy, lane);
    }
    if (lane == 0) {
      if (a.pf.scal) a.pf.flag[e] = 1;  // its next map goes into the next generating batch
      st_wt(st.ep_ret + e, 0.0);
      st_wt(st.scal + e, pack(ns));
    }
  } else if (lane == 0) {  // serial reset (the geometry has no cooperative one)
    if (a.tinfo) write_info(st, g, tab, e, s, a.tinfo + e * PE_NINFO, wfix);
    const Scal ns = reset_env(st, g, rl, tab, e, s.episode);
    st_wt(st.ep_ret + e, 0.0);
    st_wt(st.scal + e, pack(ns));
    build_obs_fresh(a, st.grid + e * g.gstride, ns, row, tab->dist, tab->pos, tab->vis, st.ldx, st.ldy);
  }
  // the LDS row / window are flat accesses here: all of them done before the caller's tile store
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
}

// waves per SIMD of the multi-word variant: 8 spills ~130 B/lane yet beats 7 / 6 (64x64/R=32:
// 110.1 / 117.3 / 112.8 us)
constexpr int kWaveWpe4 = 8;
// pe_step_wave's obs row of D >= this many floats as 16-B stores (shorter: one float per
// lane): 64x64/C64/R32 93.8 -> 90.4 us, 40x40/C48/R8 76.7 -> 75.0, but 8x8/C16/R20
// 68.0 -> 70.2 (sc1 16-B stores: 90.8 / 76.7 / 70.4; profiles/r3x/)
constexpr int kWaveRowstoreMin = 200;
template <int MAXW, bool ALN>  // the cooperative reset's row words (1 or kCoopWPR); rover-aligned rays
__global__ __launch_bounds__(64 * kWaveEnvs) __attribute__((amdgpu_waves_per_eu(MAXW == 1 ? 8 : kWaveWpe4))) void pe_step_wave(StepArgs a) {  // <= 64 VGPRs at 8
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const Geo& g = a.g;
  const Rules& rl = a.rl;
  const State& st = a.st;
  const Tables* tab = st.tab;  // global: the serial reset path's tables
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t e = (int64_t)blockIdx.x * kWaveEnvs + wv;
  const int G = g.G, R = g.R, WPR = g.WPR, NW = g.NW, D = g.D, RP = (R + 7) & ~7;
  // ---- round 1 (uniform): the packed scalars and both action words in one round
  // trip, issued before the shared header's copy (a wave's round 1 waited for the
  // header's loads and the barrier before it started) -- unconditional loads at an
  // index clamped into the batch (the action's load inside a branch on act_bytes
  // was waited for before the return's was issued: three round trips before round 2)
  const int64_t ec = e < a.n ? e : (int64_t)a.n - 1;
  const uint4 sw = st.scal[ec];
  const int ash = a.act_bytes == 8 ? 1 : 0;  // 8-byte actions: two words, low first
  const int32_t* ap = reinterpret_cast<const int32_t*>(a.actions);
  const int32_t alo = ap[ec << ash], ahi = ap[(ec << ash) + ash];
  double ret = st.ep_ret[ec];  // (needed at the commit: in flight through round 2)
  // the shared header (read after the barrier)
  const float* tsrc = reinterpret_cast<const float*>(tab);
  for (int k = threadIdx.x; k < kTabPads; k += blockDim.x) smem[k] = tsrc[k];
  int16_t* lofs = reinterpret_cast<int16_t*>(smem + kTabPads);
  {  // the probe table, 16 B per thread and pass (st.ldxy, built by pe_create -- the
     // aligned-window entries too: converted here they cost 135 VALU per pass)
    const uint4* src = reinterpret_cast<const uint4*>(st.ldxy);
    uint4* dst = reinterpret_cast<uint4*>(lofs);
    const int nq = ALN ? (g.C * RP * 3 + 15) >> 4 : g.C * RP / 8;
    for (int k = threadIdx.x; k < nq; k += blockDim.x) dst[k] = src[k];
  }
  __syncthreads();
  if (e >= a.n) return;  // wave-uniform; no workgroup barrier below
  const float* tdist = smem;
  const float* tpos = smem + kTabPos;
  const float* tvis = smem + kTabVis;
  float* base = smem + wave_hdr_floats(g.C, R, ALN) + wv * wave_lds_floats(G, R, WPR, NW, D);
  uint64_t* win = reinterpret_cast<uint64_t*>(base);
  uint32_t* lvis = reinterpret_cast<uint32_t*>(base + 2 * wave_win_words(G, R, WPR));
  float* row = base + 2 * wave_win_words(G, R, WPR) + ((7 * NW + 3) & ~3);

  Scal s = unpack(sw);
  const int64_t action = ash ? (int64_t)(((uint64_t)(uint32_t)ahi << 32) | (uint32_t)alo) : (int64_t)alo;
  bool mv = false, water = false, bad = false;
  int dxm = 0, dym = 0;
  if (action < 4) {                                        // plantos_env.py:166
    const int64_t ai = action < 0 ? action + 4 : action;   // Python negative index
    if (ai < 0) {
      bad = true;                                          // reference IndexError
    } else {
      mv = true;                                           // :186 N,E,S,W
      dxm = ai == 0 ? -1 : (ai == 2 ? 1 : 0);
      dym = ai == 1 ? 1 : (ai == 3 ? -1 : 0);
    }
  } else {
    water = true;
  }
  const int nx = s.x + dxm, ny = s.y + dym;
  const bool inb = mv && nx >= 0 && nx < G && ny >= 0 && ny < G;  // :193-195

  // ---- round 2: the window span and the visit rows, every load issued before any
  // LDS write (clamped indices: unconditional loads, one memory round trip)
  const int lo = s.x - R - 1 > 0 ? s.x - R - 1 : 0, hi = s.x + R + 1 < G - 1 ? s.x + R + 1 : G - 1;
  const int w0 = (lo * WPR) & ~1;                      // 16-B aligned (env blocks are)
  const int nq = ((hi + 1) * WPR - w0 + 1) >> 1;       // uint4s (a trailing pad word at most)
  const uint4* gsrc = reinterpret_cast<const uint4*>(st.grid + e * g.gstride + w0);
  const int vlo = s.x - 3 > 0 ? s.x - 3 : 0, vhi = s.x + 3 < G - 1 ? s.x + 3 : G - 1;
  const int nv = (vhi - vlo + 1) * NW;
  const uint32_t* vsrc = vis_env(st, g, e, s.episode) + (int64_t)vlo * NW;
  uint32_t eo = 0u, en = 0u;
  const int cell_o = s.x * G + s.y, cell_n = nx * G + (inb ? ny : s.y);
  if (inb && (s.flags & F_EXPL_BITMAP)) {
    eo = st.expl[e * g.estride + (cell_o >> 5)];
    en = st.expl[e * g.estride + (cell_n >> 5)];
  }
  const double cthr = st.cur ? st.cur[e].thr : 0.0;  // CurriculumWrapper threshold
  uint32_t vv[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int k = lane + 64 * j;
    vv[j] = vsrc[k < nv ? k : nv - 1];
  }
  {  // the window's first 256 16-B units (all of it up to 2R+3 rows of 4 words, e.g. 64x64/R32)
    uint4 gv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int q = lane + 64 * j;
      gv[j] = gsrc[q < nq ? q : nq - 1];
    }
    // every load of round 2 lands here, in one wait (asm operands): as a loop, or with
    // the loads left to the compiler, some were sunk into the conditional LDS writes
    // below and each waited for alone (64x64/R32: the visit rows, then 3 window loads)
    asm volatile("" ::"v"(vv[0]), "v"(vv[1]), "v"(gv[0].x), "v"(gv[1].x), "v"(gv[2].x), "v"(gv[3].x));
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int q = lane + 64 * j;
      if (q < nq) {
        win[2 * q] = (uint64_t)gv[j].x | ((uint64_t)gv[j].y << 32);
        win[2 * q + 1] = (uint64_t)gv[j].z | ((uint64_t)gv[j].w << 32);
      }
    }
  }
  for (int q0 = 4 * 64; q0 < nq; q0 += 4 * 64) {  // (G+2R > 128 cells with many rows)
    uint4 gv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int q = q0 + lane + 64 * j;
      gv[j] = gsrc[q < nq ? q : nq - 1];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int q = q0 + lane + 64 * j;
      if (q < nq) {
        win[2 * q] = (uint64_t)gv[j].x | ((uint64_t)gv[j].y << 32);
        win[2 * q + 1] = (uint64_t)gv[j].z | ((uint64_t)gv[j].w << 32);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int k = lane + 64 * j;
    if (k < nv) lvis[k] = vv[j];
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the wave's LDS writes before its reads (in order)

  // cell code / visit nibble from the staged window (rows outside [lo, hi] are off-map)
  auto code_at = [&](int xr, int pcol) -> int {
    if (xr < 0 || xr >= G) return OBST;
    const int bit = 2 * pcol;
    return (int)((win[xr * WPR + (bit >> 6) - w0] >> (bit & 63)) & 3u);
  };
  auto vword = [&](int xr, int col) -> int { return (xr - vlo) * NW + ((4 * (col + 2)) >> 5); };
  const uint32_t* win32 = reinterpret_cast<const uint32_t*>(win);

  // ---- transition (plantos_env.py:160-222), wave-uniform
  s.step = s.step < 65535 ? s.step + 1 : 65535;                 // :162
  bool ok = false, watered = false, wet_hyd = false;
  uint32_t n = 0u;
  double h = 0.0;
  if (mv) {
    ok = inb && code_at(nx, ny + R) != OBST;                     // :193-195 (plants walkable)
    if (ok) {
      n = (lvis[vword(nx, ny)] >> ((4 * (ny + 2)) & 31)) & 15u;
      h = n == 0u ? rl.r_exploration : rl.r_revisit;             // :197, 204-207
    } else {
      s.flags |= F_COLLIDED;                                     // :209
      s.coll = s.coll < 65535 ? s.coll + 1 : 65535;              // :210
      h = rl.r_invalid;                                          // :211
    }
  } else if (water) {
    const int cd = code_at(s.x, s.y + R);
    if (cd == THIRSTY) {                                         // fork plantos_env_new.py:237-240
      watered = true;
      h = rl.r_goal;
    } else if (cd == HYD) {                                      // fork :241-242 (root raises)
      wet_hyd = true;
      h = rl.r_mistake;
    } else {
      h = rl.r_water_empty;                                      // :221-222
    }
  }
  const uint32_t nib = n < 15u ? n + 1u : 15u;                   // :203
  uint32_t wo = eo, wn = en;
  if (ok) {
    if (s.flags & F_EXPL_BITMAP) {                               // explored[old]=1, [new]=2 (:198-200)
      const uint32_t bo = 1u << (cell_o & 31), bn = 1u << (cell_n & 31);
      if ((cell_o >> 5) == (cell_n >> 5)) {
        if (!(wo & bo)) { wo |= bo; s.expl++; }
        if (!(wo & bn)) { wo |= bn; s.expl++; }
      } else {
        if (!(wo & bo)) { wo |= bo; s.expl++; }
        if (!(wn & bn)) { wn |= bn; s.expl++; }
      }
    } else if (n == 0u) {
      s.expl++;  // derived mode: explored[new] was 0 iff never visited
    }
  }
  if (bad) s.flags |= F_POISON_ACT;
  const bool new_hyd_poison = wet_hyd && !(s.flags & F_POISON_HYD);
  if (wet_hyd) s.flags |= F_POISON_HYD;
  const int ox = s.x, oy = s.y;
  if (ok) {
    s.x = nx;                                                    // :199
    s.y = ny;
  }
  double rew = rl.r_step;                                        // :164
  rew += h;
  bool term = s.expl >= s.total;                                 // :176, 244-246, 331
  const bool trunc = s.step >= rl.max_steps;                     // :177
  if (term && !(s.flags & F_BONUS)) {                            // :179-181
    rew += rl.r_complete;
    s.flags |= F_BONUS;
  }
  // the post-step window in LDS (the rays see the watered cell, the slice the visit)
  const int kvn = ok ? vword(nx, ny) : 0;
  const uint32_t wvn = ok ? (lvis[kvn] & ~(0xFu << ((4 * (ny + 2)) & 31))) | (nib << ((4 * (ny + 2)) & 31)) : 0u;
  const int cbit = 2 * (oy + R), kw = ox * WPR + (cbit >> 6) - w0;
  const uint64_t wwr = watered ? win[kw] & ~(1ull << (cbit & 63)) : 0ull;  // code 3 -> 2
  if (lane == 0) {
    if (bad) atomicOr(st.err_bits, F_POISON_ACT);
    if (new_hyd_poison) atomicOr(st.err_bits, F_POISON_HYD);
    if (st.cur) term = curriculum_hit(st.cur, e, cthr, s.expl, s.total, rl.cur_term) || term;  // A2C_training.py:101-103
  }
  term = __builtin_amdgcn_readfirstlane((int)term) != 0;
  const bool done = term || trunc;
  // an env about to be auto-reset gets new rows: its last move / watering is not
  // stored (the terminal info accounts for the watering), unless the curriculum
  // carries its visits over
  const bool reset_now = done && a.autoreset;
  const bool commit_rows = !(reset_now && !st.cur);
  const int wfix = (watered && reset_now && !st.cur) ? 1 : 0;
  if (lane == 0) {
    if (ok) lvis[kvn] = wvn;
    if (watered) win[kw] = wwr;
    if (commit_rows) {
      if (ok) {
        const int b = (ny + 2) >> 1;  // the byte of the target's nibble in row nx
        st_wt(reinterpret_cast<uint8_t*>(vis_env(st, g, e, s.episode) + (int64_t)nx * NW) + b,
              (uint8_t)(wvn >> (8 * (b & 3))));
        // (written here, not deferred through vpend as in the headline kernel: holding the
        // pending word across this kernel spilled 29 more SGPRs, 64x64/R32 85.8 -> 90.2 us,
        // profiles/r4q/ab_g64r32.jsonl)
        visit_bump_exact(st, g, e, cell_n, n);
        if (s.flags & F_EXPL_BITMAP) {
          if (wo != eo) st.expl[e * g.estride + (cell_o >> 5)] = wo;
          if ((cell_o >> 5) != (cell_n >> 5) && wn != en) st.expl[e * g.estride + (cell_n >> 5)] = wn;
        }
      }
      if (watered) {
        const int B = (oy + R) >> 2;  // the byte of the cell's code in row ox
        st_wt(reinterpret_cast<uint8_t*>(st.grid + e * g.gstride + (int64_t)ox * WPR) + B,
              (uint8_t)(wwr >> (8 * (B & 7))));
      }
    }
    ret += rew;
    st_wt(a.reward + e, (float)rew);
    st_wt(a.term + e, (uint8_t)term);
    st_wt(a.trunc + e, (uint8_t)trunc);
    if (done) {  // Monitor's episode return / length of the ended episode
      if (a.ep_ret_out) st_wt(a.ep_ret_out + e, ret);
      if (a.ep_len_out) st_wt(a.ep_len_out + e, (int32_t)s.step);
    }
    if (commit_rows) {  // else the reset below stores the new episode's scalars
      st_wt(st.ep_ret + e, ret);
      st_wt(st.scal + e, pack(s));
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");

  // ---- observation (plantos_env.py:251-315) into the LDS row
  const int xp = s.x, yp = s.y;
  if constexpr (ALN) {  // the rover-aligned window over the raw one (every read before any write)
    const int NWA = (4 * R + 33) >> 5, tot = (2 * R + 1) * NWA;
    const uint32_t mg = 0xFFFFFFFFu / (uint32_t)NWA + 1u;  // k / NWA as a high multiply (k < 512; NWA >= 2)
    const int sw = (2 * yp) >> 5, sb = (2 * yp) & 31;
    uint32_t av[kAlnSlots];
#pragma unroll
    for (int t = 0; t < kAlnSlots; ++t) {
      if (64 * t >= tot) break;  // (uniform: slots past the window -- 40x40/R8 uses 1 of 8)
      const int k = lane + 64 * t;
      const int i = NWA == 1 ? k : (int)__umulhi((uint32_t)k, mg), w = k - i * NWA;
      const int xr = xp - R + i;
      av[t] = 0x55555555u;  // OBST (1) in every cell: rows off the map (:271-284)
      if (k < tot && (uint32_t)xr < (uint32_t)G) {
        const int q = 2 * ((int)__umul24((uint32_t)xr, (uint32_t)WPR) - w0) + sw + w;
        av[t] = __builtin_amdgcn_alignbit(win32[q + 1], win32[q], (uint32_t)sb);
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    uint32_t* awin = reinterpret_cast<uint32_t*>(win);
#pragma unroll
    for (int t = 0; t < kAlnSlots; ++t) {
      const int k = lane + 64 * t;
      if (k < tot) awin[k] = av[t];
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  }
  const char* wbyte = reinterpret_cast<const char*>(win);
  for (int i = lane; i < g.C; i += 64) {
    const uint4* orow = reinterpret_cast<const uint4*>(lofs + i * RP);
    const uint2* srow = reinterpret_cast<const uint2*>(reinterpret_cast<const uint8_t*>(lofs) + g.C * RP * 2 + i * RP);
    int dist = R, ent = EMPTY;
    for (int r0 = 0; r0 < R; r0 += 8) {  // 8 probes per 16-B offset read, their codes in flight together
      const uint4 o = orow[r0 >> 3];
      const uint32_t ow[4] = {o.x, o.y, o.z, o.w};
      uint2 os = make_uint2(0u, 0u);
      if constexpr (ALN) os = srow[r0 >> 3];
      const uint32_t sw[2] = {os.x, os.y};
      // the 8 probe codes packed 2 bits each (probe j at bits 2j), first hit by one
      // find-first-set (as the sector kernel's quad_rays); 32-bit window reads (a
      // 2-bit code never straddles a word: its bit offset is even; the row offset as a
      // full-rate 24-bit multiply, not the quarter-rate 32-bit one)
      uint32_t pk = 0u;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const uint32_t v = ow[j >> 1] >> (16 * (j & 1));
        uint32_t c;
        if constexpr (ALN) {  // the probe's LDS byte offset and bit shift; off-map rows hold OBST
          // (ubfe reads the low 5 bits of its offset operand: the shift byte needs no mask)
          c = __builtin_amdgcn_ubfe(*reinterpret_cast<const uint32_t*>(wbyte + (v & 0xFFFFu)),
                                    sw[j >> 2] >> (8 * (j & 3)), 2u);
        } else {
          const int cx = xp + (int)(int8_t)(v & 0xFFu);
          const int bit = 2 * (yp + (int)(int8_t)((v >> 8) & 0xFFu) + R);
          c = (uint32_t)cx < (uint32_t)G  // :271-284 (off-map rows: obstacle)
                  ? (win32[2 * ((int)__umul24((uint32_t)cx, (uint32_t)WPR) - w0) + (bit >> 5)] >> (bit & 31)) & 3u
                  : (uint32_t)OBST;
        }
        pk |= c << (2 * j);
      }
      if (R - r0 < 8) pk &= (1u << (2 * (R - r0))) - 1u;  // the zero-padded offsets past R
      const uint32_t nz = (pk | (pk >> 1)) & 0x5555u;
      if (nz) {
        const int f = __builtin_ctz(nz);  // 2j of the first hit
        dist = r0 + (f >> 1) + 1;
        ent = (int)((pk >> f) & 3u);
        break;
      }
    }
    row[5 * i] = tdist[dist];                                    // :288
    row[5 * i + 1] = ent == 0 ? 1.0f : 0.0f;
    row[5 * i + 2] = ent == 1 ? 1.0f : 0.0f;
    row[5 * i + 3] = ent == 2 ? 1.0f : 0.0f;
    row[5 * i + 4] = ent == 3 ? 1.0f : 0.0f;
  }
  if (lane < 25) {                                               // :298-313
    const int gx = xp + lane / 5 - 2, gy = yp + lane % 5 - 2;
    const bool in = gx >= 0 && gx < G && gy >= 0 && gy < G;
    const uint32_t v = in ? (lvis[vword(gx, gy)] >> ((4 * (gy + 2)) & 31)) & 15u : 10u;
    row[5 * g.C + 2 + lane] = tvis[v];
  } else if (lane < 27) {
    row[5 * g.C + lane - 25] = tpos[lane == 25 ? xp : yp];       // :294-296
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");

  // ---- DummyVecEnv auto-reset (rare) and terminal outputs: out of line, so that the
  // reset path's pointers and state do not shape the hot path's register allocation
  if (done) {  // the kernel's argument read in place (StepArgs is its only argument): taking
              // &a would copy the whole struct to scratch on every launch
    const StepArgs* ap = (const StepArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    wave_done<MAXW>(*ap, e, s, wfix, row, win, tdist, tpos, tvis, lane);
  }
  // the obs row: long rows as 16-B stores from the first 16-B boundary of the row on,
  // the 0-3 floats before it and the tail as single floats
  float* dst = a.obs + e * D;
  const int hd = (int)((16u - ((uint32_t)reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u) >> 2;
  const int n4 = (D - hd) >> 2;
  // (rover-aligned kernels only: in the other one its registers made the SGPRs spill, and
  // none of its geometries benched has rows that long)
  if (ALN && D >= kWaveRowstoreMin && (reinterpret_cast<uintptr_t>(dst) & 3u) == 0) {
    typedef float v4f __attribute__((ext_vector_type(4)));
    for (int k = lane; k < n4; k += 64) {
      const float* sr = row + hd + 4 * k;
      const v4f v = {sr[0], sr[1], sr[2], sr[3]};
      *reinterpret_cast<v4f*>(dst + hd + 4 * k) = v;
    }
    if (lane < hd) dst[lane] = row[lane];
    if (lane < D - hd - 4 * n4) dst[hd + 4 * n4 + lane] = row[hd + 4 * n4 + lane];
  } else {
    for (int k = lane; k < D; k += 64) dst[k] = row[k];
  }
}
