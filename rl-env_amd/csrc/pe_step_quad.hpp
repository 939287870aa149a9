// pe_step_quad.hpp -- the sector (quadrant-split) step kernel pe_step_quad<C, R, ...> with its
// move decode (QuadMove, quad_move, quad_move_cells) and per-wave compute (quad_compute).
// (a fragment of plantos_batch.hip's anonymous namespace; include after pe_quad_done.hpp)
#pragma once

// The action's move / watering decode (plantos_env.py:166, 186-195) and the window
// coordinates it implies, from the scalars before the step.
struct QuadMove {
  bool mv, water, bad, inb;      // move / water / reference IndexError / target in bounds
  int dxm, dym, nx, ny, nyc;     // direction, target, target column clamped to the map
  int yb, ybv, cell_o, cell_n;   // window's first padded grid / visit column, old / new cell
};
template <bool ONEWORD>
__device__ __forceinline__ QuadMove quad_move(const Scal& s, int64_t action, int G) {
  QuadMove m;
  m.mv = false;
  m.water = false;
  m.bad = false;
  m.dxm = 0;
  m.dym = 0;
  if (action < 4) {                                              // plantos_env.py:166
    const int64_t ai = action < 0 ? action + 4 : action;         // Python negative index
    if (ai < 0) {
      m.bad = true;                                              // reference IndexError
    } else {
      m.mv = true;                                               // :186 N,E,S,W
      m.dxm = ai == 0 ? -1 : (ai == 2 ? 1 : 0);
      m.dym = ai == 1 ? 1 : (ai == 3 ? -1 : 0);
    }
  } else {
    m.water = true;
  }
  m.nx = s.x + m.dxm;
  m.ny = s.y + m.dym;
  m.inb = m.mv && m.nx >= 0 && m.nx < G && m.ny >= 0 && m.ny < G;  // :193-195
  return m;
}
// (the window coordinates: separate, so that the kernels compute them where they did)
template <bool ONEWORD>
__device__ __forceinline__ void quad_move_cells(QuadMove& m, const Scal& s, int G) {
  m.nyc = m.inb ? m.ny : s.y;
  m.yb = ONEWORD ? 0 : (s.y > 0 ? s.y - 1 : 0);
  m.ybv = s.y > 0 ? s.y - 1 : 0;
  m.cell_o = s.x * G + s.y;
  m.cell_n = m.nx * G + m.nyc;
}

// The compute phase of the sector kernel (pe_step_quad), between the
// window barrier and the done barrier: every wave re-derives the transition
// (plantos_env.py:160-222) from the LDS window, marches its sector of rays and writes
// its part of the env's obs row into the LDS tile; the commit wave (NW-1) stores the
// state.  done / wfix: the env ended this step / its last watering is not stored.
// eo / en / cthr: the explored-bitmap words (F_EXPL_BITMAP) and the CurriculumWrapper
// threshold, loaded by the caller with round 2, or (LX) here by the commit wave in the
// modes that need them -- the persistent kernel keeps other loads in flight here, and
// a wait for a value loaded one iteration earlier is a vmcnt(0).
template <int C, int R, bool ONEWORD, int NW, bool BT, bool RT, bool LX = false, bool DV = false>
__device__ __forceinline__ void quad_compute(const StepArgs& a, const uint64_t* lrow, const uint32_t* lvis,
                                             typename std::conditional<BT, uint8_t, float>::type* rows,
                                             const float* tdist, const float* tpos, const float* tvis, int lane,
                                             int wv, int64_t e, bool live, int Cr, int Rr, const QuadMove& m,
                                             uint32_t eo, uint32_t en, double cthr, uint32_t vp0, Scal& s,
                                             double& ret, bool& done, bool& wfix) {
  using OT = typename std::conditional<BT, uint8_t, float>::type;
  constexpr int LS = kQuadEnvs, CW = NW - 1;
  const Geo& g = a.g;
  // the rules by value: a per-lane choice between two fields of a referenced struct
  // became a per-lane address select and a VMEM load of the chosen double
  const Rules rl = a.rl;
  const State& st = a.st;
  const uint64_t* gb = st.grid + e * g.gstride;
  done = false;
  wfix = false;
  // DV: the previous step's deferred overflow write (pe_device.hpp vx_pending), issued
  // now by wave 0 (not the commit wave, the block's laggard; desynchronized 10.71 ->
  // 10.60 us with the compaction below, profiles/r4ad/): every load the wave waits for
  // has landed at the barrier.  (Ordered before a same-kernel lane-path reset of the env,
  // which uses vx as scratch, by that path's __syncthreads.)
  if constexpr (DV) {
    if (wv == 0 && live && vp0) vx_apply(st, g, e, vp0);
  }
  uint32_t np = 0u;
  s.step = s.step < 65535 ? s.step + 1 : 65535;                  // :162
  bool ok = false, watered = false, wet_hyd = false;
  uint32_t n = 0u;
  int dxv = 0;
  double h = 0.0;
  if (m.mv) {
    const uint64_t rt = lrow[(Rr + 1 + m.dxm) * LS + lane];
    ok = m.inb && ((rt >> (2 * (m.nyc + Rr - m.yb))) & 3u) != OBST;     // :193-195 (plants walkable)
    if (ok) {
      n = (lvis[(3 + m.dxm) * LS + lane] >> (4 * (m.nyc + 2 - m.ybv))) & 15u;
      h = n == 0u ? rl.r_exploration : rl.r_revisit;              // :197, 204-207
      dxv = m.dxm;
    } else {
      s.flags |= F_COLLIDED;                                      // :209
      s.coll = s.coll < 65535 ? s.coll + 1 : 65535;               // :210
      h = rl.r_invalid;                                           // :211
    }
  } else if (m.water) {
    const uint64_t rc = lrow[(Rr + 1) * LS + lane];
    const int cd = (int)((rc >> (2 * (s.y + Rr - m.yb))) & 3u);
    if (cd == THIRSTY) {                                          // fork plantos_env_new.py:237-240
      watered = true;
      h = rl.r_goal;
    } else if (cd == HYD) {                                       // fork :241-242 (root raises)
      wet_hyd = true;
      h = rl.r_mistake;
    } else {
      h = rl.r_water_empty;                                       // :221-222
    }
  }
  const int xp = s.x + dxv, yp = ok ? m.ny : s.y;
  const uint32_t nib = n < 15u ? n + 1u : 15u;                    // :203
  OT* row = rows + lane * g.D;
  if (live) {
    const int kc = dxv + Rr + 1;
    const int sh = 2 * (yp - m.yb);
    const int vs = 4 * (yp - m.ybv);
    if constexpr (RT) {
      // the register-window form where pe_create found the wave's sector fits it (its header's
      // ok word, after the LDS-form table in st.ldxy), else the LDS-table form
      const uint32_t* gt = reinterpret_cast<const uint32_t*>(st.ldxy) + Cr * ((Rr + 7) & ~7);
      const rt_cptr hdr = (rt_cptr)(gt + 4 * wv);
      if (hdr[3]) {
        quad_rays_rt_reg<OT>(lrow, hdr, (rt_cptr)(gt + 16), wv * Cr / NW, (wv + 1) * Cr / NW, Rr, lane, kc, sh, watered,
                             row, tdist);
      } else {
        const uint32_t* ltab = reinterpret_cast<const uint32_t*>(reinterpret_cast<const float*>(rows) + quad_rtab_off(Cr, BT));
        quad_rays_rt<OT>(lrow, ltab, wv * Cr / NW, (wv + 1) * Cr / NW, Rr, lane, kc, sh, watered, row, tdist);
      }
    } else {
      sector_rays<C, R, NW>(wv, lrow, lane, kc, sh, watered, row, tdist);
    }
    // slice rows and position go to the non-commit waves (the commit wave is the laggard)
    if (wv != CW)
      for (int lx = wv; lx < 5; lx += NW - 1) quad_slice_row(lvis, lane, lx, dxv, vs, ok, nib, Cr, row, tvis);
    if (wv == (NW == 4 ? 2 : 5)) {                                // :294-296
      if constexpr (BT) {
        row[5 * Cr] = (uint8_t)(kCodePos + xp);
        row[5 * Cr + 1] = (uint8_t)(kCodePos + yp);
      } else {
        row[5 * Cr] = tpos[xp];
        row[5 * Cr + 1] = tpos[yp];
      }
    }
    if (wv == CW) {
      // ---- commit (plantos_env.py:160-222)
      uint32_t wo = eo, wn = en;  // explored-bitmap words after the move (bitmap mode)
      if (ok) {
        if (s.flags & F_EXPL_BITMAP) {                            // explored[old]=1, [new]=2 (:198-200)
          if constexpr (LX) {  // (loaded where used: a copy outside the branch would wait for it)
            eo = st.expl[e * g.estride + (m.cell_o >> 5)];
            en = st.expl[e * g.estride + (m.cell_n >> 5)];
            wo = eo;
            wn = en;
          }
          const uint32_t bo = 1u << (m.cell_o & 31), bn = 1u << (m.cell_n & 31);
          if ((m.cell_o >> 5) == (m.cell_n >> 5)) {
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
      if (m.bad) {
        s.flags |= F_POISON_ACT;
        atomicOr(st.err_bits, F_POISON_ACT);
      }
      if (wet_hyd && !(s.flags & F_POISON_HYD)) {
        s.flags |= F_POISON_HYD;
        atomicOr(st.err_bits, F_POISON_HYD);
      }
      const int ox = s.x;
      s.x = xp;                                                   // :199
      s.y = yp;
      double rew = rl.r_step;                                     // :164
      rew += h;
      bool term = s.expl >= s.total;                              // :176, 244-246, 331
      const bool trunc = s.step >= rl.max_steps;                  // :177
      if (term && !(s.flags & F_BONUS)) {                         // :179-181
        rew += rl.r_complete;
        s.flags |= F_BONUS;
      }
      if (st.cur) {
        if constexpr (LX) cthr = st.cur[e].thr;  // CurriculumWrapper threshold
        term = curriculum_hit(st.cur, e, cthr, s.expl, s.total, rl.cur_term) || term;  // A2C_training.py:101-103
      }
      done = term || trunc;  // terminal outputs; the reset itself only with autoreset
      // an env about to be auto-reset gets new grid and visit rows: its last move /
      // watering is not stored (the terminal info accounts for the watering), so no
      // store of this step can land after the reset's (unless the curriculum
      // carries the visits over)
      wfix = watered && done && a.autoreset && !st.cur;
      if (!(done && a.autoreset && !st.cur)) {
        if (ok) {
          // the byte holding the target's visit nibble (padded column p), rebuilt from
          // the window of row nx in LDS (padded nibbles ybv..ybv+7 hold both of its
          // nibbles): one byte store, no read of the word from memory
          const int p = m.ny + 2, b = p >> 1;
          const uint32_t wnew = (lvis[(3 + m.dxm) * LS + lane] & ~(0xFu << (4 * (p - m.ybv)))) | (nib << (4 * (p - m.ybv)));
          // (not at a saturated nibble: the store would rewrite the byte memory already holds.
          // The flagship's action stream moves into a cell at 15 in three of ten env-steps,
          // tools/visit_overflow_rate.py; the A/B: profiles/visit_overflow_ab.json)
          if (n < 15u) {
            st_wt(reinterpret_cast<uint8_t*>(vis_env(st, g, e, s.episode) + (int64_t)m.nx * g.NW) + b,
                  (uint8_t)(wnew >> (4 * (2 * b - m.ybv))));
          }
          if constexpr (DV)
            np = vx_pending(m.cell_n, n);
          else
            visit_bump_exact(st, g, e, m.cell_n, n);
          if (s.flags & F_EXPL_BITMAP) {
            uint32_t* ep_o = st.expl + e * g.estride + (m.cell_o >> 5);
            uint32_t* ep_n = st.expl + e * g.estride + (m.cell_n >> 5);
            if (wo != eo) *ep_o = wo;
            if ((m.cell_o >> 5) != (m.cell_n >> 5) && wn != en) *ep_n = wn;
          }
        }
        if (watered) {
          const int bit = 2 * (s.y + Rr);
          if constexpr (ONEWORD) {
            st_wt(const_cast<uint64_t*>(gb) + ox, (uint64_t)(lrow[(Rr + 1) * LS + lane] & ~(1ull << bit)));  // code 3 -> 2
          } else {
            // the byte holding the cell's code (padded column c; its 4 cells lie in the
            // window of row x, padded columns yb..yb+31, for R >= 2)
            const int c = s.y + Rr, B = c >> 2;
            const uint64_t wr = lrow[(Rr + 1) * LS + lane] & ~(1ull << (2 * (c - m.yb)));  // code 3 -> 2
            st_wt(reinterpret_cast<uint8_t*>(const_cast<uint64_t*>(gb) + (int64_t)ox * g.WPR) + B,
                  (uint8_t)(wr >> (2 * (4 * B - m.yb))));
          }
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
      // an env about to be auto-reset: its reset path stores the new episode's scalars
      if (!(done && a.autoreset && !st.cur)) {
        st_wt(st.ep_ret + e, ret);
        st_wt(st.scal + e, pack(s));
      }
      if constexpr (DV) {
        if (vp0 | np) st_wt(st.vpend + e, np);
      }
    }
  }
}

// BT: byte-coded obs tile (pe_coop.hpp ObsW<uint8_t>): [64 x D] bytes instead of
// floats in LDS (64x64 / 64 rays: 22 KB instead of 89 KB), expanded through the LDS
// code table at the tile store -- the f32 tile held the kernel to one workgroup per CU.
// EPB: envs per workgroup (64; 16 / 32 for small batches: more workgroups, so that
// a batch of a few thousand envs spreads over every CU -- lanes >= EPB idle).  The
// LDS layout keeps the 64-env stride LS whatever EPB.
template <int C, int R, bool ONEWORD, int NW, bool BT = false, int EPB = kQuadEnvs>
__global__ __launch_bounds__(64 * NW, NW == 8 ? 2 : 4) void pe_step_quad(StepArgs a) {  // NW=8 (the 16-env small-batch shape: one workgroup per CU, no cap); NW=4: <= 128 VGPRs (4 workgroups per CU: G=25 13.1 -> 10.5 us; 1-word C16: 122 -> 104 VGPRs)
  // C == 0 (R == 0): the runtime-(C, R) sector kernel (quad_rays_rt): C, R from the
  // geometry (up to kRtCMax -- kRtCMaxBT with the byte-coded tile -- / kRtRMax), the LDS
  // layout sized at run time
  constexpr bool RT = C == 0;
  constexpr int CM = RT ? (BT ? kRtCMaxBT : kRtCMax) : C, RM = RT ? kRtRMax : R;
  static_assert(!RT || (R == 0 && NW == 4 && EPB == kQuadEnvs), "runtime sector kernel: 4 waves, 64 envs");
  const int Cr = RT ? a.g.C : C, Rr = RT ? a.g.R : R;
  constexpr int NR = 2 * RM + 3, NV = 7, LS = kQuadEnvs, CW = NW - 1;  // CW: commit wave
  const int NRL = RT ? 2 * Rr + 3 : NR;  // window rows (the LDS layout's)
  const int tile_off = RT ? quad_tile_off_rt(Rr) : quad_tile_off<RM>();
  // after the tile (+ code table): RT's probe table (quad_rtab_off), then the staging region
  const int tail_off = tile_off + quad_rtab_off(Cr, BT);
  static_assert(EPB == 16 || EPB == 32 || EPB == 64, "envs per workgroup");
  static_assert(NW == 4 || (NW == 8 && EPB == 16), "8 waves: the 16-env small-batch shape only");
  static_assert(!BT || EPB == kQuadEnvs, "the byte-coded kernel's LDS-DMA staging predicts over all 64 lanes");

  static_assert(RT || C >= NW, "every wave owns a sector of at least one ray");
  static_assert(ONEWORD || RM <= 14, "funnel-shifted window row must hold 2R+5 cells");
  static_assert(ONEWORD || RT || R >= 2, "the watered cell's byte must lie in the window row");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* tdist = smem;
  float* tpos = smem + kTabPos;
  float* tvis = smem + kTabVis;
  uint64_t* lrow = reinterpret_cast<uint64_t*>(smem + kTabFloats);  // [NR][LS]
  uint32_t* lvis = reinterpret_cast<uint32_t*>(lrow + NRL * LS);   // [NV][LS]
  using OT = typename std::conditional<BT, uint8_t, float>::type;
  OT* rows = reinterpret_cast<OT*>(smem + tile_off);                // [LS][D] floats or codes
  float* ctab = smem + (RT ? quad_ctab_off_rt(Rr, Cr) : quad_ctab_off<RM, CM>());  // BT: code -> float
  const Geo& g = a.g;
  const Rules& rl = a.rl;
  const State& st = a.st;
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t e0 = (int64_t)blockIdx.x * EPB;
  const int64_t e = e0 + lane;
  const bool live = (EPB == LS || lane < EPB) && e < a.n;

  // ---- round 1: env-indexed loads (all waves).  Every thread also plays a LOADER
  // role for round 2: LT = 64 NW / EPB threads per env (env le < EPB, part sub), so
  // each load instruction reads LT consecutive rows of 64/LT envs instead of one row of 64.
  PE_STAMP(0);
  if (a.stagger) {  // de-phase the resident workgroups of a CU (speed only)
    const int q = (int)(blockIdx.x * kStaggerGroups / gridDim.x);
    for (int i = 0; i < q * a.stagger; ++i) __builtin_amdgcn_s_sleep(8);
  }
  constexpr int LT = NW * (LS / EPB);
  const int le = threadIdx.x / LT, sub = threadIdx.x % LT;
  const int64_t el = e0 + le;
  const bool llive = el < a.n;
  // Every round-1 load unconditional (indices clamped into the batch; the values of
  // lanes past its end are never used): a load inside a branch whose value merges
  // after it is waited for right there -- the 4-byte action load used to be, before
  // the loader scalars were even issued, i.e. two memory round trips instead of one.
  const int64_t ec = live ? e : (int64_t)a.n - 1, elc = llive ? el : (int64_t)a.n - 1;
  const uint4 sw = st.scal[ec];
  const int ash = a.act_bytes == 8 ? 1 : 0;  // 8-byte actions: two words, low first
  const int32_t* ap = reinterpret_cast<const int32_t*>(a.actions);
  const int32_t alo = ap[ec << ash], ahi = ap[(ec << ash) + ash];
  double ret = st.ep_ret[wv == CW ? ec : 0];  // (the commit wave's; the others read one shared word)
  // the deferred overflow write (pe_device.hpp vx_pending): the headline instantiation
  // only -- measured faster there (9.66 -> 9.52 us), slower in the constructor default's
  // multi-word C10R2 kernel (8.22 -> 8.69) and the 16-env small-batch shape (4.44 -> 4.61),
  // profiles/r4q/, r4v/
  // (round 5: the byte-coded twin of the headline kernel too -- config 5's codes step)
  constexpr bool DV = C == 16 && R == 6 && ONEWORD && NW == 4 && EPB == kQuadEnvs;
  const uint32_t vp0 = DV ? st.vpend[wv == CW || wv == 0 ? ec : 0] : 0u;  // (wave 0 applies, CW stores)
  // (Tried: the loader env's position by a bpermute from lane le of the wave instead of
  // this load -- 64x64 24.5 -> 25.2 us, 25x25 desync +0.4 us, the headline unchanged;
  // profiles/r3m_ab_*.jsonl.)
  const uint4 lw = st.scal[elc];
  // one-word rows (G <= 20): the loader env's whole grid block (gstride / 2 <= 10
  // 16-B units, contiguous, 3 per loader thread) comes in round 1 -- its address does
  // not depend on the position -- and only the visit rows are left for round 2
  constexpr int JG1 = (10 + LT - 1) / LT;  // gstride / 2 <= 10 16-B units (one-word: NW == 4, G <= 20)
  uint4 qg1[ONEWORD ? JG1 : 1];
  if constexpr (ONEWORD) {
    const uint4* lgq = reinterpret_cast<const uint4*>(st.grid + elc * g.gstride);
    const int nq = (int)(g.gstride >> 1);
#pragma unroll
    for (int j = 0; j < JG1; ++j) {
      const int q = sub + LT * j;
      qg1[j] = lgq[q < nq ? q : nq - 1];
    }
  }
  load_tables_hot(smem, st.tab, a.g.G, Rr);
  // the sector rays' tables (pe_quad.hpp quad_rays): dist[R+1] = 1.0, one-hot rows
  static_assert(dist_park_ok(RM, false), "ray tables inside dist[], below the one-hot rows and the done mask");
  if (threadIdx.x < 16) smem[kOneHotF + threadIdx.x] = (threadIdx.x >> 2) == (threadIdx.x & 3) ? 1.0f : 0.0f;
  if (threadIdx.x == 16) smem[Rr + 1] = 1.0f;

  if constexpr (RT) {  // the probe table (st.ldxy) into LDS: read from global memory in the ray
                       // loop, each 8-probe chunk was a vector load waited out with vmcnt(0)
    // (the LDS form's table: the sectors the register window does not take; round 6: the
    // copy's loads issued with round 1's, one unit per thread, measured slower -- 32x32/C24/R9
    // 17.05 -> 17.39 us, 40x40/C48/R8 28.57 -> 29.1, profiles/r6c/)
    const uint4* src = reinterpret_cast<const uint4*>(st.ldxy);
    uint4* dst = reinterpret_cast<uint4*>(smem + tail_off);
    for (int k = threadIdx.x; k < Cr * ((Rr + 7) & ~7) / 4; k += blockDim.x) dst[k] = src[k];  // (u32 entries)
  }
  Scal s = unpack(sw);
#ifdef PE_STAMPS
  if ((int)(s.x + lw.x) == -12345) g_stamps[0] = 1;  // consume round 1 before the stamp
#endif
  PE_STAMP(1);
  const int64_t action = ash ? (int64_t)(((uint64_t)(uint32_t)ahi << 32) | (uint32_t)alo) : (int64_t)alo;
  QuadMove m = quad_move<ONEWORD>(s, action, g.G);
  // A block whose only env to truncate this step is known from its step count
  // (:177, the steady state of desynchronized episodes: ~6 % of the blocks each
  // step): that env's prefetched record -- and, small grids, its current rows for the
  // terminal info -- go into LDS by LDS-DMA now, in the same round trip as round 2,
  // so its auto-reset (quad_done_path) makes no memory round trip of its own
  // (pe_coop.hpp pf_stage_issue; the LDS-DMA needs no VGPRs).  A termination is not
  // predictable: a block with one then takes the unstaged path.  Byte-coded kernels
  // only (64x64 desynchronized: 36.6 -> 36.2 us): at 20x20 the waits hipcc places
  // around a possibly outstanding LDS-DMA (a vmcnt(0) at the next use of any load
  // result) serialize round 2 in every block (9.39 -> 10.0 us, desync 11.52 -> 12.29).
  float* stage = smem + tail_off + (RT ? quad_rtab_floats(Cr, Rr) : 0);
  // (C >= kBtStageMinC only: the byte-coded C16 kernel -- config 5's codes step --
  // pays the same round-2 serialization as the f32 one would)
  const bool stage_ok = BT && CM >= kBtStageMinC && a.pf.scal && quad_coop(a, 1) &&
                        e0 + EPB <= a.n;  // full block: every lane live
  const bool stage_info = !st.cur && a.tinfo && pf_stage_info_fits(g.G, g.WPR, (int)a.pf.ostride);
  // (issued right after round 2's own loads: hipcc drains every memory op in flight
  // before the first use of a load result while an LDS-DMA is outstanding, so issued
  // earlier it would put a round trip of its own ahead of round 2)
  int npred = 0;
  uint64_t pm = 0ull;
  if (stage_ok) {
    pm = __ballot(s.step + 1 >= rl.max_steps);
    npred = __popcll(pm);
  }
  // (round 6) the env's current grid rows for its terminal info, when they do not fit the
  // record's LDS-DMA instructions (64x64, the runtime kernel's larger grids): register-staged
  // by the info wave (two 16-B units per lane) into the staging region after the record,
  // so that the info wave writes the terminal info beside the commit wave's reset instead
  // of the commit wave loading them after the done barrier (a round trip on its path)
  const int ng_s = pf_grid_units(g.G, g.WPR);
  const bool info_reg = BT && stage_ok && !stage_info && !st.cur && a.tinfo != nullptr && ng_s <= 128;
  uint4 iq0 = make_uint4(0u, 0u, 0u, 0u), iq1 = iq0;
  auto stage_issue = [&]() {
    if (BT && wv == CW && npred == 1)
      pf_stage_issue(a.pf, st, g, e0 + (__ffsll((unsigned long long)pm) - 1), stage, lane, stage_info);
    if (BT && info_reg && wv == kQuadInfoWave && npred == 1) {
      const uint4* src = reinterpret_cast<const uint4*>(st.grid + (e0 + (__ffsll((unsigned long long)pm) - 1)) * g.gstride);
      iq0 = src[lane < ng_s ? lane : ng_s - 1];
      iq1 = src[lane + 64 < ng_s ? lane + 64 : ng_s - 1];
    }
  };
  quad_move_cells<ONEWORD>(m, s, g.G);

  // Early record (one-word 64-env kernels): a block whose ONLY env to truncate this
  // step is known from its step count (:177; ~6 % of the blocks of a desynchronized
  // batch each step) has the commit wave load that env's prefetched record and its
  // grid rows (the terminal info) right before round 2's loads -- they land with them,
  // and the barrier after round 2 has waited for them -- so its auto-reset makes no
  // memory round trip of its own (quad_done_path).  Issued behind the compute phase
  // instead, the done path's first use waited for the commit's stores too (vmcnt
  // counts both, in order).  (The byte-coded kernel stages the same record by
  // LDS-DMA during round 2.)
  constexpr int KDQ = (5 * CM + 27 + 63) / 64, MAXWQ = ONEWORD ? 1 : kCoopWPR;
  // (one-word 64-env kernels only: the multi-word kernel is at its 128-VGPR cap and
  // spilled with it -- 25x25 desynchronized 14.0 -> 14.6 us -- and the 16-env shape of
  // small batches lost 2-5 % synchronized; profiles/r3c_ab_early_*.jsonl)
  // (round 5: the byte-coded one-word kernel too -- config 5's codes step; the record's
  // codes come in as 4-code words)
  constexpr bool kEarlyRec = ONEWORD && EPB == LS && KDQ <= 2;
  PfLoad<MAXWQ, KDQ> epl;
  Row4<MAXWQ> eir;
  int64_t e_early = -1, e_info = -1;
  constexpr bool kInfoW = kEarlyRec && NW == 4;
  static_assert(!kInfoW || dist_park_ok(RM, true), "info park words inside dist[]");
  if constexpr (kEarlyRec) {
    // (the commit wave only, for a block with exactly one: records for up to one
    // predicted env per wave took the desynchronized step 11.16 -> 11.06 us but the
    // synchronized one 9.42 -> 9.49, profiles/r3g_ab_*.jsonl; round 5: the env's rows
    // for its terminal info by the info wave)
    if ((wv == CW || (kInfoW && wv == kQuadInfoWave)) && a.pf.scal && a.autoreset && !st.cur) {
      const uint64_t pmk = __ballot(live && s.step + 1 >= rl.max_steps);
      const uint32_t plo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)pmk),
                     phi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(pmk >> 32));
      const uint64_t pmu = (uint64_t)plo | ((uint64_t)phi << 32);
      const int npk = __popcll(pmu);
      if (npk == 1) {
        const int64_t ep = e0 + (__ffsll((unsigned long long)pmu) - 1);
        if (wv == CW) {
          e_early = ep;
          coop_load_prefetched<MAXWQ, KDQ, OT>(a.pf, g, e_early, epl, lane);
          if constexpr (!kInfoW) eir = coop_info_rows<MAXWQ>(st, g, e_early, lane);
        } else {
          e_info = ep;
          eir = coop_info_rows<MAXWQ>(st, g, e_info, lane);
        }
      }
    }
  }
  static_assert(!BT || dist_park_ok(RM, true), "info park words inside dist[]");
  // ---- round 2: window rows of env le -> LDS [row][env] (loader role)
  uint32_t eo = 0u, en = 0u;
  if (llive) {
    const int lx = (int)(lw.x & 0xFF), ly = (int)((lw.x >> 8) & 0xFF);
    const uint64_t* lgb = st.grid + el * g.gstride;
    const int base = lx - Rr - 1;  // grid row of LDS row 0
    // Every load first, then the LDS writes: the loads are unconditional (row
    // indices clamped into the map, off-map rows selected away afterwards), so the
    // compiler issues all of them back to back and waits once -- with the range
    // tests around the loads it waited after each (one memory round trip per row).
    if constexpr (ONEWORD) {
      // (the grid block came with round 1: qg1, row pairs of 16 B)
      constexpr int JV = (NV + LT - 1) / LT;
      uint4 qv[JV];
      const uint32_t* lvb = vis_env(st, g, el, lw.w);  // (lw.w: the loader env's episode)
      {
#pragma unroll
        for (int j = 0; j < JV; ++j) {
          const int kk = sub + LT * j;
          const int xr = lx - 3 + kk;
          const int xc = xr < 0 ? 0 : (xr >= g.G ? g.G - 1 : xr);
          qv[j] = *reinterpret_cast<const uint4*>(lvb + (int64_t)xc * 4);  // g.NW == 4
        }
      }
      stage_issue();
      // the block's rows (pairs 2q, 2q+1) inside the window, then the off-map rows
      const int nq = (int)(g.gstride >> 1);
#pragma unroll
      for (int j = 0; j < JG1; ++j) {
        const int q = sub + LT * j, ka = 2 * q - base;
        if (q < nq) {
          const uint64_t lo = (uint64_t)qg1[j].x | ((uint64_t)qg1[j].y << 32);
          const uint64_t hi = (uint64_t)qg1[j].z | ((uint64_t)qg1[j].w << 32);
          if (ka >= 0 && ka < NRL) lrow[ka * LS + le] = lo;
          if (ka + 1 >= 0 && ka + 1 < NRL && 2 * q + 1 < g.G) lrow[(ka + 1) * LS + le] = hi;
        }
      }
#pragma unroll
      for (int j = 0; j < (NR + LT - 1) / LT; ++j) {
        const int k = sub + LT * j, xr = base + k;
        if (k < NRL && (xr < 0 || xr >= g.G)) lrow[k * LS + le] = kEven64;  // off-map rows: obstacles
      }
      // visit rows: one 16-B row per load, funnel-shifted to ybv
      const int lybv = ly > 0 ? ly - 1 : 0;
      const int vw = (4 * lybv) >> 5, vo = (4 * lybv) & 31;
#pragma unroll
      for (int j = 0; j < JV; ++j) {
        const int k = sub + LT * j;
        if (k < NV) {
          const int xr = lx - 3 + k;
          uint32_t lo = 0xAAAAAAAAu, hi = 0xAAAAAAAAu;  // off-map row: visit 10 (reads 1.0)
          if (xr >= 0 && xr < g.G) {
            const uint4 q = qv[j];
            lo = vw == 0 ? q.x : (vw == 1 ? q.y : q.z);
            hi = vw == 0 ? q.y : (vw == 1 ? q.z : q.w);
          }
          lvis[k * LS + le] = vo ? ((lo >> vo) | (hi << (32 - vo))) : lo;
        }
      }
    } else {
      const int lyb = ly > 0 ? ly - 1 : 0;
      const int w0 = (2 * lyb) >> 6, o = (2 * lyb) & 63;
      const int w1 = w0 + 1 < g.WPR ? w0 + 1 : w0;  // in bounds; its word is dropped when w0 is the last
      constexpr int JG = (NR + LT - 1) / LT, JV = (NV + LT - 1) / LT;
      uint64_t glo[JG], ghi[JG];
      uint32_t vlo[JV], vhi[JV];
      if (g.WPR == 2) {  // (G <= 52, e.g. the training scripts' 25x25) a row is one aligned 16-B load
#pragma unroll
        for (int j = 0; j < JG; ++j) {
          const int xr = base + sub + LT * j;
          const int xc = xr < 0 ? 0 : (xr >= g.G ? g.G - 1 : xr);
          const uint4 q = *reinterpret_cast<const uint4*>(lgb + (int64_t)xc * 2);
          const uint64_t lo64 = (uint64_t)q.x | ((uint64_t)q.y << 32), hi64 = (uint64_t)q.z | ((uint64_t)q.w << 32);
          glo[j] = w0 ? hi64 : lo64;
          ghi[j] = hi64;
        }
      } else {
#pragma unroll
        for (int j = 0; j < JG; ++j) {
          const int xr = base + sub + LT * j;
          const int xc = xr < 0 ? 0 : (xr >= g.G ? g.G - 1 : xr);
          const uint64_t* p = lgb + (int64_t)xc * g.WPR;
          glo[j] = p[w0];
          ghi[j] = p[w1];
        }
      }
      const int lybv = ly > 0 ? ly - 1 : 0;
      const int vw = (4 * lybv) >> 5, vo = (4 * lybv) & 31;
      const uint32_t* vb = vis_env(st, g, el, lw.w) + vw;
#pragma unroll
      for (int j = 0; j < JV; ++j) {
        const int xr = lx - 3 + sub + LT * j;
        const int xc = xr < 0 ? 0 : (xr >= g.G ? g.G - 1 : xr);
        vlo[j] = vb[(int64_t)xc * g.NW];
        vhi[j] = vb[(int64_t)xc * g.NW + 1];  // vw + 1 < NW always (one spare word per row)
      }
      stage_issue();
#pragma unroll
      for (int j = 0; j < JG; ++j) {
        const int k = sub + LT * j;
        if (k < NRL) {
          const int xr = base + k;
          uint64_t v = kEven64;  // off-map rows read as obstacles
          if (xr >= 0 && xr < g.G) {
            const uint64_t hi = w0 + 1 < g.WPR ? ghi[j] : 0ull;
            v = o ? ((glo[j] >> o) | (hi << (64 - o))) : glo[j];
          }
          lrow[k * LS + le] = v;
        }
      }
#pragma unroll
      for (int j = 0; j < JV; ++j) {
        const int k = sub + LT * j;
        if (k < NV) {
          const int xr = lx - 3 + k;
          uint32_t lo = 0xAAAAAAAAu, hi = 0xAAAAAAAAu;
          if (xr >= 0 && xr < g.G) {
            lo = vlo[j];
            hi = vhi[j];
          }
          lvis[k * LS + le] = vo ? ((lo >> vo) | (hi << (32 - vo))) : lo;
        }
      }
    }
  }
  // the info wave's register-staged rows into the LDS staging region (after round 2's LDS
  // writes: the wait for them is the last of the round)
  if (BT && info_reg && wv == kQuadInfoWave && npred == 1) {
    uint4* d = reinterpret_cast<uint4*>(stage) + 1 + ng_s + (int)a.pf.ostride / 16;
    if (lane < ng_s) d[lane] = iq0;
    if (lane + 64 < ng_s) d[lane + 64] = iq1;
  }
  // what the state commit needs beyond the window rows (lane = env): only in the
  // curriculum / injected-state modes (the visit and grid words it rewrites are
  // rebuilt from the window rows, see the commit)
  double cthr = 0.0;
  if (live && wv == CW) {
    if (st.cur) cthr = st.cur[e].thr;  // CurriculumWrapper threshold
    if (m.inb && (s.flags & F_EXPL_BITMAP)) {
      eo = st.expl[e * g.estride + (m.cell_o >> 5)];
      en = st.expl[e * g.estride + (m.cell_n >> 5)];
    }
  }
#ifdef PE_STAMPS
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
#endif
  // the commit wave's early record landed with round 2: a wait the compiler tracks
  // (not asm), so that the done path's first use of it carries none -- otherwise it
  // waits vmcnt(0) there, i.e. for the commit's stores too (in-order counter)
  if constexpr (kEarlyRec) {
    if (wv == CW || (kInfoW && wv == kQuadInfoWave)) __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
  }
  PE_STAMP(2);
  __syncthreads();
  PE_STAMP(3);

  // ---- transition from LDS (every wave; wave 0 commits)
  // the commit wave is the block's laggard through this phase (its state stores come
  // on top of its sector): issue priority until the done barrier (same-box A/B: 9.73
  // -> 9.65 us synchronized, 12.88 -> 12.43 us desynchronized; for the whole kernel
  // it slowed the synchronized step)
  if (wv == CW) __builtin_amdgcn_s_setprio(2);
  // BT: the LDS code table from the LDS tables (complete at the barrier above; read after the
  // done barrier).  It was a per-code if-chain of global loads in round 1, each waited out
  // at once (three dependent round trips), then the candidate loads issued with round 1
  // (profiles/r5s/ab_code_table_*.txt)
  if constexpr (BT) {
    if (threadIdx.x < 256) ctab_from_lds(smem, ctab, Rr, g.G, (int)threadIdx.x, kOneHotF + 1);
  }
  // (Tried: the early record's state writes issued here, at the start of the compute
  // phase, instead of in the done path: the commit wave then waited for them before
  // re-using their data registers -- desynchronized 11.12 -> 12.05 us, synchronized
  // 9.47 -> 9.59; profiles/r3i_ab_*.jsonl.)
  bool done = false, wfix = false;
  quad_compute<C, R, ONEWORD, NW, BT, RT, false, DV>(a, lrow, lvis, rows, tdist, tpos, tvis, lane, wv, e, live, Cr,
                                                     Rr, m, eo, en, cthr, vp0, s, ret, done, wfix);
  if constexpr (kInfoW) {  // the early env's post-step scalars for the info wave (read after the done barrier)
    if (wv == CW && e_early >= 0 && e == e_early) {
      const uint4 pk = pack(s);
      smem[kInfoParkF] = __int_as_float((int)pk.x);
      smem[kInfoParkF + 1] = __int_as_float((int)pk.y);
      smem[kInfoParkF + 2] = __int_as_float((int)pk.z);
      smem[kInfoParkF + 3] = __int_as_float((int)pk.w);
      smem[kInfoParkF + 4] = __int_as_float((int)wfix);
    }
  }
  if constexpr (BT && !kEarlyRec && NW > kQuadInfoWave) {  // a block's one done env's post-step scalars for the
                                                            // info wave (as kInfoW)
    if (wv == CW) {
      const uint64_t dm1 = __ballot(done);
      if (__popcll(dm1) == 1 && done) {
        const uint4 pk = pack(s);
        smem[kInfoParkF] = __int_as_float((int)pk.x);
        smem[kInfoParkF + 1] = __int_as_float((int)pk.y);
        smem[kInfoParkF + 2] = __int_as_float((int)pk.z);
        smem[kInfoParkF + 3] = __int_as_float((int)pk.w);
        smem[kInfoParkF + 4] = __int_as_float((int)wfix);
      }
    }
  }
  PE_STAMP(4);
  // ---- DummyVecEnv auto-reset (rare): commit wave, after the whole obs row is in LDS
  // any env of the block done (the usual answer: no)?  The commit wave's done mask
  // goes to an unused LDS table word (kDoneMaskF, above the ray tables: dist_park_ok) for the
  // count the reset path needs.
  if (wv == CW) {
    const uint64_t dm = __ballot(done);
    if (lane == 0) reinterpret_cast<uint64_t*>(smem)[kDoneMask64] = dm;
  }
  // The block barrier (obs rows and the done mask complete in LDS) WITHOUT a memory
  // fence: __syncthreads() would make the commit wave wait for its state stores to
  // land first (s_waitcnt vmcnt(0)), although nothing in this launch reads them
  // back -- the reset path orders its own accesses (see quad_done_path).
  if (wv == CW) __builtin_amdgcn_s_setprio(0);
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  const uint64_t dmask = reinterpret_cast<const uint64_t*>(smem)[kDoneMask64];  // after the asm barrier ("memory")
  const uint64_t dmu = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)dmask) |
                       ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(dmask >> 32)) << 32);
  const bool any_done = dmu != 0ull;
  const int ndone = __popcll(dmu);
  // (Tried: a single-done fast path -- the early record checked before the done barrier,
  // no barrier after the reset, the commit wave storing its env's chunks of the tile and
  // the other waves the rest at once: desync 11.14 -> 11.38 us, synchronized 9.46 -> 9.60;
  // profiles/r3n_ab_*.jsonl.)
  PE_STAMP(5);
  // auto-reset slow path, out of line (its registers stay off the hot path)
  // (RT: the region is sized by the actual R -- pe_create checks these at run time)
  static_assert(RT || 2 * C * R <= (NR * 8 + NV * 4) * LS, "LIDAR offset tables must fit the window region");
  static_assert(RT || 5 * 4 * LS + 8 <= (NR * 8 + NV * 4) * LS, "reset staging must fit the window region");
  const int64_t valid = a.n - e0 < EPB ? a.n - e0 : EPB;
  if (__builtin_expect(any_done, 0)) {  // cold: laid out after the hot path
    const bool staged = stage_ok && npred == 1 && ndone == 1;  // then the done env is the predicted one
    const uint4 ns = quad_done_path<NW, ONEWORD, (5 * CM + 27 + 63) / 64, BT>(
        kernargs(), tile_off, Cr, Rr, lane, wv, CW, e0, done, pack(s), ret, ndone, wfix, ctab,
        staged ? stage : nullptr, staged && stage_info, e_early, &epl, &eir, e_info, false, staged && info_reg);
    s = unpack(ns);
  }
  // the obs tile goes out through the waves other than the commit wave: its state
  // stores are still in flight (no fence at the barrier above), and the compiler
  // would make every iteration of its store loop wait for them (s_waitcnt vmcnt(0)
  // before re-using a store's data registers)
  if constexpr (CM >= 64) {  // long rows: the commit wave's share pays for its wait (64x64: 33.2 -> 32.7 us)
    if (wv == CW) __builtin_amdgcn_s_waitcnt(0x0F70);  // tracked vmcnt(0): no wait inside the loop
    if constexpr (BT) {
      if (a.obs_codes)
        store_tile_bytes(rows, a.obs_codes + e0 * g.D, (int)valid, g.D, (int)threadIdx.x, (int)blockDim.x);
      else
        store_tile_codes(rows, ctab, a.obs + e0 * g.D, (int)valid, g.D, (int)threadIdx.x, (int)blockDim.x);
    } else
      store_tile(rows, a.obs + e0 * g.D, (int)valid, g.D, g.D);
  } else {
    if (wv != CW) {
      if constexpr (BT) {
        if (a.obs_codes)
          store_tile_bytes(rows, a.obs_codes + e0 * g.D, (int)valid, g.D, (int)threadIdx.x, 64 * (NW - 1));
        else
          store_tile_codes(rows, ctab, a.obs + e0 * g.D, (int)valid, g.D, (int)threadIdx.x, 64 * (NW - 1));
      } else
        store_tile(rows, a.obs + e0 * g.D, (int)valid, g.D, g.D, (int)threadIdx.x, 64 * (NW - 1));
    }
  }
  if constexpr (BT) {
    if (any_done && a.autoreset && !quad_coop(a, ndone)) {
      // the tile store above wrote stale values (the terminal codes) into the done rows:
      // drain it, then overwrite those rows with the fresh obs built from the env's rows
      // in HBM (the f32 tile's lane path left its fresh rows in the tile: dense_reset_commit)
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      quad_done_obs<NW, BT>(kernargs(), tile_off, lane, e, done, pack(s));
    }
  }
#ifdef PE_STAMPS_RESET
  if (!BT && any_done && !quad_coop(a, ndone)) {  // R5: the block's tile (fresh rows included) has landed
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    PE_RSTAMP(5);
  }
#endif
  PE_STAMP(6);
#ifdef PE_STAMPS
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
  PE_STAMP(7);
}
