// pe_quad_done.hpp -- the sector kernels' LDS layout (quad_tile_off and what follows the tile) and
// their auto-reset slow path: kernargs, quad_coop, el_info_hit, dense_reset_commit, quad_done_path,
// quad_done_obs.  pe_step_quad and pe_step_far (pe_far.hpp) both end in it.
// (a fragment of plantos_batch.hip's anonymous namespace; include after pe_quad.hpp, pe_obs.hpp,
// pe_tile.hpp and pe_stamps.hpp)
#pragma once

// (The round-1 phase ablations and the round-2 timing probes -- PE_ABLATE, PE_PROBE_*,
// PE_VIS_R1 -- were separate libraries built from this file; their results are in
// DESIGN.md §8 and profiles/r1d_ablation.json, profiles/r2ag_*; the probes are gone.)
// (The sector kernel's closed compile-time A/Bs -- the grid block in round 2, buffer tile stores,
// the register-staged record, the two-word grid block in round 1, two early records and the
// rest -- are recorded in DESIGN.md §8; their code is gone.)
// byte-coded kernels stage the predicted record by LDS-DMA from this C on (see stage_ok in
// pe_step_quad: the byte-coded C16 kernel would pay for it in round 2)
constexpr int kBtStageMinC = 64;
constexpr int kStaggerGroups = 4;  // sector kernel: the grid's start-delay groups

// Quadrant-split fused step (pe_quad.hpp): 4 waves x 64 envs per workgroup.
// Same semantics as pe_step_wave.
template <int R>
constexpr int quad_tile_off() {
  return (kTabFloats + (2 * R + 3) * kQuadEnvs * 2 + 7 * kQuadEnvs + 3) & ~3;
}
// the runtime sector kernel (pe_step_quad<0, 0, ...>): maxima and its layout -- C up to
// 32 with the f32 tile, up to 64 with the byte-coded one (the f32 tile of 64 rays holds
// the kernel to one workgroup per CU)
constexpr int kRtCMax = 32, kRtCMaxBT = 64, kRtRMax = 14;
__host__ __device__ constexpr int quad_tile_off_rt(int R) {
  return (kTabFloats + (2 * R + 3) * kQuadEnvs * 2 + 7 * kQuadEnvs + 3) & ~3;
}
// byte-coded tile (BT): the code table ctab[256] after the [64 x D] code tile
template <int R, int C>
constexpr int quad_ctab_off() {
  return quad_tile_off<R>() + ((kQuadEnvs * (5 * C + 27) + 15) / 16) * 4;
}
__host__ __device__ constexpr int quad_ctab_off_rt(int R, int C) {
  return quad_tile_off_rt(R) + ((kQuadEnvs * (5 * C + 27) + 15) / 16) * 4;
}
// offset (floats) from the tile to what follows it (+ the code table)
__host__ __device__ constexpr int quad_rtab_off(int C, bool bt) {
  return bt ? ((kQuadEnvs * (5 * C + 27) + 15) / 16) * 4 + 256 : kQuadEnvs * (5 * C + 27);
}
// the runtime sector kernel's probe table in LDS (floats; C rays x R rounded up to 8
// int16 entries), placed after the tile (+ code table) and before the staging region
__host__ __device__ constexpr int quad_rtab_floats(int C, int R) { return C * ((R + 7) & ~7); }  // u32 entries

// ---- pe_step_quad's auto-reset slow path (a block with a done env), out of line:
// kept in separate functions so that their register demand (map generation, the
// cooperative reset) does not raise the hot path's.  `ka` is the kernel's
// argument segment (StepArgs); LDS is the kernel's dynamic LDS (same layout).
// the kernel's argument segment as a generic pointer (constant and global
// addresses coincide in the flat space)
__device__ __forceinline__ const void* kernargs() {
  return reinterpret_cast<const void*>(reinterpret_cast<uintptr_t>(__builtin_amdgcn_kernarg_segment_ptr()));
}

__device__ __forceinline__ bool quad_coop(const StepArgs& a, int ndone) {
  return a.autoreset && ndone <= a.coop_max_done;
}

// The single-done early record's terminal info by a second wave (round 5): the commit
// wave loads the record, the info wave (kQuadInfoWave) the env's current rows in round
// 2; at the done path the info wave reduces and stores the info while the commit wave
// takes the record -- the info's wave reductions off the one-done block's critical path.
// The commit wave parks the env's post-step scalars + wfix in free table words
// (kInfoParkF, pe_device.hpp's map of dist[]) before the done barrier.
constexpr int kQuadInfoWave = 2;  // (4-wave kernels; the slice / position wave)
__device__ __forceinline__ bool el_info_hit(int64_t e_info, int64_t e0, const float* smem) {
  // the block's one done env (the done mask, kDoneMaskF) is the info wave's early env
  const uint64_t dmw = reinterpret_cast<const uint64_t*>(smem)[kDoneMask64];
  return e_info >= 0 && e_info == e0 + (__ffsll((unsigned long long)dmw) - 1);
}

// The second half of the lane-per-env reset of a block with many done envs (quad_done_path,
// f32 tile), run by the commit wave with all lanes: each done lane's map lies as a grid
// image in its own tile row (reset_env_image).  Lane l marches its env's rays from the image
// (the results parked as bytes in `rays` [C][64]); then the wave as a whole copies the
// images to the envs' grid blocks and writes the fresh visit slots with consecutive lanes on
// consecutive words (one lane per env put every store of a wave instruction into a line of
// its own); lane l stores its scalars and writes the fresh obs row over the dead image, so
// that the tile store emits every row once.  Returns lane l's scalars.
__device__ __forceinline__ Scal dense_reset_commit(const StepArgs& a, const Tables* ltab, float* rowsf, uint8_t* rays,
                                                   const signed char* ldx, const signed char* ldy, int64_t e0, int lane,
                                                   bool done, bool keep, Scal s) {
  const Geo& g = a.g;
  const State& st = a.st;
  const int D = g.D, C = g.C, R = g.R, GW = g.G * g.WPR;
  const uint64_t dm = __ballot(done);
  const float* tdist = ltab->dist;
  const float* tpos = ltab->pos;
  const float* tvis = ltab->vis;
  if (done) {  // as build_obs_fresh (plantos_env.py:260-292): distance | entity << 6
    const uint64_t* sg = reinterpret_cast<const uint64_t*>(rowsf + lane * D + ((lane * D) & 1));
    for (int i = 0; i < C; ++i) {
      int dist = R, ent = EMPTY;
      for (int r = 1; r <= R; ++r) {
        const int cx = s.x + ldx[i * R + r - 1];
        const int cy = s.y + ldy[i * R + r - 1];
        const int code = (cx >= 0 && cx < g.G) ? img_code(sg, g, cx, cy + R) : OBST;  // :271-284
        if (code != EMPTY) {
          dist = r;
          ent = code;
          break;
        }
      }
      rays[i * kQuadEnvs + lane] = (uint8_t)(dist | (ent << 6));
    }
  }
  // the terminal info's reads of the old grid rows are consumed, and the commit's stores to
  // them (the curriculum's watering / visit) have landed, before other lanes rewrite the rows
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  for (int u = lane; u < kQuadEnvs * GW; u += 64) {  // grid images -> grid blocks, 8-B words
    const int l = u / GW, k = u - l * GW;
    if ((dm >> l) & 1ull) {
      const uint64_t* sl = reinterpret_cast<const uint64_t*>(rowsf + l * D + ((l * D) & 1));
      st.grid[(e0 + l) * g.gstride + k] = sl[k];
    }
  }
  // fresh visit slots (reset_visits: vis_pad everywhere, the rover's nibble 1) of the done
  // envs that do not carry their counts; env l's new position / slot from lane l
  const uint32_t pv = (uint32_t)s.x | ((uint32_t)s.y << 8) | ((s.episode & 1u) << 16) |
                      ((s.flags & F_NOROOM) ? 1u << 17 : 0u) | ((done && !keep) ? 1u << 18 : 0u);
  const int VS = (int)g.vslot, NWv = g.NW;
  auto vword = [&](uint32_t q, int k) -> uint32_t {  // word k of env q's fresh slot
    const int row = k / NWv, w = k - row * NWv;
    const int bit = 4 * ((int)((q >> 8) & 0xFFu) + 2);
    uint32_t v = ltab->vis_pad[w];
    if (!(q & (1u << 17)) && row == (int)(q & 0xFFu) && w == (bit >> 5)) v = (v & ~(0xFu << (bit & 31))) | (1u << (bit & 31));
    return v;
  };
  if ((VS & 3) == 0 && (reinterpret_cast<uintptr_t>(st.vis) & 15u) == 0) {  // 16-B units (vstride = 2 vslot)
    const int U = VS >> 2;
    for (int u = lane; u < kQuadEnvs * U; u += 64) {
      const int l = u / U, k = u - l * U;
      const uint32_t q = (uint32_t)__shfl((int)pv, l);
      if (q & (1u << 18)) {
        const uint4 v = make_uint4(vword(q, 4 * k), vword(q, 4 * k + 1), vword(q, 4 * k + 2), vword(q, 4 * k + 3));
        *reinterpret_cast<uint4*>(st.vis + (e0 + l) * g.vstride + (int64_t)((q >> 16) & 1u) * g.vslot + 4 * k) = v;
      }
    }
  } else {
    for (int u = lane; u < kQuadEnvs * VS; u += 64) {
      const int l = u / VS, k = u - l * VS;
      const uint32_t q = (uint32_t)__shfl((int)pv, l);
      if (q & (1u << 18)) st.vis[(e0 + l) * g.vstride + (int64_t)((q >> 16) & 1u) * g.vslot + k] = vword(q, k);
    }
  }
  if (done) {
    if (keep) new_episode_visits(st, g, ltab, e0 + lane, s, true);  // carried counts: lane by lane
    st.ep_ret[e0 + lane] = 0.0;
    st.scal[e0 + lane] = pack(s);
  }
  PE_RSTAMP(3);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // every image is read out (LDS in order; the compiler: no reordering)
  if (done) {  // as build_obs_fresh, into the env's tile row
    float* out = rowsf + lane * D;
    for (int i = 0; i < C; ++i) {
      const int b = rays[i * kQuadEnvs + lane], ent = b >> 6;
      out[5 * i] = tdist[b & 63];
      out[5 * i + 1] = ent == 0 ? 1.0f : 0.0f;
      out[5 * i + 2] = ent == 1 ? 1.0f : 0.0f;
      out[5 * i + 3] = ent == 2 ? 1.0f : 0.0f;
      out[5 * i + 4] = ent == 3 ? 1.0f : 0.0f;
    }
    out[5 * C] = tpos[s.x];
    out[5 * C + 1] = tpos[s.y];
    for (int lx = 0; lx < 5; ++lx)
      for (int ly = 0; ly < 5; ++ly) {
        const int gx = s.x + lx - 2, gy = s.y + ly - 2;
        const bool in = gx >= 0 && gx < g.G && gy >= 0 && gy < g.G;  // :307-311
        const bool rover = lx == 2 && ly == 2 && !(s.flags & F_NOROOM);
        out[5 * C + 2 + 5 * lx + ly] = !in ? tvis[10] : (rover ? tvis[1] : tvis[0]);
      }
  }
  PE_RSTAMP(4);
  return s;
}

// BT: the obs tile holds byte codes (ctab: the LDS code table), see pe_step_quad.
// DB: the row copies as batched reads, then writes -- where the registers are there: rows of at most
// 128 values, or a path out of line (the far kernel's far_done); inlined into the C64 / runtime
// byte-tile kernels (KD = 6) it cost their hot path (64x64/C64 24.15 -> 25.0 us, profiles/r6h/)
template <int NW, bool ONEWORD, int KD, bool BT = false, bool DB = (KD <= 2)>  // one copy per kernel: each
                                                                              // inherits its kernel's register budget
__device__ __forceinline__ uint4 quad_done_path(const void* ka, int tile_off, int C, int R, int lane, int wv, int CW,
                                                int64_t e0, bool done, uint4 sp, double ret, int ndone, bool wfix,
                                                const float* ctab = nullptr, const float* stage = nullptr,
                                                bool stage_info = false, int64_t e_early = -1,
                                                const PfLoad<ONEWORD ? 1 : kCoopWPR, KD>* early = nullptr,
                                                const Row4<ONEWORD ? 1 : kCoopWPR>* early_rows = nullptr,
                                                int64_t e_info = -1, bool stage_reg = false, bool info_iw = false) {
  // stage_reg: always false -- `stage` written by register-staged copies, a path since removed.
  // The parameter stays only because without it hipcc lays out the cold blocks of far_done and
  // of the byte-tile kernels that stage by LDS-DMA differently (2-20 instructions): dropping
  // it belongs to a change that may move instruction streams.
  // info_iw: the env's terminal-info rows were register-staged into `stage` (after the record) by
  // the info wave (kQuadInfoWave), which writes the terminal info beside the commit wave's reset
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const StepArgs& a = *reinterpret_cast<const StepArgs*>(ka);
  const Geo& g = a.g;
  const Rules& rl = a.rl;
  const State& st = a.st;
  float* tdist = smem;
  float* tpos = smem + kTabPos;
  float* tvis = smem + kTabVis;
  const Tables* ltab = reinterpret_cast<const Tables*>(smem);
  uint64_t* lrow = reinterpret_cast<uint64_t*>(smem + kTabFloats);
  using OT = typename std::conditional<BT, uint8_t, float>::type;
  OT* rows = reinterpret_cast<OT*>(smem + tile_off);
  OT* row = rows + lane * g.D;
  const int64_t e = e0 + lane;
  Scal s = unpack(sp);
  constexpr int MAXW = ONEWORD ? 1 : kCoopWPR;
  // the early record's terminal info is the info wave's (the kernel's kInfoW)
  constexpr bool kIW = NW == 4 && ONEWORD && KD <= 2;
  // done path without the early record: every load (record, terminal-info rows, terminal obs)
  // issued before any store, one wait, then the stores -- vmcnt counts stores too, in order, so
  // a load consumed after a store waits for that store.  The one-word f32 kernels only (the
  // multi-word and byte-tile ones measured slower with it)
  constexpr bool kOneWait = DB && ONEWORD && !BT;
  // the table reads of the reset / info helpers as LDS reads of ltab (pe_coop.hpp LdsTables):
  // the one-word f32 kernels (the others measured slower with them, 64x64 +0.2 us desync)
  constexpr bool kLT = ONEWORD && !BT;
  // an obs tile value as a float (BT: expand the code)
  auto tval = [&](const OT* r, int k) -> float {
    if constexpr (BT) return ctab[r[k]];
    else return r[k];
  };
  // a prefetched record's fresh obs row into tile row `o` once taken (BT: codes)
  auto take = [&](int64_t el, uint32_t episode, const PfLoad<MAXW, KD>& pl, Row4<MAXW>& rw, Scal& ns, OT* o) -> bool {
    return coop_take_prefetched<MAXW, KD, OT>(a.pf, g, el, episode, pl, rw, ns, o, lane);
  };
  if (ndone == 1 && quad_coop(a, ndone)) {
    // One done env (the usual case with desynchronized episodes): the commit wave,
    // which holds its scalars, resets it alone -- no staging, one barrier.
    if (wv == CW) {
      PE_DSTAMP(0);
      const uint64_t dmw = reinterpret_cast<const uint64_t*>(smem)[kDoneMask64];
      const int l = __ffsll((unsigned long long)dmw) - 1;
      const int64_t el = e0 + l;
      OT* orow = rows + l * g.D;
      // early: the kernel loaded this env's record and rows behind the compute phase
      const bool early_hit = KD <= 2 && early != nullptr && el == e_early;
      if (early_hit) {
        // the record and the env's rows were loaded behind the compute phase (the
        // kernel's early record): every wait here is for loads issued ~1 us ago.
        // Terminal obs held in registers while the fresh row replaces it in the tile;
        // stores only after every load is consumed.
        const int wf = __builtin_amdgcn_readlane((int)wfix, l);
        const Scal sv = unpack(make_uint4((uint32_t)__builtin_amdgcn_readlane((int)sp.x, l),
                                          (uint32_t)__builtin_amdgcn_readlane((int)sp.y, l),
                                          (uint32_t)__builtin_amdgcn_readlane((int)sp.z, l),
                                          (uint32_t)__builtin_amdgcn_readlane((int)sp.w, l)));
        float tv[KD];
#pragma unroll
        for (int j = 0; j < KD; ++j) tv[j] = lane + 64 * j < g.D ? tval(orow, lane + 64 * j) : 0.0f;
        PE_DSTAMP(1);
        // (the terminal info: the info wave's, below, when it loaded the env's rows)
        if (a.tinfo && !kIW) coop_info_store<MAXW, kLT>(st, g, *early_rows, sv, a.tinfo + el * PE_NINFO, lane, wf, ltab);
        PE_DSTAMP(2);
        Row4<MAXW> rw;
        Scal ns;
        asm volatile("" ::: "memory");  // terminal obs read out of the row before the fresh one goes in
        if (take(el, sv.episode, *early, rw, ns, orow)) {
          ns = coop_apply_reset<MAXW, kLT>(st, g, el, ns, false, rw, lane, ltab, true);
        } else {  // the record is not this reset's (not generated yet): generate in place
          uint64_t* scr = reinterpret_cast<uint64_t*>(lrow) + 162 + wv * coop_scratch_words(g.G, g.WPR);
          ns = coop_reset_env<MAXW, kLT>(st, g, rl, el, sv.episode, false, rw, lane, scr, ltab);
          coop_fresh_obs<MAXW>(g, rw, ns, orow, tdist, tpos, tvis, st.ldx, st.ldy, lane);
        }
        PE_DSTAMP(3);
        if (a.tobs) {
          float* t = a.tobs + el * g.D;
#pragma unroll
          for (int j = 0; j < KD; ++j)
            if (lane + 64 * j < g.D) t[lane + 64 * j] = tv[j];
        }
        if (lane == 0) a.pf.flag[el] = 1;  // its next map goes into the next generating batch
        PE_DSTAMP(4);
        if (done) {  // lane l: program order after its commit stores
          s = ns;
          st.ep_ret[e] = 0.0;
          st.scal[e] = pack(s);
        }
        PE_DSTAMP(5);
      } else {
        // the record: staged into LDS before the done barrier (stage), or loaded now
        PfLoad<MAXW, KD> pl;
        if (a.pf.scal && !stage) coop_load_prefetched<MAXW, KD, OT>(a.pf, g, el, pl, lane);  // in flight from here on
        bool keep = false;
        if (done && st.cur) keep = curriculum_on_reset(st.cur, e, rl);  // A2C_training.py:56-95
        const bool kp = __builtin_amdgcn_readlane((int)keep, l) != 0;
        const int wf = __builtin_amdgcn_readlane((int)wfix, l);
        const Scal sv = unpack(make_uint4((uint32_t)__builtin_amdgcn_readlane((int)sp.x, l),
                                          (uint32_t)__builtin_amdgcn_readlane((int)sp.y, l),
                                          (uint32_t)__builtin_amdgcn_readlane((int)sp.z, l),
                                          (uint32_t)__builtin_amdgcn_readlane((int)sp.w, l)));
        if constexpr (kOneWait) {
          // loads first (the record above, the info rows, the terminal obs out of the
          // tile), one wait, then every store
          if (st.cur) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the commit's rows landed
          const bool iload = a.tinfo && !info_iw && !stage_info;
          Row4<MAXW> ir{0ull, 0ull, 0ull, 0ull};
          if (iload) ir = coop_info_rows<MAXW>(st, g, el, lane);
          float tv[KD];
#pragma unroll
          for (int j = 0; j < KD; ++j) tv[j] = a.tobs && lane + 64 * j < g.D ? tval(orow, lane + 64 * j) : 0.0f;
          __builtin_amdgcn_s_waitcnt(0x0F70);  // (tracked: no later wait for these loads; stage: the DMA)
          PE_DSTAMP(1);
          if (a.tinfo && !info_iw) {
            if (stage_info)
              coop_info_store<MAXW, kLT>(st, g,
                                    pf_stage_rows<MAXW>(reinterpret_cast<const uint64_t*>(
                                                            stage + 4 + 4 * pf_grid_units(g.G, g.WPR) + a.pf.ostride / 4),
                                                        g, lane),
                                    sv, a.tinfo + el * PE_NINFO, lane, wf, ltab);
            else
              coop_info_store<MAXW, kLT>(st, g, ir, sv, a.tinfo + el * PE_NINFO, lane, wf, ltab);
          }
          PE_DSTAMP(2);
          Row4<MAXW> rw;
          Scal ns;
          asm volatile("" ::: "memory");  // terminal obs read out of the row before the fresh one goes in
          const bool took = stage ? pf_stage_take<MAXW, OT, KD>(stage, g, (int)a.pf.ostride, sv.episode, rw, ns, orow, lane)
                                  : (a.pf.scal && take(el, sv.episode, pl, rw, ns, orow));
          if (took) {
            ns = coop_apply_reset<MAXW, kLT>(st, g, el, ns, kp, rw, lane, ltab, true);
          } else {
            uint64_t* scr = reinterpret_cast<uint64_t*>(lrow) + 162 + wv * coop_scratch_words(g.G, g.WPR);
            ns = coop_reset_env<MAXW, kLT>(st, g, rl, el, sv.episode, kp, rw, lane, scr, ltab);
            coop_fresh_obs<MAXW>(g, rw, ns, orow, tdist, tpos, tvis, st.ldx, st.ldy, lane);
          }
          PE_DSTAMP(3);
          if (a.tobs) {
            float* t = a.tobs + el * g.D;
#pragma unroll
            for (int j = 0; j < KD; ++j)
              if (lane + 64 * j < g.D) t[lane + 64 * j] = tv[j];
          }
          if (a.pf.scal && lane == 0) a.pf.flag[el] = 1;  // its next map goes into the next generating batch
          PE_DSTAMP(4);
          if (done) {  // lane l: program order after its commit stores
            s = ns;
            st.ep_ret[e] = 0.0;
            st.scal[e] = pack(s);
          }
          PE_DSTAMP(5);
        } else {
          if (a.tobs) {  // (the row's reads first, then the stores: one LDS round trip, not one per 64 values)
            float* t = a.tobs + el * g.D;
            if constexpr (DB) {
              float tv[KD];
#pragma unroll
              for (int j = 0; j < KD; ++j) tv[j] = lane + 64 * j < g.D ? tval(orow, lane + 64 * j) : 0.0f;
#pragma unroll
              for (int j = 0; j < KD; ++j)
                if (lane + 64 * j < g.D) t[lane + 64 * j] = tv[j];
            } else {
              for (int k2 = lane; k2 < g.D; k2 += 64) t[k2] = tval(orow, k2);
            }
          }
          // with the curriculum the commit stored this env's rows: they must land before
          // the info reads them and the reset rewrites them
          if (st.cur || (stage && !stage_reg)) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (stage: the LDS-DMA landed)
          PE_DSTAMP(1);
          if (a.tinfo && !info_iw) {  // (register-staged info rows: the info wave's)
            if (stage_info)  // the env's rows came with the record
              coop_info_store<MAXW, kLT>(st, g,
                                    pf_stage_rows<MAXW>(reinterpret_cast<const uint64_t*>(
                                                            stage + 4 + 4 * pf_grid_units(g.G, g.WPR) + a.pf.ostride / 4),
                                                        g, lane),
                                    sv, a.tinfo + el * PE_NINFO, lane, wf, ltab);
            else
              coop_write_info<MAXW, kLT>(st, g, el, sv, a.tinfo + el * PE_NINFO, lane, wf, ltab);
          }
          PE_DSTAMP(2);
          Row4<MAXW> rw;
          Scal ns;
          asm volatile("" ::: "memory");  // terminal obs read out of the row before the fresh one goes in
          const bool took = stage ? pf_stage_take<MAXW, OT, DB ? KD : 0>(stage, g, (int)a.pf.ostride, sv.episode, rw, ns, orow, lane)
                                  : (a.pf.scal && take(el, sv.episode, pl, rw, ns, orow));
          if (took) {
            ns = coop_apply_reset<MAXW, kLT>(st, g, el, ns, kp, rw, lane, ltab, true);
          } else {
            uint64_t* scr = reinterpret_cast<uint64_t*>(lrow) + 162 + wv * coop_scratch_words(g.G, g.WPR);
            ns = coop_reset_env<MAXW, kLT>(st, g, rl, el, sv.episode, kp, rw, lane, scr, ltab);
            coop_fresh_obs<MAXW>(g, rw, ns, orow, tdist, tpos, tvis, st.ldx, st.ldy, lane);
          }
          PE_DSTAMP(3);
          if (a.pf.scal && lane == 0) a.pf.flag[el] = 1;  // its next map goes into the next generating batch
          PE_DSTAMP(4);
          if (done) {  // lane l: program order after its commit stores
            s = ns;
            st.ep_ret[e] = 0.0;
            st.scal[e] = pack(s);
          }
          PE_DSTAMP(5);
        }
      }
    } else if (kIW && a.tinfo && wv == kQuadInfoWave && el_info_hit(e_info, e0, smem)) {
      // the terminal info of the early-record env (_get_info, plantos_env.py:317-336) by
      // the info wave, beside the commit wave's reset: the env's rows came with round 2,
      // its post-step scalars through LDS (quad_info_park)
      const float* pk = smem + kInfoParkF;
      const uint4 spk = make_uint4((uint32_t)__builtin_amdgcn_readfirstlane(__float_as_int(pk[0])),
                                   (uint32_t)__builtin_amdgcn_readfirstlane(__float_as_int(pk[1])),
                                   (uint32_t)__builtin_amdgcn_readfirstlane(__float_as_int(pk[2])),
                                   (uint32_t)__builtin_amdgcn_readfirstlane(__float_as_int(pk[3])));
      const int wf = __builtin_amdgcn_readfirstlane(__float_as_int(pk[4]));
      coop_info_store<MAXW, kLT>(st, g, *early_rows, unpack(spk), a.tinfo + e_info * PE_NINFO, lane, wf, ltab);
    } else if (info_iw && a.tinfo && wv == kQuadInfoWave) {
      // the terminal info of the staged env (the block's one done env: its truncation was
      // predicted) by the info wave from its rows register-staged in round 2 and its
      // post-step scalars parked by the commit wave (kInfoParkF)
      const uint64_t dmw = reinterpret_cast<const uint64_t*>(smem)[kDoneMask64];
      const int64_t el = e0 + (__ffsll((unsigned long long)dmw) - 1);
      const float* pk = smem + kInfoParkF;
      const uint4 spk = make_uint4((uint32_t)__builtin_amdgcn_readfirstlane(__float_as_int(pk[0])),
                                   (uint32_t)__builtin_amdgcn_readfirstlane(__float_as_int(pk[1])),
                                   (uint32_t)__builtin_amdgcn_readfirstlane(__float_as_int(pk[2])),
                                   (uint32_t)__builtin_amdgcn_readfirstlane(__float_as_int(pk[3])));
      const int wf = __builtin_amdgcn_readfirstlane(__float_as_int(pk[4]));
      coop_info_store<MAXW, kLT>(st, g,
                            pf_stage_rows<MAXW>(reinterpret_cast<const uint64_t*>(
                                                    stage + 4 + 4 * pf_grid_units(g.G, g.WPR) + a.pf.ostride / 4),
                                                g, lane),
                            unpack(spk), a.tinfo + el * PE_NINFO, lane, wf, ltab);
    }
    __syncthreads();  // the fresh obs row is in the tile
    __builtin_amdgcn_s_waitcnt(0x0F70);  // see the end of the path below
    return pack(s);
  }
  if (quad_coop(a, ndone)) {
    // A few done envs: wave-cooperative resets (pe_coop.hpp), spread over the
    // block's waves (the k-th done env to wave k % NW).  For each, the 64 lanes
    // copy the terminal obs row out, write the terminal info, generate the map,
    // write grid + visit rows and build the fresh obs into the env's tile row,
    // which the tile store then streams out with the others.  The commit wave
    // stages each done env's scalars in the (dead) window region of LDS and
    // stores the new ones afterwards: every store to an env's scalars stays in
    // its own lane, in program order.
    uint32_t* stage = reinterpret_cast<uint32_t*>(lrow);  // [64][5]: packed scalars, keep
    uint64_t* dmask = reinterpret_cast<uint64_t*>(stage + 5 * kQuadEnvs);
    const int NWv = blockDim.x >> 6;
    if (wv == CW) {
      bool keep = false;
      if (done) {
        if (st.cur) keep = curriculum_on_reset(st.cur, e, rl);  // A2C_training.py:56-95
        stage[5 * lane] = sp.x;
        stage[5 * lane + 1] = sp.y;
        stage[5 * lane + 2] = sp.z;
        stage[5 * lane + 3] = sp.w;
        stage[5 * lane + 4] = (uint32_t)keep | ((uint32_t)wfix << 1);
      }
      const uint64_t dm = __ballot(done);
      if (lane == 0) *dmask = dm;
      // with the curriculum, the commit's grid / visit stores of a done env
      // (watering, the carried visit) must land before other waves read its rows
      // (terminal info) and write new ones; otherwise it made none (see the commit)
      if (st.cur) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    {
      const uint64_t dml = *dmask;  // uniform: read into scalar registers
      uint64_t dm = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)dml) |
                    ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(dml >> 32)) << 32);
      for (int k = 0; dm; ++k) {
        const int l = __ffsll((unsigned long long)dm) - 1;
        dm &= dm - 1;
        if (k % NWv != wv) continue;
        const int64_t el = e0 + l;
        OT* orow = rows + l * g.D;
        if constexpr (kOneWait) {
          // loads first (the record, the info rows, the terminal obs), one wait, then
          // every store (as the single-done path)
          const uint4 sl = make_uint4((uint32_t)__builtin_amdgcn_readfirstlane((int)stage[5 * l]),
                                      (uint32_t)__builtin_amdgcn_readfirstlane((int)stage[5 * l + 1]),
                                      (uint32_t)__builtin_amdgcn_readfirstlane((int)stage[5 * l + 2]),
                                      (uint32_t)__builtin_amdgcn_readfirstlane((int)stage[5 * l + 3]));
          const int kw = __builtin_amdgcn_readfirstlane((int)stage[5 * l + 4]);
          const bool kp = (kw & 1) != 0;
          const Scal sv = unpack(sl);
          const bool eh = KD <= 2 && early != nullptr && el == e_early;
          const bool erows = eh && (!kIW || e_info == el);  // (as below)
          PfLoad<MAXW, KD> pl;
          if (a.pf.scal && !eh) coop_load_prefetched<MAXW, KD, OT>(a.pf, g, el, pl, lane);
          Row4<MAXW> ir{0ull, 0ull, 0ull, 0ull};
          if (a.tinfo && !erows) ir = coop_info_rows<MAXW>(st, g, el, lane);
          float tv[KD];
#pragma unroll
          for (int j = 0; j < KD; ++j) tv[j] = a.tobs && lane + 64 * j < g.D ? tval(orow, lane + 64 * j) : 0.0f;
          __builtin_amdgcn_s_waitcnt(0x0F70);
          if (a.tinfo) coop_info_store<MAXW, kLT>(st, g, erows ? *early_rows : ir, sv, a.tinfo + el * PE_NINFO, lane, kw >> 1, ltab);
          Row4<MAXW> rw;
          Scal ns;
          asm volatile("" ::: "memory");  // terminal obs read out of the row before the fresh one goes in
          if (a.pf.scal && take(el, sv.episode, eh ? *early : pl, rw, ns, orow)) {
            ns = coop_apply_reset<MAXW, kLT>(st, g, el, ns, kp, rw, lane, ltab, true);
          } else {
            uint64_t* scr = reinterpret_cast<uint64_t*>(lrow) + 162 + wv * coop_scratch_words(g.G, g.WPR);
            ns = coop_reset_env<MAXW, kLT>(st, g, rl, el, sv.episode, kp, rw, lane, scr, ltab);
            coop_fresh_obs<MAXW>(g, rw, ns, orow, tdist, tpos, tvis, st.ldx, st.ldy, lane);
          }
          if (a.tobs) {
            float* t = a.tobs + el * g.D;
#pragma unroll
            for (int j = 0; j < KD; ++j)
              if (lane + 64 * j < g.D) t[lane + 64 * j] = tv[j];
          }
          if (a.pf.scal && lane == 0) a.pf.flag[el] = 1;  // its next map goes into the next generating batch
          const uint4 np = pack(ns);
          if (lane == 0) {
            stage[5 * l] = np.x;
            stage[5 * l + 1] = np.y;
            stage[5 * l + 2] = np.z;
            stage[5 * l + 3] = np.w;
          }
          continue;
        }
        if (a.tobs) {  // (the row's reads first, then the stores: one LDS round trip, not one per 64 values)
          float* t = a.tobs + el * g.D;
          if constexpr (DB) {
            float tv[KD];
#pragma unroll
            for (int j = 0; j < KD; ++j) tv[j] = lane + 64 * j < g.D ? tval(orow, lane + 64 * j) : 0.0f;
#pragma unroll
            for (int j = 0; j < KD; ++j)
              if (lane + 64 * j < g.D) t[lane + 64 * j] = tv[j];
          } else {
            for (int k2 = lane; k2 < g.D; k2 += 64) t[k2] = tval(orow, k2);
          }
        }
        const uint4 sl = make_uint4((uint32_t)__builtin_amdgcn_readfirstlane((int)stage[5 * l]),
                                    (uint32_t)__builtin_amdgcn_readfirstlane((int)stage[5 * l + 1]),
                                    (uint32_t)__builtin_amdgcn_readfirstlane((int)stage[5 * l + 2]),
                                    (uint32_t)__builtin_amdgcn_readfirstlane((int)stage[5 * l + 3]));
        const int kw = __builtin_amdgcn_readfirstlane((int)stage[5 * l + 4]);
        const bool kp = (kw & 1) != 0;
        const Scal sv = unpack(sl);
        // the prefetched record's loads go out first, the terminal info's after them --
        // or both came with round 2 (the kernel's early record of this wave's env)
        const bool eh = KD <= 2 && early != nullptr && el == e_early;
        PfLoad<MAXW, KD> pl;
        if (a.pf.scal && !eh) coop_load_prefetched<MAXW, KD, OT>(a.pf, g, el, pl, lane);
        if (a.tinfo) {
          // (with the info wave the single early env's rows are that wave's, not this one's)
          if (eh && (!kIW || e_info == el))
            coop_info_store<MAXW, kLT>(st, g, *early_rows, sv, a.tinfo + el * PE_NINFO, lane, kw >> 1, ltab);
          else
            coop_write_info<MAXW, kLT>(st, g, el, sv, a.tinfo + el * PE_NINFO, lane, kw >> 1, ltab);
        }
        Row4<MAXW> rw;
        Scal ns;
        asm volatile("" ::: "memory");  // terminal obs read out of the row before the fresh one goes in
        if (a.pf.scal && take(el, sv.episode, eh ? *early : pl, rw, ns, orow)) {
          ns = coop_apply_reset<MAXW, kLT>(st, g, el, ns, kp, rw, lane, ltab, true);
        } else {
          uint64_t* scr = reinterpret_cast<uint64_t*>(lrow) + 162 + wv * coop_scratch_words(g.G, g.WPR);
          ns = coop_reset_env<MAXW, kLT>(st, g, rl, el, sv.episode, kp, rw, lane, scr, ltab);
          coop_fresh_obs<MAXW>(g, rw, ns, orow, tdist, tpos, tvis, st.ldx, st.ldy, lane);
        }
        if (a.pf.scal && lane == 0) a.pf.flag[el] = 1;  // its next map goes into the next generating batch
        const uint4 np = pack(ns);
        if (lane == 0) {
          stage[5 * l] = np.x;
          stage[5 * l + 1] = np.y;
          stage[5 * l + 2] = np.z;
          stage[5 * l + 3] = np.w;
        }
      }
    }
    __syncthreads();  // fresh tile rows and new scalars complete
    if (wv == CW && done) {
      s = unpack(make_uint4(stage[5 * lane], stage[5 * lane + 1], stage[5 * lane + 2], stage[5 * lane + 3]));
      st.ep_ret[e] = 0.0;
      st.scal[e] = pack(s);
    }
    // vmcnt(0) as an instruction the compiler tracks (not asm): nothing of this path
    // is pending where it rejoins the hot path, so the tile store loop after it
    // carries no per-iteration wait (only the commit wave waits here, and it does
    // not take part in the tile store)
    __builtin_amdgcn_s_waitcnt(0x0F70);
    return pack(s);
  }
  // Many done envs (a synchronized batch truncating together): one lane per env.
  // The done env's own obs-tile row is free once its terminal obs is copied out:
  // the new map is generated there when it can hold the grid image (LDS latency
  // for the rejection-sampling scans); the fresh obs row then replaces the image
  // and goes out with the tile (dense_reset_commit)
  // (BT: the tile row holds D bytes, never the image; the fresh obs of that case is
  // built from the env's grid in HBM after the tile store, quad_done_obs)
  const bool scratch_ok = !BT && reset_scratch_bytes(g.G, g.WPR, rl.P) <= 4 * g.D;
  // 8-B aligned start inside the row (rows is 16-B aligned, D is odd)
  uint64_t* sg = reinterpret_cast<uint64_t*>(reinterpret_cast<float*>(rows) + lane * g.D + ((lane * g.D) & 1));
  // LIDAR offsets for the reset-path obs builders, staged in the (now dead) window region
  const signed char* lldx = reinterpret_cast<const signed char*>(lrow);
  const signed char* lldy = lldx + C * R;
  PE_RSTAMP(0);
  PE_RSTAMP_HWID(6);
  load_tables_cold(smem, st.tab);
  for (int k = threadIdx.x; k < C * R; k += blockDim.x) {
    reinterpret_cast<signed char*>(lrow)[k] = st.ldx[k];
    reinterpret_cast<signed char*>(lrow)[C * R + k] = st.ldy[k];
  }
  __syncthreads();
  if constexpr (!BT) {
    // f32 tile: the terminal obs rows go out by the whole block, lanes across a row,
    // before the generator reuses the rows (one lane per env wrote D stores at a
    // D-float lane stride: every store of a wave instruction in a line of its own)
    if (a.tobs) {
      const uint64_t dml = reinterpret_cast<const uint64_t*>(smem)[kDoneMask64];
      uint64_t dm = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)dml) |
                    ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(dml >> 32)) << 32);
      if (dm == ~0ull) {  // every env of a full block: the tile as it is
        store_tile(reinterpret_cast<const float*>(rows), a.tobs + e0 * g.D, kQuadEnvs, g.D, g.D);
      } else {  // done rows only, the k-th to wave k % NW
        const int NWv = blockDim.x >> 6;
        for (int k = 0; dm; ++k) {
          const int l = __ffsll((unsigned long long)dm) - 1;
          dm &= dm - 1;
          if (k % NWv != wv) continue;
          const float* r = reinterpret_cast<const float*>(rows) + l * g.D;
          float* t = a.tobs + (e0 + l) * g.D;
          for (int k2 = lane; k2 < g.D; k2 += 64) t[k2] = r[k2];
        }
      }
      __syncthreads();  // the rows are read out
    }
  }
  bool keep = false;
  if (done) {
    if constexpr (BT) {
      if (a.tobs) {
        float* t = a.tobs + e * g.D;
        for (int k = 0; k < g.D; ++k) t[k] = tval(row, k);
      }
    }
    PE_RSTAMP(1);
    if (a.tinfo) write_info(a.st, a.g, ltab, e, s, a.tinfo + e * PE_NINFO, wfix);
    PE_RSTAMP(2);
    if (!a.autoreset) {
    } else if (scratch_ok) {
      // the map into the env's tile row; grid, visits, scalars and the fresh obs row
      // follow from the commit wave as a whole (dense_reset_commit)
      s = reset_env_image(st, g, rl, ltab, e, s.episode, sg, keep);
    } else {
      s = reset_env(st, g, rl, ltab, e, s.episode);
      if constexpr (!BT) build_obs_fresh(a, st.grid + e * g.gstride, s, row, tdist, tpos, tvis, lldx, lldy);
      st.ep_ret[e] = 0.0;
      st.scal[e] = pack(s);
    }
  }
  if constexpr (!BT) {
    if (a.autoreset && scratch_ok && wv == CW) {
      // the marched rays wait as bytes [C][64] behind the LIDAR offsets in the window region
      uint8_t* rays = reinterpret_cast<uint8_t*>(lrow) + ((2 * C * R + 15) & ~15);
      s = dense_reset_commit(a, ltab, reinterpret_cast<float*>(rows), rays, lldx, lldy, e0, lane, done, keep, s);
    }
  }
  __syncthreads();
  return pack(s);
}

// The lane-per-env path's fresh obs, after the tile store (see quad_done_path): the byte-tile
// kernels' (the f32 kernels write the fresh row into the tile, dense_reset_commit).
template <int NW, bool BT = false>
__device__ __forceinline__ void quad_done_obs(const void* ka, int tile_off, int lane, int64_t e, bool done, uint4 sp) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const StepArgs& a = *reinterpret_cast<const StepArgs*>(ka);
  const Geo& g = a.g;
  float* row = smem + tile_off + lane * g.D;
  // the grid image: the LDS scratch in the env's tile row, or (BT) the env's rows in HBM
  const uint64_t* sg = BT ? a.st.grid + e * g.gstride : reinterpret_cast<const uint64_t*>(row + ((lane * g.D) & 1));
  const signed char* lldx = reinterpret_cast<const signed char*>(smem + kTabFloats);
  PE_RSTAMP(4);
  if (done) {
    if (BT && a.obs_codes)
      build_obs_fresh_codes(a, sg, unpack(sp), a.obs_codes + e * g.D, lldx, lldx + g.C * g.R);
    else
      build_obs_fresh(a, sg, unpack(sp), a.obs + e * g.D, smem, smem + kTabPos, smem + kTabVis, lldx, lldx + g.C * g.R);
  }
  PE_RSTAMP(5);
}
