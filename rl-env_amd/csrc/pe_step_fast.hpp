// pe_step_fast.hpp -- pe_step_fast<C, R, ONEWORD>: the lane-per-env fused step with compile-time
// C and R (pe_fast.hpp holds its register window).
// (a fragment of plantos_batch.hip's anonymous namespace; include after pe_fast.hpp, pe_obs.hpp
// and pe_tile.hpp)
#pragma once

// ------------------------------------------------------------------ kernels
// Specialized fused step (compile-time C, R): two load rounds per lane, the rest
// from registers (pe_fast.hpp).  Same semantics as pe_step_wave.
template <int C, int R, bool ONEWORD>
__global__ __launch_bounds__(kBlock) void pe_step_fast(StepArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* tpos = smem + kTabPos;
  float* tvis = smem + kTabVis;
  float* rows = smem + kTabFloats;
  const Geo& g = a.g;
  const Rules& rl = a.rl;
  const State& st = a.st;
  const int64_t e0 = (int64_t)blockIdx.x * kBlock;
  const int64_t e = e0 + threadIdx.x;
  const bool live = e < a.n;
  float* row = rows + threadIdx.x * g.DS;
  // ---- round 1: env-indexed loads
  uint4 sw = make_uint4(0u, 0u, 0u, 0u);
  int64_t action = 0;
  double ret = 0.0;
  if (live) {
    sw = st.scal[e];
    action = a.act_bytes == 8 ? reinterpret_cast<const int64_t*>(a.actions)[e]
                              : (int64_t)reinterpret_cast<const int32_t*>(a.actions)[e];
    ret = st.ep_ret[e];
  }
  load_tables(smem, st.tab);
  const Tables* ltab = reinterpret_cast<const Tables*>(smem);
  __syncthreads();
  if (live) {
    Scal s = unpack(sw);
    s.step = s.step < 65535 ? s.step + 1 : 65535;                  // plantos_env.py:162
    bool mv = false, water = false;
    int dxm = 0, dym = 0;
    if (action < 4) {                                              // :166
      const int64_t ai = action < 0 ? action + 4 : action;         // Python negative index
      if (ai < 0) {
        s.flags |= F_POISON_ACT;                                   // reference IndexError
        atomicOr(st.err_bits, F_POISON_ACT);
      } else {
        mv = true;                                                 // :186 N,E,S,W
        dxm = ai == 0 ? -1 : (ai == 2 ? 1 : 0);
        dym = ai == 1 ? 1 : (ai == 3 ? -1 : 0);
      }
    } else {
      water = true;
    }
    const int nx = s.x + dxm, ny = s.y + dym;
    const bool inb = mv && nx >= 0 && nx < g.G && ny >= 0 && ny < g.G;
    // ---- round 2: position-indexed loads
    Window<R, ONEWORD> w;
    w.load(st, g, e, s.episode, s.x, s.y);
    const int cell_o = s.x * g.G + s.y, cell_n = nx * g.G + ny;
    uint32_t* ep_o = st.expl + e * g.estride + (cell_o >> 5);
    uint32_t* ep_n = st.expl + e * g.estride + ((inb ? cell_n : cell_o) >> 5);
    const bool bitmap = (s.flags & F_EXPL_BITMAP) != 0u;
    uint32_t eo = 0u, en = 0u;
    if (inb) {
      if (bitmap) {
        eo = *ep_o;
        en = *ep_n;
      }
    }
    double h = 0.0;
    int dxv = 0;
    if (mv) {
      const bool ok = inb && w.code(dxm, ny) != OBST;              // :193-195
      if (ok) {
        const uint32_t n = (sel3<uint32_t>(dxm, w.vis32(2), w.vis32(3), w.vis32(4)) >> (4 * (ny + 2 - w.ybv))) & 15u;
        const bool never = n == 0u;                                // :197
        const uint32_t nib = n < 15u ? n + 1u : 15u;               // :203
        visit_bump_exact(st, g, e, cell_n, n);
        const int pb = 4 * (ny + 2) - 32 * ((4 * w.ybv) >> 5);
        uint32_t* vrow = vis_env(st, g, e, s.episode) + (int64_t)nx * g.NW + ((4 * w.ybv) >> 5);
#pragma unroll
        for (int k = 2; k <= 4; ++k) {
          if (k == 3 + dxm) {
            if (pb < 32) {
              w.vlo[k] = (w.vlo[k] & ~(0xFu << pb)) | (nib << pb);
              vrow[0] = w.vlo[k];
            } else {
              w.vhi[k] = (w.vhi[k] & ~(0xFu << (pb - 32))) | (nib << (pb - 32));
              vrow[1] = w.vhi[k];
            }
          }
        }
        if (bitmap) {
          const uint32_t bo = 1u << (cell_o & 31), bn = 1u << (cell_n & 31);
          if ((cell_o >> 5) == (cell_n >> 5)) {                    // explored[old]=1, [new]=2 (:198-200)
            uint32_t wv = eo;
            if (!(wv & bo)) { wv |= bo; s.expl++; }
            if (!(wv & bn)) { wv |= bn; s.expl++; }
            if (wv != eo) *ep_o = wv;
          } else {
            if (!(eo & bo)) { *ep_o = eo | bo; s.expl++; }
            if (!(en & bn)) { *ep_n = en | bn; s.expl++; }
          }
        } else if (never) {
          s.expl++;                                                // derived explored mode
        }
        s.x = nx;                                                  // :199
        s.y = ny;
        dxv = dxm;
        h = never ? rl.r_exploration : rl.r_revisit;               // :204-207
      } else {
        s.flags |= F_COLLIDED;                                     // :209
        s.coll = s.coll < 65535 ? s.coll + 1 : 65535;              // :210
        h = rl.r_invalid;                                          // :211
      }
    } else if (water) {
      const int cd = w.code(0, s.y);
      if (cd == THIRSTY) {                                         // fork plantos_env_new.py:237-240
        const int pb = 2 * (s.y + R) - 64 * ((2 * w.yb) >> 6);
        uint64_t* grow = st.grid + e * g.gstride + (int64_t)s.x * g.WPR + ((2 * w.yb) >> 6);
        if (pb < 64) {
          w.clo &= ~(1ull << pb);                                  // code 3 -> 2: clear the low bit
          grow[0] = w.clo;
        } else {
          w.chi &= ~(1ull << (pb - 64));
          grow[1] = w.chi;
        }
        w.refresh_centre();
        h = rl.r_goal;
      } else if (cd == HYD) {                                      // fork :241-242 (root raises)
        h = rl.r_mistake;
        if (!(s.flags & F_POISON_HYD)) atomicOr(st.err_bits, F_POISON_HYD);
        s.flags |= F_POISON_HYD;
      } else {
        h = rl.r_water_empty;                                      // :221-222
      }
    }
    double rew = rl.r_step;                                        // :164
    rew += h;
    bool term = s.expl >= s.total;                                 // :176, 244-246, 331
    const bool trunc = s.step >= rl.max_steps;                     // :177
    if (term && !(s.flags & F_BONUS)) {                            // :179-181
      rew += rl.r_complete;
      s.flags |= F_BONUS;
    }
    ret += rew;
    if (st.cur) term = curriculum_hit(st.cur, e, st.cur[e].thr, s.expl, s.total, rl.cur_term) || term;
    a.reward[e] = (float)rew;
    a.term[e] = term;
    a.trunc[e] = trunc;
    if (term || trunc) {                                           // ended: terminal outputs
      if (a.tobs) {
        obs_from_window<C, R, ONEWORD>(w, g.G, dxv, s.x, s.y, row, tpos, tvis);
        float* t = a.tobs + e * g.D;
        for (int k = 0; k < g.D; ++k) t[k] = row[k];
      }
      if (a.ep_ret_out) a.ep_ret_out[e] = ret;
      if (a.ep_len_out) a.ep_len_out[e] = s.step;
      if (a.tinfo) write_info(a.st, a.g, ltab, e, s, a.tinfo + e * PE_NINFO);
    }
    if ((term || trunc) && a.autoreset) {                          // DummyVecEnv auto-reset
      s = reset_env(st, g, rl, ltab, e, s.episode);
      st.ep_ret[e] = 0.0;
      st.scal[e] = pack(s);
      build_obs_fresh(a, st.grid + e * g.gstride, s, row, smem, tpos, tvis, a.st.ldx, a.st.ldy);  // rare path
    } else {
      st.ep_ret[e] = ret;
      st.scal[e] = pack(s);
      obs_from_window<C, R, ONEWORD>(w, g.G, dxv, s.x, s.y, row, tpos, tvis);
    }
  }
  __syncthreads();
  const int64_t valid = a.n - e0 < kBlock ? a.n - e0 : kBlock;
  store_tile(rows, a.obs + e0 * g.D, (int)valid, g.D, g.DS);
}
