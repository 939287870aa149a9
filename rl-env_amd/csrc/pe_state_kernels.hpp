// pe_state_kernels.hpp -- the small kernels behind the state API: info, get / set state, zeroed
// episode counters, the deferred visit-count flush, curriculum init, synthetic actions.
// (a fragment of plantos_batch.hip's anonymous namespace; include after pe_step_args.hpp)
#pragma once

// _get_info (plantos_env.py:317-336), integer columns.
__global__ void pe_info_kernel(StepArgs a, int32_t* info) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= a.n) return;
  const Geo& g = a.g;
  static_assert(PE_NINFO == 11 && PE_I_POISONED == 10, "write_info column layout");
  write_info(a.st, g, a.st.tab, e, unpack(a.st.scal[e]), info + e * PE_NINFO);
}

// get_state: one thread per (env, cell).
__global__ void pe_get_cells_kernel(StepArgs a, uint8_t* cells, int32_t* visits, int8_t* explored) {
  const Geo& g = a.g;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)a.n * g.GG) return;
  const int64_t e = t / g.GG;
  const int c = (int)(t - e * g.GG);
  const int row = c / g.G, col = c - row * g.G;
  if (cells) cells[t] = (uint8_t)grid_code(a.st, g, e, row, col + g.R);
  const Scal s = unpack(a.st.scal[e]);
  if (visits) visits[t] = visit_exact(a.st, g, e, s.episode, row, col);
  if (explored) {
    int8_t v;
    if (s.flags & F_EXPL_BITMAP) {
      uint32_t w = a.st.expl[e * g.estride + (c >> 5)];
      v = (w >> (c & 31)) & 1u ? 1 : 0;
    } else {
      v = nibble_get(a.st, g, e, s.episode, row, col) ? 1 : 0;  // explored_map > 0 <=> visit > 0
    }
    if (v && s.x == row && s.y == col) v = 2;  // plantos_env.py:200, 236
    explored[t] = v;
  }
}

__global__ void pe_get_scal_kernel(StepArgs a, int32_t* scal) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= a.n) return;
  Scal s = unpack(a.st.scal[e]);
  int32_t* o = scal + e * PE_NSCAL;
  o[PE_S_X] = s.x;
  o[PE_S_Y] = s.y;
  o[PE_S_STEP] = s.step;
  o[PE_S_COLL] = s.coll;
  o[PE_S_COLLIDED] = (s.flags & F_COLLIDED) ? 1 : 0;
  o[PE_S_BONUS] = (s.flags & F_BONUS) ? 1 : 0;
  o[PE_S_POISONED] = (int)((s.flags >> 2) & 7u);
  o[PE_S_EPISODE] = (int32_t)s.episode;
}

// set_state: one thread per env, in this order: (1) if explored stays derived but
// visits change, freeze the current explored map into the bitmap; (2) cells,
// (3) visits, (4) explored, (5) scalars; (6) derived counters and the explored
// mode: derived (bitmap not read) iff explored_map > 0 <=> visit > 0 everywhere.
__global__ void pe_set_env_kernel(StepArgs a, const uint8_t* cells, const int32_t* visits, const int8_t* explored,
                                  const int32_t* scal) {
  const Geo& g = a.g;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= a.n) return;
  Scal s = unpack(a.st.scal[e]);
  // the visit rows live in the slot of the episode counter (pe_device.hpp vis_env): the
  // new counter's, when the scalars are set too
  const uint32_t ep0 = s.episode, ep1 = scal ? (uint32_t)scal[e * PE_NSCAL + PE_S_EPISODE] : ep0;
  uint32_t* eb = a.st.expl + e * g.estride;
  if (!(s.flags & F_EXPL_BITMAP) && visits && !explored) {
    for (int w = 0; w < g.estride; ++w) eb[w] = 0u;
    for (int c = 0; c < g.GG; ++c)
      if (nibble_get(a.st, g, e, ep0, c / g.G, c % g.G)) eb[c >> 5] |= 1u << (c & 31);
    s.flags |= F_EXPL_BITMAP;
  }
  if (cells) {
    for (int row = 0; row < g.G; ++row) {
      for (int w = 0; w < g.WPR; ++w) a.st.grid[e * g.gstride + (int64_t)row * g.WPR + w] = a.st.tab->grid_pad[w];
      for (int col = 0; col < g.G; ++col) {
        int code = cells[e * g.GG + row * g.G + col] & 3;
        if (code) grid_set(a.st, g, e, row, col + g.R, code);
      }
    }
  }
  if (visits) {
    uint32_t* vb = vis_env(a.st, g, e, ep1);
    for (int row = 0; row < g.G; ++row) {
      for (int w = 0; w < g.NW; ++w) vb[(int64_t)row * g.NW + w] = a.st.tab->vis_pad[w];
      for (int col = 0; col < g.G; ++col) {
        int32_t v = visits[e * g.GG + row * g.G + col];
        uint32_t vc = v <= 0 ? 0u : (uint32_t)v;
        a.st.vx[e * g.hstride + row * g.G + col] = vc;
        vis_set(a.st, g, e, ep1, row, col, vc < 15u ? vc : 15u);
      }
    }
  } else if ((ep0 ^ ep1) & 1u) {
    carry_visits(a.st, g, e, ep1);  // the counts move with the counter's parity
  }
  if (explored) {
    for (int w = 0; w < g.estride; ++w) {
      uint32_t bits = 0;
      for (int b = 0; b < 32; ++b) {
        int c = w * 32 + b;
        if (c < g.GG && explored[e * g.GG + c] > 0) bits |= 1u << b;
      }
      eb[w] = bits;
    }
    s.flags |= F_EXPL_BITMAP;
  }
  // the prefetched record stays valid only if the counter stays (its key, ep0 + 1, is
  // still the next episode's, and its fresh rows in slot (ep0 + 1) & 1 untouched): a
  // counter moved back would turn an old key into a future one over rows since reused
  if (a.pf.scal && ep1 != ep0) a.pf.scal[e].w = 0u;
  if (scal) {
    const int32_t* i = scal + e * PE_NSCAL;
    s.x = i[PE_S_X];
    s.y = i[PE_S_Y];
    s.step = i[PE_S_STEP] < 0 ? 0 : (i[PE_S_STEP] > 65535 ? 65535 : i[PE_S_STEP]);
    s.coll = i[PE_S_COLL] < 0 ? 0 : (i[PE_S_COLL] > 65535 ? 65535 : i[PE_S_COLL]);
    s.flags = (s.flags & F_EXPL_BITMAP) | (i[PE_S_COLLIDED] ? F_COLLIDED : 0u) | (i[PE_S_BONUS] ? F_BONUS : 0u) |
              ((uint32_t)(i[PE_S_POISONED] & 7) << 2);
    s.episode = (uint32_t)i[PE_S_EPISODE];
  }
  int ex = 0, ob = 0;
  if (s.flags & F_EXPL_BITMAP) {
    bool same = true;
    for (int c = 0; c < g.GG; ++c) {
      const bool bit = (eb[c >> 5] >> (c & 31)) & 1u;
      ex += bit;
      same = same && (bit == (nibble_get(a.st, g, e, ep1, c / g.G, c % g.G) != 0u));
    }
    if (same) s.flags &= ~F_EXPL_BITMAP;
  } else {
    for (int c = 0; c < g.GG; ++c) ex += nibble_get(a.st, g, e, ep1, c / g.G, c % g.G) != 0u;
  }
  for (int row = 0; row < g.G; ++row)
    for (int w = 0; w < g.WPR; ++w) {
      uint64_t v = a.st.grid[e * g.gstride + (int64_t)row * g.WPR + w];
      ob += __popcll(v & ~(v >> 1) & a.st.tab->grid_real[w] & kEven64);
    }
  s.expl = ex;
  s.total = g.GG - ob;
  a.st.scal[e] = pack(s);
}

// pe_seed(reset_episode_counters): episode := 0, an odd episode's visit rows copied
// to slot 0.  A prefetched record keyed k promises fresh rows of episode k in slot
// k & 1; with the counter moved back, an old key becomes a future one (an env at
// episode 1 holds the record of episode 2, whose slot-0 rows the copy just
// overwrote, and the counter reaches 1 again), so every record is dropped except
// episode 1's of an env still at episode 0 (slot 1 untouched since the prefetch).
__global__ void pe_zero_episodes_kernel(StepArgs a) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= a.n) return;
  uint4 w = a.st.scal[e];
  if (w.w & 1u) {
    const uint32_t* src = vis_env(a.st, a.g, e, 1u);
    uint32_t* dst = vis_env(a.st, a.g, e, 0u);
    for (int64_t k = 0; k < a.g.vslot; ++k) dst[k] = src[k];
  }
  if (a.pf.scal && w.w != 0u) a.pf.scal[e].w = 0u;
  w.w = 0u;
  a.st.scal[e] = w;
}

// The deferred overflow writes (pe_device.hpp vx_pending) of every env applied and
// cleared: before any API call that reads the exact visit counts or replaces them.
__global__ void pe_vx_flush_kernel(StepArgs a) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= a.n) return;
  const uint32_t p = a.st.vpend[e];
  if (p) {
    vx_apply(a.st, a.g, e, p);
    a.st.vpend[e] = 0u;
  }
}

// CurriculumWrapper.__init__ state of every env (A2C_training.py:41-54).
__global__ void pe_cur_init_kernel(CurRec* cur, int n, double thr) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  CurRec c;
  c.thr = thr;
  c.episodes = c.successes = c.on_maze = c.flags = 0u;
  c.pad[0] = c.pad[1] = 0u;
  cur[e] = c;
}

__global__ void pe_synth_kernel(int n, uint64_t seed, uint32_t env_off, uint32_t t, int32_t* actions) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  uint4 o = philox(make_uint4(t, env_off + (uint32_t)e, 0u, kDomainAction), (uint32_t)seed, (uint32_t)(seed >> 32));
  actions[e] = (int32_t)(o.x % 5u);
}
