// pe_reset_kernels.hpp -- the kernels that start episodes outside a step: the wave-per-env and
// lane-per-env reset, the prefetch of the next episodes' records and its compaction, pe_load_maps.
// (a fragment of plantos_batch.hip's anonymous namespace; include after pe_coop.hpp and pe_obs.hpp)
#pragma once

// reset() with one wave per env (pe_coop.hpp): the map, grid/visit rows and the
// fresh obs of env e by the 64 lanes of wave e % 4 of block e / 4 -- 65536 envs
// are 65536 waves, so the whole chip generates maps at once (the lane-per-env
// kernel below gives one env per lane: 29 ms at 64x64, where it scans its grid
// image in HBM).  Unmasked envs rebuild their obs from the current state.
template <int MAXW>
__global__ __launch_bounds__(256) void pe_reset_coop_kernel(StepArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const Geo& g = a.g;
  load_tables(smem, a.st.tab);
  __syncthreads();
  const float* tdist = smem;
  const float* tpos = smem + kTabPos;
  const float* tvis = smem + kTabVis;
  const int lane = threadIdx.x & 63;
  const int64_t e = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (e >= a.n) return;  // wave-uniform
  const Scal s = unpack(a.st.scal[e]);
  const bool resetting = !a.mask || a.mask[e];
  if (resetting) {
    bool keep = false;
    if (a.st.cur && lane == 0) keep = curriculum_on_reset(a.st.cur, e, a.rl);  // A2C_training.py:56-95
    keep = __builtin_amdgcn_readfirstlane((int)keep) != 0;
    Row4<MAXW> rw;
    uint64_t* scr = reinterpret_cast<uint64_t*>(smem + kTabFloats) + (threadIdx.x >> 6) * coop_scratch_words(g.G, g.WPR);
    const Scal ns = coop_reset_env<MAXW>(a.st, g, a.rl, e, s.episode, keep, rw, lane, scr);
    if (lane == 0) {
      a.st.ep_ret[e] = 0.0;
      a.st.scal[e] = pack(ns);
    }
    if (a.obs) coop_fresh_obs<MAXW>(g, rw, ns, a.obs + e * g.D, tdist, tpos, tvis, a.st.ldx, a.st.ldy, lane);
  } else if (a.obs && lane == 0) {
    build_obs_generic(a, e, s.episode, s.x, s.y, a.obs + e * g.D, tdist, tpos, tvis, a.st.ldx, a.st.ldy);
  }
}

// The envs flagged by step kernels since the last prefetch launch, compacted into
// pf.queue (256 envs per workgroup, one atomic per workgroup with a flagged env: one per
// wave was 1024 atomics on one counter), flags cleared.  Runs right before the
// queue-mode prefetch launch, on the same stream.
__global__ __launch_bounds__(256) void pe_pf_compact_kernel(Prefetch pf, int n) {
  const int lane = threadIdx.x & 63;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool f = e < n && pf.flag[e] != 0;
  const uint64_t m = __ballot(f);
  __shared__ uint32_t wc[4], bb;
  const int w = threadIdx.x >> 6;
  if (lane == 0) wc[w] = (uint32_t)__popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t tot = wc[0] + wc[1] + wc[2] + wc[3];
    bb = tot ? atomicAdd(pf.qn, tot) : 0u;
  }
  __syncthreads();
  uint32_t base = bb;
  for (int k = 0; k < w; ++k) base += wc[k];
  if (f) {
    pf.queue[base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = (uint32_t)e;
    pf.flag[e] = 0;
  }
}

// Prefetched resets (pe_coop.hpp Prefetch): generate the next reset's map, grid
// rows and fresh obs of the envs queued by the step kernel (all == 0; grid-stride
// over the queue, then the last workgroup clears the queue), or of every env
// (all != 0: one wave per env; after create / reset()), skipping envs whose
// record already holds the reset of their current episode counter.
template <int MAXW, bool BT = false>  // BT: the records' obs rows as byte codes (a byte-coded step tile)
__global__ __launch_bounds__(256) void pe_prefetch_kernel(StepArgs a, int all) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const Geo& g = a.g;
  const Prefetch& pf = a.pf;
  const uint32_t queued = all ? 0u : (uint32_t)__builtin_amdgcn_readfirstlane((int)pf.qn[0]);
  if (!all && queued == 0u) return;  // nothing queued (the usual launch between synchronized resets)
  load_tables(smem, a.st.tab);
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int64_t wid = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * 4;
  uint64_t* scr = reinterpret_cast<uint64_t*>(smem + kTabFloats) + (threadIdx.x >> 6) * coop_scratch_words(g.G, g.WPR);
  const int64_t cnt = all ? (int64_t)a.n : (int64_t)(queued < (uint32_t)a.n ? queued : (uint32_t)a.n);
  for (int64_t i = wid; i < cnt; i += nwaves) {
    const int64_t e = all ? i : (int64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)pf.queue[i]);
    const uint32_t ep = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.st.scal[e].w);
    if ((uint32_t)__builtin_amdgcn_readfirstlane((int)pf.scal[e].w) == ep + 1u) continue;  // already there
    Row4<MAXW> rw;
    const Scal s = coop_gen_map<MAXW>(g, a.rl, a.st.tab, rw, a.rl.env_off + (uint32_t)e, ep, lane, scr);
    if (lane < g.G) {
      uint64_t* dst = pf.grid + e * g.gstride + (int64_t)lane * g.WPR;
#pragma unroll
      for (int w = 0; w < MAXW; ++w)
        if (MAXW == 1 || w < g.WPR) dst[w] = rw.get(w);
    }
    // the new episode's fresh visit rows into its slot -- the env's idle one (episode
    // ep + 1 vs the running ep): the step that takes this record stores no visit row
    coop_fresh_visits<true>(a.st, g, e, s, lane, reinterpret_cast<const Tables*>(smem));
    if constexpr (BT)
      coop_fresh_obs<MAXW>(g, rw, s, reinterpret_cast<uint8_t*>(pf_obs_row(pf, e)), smem, smem + kTabPos, smem + kTabVis,
                           a.st.ldx, a.st.ldy, lane);
    else
      coop_fresh_obs<MAXW>(g, rw, s, pf_obs_row(pf, e), smem, smem + kTabPos, smem + kTabVis, a.st.ldx, a.st.ldy, lane);
    if (lane == 0) pf.scal[e] = pack(s);  // read by a later launch only
  }
  if (!all) {
    __syncthreads();  // every wave of this workgroup has read the count
    if (threadIdx.x == 0 && atomicAdd(pf.qn + 1, 1u) == gridDim.x - 1) {
      pf.qn[0] = 0u;  // the last workgroup: nobody reads the count any more
      pf.qn[1] = 0u;
    }
  }
}

// reset(): masked device-rng reset, then obs of every env (obs may be NULL).
__global__ __launch_bounds__(kBlock) void pe_reset_kernel(StepArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* tdist = smem;
  float* tpos = smem + kTabPos;
  float* tvis = smem + kTabVis;
  float* rows = smem + kTabFloats;
  const Geo& g = a.g;
  // LIDAR offsets after the tile (read by the obs builders in dependent chains)
  signed char* lldx = reinterpret_cast<signed char*>(rows + kBlock * g.DS);
  signed char* lldy = lldx + g.C * g.R;
  load_tables(smem, a.st.tab);
  for (int k = threadIdx.x; k < g.C * g.R; k += blockDim.x) {
    lldx[k] = a.st.ldx[k];
    lldy[k] = a.st.ldy[k];
  }
  const Tables* ltab = reinterpret_cast<const Tables*>(smem);
  __syncthreads();
  const int64_t e0 = (int64_t)blockIdx.x * kBlock;
  const int64_t e = e0 + threadIdx.x;
  float* row = rows + threadIdx.x * g.DS;
  // a resetting env generates its map in its own tile row (LDS), cf. pe_step_quad
  const bool scratch_ok = reset_scratch_bytes(g.G, g.WPR, a.rl.P) <= 4 * g.DS;
  uint64_t* sg = reinterpret_cast<uint64_t*>(row + ((threadIdx.x * g.DS) & 1));
  bool resetting = false;
  Scal s;
  if (e < a.n) {
    s = unpack(a.st.scal[e]);
    resetting = !a.mask || a.mask[e];
    if (resetting) {
      s = scratch_ok ? reset_env_scratch(a.st, g, a.rl, ltab, e, s.episode, sg)
                     : reset_env(a.st, g, a.rl, ltab, e, s.episode);
      a.st.ep_ret[e] = 0.0;
      a.st.scal[e] = pack(s);
    }
    if (a.obs && resetting && !scratch_ok)
      build_obs_fresh(a, a.st.grid + e * g.gstride, s, row, tdist, tpos, tvis, lldx, lldy);
    else if (a.obs && !resetting)
      build_obs_generic(a, e, s.episode, s.x, s.y, row, tdist, tpos, tvis, lldx, lldy);
  }
  if (!a.obs) return;
  __syncthreads();
  const int64_t valid = a.n - e0 < kBlock ? a.n - e0 : kBlock;
  store_tile(rows, a.obs + e0 * g.D, (int)valid, g.D, g.DS);
  if (scratch_ok) {  // overwrite the scratch rows the tile store wrote
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (resetting) build_obs_fresh(a, sg, s, a.obs + e * g.D, tdist, tpos, tvis, lldx, lldy);
  }
}

// pe_load_maps: host-supplied layouts (CPython-stream reset mode).
__global__ __launch_bounds__(kBlock) void pe_load_maps_kernel(StepArgs a, int k, const int32_t* idx,
                                                              const uint8_t* cells, const int32_t* rover) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* tdist = smem;
  float* tpos = smem + kTabPos;
  float* tvis = smem + kTabVis;
  float* rows = smem + kTabFloats;
  load_tables(smem, a.st.tab);
  const Tables* ltab = reinterpret_cast<const Tables*>(smem);
  __syncthreads();
  const int j = blockIdx.x * kBlock + threadIdx.x;
  if (j >= k) return;
  const Geo& g = a.g;
  const int64_t e = idx[j];
  const uint8_t* c = cells + (int64_t)j * g.GG;
  const bool keep = a.st.cur ? curriculum_on_reset(a.st.cur, e, a.rl) : false;  // A2C_training.py:56-95
  int n_obst = 0;
  for (int row = 0; row < g.G; ++row) {
    for (int w = 0; w < g.WPR; ++w) a.st.grid[e * g.gstride + (int64_t)row * g.WPR + w] = ltab->grid_pad[w];
    for (int col = 0; col < g.G; ++col) {
      int code = c[row * g.G + col] & 3;
      n_obst += code == OBST;
      if (code) grid_set(a.st, g, e, row, col + g.R, code);
    }
  }
  Scal s = unpack(a.st.scal[e]);
  s.x = rover[2 * j];
  s.y = rover[2 * j + 1];
  s.step = 0;
  s.coll = 0;
  s.flags = 0;
  s.episode += 1u;
  s.total = g.GG - n_obst;
  s.expl = 1;
  new_episode_visits(a.st, g, ltab, e, s, keep);  // plantos_env.py:146-147, 236
  a.st.scal[e] = pack(s);
  a.st.ep_ret[e] = 0.0;
  float* row = rows + threadIdx.x * g.DS;
  // reset() obs of the fresh episode (a carried CurriculumWrapper visit map is
  // installed after env.reset() returned, A2C_training.py:90-91: not in this obs)
  build_obs_fresh(a, a.st.grid + e * g.gstride, s, row, tdist, tpos, tvis, a.st.ldx, a.st.ldy);
  if (a.obs)
    for (int q = 0; q < g.D; ++q) a.obs[(int64_t)j * g.D + q] = row[q];
}
