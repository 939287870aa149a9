// pe_obs.hpp -- the lane-per-env obs builders (_get_lidar_obs from the env's state, from a fresh
// grid image as floats and as byte codes) and the loaders of the Tables image into LDS.
// (a fragment of plantos_batch.hip's anonymous namespace; include after pe_step_args.hpp)
#pragma once

// ------------------------------------------------------------------ obs builders
// _get_lidar_obs, plantos_env.py:251-315, into one LDS row.
// The three builders below repeat the ray march on purpose: folded into one template over a cell
// reader, 23 of the unit's 45 device symbols compile differently ("Next").

// Generic: runtime (G, C, R), LIDAR offsets from the handle's table.
__device__ __forceinline__ void build_obs_generic(const StepArgs& a, int64_t e, uint32_t ep, int x, int y, float* row,
                                                  const float* tdist, const float* tpos, const float* tvis,
                                                  const signed char* ldx, const signed char* ldy) {
  const Geo& g = a.g;
  const int R = g.R, C = g.C;
  for (int i = 0; i < C; ++i) {
    int dist = R, ent = EMPTY;
    for (int r = 1; r <= R; ++r) {
      int cx = x + ldx[i * R + r - 1];
      int cy = y + ldy[i * R + r - 1];
      int code = (cx >= 0 && cx < g.G) ? grid_code(a.st, g, e, cx, cy + R) : OBST;  // :271-284
      if (code != EMPTY) {
        dist = r;
        ent = code;
        break;
      }
    }
    row[5 * i] = tdist[dist];
    row[5 * i + 1] = ent == 0 ? 1.0f : 0.0f;
    row[5 * i + 2] = ent == 1 ? 1.0f : 0.0f;
    row[5 * i + 3] = ent == 2 ? 1.0f : 0.0f;
    row[5 * i + 4] = ent == 3 ? 1.0f : 0.0f;
  }
  row[5 * C] = tpos[x];
  row[5 * C + 1] = tpos[y];
  for (int lx = 0; lx < 5; ++lx) {
    int xr = x + lx - 2;
    uint32_t win = (xr >= 0 && xr < g.G) ? vis_window(a.st, g, e, ep, xr, y) : 0xAAAAAu;
    for (int ly = 0; ly < 5; ++ly) row[5 * C + 2 + 5 * lx + ly] = tvis[(win >> (4 * ly)) & 15u];
  }
}

// obs of a freshly reset env (all visits 0 but the rover's 1) from its grid image
// sg, written to `out` (HBM).  Same values as build_obs_generic on that state.
__device__ inline void build_obs_fresh(const StepArgs& a, const uint64_t* sg, const Scal& s, float* out,
                                       const float* tdist, const float* tpos, const float* tvis,
                                       const signed char* ldx, const signed char* ldy) {
  const Geo& g = a.g;
  const int R = g.R, C = g.C, x = s.x, y = s.y;
  for (int i = 0; i < C; ++i) {
    int dist = R, ent = EMPTY;
    for (int r = 1; r <= R; ++r) {
      const int cx = x + ldx[i * R + r - 1];
      const int cy = y + ldy[i * R + r - 1];
      const int code = (cx >= 0 && cx < g.G) ? img_code(sg, g, cx, cy + R) : OBST;  // :271-284
      if (code != EMPTY) {
        dist = r;
        ent = code;
        break;
      }
    }
    out[5 * i] = tdist[dist];
    out[5 * i + 1] = ent == 0 ? 1.0f : 0.0f;
    out[5 * i + 2] = ent == 1 ? 1.0f : 0.0f;
    out[5 * i + 3] = ent == 2 ? 1.0f : 0.0f;
    out[5 * i + 4] = ent == 3 ? 1.0f : 0.0f;
  }
  out[5 * C] = tpos[x];
  out[5 * C + 1] = tpos[y];
  for (int lx = 0; lx < 5; ++lx)
    for (int ly = 0; ly < 5; ++ly) {
      const int gx = x + lx - 2, gy = y + ly - 2;
      const bool in = gx >= 0 && gx < g.G && gy >= 0 && gy < g.G;       // :307-311
      const bool rover = lx == 2 && ly == 2 && !(s.flags & F_NOROOM);
      out[5 * C + 2 + 5 * lx + ly] = !in ? tvis[10] : (rover ? tvis[1] : tvis[0]);
    }
}

// The same obs as byte codes (pe_coop.hpp ObsW<uint8_t>: dist r -> r, one-hot 0 / 1 ->
// 0 / R+1, vis v -> kCodeVis + v, pos x -> kCodePos + x).
__device__ inline void build_obs_fresh_codes(const StepArgs& a, const uint64_t* sg, const Scal& s, uint8_t* out,
                                             const signed char* ldx, const signed char* ldy) {
  const Geo& g = a.g;
  const int R = g.R, C = g.C, x = s.x, y = s.y;
  for (int i = 0; i < C; ++i) {
    int dist = R, ent = EMPTY;
    for (int r = 1; r <= R; ++r) {
      const int cx = x + ldx[i * R + r - 1];
      const int cy = y + ldy[i * R + r - 1];
      const int code = (cx >= 0 && cx < g.G) ? img_code(sg, g, cx, cy + R) : OBST;  // :271-284
      if (code != EMPTY) {
        dist = r;
        ent = code;
        break;
      }
    }
    out[5 * i] = (uint8_t)dist;
    for (int k = 0; k < 4; ++k) out[5 * i + 1 + k] = (uint8_t)(ent == k ? R + 1 : 0);
  }
  out[5 * C] = (uint8_t)(kCodePos + x);
  out[5 * C + 1] = (uint8_t)(kCodePos + y);
  for (int lx = 0; lx < 5; ++lx)
    for (int ly = 0; ly < 5; ++ly) {
      const int gx = x + lx - 2, gy = y + ly - 2;
      const bool in = gx >= 0 && gx < g.G && gy >= 0 && gy < g.G;       // :307-311
      const bool rover = lx == 2 && ly == 2 && !(s.flags & F_NOROOM);
      out[5 * C + 2 + 5 * lx + ly] = (uint8_t)(kCodeVis + (!in ? 10 : (rover ? 1 : 0)));
    }
}


__device__ __forceinline__ void load_tables(float* smem, const Tables* tab) {
  const float* src = reinterpret_cast<const float*>(tab);
  for (int k = threadIdx.x; k < kTabFloats; k += blockDim.x) smem[k] = src[k];
}

// The tables the step reads: dist[0..R], pos[0..G), vis[0..16) (hot path) and the
// pad masks (floats kTabPads.., reset paths: read from LDS there, never from global
// memory under the obs stores' traffic).
__device__ __forceinline__ void load_tables_hot(float* smem, const Tables* tab, int G, int R) {
  const float* src = reinterpret_cast<const float*>(tab);
  constexpr int NV = kTabPads - kTabVis;  // vis[] whole
  const int n = (R + 1) + G + NV + (kTabFloats - kTabPads);
  for (int k = threadIdx.x; k < n; k += blockDim.x) {
    const int f = k <= R ? kTabDist + k
                         : (k < R + 1 + G ? kTabPos + (k - R - 1)
                                          : (k < R + 1 + G + NV ? kTabVis + (k - R - 1 - G)
                                                                : kTabPads + (k - R - 1 - G - NV)));
    smem[f] = src[f];
  }
}

// The rest (pad masks, read by map generation / info): loaded on the rare reset path.
__device__ __forceinline__ void load_tables_cold(float* smem, const Tables* tab) {
  const float* src = reinterpret_cast<const float*>(tab);
  for (int k = kTabPads + (int)threadIdx.x; k < kTabFloats; k += blockDim.x) smem[k] = src[k];
}
