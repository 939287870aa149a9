// pe_plan.hpp -- the device-free half of handle creation (a part of plantos_batch.hip, included
// after the kernels' headers: it reads their limits and LDS layouts).
//
// make_plan() decides everything pe_create decides before its first allocation -- geometry,
// rules, the step kernel, its workgroup shape, the reset paths, the ray-table format and the
// carve of both device allocations -- as a pure function of (pe_config, n_envs, CU count, Knobs).
// It makes no HIP call, so kernel selection can be examined without a GPU (pe_internal_plan,
// tests/test_plan_host.py).  The host tables that pe_create uploads are built here too, by
// functions that return their bytes.
//
// The step kernel is a StepKernel (pe_handle.hpp): family, compile-time (C, R) or runtime,
// one-word, byte tile, envs per workgroup, waves.  A new kernel is one row of PE_QUAD_KERNELS
// (or a family) and one rung of the ladder in make_plan().
#pragma once

#include <optional>

namespace {

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

constexpr size_t kLdsMax = 160 * 1024;  // LDS per workgroup (gfx950)

// ---------------------------------------------------------------------- LDS sizes
// the lane-per-env kernels' dynamic LDS (pe_reset_kernel, pe_load_maps_kernel, pe_step_fast)
size_t lds_bytes(const Geo& g) {
  return sizeof(float) * (size_t)(kTabFloats + kBlock * g.DS) + align_up(2 * (size_t)g.C * g.R, 16);
}

// the cooperative reset's and the prefetch kernel's (pe_reset_coop_kernel, pe_prefetch_kernel)
size_t coop_lds_bytes(const Geo& g) {
  return sizeof(float) * (size_t)kTabFloats + 4 * 8 * (size_t)coop_scratch_words(g.G, g.WPR);
}

// pe_step_wave<., ALN>: the rover-aligned window where it fits (its LDS header, its ray table)
bool wave_aligned(const Geo& g) { return wave_aln_ok(g.G, g.R, g.WPR); }

// pe_step_wave's: its header + 8 per-wave regions
size_t wave_lds_bytes(const Geo& g) {
  return sizeof(float) * ((size_t)wave_hdr_floats(g.C, g.R, wave_aligned(g)) +
                          kWaveEnvs * (size_t)wave_lds_floats(g.G, g.R, g.WPR, g.NW, g.D));
}

// the prefetched records' obs row stride (bytes; pe_device.hpp Prefetch)
size_t pf_ostride(const Geo& g, bool codes) { return align_up((size_t)(codes ? g.D : 4 * g.D), 16); }

size_t quad_lds_bytes(const Geo& g, bool codes, bool rt) {
  const size_t off = (size_t)((kTabFloats + (2 * g.R + 3) * kQuadEnvs * 2 + 7 * kQuadEnvs + 3) & ~3) +
                     (rt ? (size_t)quad_rtab_floats(g.C, g.R) : 0);  // (+ the runtime kernel's probe table)
  // + the single-done record's LDS-DMA staging region (pe_coop.hpp pf_stage_issue)
  size_t stage = (size_t)pf_stage_bytes(g.G, g.WPR, (int)pf_ostride(g, codes));
  // (f32 kernels: slack left from a removed staging path; shrinking it moves occupancy -- a measured change)
  const int ng = pf_grid_units(g.G, g.WPR), no = (int)pf_ostride(g, codes) / 16;
  if (!codes && 1 + ng + no <= 64) stage = std::max(stage, (size_t)((1 + 2 * ng + no + 63) / 64) * 1024);
  // (byte-coded kernels that stage by LDS-DMA: the record, then the info wave's rows)
  if (codes && (rt || g.C >= kBtStageMinC) && ng <= 128)
    stage = std::max(stage, (size_t)((1 + 2 * ng + no + 63) / 64) * 1024);
  if (codes)  // byte tile + code table (quad_ctab_off)
    return sizeof(float) * (off + (size_t)((kQuadEnvs * g.D + 15) / 16) * 4 + 256) + stage;
  return sizeof(float) * (off + (size_t)kQuadEnvs * g.D) + stage;
}

// ---------------------------------------------------------------------- the step kernels
// Every pe_step_quad instantiation the library holds: X(C, R, ONEWORD, NW, BT, EPB).  launch_step
// launches the row that equals the handle's StepKernel; make_plan() refuses a choice with no row.
// The quadrant kernels (4 waves x 64 envs per workgroup) are the default for the specialized
// geometries (compile-time C, R: the LIDAR offsets of lidar_tables.inc); 0, 0: the runtime table.
// (Rows may stand in any order.  This one is the order of the switch the list replaced: the
// compiler emits the kernels in it, and with it the device assembly stayed identical down to the
// label numbers, profiles/isa_equiv_plan_split.txt.)
#define PE_QUAD_KERNELS(X)                                                                \
  /* the headline geometry, one-word (G <= 20): its workgroup shapes, its byte tile */    \
  X(16, 6, true, 8, false, 16) X(16, 6, true, 4, false, 16) X(16, 6, true, 4, false, 32)  \
  X(16, 6, true, 4, true, 64) X(16, 6, true, 4, false, 64)                                \
  X(16, 6, false, 4, false, 64) X(64, 6, false, 4, true, 64)                              \
  /* plantos_env.py:25-26 constructor default (C=10, R=2; G=21: multi-word) */            \
  X(10, 2, true, 4, false, 64) X(10, 2, false, 4, false, 64)                              \
  /* test_environment.py:24 (G=15, C=16, R=4): one-word; multi-word in the last row */    \
  X(16, 4, true, 4, false, 64)                                                            \
  /* runtime (C, R): every other geometry with C <= 64, 2 <= R <= 14 */                   \
  X(0, 0, true, 4, true, 64) X(0, 0, true, 4, false, 64) X(0, 0, false, 4, true, 64)      \
  X(0, 0, false, 4, false, 64)                                                            \
  X(16, 4, false, 4, false, 64)

bool is_kernel(const StepKernel& k, StepFamily f, int C, int R) { return k.family == f && k.C == C && k.R == R; }
bool is_quad(const StepKernel& k) { return k.family == StepFamily::quad; }
bool is_far(const StepKernel& k) { return k.family == StepFamily::far; }
bool is_rt(const StepKernel& k) { return is_kernel(k, StepFamily::quad, 0, 0); }  // rays from the runtime table
// the headline geometry's sector kernel: the only one with workgroup shapes and an optional byte tile
bool is_headline(const StepKernel& k) { return is_kernel(k, StepFamily::quad, 16, 6) && k.oneword; }

bool quad_kernel_exists(const StepKernel& k) {
#define PE_ROW(KC, KR, OW, NW, BT, EPB) \
  if (k.C == KC && k.R == KR && k.oneword == OW && k.waves == NW && k.bytetile == BT && k.epb == EPB) return true;
  PE_QUAD_KERNELS(PE_ROW)
#undef PE_ROW
  return false;
}

StepKernel wave_kernel() { return {StepFamily::wave, 0, 0, false, false, kWaveEnvs, kWaveEnvs}; }
StepKernel fast_kernel(int C, int R, bool oneword) { return {StepFamily::fast, C, R, oneword, false, kBlock, kBlock / 64}; }
// (4 waves: measured best at C=16 and C=64, profiles/r1c-r1e; 8: the 16-env shape of small batches)
StepKernel quad_kernel(int C, int R, bool oneword) { return {StepFamily::quad, C, R, oneword, false, kQuadEnvs, 4}; }
StepKernel far_kernel(int C, int R) { return {StepFamily::far, C, R, false, true, kQuadEnvs, kFarWaves}; }

// pe_kernel_variant()'s numbers: an identifier per (family, table, one-word), not an order --
// nothing may compute with them
int kernel_variant(const StepKernel& k) {
  switch (k.family) {
    case StepFamily::wave: return 0;
    case StepFamily::fast: return k.C == 64 ? 3 : (k.oneword ? 1 : 2);
    case StepFamily::far: return 13;  // pe_step_far<64, 32>: SURVEY §8(d)'s R = 32 stress variant
    case StepFamily::quad: break;
  }
  if (is_kernel(k, StepFamily::quad, 16, 6)) return k.oneword ? 4 : 5;
  if (is_kernel(k, StepFamily::quad, 64, 6)) return 6;
  if (is_kernel(k, StepFamily::quad, 10, 2)) return k.oneword ? 7 : 8;
  if (is_kernel(k, StepFamily::quad, 16, 4)) return k.oneword ? 9 : 10;
  return k.oneword ? 11 : 12;  // runtime (C, R)
}

// pe_kernel_name()'s text
void kernel_name(const StepKernel& k, char (&out)[64]) {
  if (k.family == StepFamily::wave) {
    std::snprintf(out, sizeof(out), "pe_step_wave");
    return;
  }
  char rays[32] = "runtime C,R";
  if (k.C) std::snprintf(rays, sizeof(rays), "C%d,R%d", k.C, k.R);
  char shape[32] = "";  // the workgroup shape of small batches, or the byte-coded tile instantiation
  if (is_quad(k) && k.epb != kQuadEnvs)
    std::snprintf(shape, sizeof(shape), "%s,E%d", k.waves == 8 ? ",W8" : "", k.epb);
  else if (k.bytetile)
    std::snprintf(shape, sizeof(shape), ",bytetile");
  std::snprintf(out, sizeof(out), "pe_step_%s<%s%s%s>",
                k.family == StepFamily::fast ? "fast" : (is_far(k) ? "far" : "quad"), rays, k.oneword ? ",1word" : "",
                shape);
}

// the step kernel's dynamic LDS
size_t step_lds_bytes(const Geo& g, const StepKernel& k) {
  switch (k.family) {
    case StepFamily::wave: return wave_lds_bytes(g);
    case StepFamily::fast: return lds_bytes(g);
    case StepFamily::far: return sizeof(float) * (size_t)far_lds_floats(g.G, g.WPR, g.C, g.R);
    case StepFamily::quad: break;
  }
  return quad_lds_bytes(g, k.bytetile, is_rt(k));
}

// ---------------------------------------------------------------------- host tables
// The LIDAR probe offsets [C][R] (plantos_env.py:261-267).
void lidar_offsets(int C, int R, std::vector<int8_t>& ldx, std::vector<int8_t>& ldy) {
  ldx.assign((size_t)C * R, 0);
  ldy.assign((size_t)C * R, 0);
  const double pi = 3.141592653589793;  // math.pi; plantos_env.py:261-267
  for (int i = 0; i < C; ++i) {
    double angle = ((2.0 * pi) * (double)i) / (double)C;
    for (int r = 1; r <= R; ++r) {
      ldx[i * R + r - 1] = (int8_t)(int)((double)r * std::cos(angle));
      ldy[i * R + r - 1] = (int8_t)(int)((double)r * std::sin(angle));
    }
  }
}

template <int C, int R>
bool table_matches(const std::vector<int8_t>& dx, const std::vector<int8_t>& dy) {
  for (int i = 0; i < C; ++i)
    for (int r = 0; r < R; ++r)
      if (LidarTab<C, R>::dx[i][r] != dx[i * R + r] || LidarTab<C, R>::dy[i][r] != dy[i * R + r]) return false;
  return true;
}

Tables make_tables(const Geo& g) {
  const int G = g.G, R = g.R;
  Tables tab;
  std::memset(&tab, 0, sizeof(tab));
  for (int r = 0; r <= R; ++r) tab.dist[r] = (float)((double)r / (double)R);
  for (int x = 0; x < G; ++x) tab.pos[x] = (float)((double)x / (double)G);
  for (int v = 0; v < 16; ++v) tab.vis[v] = (float)((double)(v < 10 ? v : 10) / 10.0);
  for (int p = 0; p < G + 2 * R; ++p) {
    int w = (2 * p) / 64, b = (2 * p) % 64;
    if (p < R || p >= G + R)
      tab.grid_pad[w] |= 1ull << b;
    else
      tab.grid_real[w] |= 1ull << b;
  }
  for (int p = 0; p < G + 4; ++p)
    if (p < 2 || p >= G + 2) tab.vis_pad[(4 * p) / 32] |= 10u << ((4 * p) % 32);
  return tab;
}

// State::ldxy's formats (pe_device.hpp): RP = R rounded up to 8 entries per ray
enum class RayTab { plain, wave_aligned, runtime };
int ray_pitch(int R) { return (R + 7) & ~7; }

size_t ray_table_bytes(RayTab f, int C, int R) {
  const size_t n = (size_t)C * ray_pitch(R);
  switch (f) {
    case RayTab::wave_aligned: return (n * 3 + 15) & ~(size_t)15;
    case RayTab::runtime: return (2 * n + 16) * 4;  // the LDS-form entries, then the register-window header
                                                    // [4][4] and entries (pe_quad.hpp)
    case RayTab::plain: break;
  }
  return n * 2;
}

template <class T>
std::vector<uint8_t> bytes_of(const std::vector<T>& v) {
  const uint8_t* p = reinterpret_cast<const uint8_t*>(v.data());
  return std::vector<uint8_t>(p, p + v.size() * sizeof(T));
}

// plain: [C][RP] i16 (dx & 0xFF) | dy << 8, zero-padded
std::vector<int16_t> ray_table_plain(int C, int R, const std::vector<int8_t>& ldx, const std::vector<int8_t>& ldy) {
  const int RP = ray_pitch(R);
  std::vector<int16_t> ldxy((size_t)C * RP, 0);
  for (int i = 0; i < C; ++i)
    for (int r = 0; r < R; ++r)
      ldxy[(size_t)i * RP + r] = (int16_t)((uint8_t)ldx[i * R + r] | ((int)ldy[i * R + r] << 8));
  return ldxy;
}

// pe_step_wave<., true>'s LDS header entries: [C][RP] u16 byte offsets into the aligned window,
// then [C][RP] u8 bit shifts
std::vector<uint8_t> ray_table_wave_aligned(int C, int R, const std::vector<int8_t>& ldx,
                                            const std::vector<int8_t>& ldy) {
  const std::vector<int16_t> ldxy = ray_table_plain(C, R, ldx, ldy);
  std::vector<uint8_t> aln(((ldxy.size() * 3 + 15) & ~(size_t)15), 0);
  for (size_t k = 0; k < ldxy.size(); ++k) {
    const uint32_t en = aln_entry((uint16_t)ldxy[k], R, (4 * R + 33) >> 5);
    const uint16_t off = (uint16_t)(4u * (en & 0x7FFu));
    std::memcpy(aln.data() + 2 * k, &off, 2);
    aln[2 * ldxy.size() + k] = (uint8_t)((en >> 11) & 31u);
  }
  return aln;
}

// the runtime sector kernel's entries (pe_quad.hpp quad_rays_rt): the probe's LDS byte offset from
// the rover row (dx rows of 64 envs x 8 B) | its bit shift 2(dy+R) << 16
std::vector<uint32_t> ray_table_runtime(int C, int R, const std::vector<int8_t>& ldx, const std::vector<int8_t>& ldy) {
  const int RP = ray_pitch(R);
  std::vector<uint32_t> rt(2 * (size_t)C * RP + 16, 0u);
  for (int i = 0; i < C; ++i)
    for (int r = 0; r < R; ++r)
      rt[(size_t)i * RP + r] = (uint32_t)(uint16_t)(int16_t)(ldx[i * R + r] * kQuadEnvs * 8) |
                               ((uint32_t)(2 * (ldy[i * R + r] + R)) << 16);
  // the register-window form (pe_quad.hpp quad_rays_rt_reg): per wave w (rays [wC/4, (w+1)C/4))
  // the header {LO, DLO, NROWS, ok}, per probe (dx - LO) | 2(dy - DLO) << 8
  uint32_t* hdr = rt.data() + (size_t)C * RP;
  uint32_t* ent = hdr + 16;
  for (int w = 0; w < 4; ++w) {
    const int i0 = w * C / 4, i1 = (w + 1) * C / 4;
    int lo = 1 << 20, hi = -(1 << 20), dlo = 1 << 20, dhi = -(1 << 20);
    for (int i = i0; i < i1; ++i)
      for (int r = 0; r < R; ++r) {
        lo = std::min(lo, (int)ldx[i * R + r]);
        hi = std::max(hi, (int)ldx[i * R + r]);
        dlo = std::min(dlo, (int)ldy[i * R + r]);
        dhi = std::max(dhi, (int)ldy[i * R + r]);
      }
    const bool ok = i1 > i0 && hi - lo + 1 <= kRtRegRows && dhi - dlo + 1 <= 16;
    hdr[4 * w] = (uint32_t)lo;
    hdr[4 * w + 1] = (uint32_t)dlo;
    hdr[4 * w + 2] = (uint32_t)(hi - lo + 1);
    hdr[4 * w + 3] = ok ? 1u : 0u;
    if (ok)
      for (int i = i0; i < i1; ++i)
        for (int r = 0; r < R; ++r)
          ent[(size_t)i * RP + r] = (uint32_t)(ldx[i * R + r] - lo) | ((uint32_t)(2 * (ldy[i * R + r] - dlo)) << 8);
  }
  return rt;
}

std::vector<uint8_t> ray_table(RayTab f, int C, int R, const std::vector<int8_t>& ldx, const std::vector<int8_t>& ldy) {
  switch (f) {
    case RayTab::wave_aligned: return ray_table_wave_aligned(C, R, ldx, ldy);
    case RayTab::runtime: return bytes_of(ray_table_runtime(C, R, ldx, ldy));
    case RayTab::plain: break;
  }
  return bytes_of(ray_table_plain(C, R, ldx, ldy));
}

// ---------------------------------------------------------------------- the plan
// A/B knobs of the measurement tools (tools/ab_build.sh builds a SEPARATE library with
// -DPE_DEBUG_KNOBS, whose knobs_from_env() fills this); the product library passes the defaults
// and reads no environment variable.  make_plan() applies each where the ladder needs it: the
// results depend on that order.
struct Knobs {
  bool lane_kernels = false;      // PE_STEP_KERNEL=lane: the lane-per-env twins at C16R6 / C64R6, no sector kernel
  bool wave_kernel = false;       // PE_STEP_KERNEL=wave: the one-wave-per-env kernel
  std::optional<int> stagger;     // PE_STAGGER
  std::optional<size_t> lds_floor;  // PE_LDS_FLOOR
  std::optional<int> tile_codes;  // PE_TILE_CODES (the headline kernel only)
  std::optional<int> quad_epb;    // PE_QUAD_EPB (the headline kernel's f32 form only)
};

#ifdef PE_DEBUG_KNOBS
Knobs knobs_from_env() {
  Knobs kb;
  if (const char* kenv = std::getenv("PE_STEP_KERNEL")) {
    kb.lane_kernels = std::strcmp(kenv, "lane") == 0;
    kb.wave_kernel = std::strcmp(kenv, "wave") == 0;
  }
  if (const char* sg = std::getenv("PE_STAGGER")) kb.stagger = std::atoi(sg);
  if (const char* lf = std::getenv("PE_LDS_FLOOR")) kb.lds_floor = std::strtoul(lf, nullptr, 10);
  if (const char* tc = std::getenv("PE_TILE_CODES")) kb.tile_codes = std::atoi(tc);
  if (const char* ep = std::getenv("PE_QUAD_EPB")) kb.quad_epb = std::atoi(ep);
  return kb;
}
#endif

// One device allocation carved into 256-B aligned arrays.
struct Carve {
  size_t off = 0;
  size_t operator()(size_t bytes) {
    size_t o = off;
    off = align_up(off + bytes, 256);
    return o;
  }
};
struct StateLayout {  // the main allocation (State's arrays)
  size_t tab, ldx, ldy, ldxy, err, scal, ret, grid, vis, vx, vpend, expl, bytes;
};
struct PrefetchLayout {  // the prefetched resets' allocation (Prefetch's arrays); bytes == 0: none
  size_t scal, grid, obs, queue, qn, flag, bytes;
  uint32_t ostride;
};

struct Plan {
  Geo g;
  Rules rl;
  StepKernel k;
  int obs_codes;      // pe_config.obs_codes: the byte-coded obs boundary (implies k.bytetile)
  int stagger;        // sector-kernel start delay per block quarter
  size_t lds_floor;   // minimum dynamic LDS per step workgroup (diagnostics)
  int coop_max_done;  // wave-cooperative auto-resets up to this many done envs per block; 0: never
  int pf_every;       // steps between queue-mode prefetch launches; 0: no prefetched resets
  char kname[64];
  RayTab ray_tab;
  std::vector<int8_t> ldx, ldy;  // the LIDAR offsets [C][R]
  StateLayout mem;
  PrefetchLayout pf;
};

struct PlanError {
  int code = PE_OK;
  const char* msg = "";
};

PlanError make_plan(const pe_config& cfg, int n_envs, int num_cus, const Knobs& kb, Plan& p) {
  const pe_config* c = &cfg;
  if (c->abi_version != PE_ABI_VERSION) return {PE_ERR_ARG, "ABI version mismatch"};
  const int G = c->grid_size, R = c->lidar_range, C = c->lidar_channels, P = c->num_plants, O = c->num_obstacles;
  if (G < 1 || G > 128) return {PE_ERR_ARG, "grid_size must be in [1, 128]"};
  if (R < 1 || R > 64) return {PE_ERR_ARG, "lidar_range must be in [1, 64]"};
  if (C < 1 || C > 256) return {PE_ERR_ARG, "lidar_channels must be in [1, 256]"};
  if (P < 0 || P >= G * G) return {PE_ERR_ARG, "num_plants must be in [0, G*G)"};
  if (O < 0) return {PE_ERR_ARG, "num_obstacles must be >= 0"};
  if (O / 3 > 0 && G < 5) return {PE_ERR_ARG, "randint(2, G-3) needs grid_size >= 5 (plantos_env.py:344)"};
  if (c->max_steps < 1 || c->max_steps > 65535) return {PE_ERR_ARG, "max_steps must be in [1, 65535]"};
  if (c->map_generation_algo != PE_MAP_ORIGINAL && c->map_generation_algo != PE_MAP_MAZE)
    return {PE_ERR_ARG, "map_generation_algo must be PE_MAP_ORIGINAL or PE_MAP_MAZE"};
  if (c->map_generation_algo == PE_MAP_MAZE && G < 7)
    return {PE_ERR_ARG, "the maze needs grid_size >= 7 (randint(0, (G-1)//6 - 1), plantos_env_new.py:427)"};
  if (n_envs < 1) return {PE_ERR_ARG, "n_envs must be >= 1"};
  if (2 * (G + 2 * R) > 64 * kMaxWPR) return {PE_ERR_ARG, "G + 2R too large"};

  p = Plan();
  Geo& g = p.g;
  g.G = G;
  g.C = C;
  g.R = R;
  g.D = 5 * C + 27;
  g.DS = g.D | 1;
  g.GG = G * G;
  g.WPR = (2 * (G + 2 * R) + 63) / 64;
  // visit row words: the padded row's G+4 nibbles + a spare word, so that the 8-nibble
  // window starting at any padded column y-1 (words vw, vw+1) stays inside the row.
  // (Tried: 4 words up to G = 25 -- 16-B rows, one load per window row in the
  // multi-word kernel: 25x25 10.38 -> 10.97 us, 21x21/C10/R2 one-word 8.05 -> 8.14;
  // profiles/r3j_ab_*.jsonl.)
  g.NW = (4 * (G + 4) + 31) / 32 + 1;
  if (g.NW < 4) g.NW = 4;  // 16-B visit rows: one dwordx4 per row in the sector kernel
  g.EW = (g.GG + 31) / 32;
  g.gstride = (int64_t)align_up((size_t)G * g.WPR, 2);  // 16-B aligned env blocks (row-pair loads)
  // two visit slots per env, 16-B aligned (episode k's visits in slot k & 1: pe_device.hpp vis_env)
  g.vslot = (int64_t)align_up((size_t)G * g.NW, 4);
  g.vstride = 2 * g.vslot;
  g.hstride = (int64_t)align_up((size_t)g.GG, 8);
  // explored words; also the picks scratch of a curriculum reset that keeps visits
  g.estride = (int64_t)align_up((size_t)std::max(g.EW, (P + 1) / 2), 4);
  // LDS limits: the lane-per-env kernels that every geometry keeps (pe_load_maps_kernel,
  // and pe_reset_kernel where the cooperative reset does not apply) hold a [64 x D]
  // obs tile -- this caps C at 120 whatever the step kernel; the one-wave-per-env step
  // kernel (the step kernel of every geometry without a sector kernel) its header +
  // 8 per-wave regions.
  if (lds_bytes(g) > kLdsMax) return {PE_ERR_ARG, "observation tile does not fit LDS (lidar_channels <= 120)"};
  if (wave_lds_bytes(g) > kLdsMax)
    return {PE_ERR_ARG, "the one-wave-per-env step kernel's window does not fit LDS"};

  Rules& rl = p.rl;
  rl.r_goal = c->r_goal;
  rl.r_mistake = c->r_mistake;
  rl.r_invalid = c->r_invalid;
  rl.r_water_empty = c->r_water_empty;
  rl.r_step = c->r_step;
  rl.r_exploration = c->r_exploration;
  rl.r_revisit = c->r_revisit;
  rl.r_complete = c->r_complete;
  rl.p_thirsty = c->thirsty_plant_prob;
  rl.seed = c->seed;
  rl.env_off = c->env_id_offset;
  rl.P = P;
  rl.O = O;
  rl.map_algo = c->map_generation_algo;
  rl.max_steps = c->max_steps;
  // Auto-resets in the step kernel: wave-cooperative (pe_coop.hpp: one env at a
  // time per wave, ~10 us each at 20x20) when a block has few done envs; one lane
  // per env (all of a wave's envs at once, ~0.26 ms for a whole batch at 20x20)
  // when many are done together -- unless the lane path would have to scan its
  // grid image in HBM (no room for it in the obs-tile row), where it is ~30x
  // slower (29 ms for a whole 64x64 batch) and the cooperative path always wins.
  const bool coop_ok = coop_reset_ok(G, R, g.WPR, g.NW, P, C, c->map_generation_algo);
  if (!coop_ok)
    p.coop_max_done = 0;
  else if (reset_scratch_bytes(G, g.WPR, P) <= 4 * g.D)
    p.coop_max_done = kCoopMaxDone;
  else
    p.coop_max_done = kQuadEnvs;

  // ---- the step kernel.  The one-wave-per-env kernel runs any geometry; each rung below
  // replaces it where a faster kernel applies.
  lidar_offsets(C, R, p.ldx, p.ldy);
  StepKernel& k = p.k;
  k = wave_kernel();
  // the one-word form (whole padded row in one u64) needs WPR == 1 and 16-B visit
  // rows (NW == 4: G <= 20); otherwise the multi-word (funnel-shifted) form
  // (C16R6: WPR == 1 at R = 6 means 2 (G + 12) <= 64, so G <= 20 and NW == 4)
  const bool oneword = g.WPR == 1 && g.NW == 4;
  // compile-time tables with a lane-per-env twin (PE_STEP_KERNEL=lane, debug builds, for A/B
  // measurement at C16R6 / C64R6)
  if (C == 16 && R == 6 && table_matches<16, 6>(p.ldx, p.ldy))
    k = kb.lane_kernels ? fast_kernel(16, 6, oneword) : quad_kernel(16, 6, oneword);
  if (C == 64 && R == 6 && table_matches<64, 6>(p.ldx, p.ldy))
    k = kb.lane_kernels ? fast_kernel(64, 6, false) : quad_kernel(64, 6, false);
  if (!kb.lane_kernels) {
    // sector kernels of the other specialized geometries (4 waves; no lane-kernel twin)
    if (C == 10 && R == 2 && table_matches<10, 2>(p.ldx, p.ldy)) k = quad_kernel(10, 2, oneword);
    if (C == 16 && R == 4 && table_matches<16, 4>(p.ldx, p.ldy)) k = quad_kernel(16, 4, oneword);
    // R > 14 with a compile-time table: the far sector kernel (its rows and the auto-reset
    // path's are kCoopWPR words: 96 < G + 2R <= 128)
    if (C == 64 && R == 32 && g.WPR == kCoopWPR && table_matches<64, 32>(p.ldx, p.ldy)) k = far_kernel(64, 32);
    // every other geometry with 4 <= C <= 32 and 2 <= R <= 14: the sector kernel with
    // table-driven rays (quad_rays_rt) instead of one wave per env -- 64 envs per
    // workgroup share the per-env work the wave kernel repeats per wave
    // (33 <= C <= 64: with the byte-coded tile, below)
    if (k.family == StepFamily::wave && C >= 4 && C <= kRtCMaxBT && R >= 2 && R <= kRtRMax)
      k = quad_kernel(0, 0, oneword);
  }
  // byte-coded obs tile where the f32 tile limits the sector kernel's occupancy
  // (C = 64: 89 KB -> 22 KB of LDS per workgroup)
  k.bytetile = is_kernel(k, StepFamily::quad, 64, 6) || is_far(k) || (is_rt(k) && C > kRtCMax);
  // the runtime kernel with C <= 32 too, where its f32 tile holds fewer workgroups per CU than
  // the byte tile and the batch needs more than one round of them (32x32 / C24 / R9: 54 KB, two
  // per CU -- 65536 envs ran as two waves of workgroups, the second starting ~13 us in,
  // profiles/r5s/stamps_g32.json); small batches keep the f32 tile (no expansion at the store)
  if (!k.bytetile && is_rt(k)) {
    auto per_cu = [](size_t l) { return std::min<size_t>(4, kLdsMax / l); };
    const size_t lf = quad_lds_bytes(g, false, true), lb = quad_lds_bytes(g, true, true);
    const int64_t blocks = ((int64_t)n_envs + kQuadEnvs - 1) / kQuadEnvs;
    if (per_cu(lb) > per_cu(lf) && blocks > (int64_t)num_cus * (int64_t)per_cu(lf)) k.bytetile = true;
  }
  if (kb.tile_codes && is_headline(k)) k.bytetile = *kb.tile_codes != 0;
  // obs as byte codes at the boundary (pe_step_codes): the byte-coded tile kernels
  p.obs_codes = c->obs_codes ? 1 : 0;
  if (p.obs_codes) {
    if (!(is_headline(k) || is_kernel(k, StepFamily::quad, 64, 6) || is_rt(k) || is_far(k)))
      return {PE_ERR_ARG, "obs_codes needs a byte-coded sector kernel (C=16/R=6 with G<=20, C=64/R=6, or "
                          "4<=C<=64 with 2<=R<=14 and no compile-time kernel)"};
    k.bytetile = true;
  }
  if (k.bytetile) {
    // (not the byte-coded C16 kernel -- config 5's codes step: its quarters started apart
    // cost it ~0.9 us desynchronized, 11.68 -> 10.75 us without, profiles/r6c/ab_codesstag;
    // the runtime byte-tile kernel keeps it: 32x32/C24/R9 17.0 -> 18.1 us without)
    // all 1024 workgroups of a 65536-env batch are resident at once (4 per CU) and
    // would run their load, compute and 89-KB store phases in lockstep: starting the
    // grid's quarters ~0.85 us apart overlaps one quarter's stores with the next
    // one's loads (64x64 / 64 rays, same-box: 28.7 -> 26.3 us; 2x that: 27.0)
    // (the far kernel: 8 -- 52.8 -> 52.1 us, desynchronized unchanged, profiles/r6d/ab_farstag)
    p.stagger = is_headline(k) ? 0 : (is_far(k) ? 8 : 4);
  }
  if (kb.stagger) p.stagger = *kb.stagger;  // (overrides the byte-tile default)
  if (kb.lds_floor) p.lds_floor = std::min<size_t>(*kb.lds_floor, kLdsMax);
  // a sector kernel whose LDS does not fit: its lane-per-env twin where it has one, else the wave kernel
  if ((is_quad(k) || is_far(k)) && step_lds_bytes(g, k) > kLdsMax)
    k = is_quad(k) && k.R == 6 && k.C != 0 ? fast_kernel(k.C, k.R, k.oneword) : wave_kernel();
  if (kb.wave_kernel) k = wave_kernel();  // A/B: the one-wave-per-env kernel (after the fallback)
  if (p.obs_codes && !k.bytetile) return {PE_ERR_ARG, "obs_codes: the byte-coded tile does not fit this geometry"};
  // envs per workgroup: a batch too small to give every CU four 64-env workgroups
  // (1024 at 65536 envs) is cut into 16- or 32-env workgroups instead, so that it
  // still spreads over all 256 CUs (headline geometry's kernel only; 4 waves, f32 tile)
  // (up to 4096 envs: 8 waves x 16 envs -- two waves per SIMD on every CU, sectors of 2
  // rays: 2048 envs 4.56 -> 4.41 us, 4096 4.56 -> 4.49; 8192 4.82 -> 4.98 us, kept at 4)
  // batch sizes up to which the headline kernel runs 16- / 32-env workgroups
  // (same-box A/B, profiles/r3b_ab_epb*.jsonl: 4096 envs 5.06 -> 4.55 us with 16-env
  // workgroups, 8192: 16 ~ 32, 16384: 32 best, 32768: 32 ~ 64)
  constexpr int kSmallBatch16 = 8192, kSmallBatch32 = 32768, kSmallBatch8W = 4096;
  if (is_headline(k) && !k.bytetile) {
    k.epb = n_envs <= kSmallBatch16 ? 16 : (n_envs <= kSmallBatch32 ? 32 : kQuadEnvs);
    if (n_envs <= kSmallBatch8W) k.waves = 8;
    if (kb.quad_epb) {
      k.epb = *kb.quad_epb == 16 || *kb.quad_epb == 32 ? *kb.quad_epb : kQuadEnvs;
      if (k.epb != 16) k.waves = 4;  // (the 8-wave kernel exists with 16 envs only)
    }
  }
  if (is_quad(k) && !quad_kernel_exists(k)) return {PE_ERR_ARG, "internal: no sector kernel instantiated for the plan"};
  kernel_name(k, p.kname);
  // explicit reset-path tuning (pe_config.coop_max_done; -1: the choice above) --
  // applied before the prefetch decision, which depends on it
  if (c->coop_max_done >= 0 && coop_ok) p.coop_max_done = std::min(c->coop_max_done, kQuadEnvs);
  // Prefetched resets (pe_coop.hpp Prefetch) where the sector kernel takes the
  // cooperative path.  The done-count threshold above stays: a whole block done at
  // once (a synchronized batch truncating) is cheaper through the lane-per-env path,
  // which consumes no record and so queues no regeneration (20x20: 0.26 ms per
  // batch reset, against 0.09 ms for the copies + ~0.3 ms to regenerate 65536 maps).
  p.pf_every = c->prefetch_every >= 0 ? c->prefetch_every : kPrefetchEvery;
  if (k.family == StepFamily::fast || p.coop_max_done <= 0 || !c->autoreset) p.pf_every = 0;

  // ---- the allocations
  p.ray_tab = is_rt(k) ? RayTab::runtime  // u32 probe entries (quad_rays_rt)
                       : (k.family == StepFamily::wave && wave_aligned(g) ? RayTab::wave_aligned  // pe_step_wave<., true>
                                                                                   : RayTab::plain);
  const size_t n = (size_t)n_envs, nl = (size_t)C * R;
  Carve carve;
  StateLayout& m = p.mem;
  m.tab = carve(sizeof(Tables));
  m.ldx = carve(nl);
  m.ldy = carve(nl);
  m.ldxy = carve(ray_table_bytes(p.ray_tab, C, R));
  m.err = carve(sizeof(uint32_t));
  m.scal = carve(n * sizeof(uint4));
  m.ret = carve(n * sizeof(double));
  m.grid = carve(n * (size_t)g.gstride * 8);
  m.vis = carve(n * (size_t)g.vstride * 4);
  m.vx = carve(n * (size_t)g.hstride * 4);
  m.vpend = carve(n * sizeof(uint32_t));
  m.expl = carve(n * (size_t)g.estride * 4);
  m.bytes = carve.off;
  if (is_far(k)) {
    // pe_step_far loads a quadrant's off-map rows UNCLAMPED (pe_far.hpp far_sector: up to
    // R rows before the env's grid block and R rows + one raw word after it, selected away
    // afterwards): the first env's must land in the arrays carved before the grid, the last
    // env's in those after it -- inside this one allocation
    const size_t row_b = (size_t)kFarRow32 * 4, grid_end = m.grid + n * (size_t)g.gstride * 8;
    if (g.WPR != kCoopWPR || m.grid < (size_t)R * row_b || m.bytes - grid_end < (size_t)(R + 1) * row_b)
      return {PE_ERR_ARG, "pe_step_far: the allocation leaves less than R padded grid rows of slack around the "
                          "grid array (its off-map row loads would leave the allocation)"};
  }
  if (p.pf_every > 0) {
    Carve pcarve;
    PrefetchLayout& f = p.pf;
    f.ostride = (uint32_t)pf_ostride(g, k.bytetile);
    f.scal = pcarve(n * sizeof(uint4));
    f.grid = pcarve(n * (size_t)g.gstride * 8);
    f.obs = pcarve(n * (size_t)f.ostride);
    f.queue = pcarve(n * 4);
    f.qn = pcarve(2 * 4);
    f.flag = pcarve(n);
    f.bytes = pcarve.off;
  }
  return {};
}

}  // namespace
