// pe_render.hip -- batched rgb_array frames of env state (include/plantos_batch.h
// pe_render / pe_render_tables): the sprite-less fallback path of the fork's
// _render_frame (gradio-app/plantos_env_new.py:697-762), one frame per env, drawn on the
// device straight from the SoA state.
//
// The frame.  s = cell_size, H = W = G*s, uint8 [H][W][3] RGB, row-major; image row <->
// grid row x, image column <-> grid column y.  Later layers overwrite earlier ones:
//   1. background: every pixel (34,139,34)                                        :706-710
//   2. explored overlay: cells with explored_map > 0 become (200,200,200, a=100) blended
//      over the background, per channel ((d<<8) + (s-d)*a + s) >> 8 = (99,163,99) :712-718
//   3. obstacles (105,105,105)                                                    :720-723
//   4. plants: thirsty (255,165,0), hydrated (0,255,0)                            :725-730
//   5. LIDAR rays, rover at (x, y): centre (cx, cy) = (y*s + s/2, x*s + s/2) in (column,
//      row) pixels; ray i at angle 2*pi*i/C; hit distance h = the first r in 1..R whose
//      cell (x + int(r cos), y + int(r sin)) is off the map, an obstacle or ANY plant,
//      else R -- the observation's march, (0,0) offsets included (:737-746); end point
//      (cx + int(h*s*sin), cy + int(h*s*cos)), the integer h*s formed first, the product
//      in double, truncated toward zero (:748-749: sin/cos swapped against the march).
//      A 1-px line centre -> end in (100,100,255): integer Bresenham, both end points
//      plotted (dx = |x2-x1|, dy = |y2-y1|, err = trunc((dx > dy ? dx : -dy) / 2); loop:
//      plot; e2 = err; if e2 > -dx { err -= dy; step x }; if e2 < dy { err += dx; step
//      y }, until the end point has been plotted), then a disc at the end point: pixels
//      with ddx^2 + ddy^2 <= 4.  The unclipped line is walked; pixels off the canvas are
//      dropped.                                                                   :750-751
//   6. rover cell (0,0,255)                                                       :753-756
//   7. grid lines: pixel rows and columns j*s, j = 0..G-1, (200,200,200)         :758-760
//      (the reference's j = G line falls off the canvas)
// Out of scope: the sprite path (PNG textures + pygame.transform.scale), 'human' windows,
// the Ursina viewer, and the root env's differently styled _render_2d.  The line, the
// disc and the blend are this project's definitions of the pygame primitives.
//
// The kernel.  The work is store-bound (3*W*H bytes out per frame against a few hundred
// bytes in).  One 256-thread workgroup per (frame, band of pixel rows), all in LDS until
// the last phase:
//   A  stage the env's G*G cell classes (palette index of layers 1-4: grid code +
//      explored bit), the per-column cell / grid-line table and the palette;
//   B  one strip of palette indices per cell row the band meets: the cell class, or --
//      since layers 6 and 7 overwrite the rays anyway -- the rover / grid-line index
//      where those apply; beside it, one lane per ray: march (from the staged classes)
//      and end point (the per-cell_size table);
//   C  the band, 16 pixels per lane: each pixel row is its cell row's strip, or all grid
//      line;
//   D  the rays, ray after ray, one pixel per lane: pixel t of the Bresenham walk above in
//      closed form (x-major, dx > dy: x = x1 + sx*t, y = y1 + sy*ceil((t*dy - dx/2)/dx);
//      else y = y1 + sy*t, x = x1 + sx*ceil((t*dx - dy/2)/dy); ceil of a negative = 0),
//      then the disc; written wherever the pixel is not already rover / grid line (all
//      writers store the same byte: no atomics);
//   E  expand to RGB: one 16-B store per lane (six pixels' colours shifted to the row's
//      byte phase) over the 16-B aligned interior of each row, byte stores for the
//      (< 16 B) unaligned head and tail of a row.
// Nothing is written outside the 3W bytes of the k frames' rows; the state is only read.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/plantos_batch.h"
#include "pe_device.hpp"
#include "pe_handle.hpp"
#include "pe_host.hpp"

namespace {
using namespace pe;

// palette order (pe_render_tables): the index is what the LDS band holds
enum : int { PAL_BG = 0, PAL_EXPLORED, PAL_OBSTACLE, PAL_THIRSTY, PAL_HYDRATED, PAL_RAY, PAL_ROVER, PAL_LINE, PAL_N };
constexpr uint8_t kPalette[PAL_N][3] = {
    {34, 139, 34},    // background
    {99, 163, 99},    // explored: (200,200,200, a=100) over the background
    {105, 105, 105},  // obstacle
    {255, 165, 0},    // thirsty plant
    {0, 255, 0},      // hydrated plant
    {100, 100, 255},  // LIDAR ray + end disc
    {0, 0, 255},      // rover cell
    {200, 200, 200},  // grid lines
};

constexpr int kThreads = 256;
// LDS band: palette indices of up to this many pixels.  Smaller bands measured slower (1024 frames
// of 160 x 160: 30.6 us at 16384, 41.1 at 8192, 52.9 at 4096, 76.9 at 2048).
constexpr int kBandBytes = 16384;
constexpr int kMinCell = 2, kMaxCell = 64, kMaxWidth = 4096;

// u / d for u * d < 2^32 as a multiply: magic = ceil(2^32 / d) (d >= 2), 0 for d == 1
struct Div {
  uint32_t d, magic;
};
__host__ inline Div make_div(uint32_t d) { return Div{d, d == 1 ? 0u : 0xFFFFFFFFu / d + 1u}; }
__device__ __forceinline__ uint32_t div_by(uint32_t u, Div v) { return v.d == 1 ? u : __umulhi(u, v.magic); }

struct RenderArgs {
  State st;
  Geo g;
  int n;
  const int32_t* env_index;
  const int32_t* ends;  // [C][R+1][2] end offsets (column px, row px) of this cell_size
  uint8_t* out;
  int64_t frame_stride, row_stride;
  int s, W, WP;    // cell_size, G*s, W rounded up to 16 (LDS row pitch)
  int nb, BR, NS;  // bands per frame, pixel rows per band, cell rows a band can meet
  Div by_s, by_upr, by_slots;  // cell_size, 16-px units per row, store slots per row
  uint32_t pal[PAL_N];         // r | g << 8 | b << 16
};

// LDS layout (byte offsets, all multiples of 16)
struct Lds {
  int cls, colc, pal, rays, strips, band, total;
};
__host__ __device__ inline Lds lds_layout(int GG, int C, int WP, int NS, int BR) {
  Lds l;
  l.cls = 0;                               // u8 [G*G] palette index of the cell layers
  l.colc = (GG + 15) & ~15;                // u8 [WP] column -> cell column | 0x80 on a grid line
  l.pal = l.colc + WP;                     // u32[8]
  l.rays = l.pal + 32;                     // i32[C][2] end points (column, row)
  l.strips = l.rays + ((8 * C + 15) & ~15);  // u8 [NS][WP]
  l.band = l.strips + NS * WP;             // u8 [BR][WP] + 16 (phase E reads up to 11 B past a pixel)
  l.total = l.band + BR * WP + 16;
  return l;
}

__global__ __launch_bounds__(kThreads) void pe_render_kernel(RenderArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const Geo& g = a.g;
  const int j = blockIdx.x / a.nb, band_id = blockIdx.x - j * a.nb;
  const int64_t e = a.env_index ? (int64_t)a.env_index[j] : (int64_t)j;
  if (e < 0 || e >= a.n) return;  // (whole workgroup) a bad index: the frame is not written
  const int G = g.G, s = a.s, W = a.W, WP = a.WP, H = W;
  const Lds L = lds_layout(g.GG, g.C, WP, a.NS, a.BR);
  uint8_t* cls = lds + L.cls;
  uint8_t* colc = lds + L.colc;
  uint32_t* pal = reinterpret_cast<uint32_t*>(lds + L.pal);
  int32_t* rays = reinterpret_cast<int32_t*>(lds + L.rays);
  uint8_t* strips = lds + L.strips;
  uint8_t* band = lds + L.band;
  const int y0 = band_id * a.BR, y1 = min(y0 + a.BR, H);
  const int c0 = y0 / s, ncr = (y1 - 1) / s - c0 + 1;  // the band's cell rows c0 .. c0 + ncr - 1
  const Scal sc = unpack(a.st.scal[e]);
  const int tid = threadIdx.x;

  // A: cell classes, column table, palette
  for (int c = tid; c < g.GG; c += kThreads) {
    const int row = c / G, col = c - row * G;
    const int code = grid_code(a.st, g, e, row, col + g.R);
    bool ex;
    if (sc.flags & F_EXPL_BITMAP)
      ex = (a.st.expl[e * g.estride + (c >> 5)] >> (c & 31)) & 1u;
    else
      ex = nibble_get(a.st, g, e, sc.episode, row, col) != 0;  // explored_map > 0 <=> visit > 0
    cls[c] = (uint8_t)(code == OBST ? PAL_OBSTACLE
                                    : code == THIRSTY ? PAL_THIRSTY : code == HYD ? PAL_HYDRATED
                                                                                  : ex ? PAL_EXPLORED : PAL_BG);
  }
  for (int x = tid; x < WP; x += kThreads) {
    const int cy = x / s;
    colc[x] = x < W ? (uint8_t)(cy | (x - cy * s == 0 ? 0x80 : 0)) : (uint8_t)0;
  }
  if (tid < PAL_N) pal[tid] = a.pal[tid];
  __syncthreads();

  // B: the strips, four pixels per lane; the rays' end points, one lane per ray
  const int upr4 = WP >> 2;
  for (int u = tid; u < ncr * upr4; u += kThreads) {
    const int c = u / upr4, x0 = (u - c * upr4) << 2;
    const int cx = c0 + c;
    const uint32_t cc = *reinterpret_cast<const uint32_t*>(colc + x0);
    uint32_t v = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint32_t c8 = (cc >> (8 * q)) & 0xFFu;
      const int cy = (int)(c8 & 0x7Fu);
      uint32_t p = cls[cx * G + cy];
      if (cx == sc.x && cy == sc.y) p = PAL_ROVER;
      if (c8 & 0x80u) p = PAL_LINE;
      v |= p << (8 * q);
    }
    *reinterpret_cast<uint32_t*>(strips + c * WP + x0) = v;
  }
  const int ccx = sc.y * s + s / 2, ccy = sc.x * s + s / 2;
  for (int i = tid; i < g.C; i += kThreads) {
    int h = g.R;
    for (int r = 1; r <= g.R; ++r) {
      const int px = sc.x + a.st.ldx[i * g.R + r - 1], py = sc.y + a.st.ldy[i * g.R + r - 1];
      if (px < 0 || px >= G || py < 0 || py >= G || cls[px * G + py] >= PAL_OBSTACLE) {
        h = r;
        break;
      }
    }
    const int32_t* en = a.ends + ((int64_t)i * (g.R + 1) + h) * 2;
    rays[2 * i] = ccx + en[0];
    rays[2 * i + 1] = ccy + en[1];
  }
  __syncthreads();

  // C: the band without the rays, 16 pixels per lane
  for (int u = tid; u < (y1 - y0) * (int)a.by_upr.d; u += kThreads) {
    const int r = (int)div_by((uint32_t)u, a.by_upr), x0 = (u - r * (int)a.by_upr.d) << 4;
    const int y = y0 + r, cx = (int)div_by((uint32_t)y, a.by_s);
    uint4 v = make_uint4(0x01010101u * PAL_LINE, 0x01010101u * PAL_LINE, 0x01010101u * PAL_LINE,
                         0x01010101u * PAL_LINE);
    if (y - cx * s != 0) v = *reinterpret_cast<const uint4*>(strips + (cx - c0) * WP + x0);
    *reinterpret_cast<uint4*>(band + r * WP + x0) = v;
  }
  __syncthreads();

  // D: rays.  Item t of a ray: t <= n is pixel t of the line, the next 25 the disc's 5 x 5 box.
  for (int i = 0; i < g.C; ++i) {
    const int x2 = rays[2 * i], y2 = rays[2 * i + 1];
    if (max(ccy, y2) + 2 < y0 || min(ccy, y2) - 2 >= y1) continue;  // (uniform) misses this band
    const int dx = abs(x2 - ccx), dy = abs(y2 - ccy), n = max(dx, dy);
    const int sx = ccx < x2 ? 1 : -1, sy = ccy < y2 ? 1 : -1;
    for (int t = tid; t <= n + 25; t += kThreads) {
      int x, y;
      if (t <= n) {
        if (dx > dy) {
          const int num = t * dy - dx / 2;
          x = ccx + sx * t;
          y = ccy + sy * (num <= 0 ? 0 : (num + dx - 1) / dx);
        } else {
          const int num = t * dx - dy / 2;
          y = ccy + sy * t;
          x = ccx + sx * (num <= 0 ? 0 : (num + dy - 1) / dy);  // (num > 0 implies dy > 0)
        }
      } else {
        const int q = t - n - 1, qy = q / 5, ddx = q - 5 * qy - 2, ddy = qy - 2;
        if (ddx * ddx + ddy * ddy > 4) continue;
        x = x2 + ddx;
        y = y2 + ddy;
      }
      if (x < 0 || x >= W || y < y0 || y >= y1) continue;  // off the canvas / another band's
      uint8_t* p = band + (y - y0) * WP + x;
      if (*p < PAL_ROVER) *p = PAL_RAY;  // the rover cell and the grid lines are drawn over the rays
    }
  }
  __syncthreads();

  // E: RGB.  Row byte b is channel b % 3 of pixel b / 3.  An aligned 16-B chunk at row byte
  // b0 holds bytes of the six pixels b0 / 3 .. b0 / 3 + 5, starting at byte b0 % 3 of the first.
  const int RB = 3 * W;  // bytes per row; slots per row: head | 16-B chunks | tail
  uint8_t* frame = a.out + (int64_t)j * a.frame_stride;
  for (int u = tid; u < (y1 - y0) * (int)a.by_slots.d; u += kThreads) {
    const int r = (int)div_by((uint32_t)u, a.by_slots), sl = u - r * (int)a.by_slots.d;
    uint8_t* row = frame + (int64_t)(y0 + r) * a.row_stride;
    const uint8_t* bi = band + r * WP;
    const int head = min((int)((16u - (uint32_t)(reinterpret_cast<uintptr_t>(row) & 15u)) & 15u), RB);
    const int b0 = sl == 0 ? 0 : head + 16 * (sl - 1);
    const int b1 = sl == 0 ? head : min(b0 + 16, RB);
    if (b0 >= b1) continue;
    if (b1 - b0 == 16 && sl != 0) {
      const int px = b0 / 3, ph = b0 - 3 * px;
      const uint32_t* wi = reinterpret_cast<const uint32_t*>(bi + (px & ~3));
      const uint32_t sh = 8u * (uint32_t)(px & 3);
      const uint32_t i0 = __funnelshift_r(wi[0], wi[1], sh), i1 = __funnelshift_r(wi[1], wi[2], sh);
      const uint32_t p0 = pal[i0 & 0xFFu], p1 = pal[(i0 >> 8) & 0xFFu], p2 = pal[(i0 >> 16) & 0xFFu];
      const uint32_t p3 = pal[i0 >> 24], p4 = pal[i1 & 0xFFu], p5 = pal[(i1 >> 8) & 0xFFu];
      // the six pixels' 18 bytes as dwords, then shifted down by the phase
      const uint32_t w0 = p0 | (p1 << 24), w1 = (p1 >> 8) | (p2 << 16), w2 = (p2 >> 16) | (p3 << 8);
      const uint32_t w3 = p4 | (p5 << 24), w4 = p5 >> 8;
      const uint32_t ps = 8u * (uint32_t)ph;
      *reinterpret_cast<uint4*>(row + b0) = make_uint4(__funnelshift_r(w0, w1, ps), __funnelshift_r(w1, w2, ps),
                                                       __funnelshift_r(w2, w3, ps), __funnelshift_r(w3, w4, ps));
    } else {
      for (int b = b0; b < b1; ++b) {
        const int px = b / 3, ph = b - 3 * px;
        row[b] = (uint8_t)(pal[bi[px]] >> (8 * ph));
      }
    }
  }
}

// ---------------------------------------------------------------- host side
// The per-cell_size device tables of one handle.  A table is uploaded once, before its
// first launch, into memory of its own and never written again, so an earlier launch
// still running on the stream reads its table undisturbed; all are freed by pe_destroy.
struct RenderCache {
  struct Entry {
    int cell_size;
    int32_t* ends;
  };
  std::vector<Entry> entries;
};

void ray_ends(int C, int R, int s, int32_t* out) {
  const double pi = 3.141592653589793;  // math.pi
  for (int i = 0; i < C; ++i) {
    const double angle = ((2.0 * pi) * (double)i) / (double)C;  // plantos_env_new.py:738
    for (int h = 0; h <= R; ++h) {
      const double hs = (double)(h * s);  // the integer product first (:748-749)
      out[((size_t)i * (R + 1) + h) * 2 + 0] = (int32_t)(hs * std::sin(angle));
      out[((size_t)i * (R + 1) + h) * 2 + 1] = (int32_t)(hs * std::cos(angle));
    }
  }
}

}  // namespace

extern "C" {

int pe_render_tables(const pe_config* c, int32_t cell_size, int32_t* ends, uint8_t* palette) {
  if (!c || (!ends && !palette)) return fail(PE_ERR_ARG, "null argument");
  if (c->lidar_channels < 1 || c->lidar_channels > 256 || c->lidar_range < 1 || c->lidar_range > 64)
    return fail(PE_ERR_ARG, "lidar_channels must be in [1, 256], lidar_range in [1, 64]");
  if (cell_size < 1 || cell_size > kMaxWidth) return fail(PE_ERR_ARG, "cell_size must be in [1, 4096]");
  if (ends) ray_ends(c->lidar_channels, c->lidar_range, cell_size, ends);
  if (palette) std::memcpy(palette, kPalette, sizeof(kPalette));
  return PE_OK;
}

// pe_destroy's hook (plantos_batch.hip); the handle's device is current.
void pe_internal_render_free(pe_handle* h) {
  RenderCache* rc = static_cast<RenderCache*>(h->render_cache);
  if (!rc) return;
  for (const RenderCache::Entry& en : rc->entries) (void)hipFree(en.ends);
  delete rc;
  h->render_cache = nullptr;
}

int pe_render(pe_handle* h, int32_t k, const int32_t* env_index, int32_t cell_size, uint8_t* out,
              int64_t frame_stride, int64_t row_stride, void* stream) {
  if (!h) return fail(PE_ERR_ARG, "null handle");
  if (k < 0) return fail(PE_ERR_ARG, "k must be >= 0");
  if (!env_index && k > h->n) return fail(PE_ERR_ARG, "k exceeds the number of envs (no env_index)");
  const int G = h->g.G;
  if (cell_size < kMinCell || cell_size > kMaxCell || G * cell_size > kMaxWidth)
    return fail(PE_ERR_ARG, "cell_size must be in [2, 64] with grid_size * cell_size <= 4096");
  const int W = G * cell_size;
  if (row_stride < 3 * (int64_t)W) return fail(PE_ERR_ARG, "row_stride must be >= 3 * grid_size * cell_size");
  if (frame_stride < 0 || (k > 1 && frame_stride < 3 * (int64_t)W))
    return fail(PE_ERR_ARG, "frame_stride must be >= 3 * grid_size * cell_size");
  if (k == 0) return PE_OK;
  if (!out) return fail(PE_ERR_ARG, "null argument");
  RenderArgs a;
  a.s = cell_size;
  a.W = W;
  a.WP = (W + 15) & ~15;
  a.nb = (int)(((int64_t)W * a.WP + kBandBytes - 1) / kBandBytes);
  a.BR = (W + a.nb - 1) / a.nb;
  a.nb = (W + a.BR - 1) / a.BR;  // no empty band
  a.NS = (a.BR - 1) / cell_size + 2;
  a.by_s = make_div((uint32_t)cell_size);
  a.by_upr = make_div((uint32_t)(a.WP >> 4));
  a.by_slots = make_div((uint32_t)((3 * W + 15) / 16 + 1));
  if ((int64_t)k * a.nb > (1 << 22)) return fail(PE_ERR_ARG, "too many frames for one call");
  DeviceGuard dg(h->device);
  if (dg.rc) return dg.rc;

  RenderCache* rc = static_cast<RenderCache*>(h->render_cache);
  if (!rc) {
    rc = new (std::nothrow) RenderCache();
    if (!rc) return fail(PE_ERR_NOMEM, "host allocation failed");
    h->render_cache = rc;
  }
  const int32_t* ends = nullptr;
  for (const RenderCache::Entry& en : rc->entries)
    if (en.cell_size == cell_size) ends = en.ends;
  if (!ends) {
    std::vector<int32_t> host((size_t)h->g.C * (h->g.R + 1) * 2);
    ray_ends(h->g.C, h->g.R, cell_size, host.data());
    int32_t* dev = nullptr;
    hipError_t me = hipMalloc(&dev, host.size() * sizeof(int32_t));
    if (me != hipSuccess) return fail(PE_ERR_NOMEM, std::string("hipMalloc: ") + hipGetErrorString(me));
    me = hipMemcpy(dev, host.data(), host.size() * sizeof(int32_t), hipMemcpyHostToDevice);  // done on return
    if (me != hipSuccess) {
      (void)hipFree(dev);
      return hip_fail(me, "hipMemcpy");
    }
    rc->entries.push_back({cell_size, dev});
    ends = dev;
  }

  a.st = h->st;
  a.g = h->g;
  a.n = h->n;
  a.env_index = env_index;
  a.ends = ends;
  a.out = out;
  a.frame_stride = frame_stride;
  a.row_stride = row_stride;
  for (int q = 0; q < PAL_N; ++q)
    a.pal[q] = (uint32_t)kPalette[q][0] | ((uint32_t)kPalette[q][1] << 8) | ((uint32_t)kPalette[q][2] << 16);
  const size_t lds = (size_t)lds_layout(h->g.GG, h->g.C, a.WP, a.NS, a.BR).total;
  hipLaunchKernelGGL(pe_render_kernel, dim3((unsigned)(k * a.nb)), dim3(kThreads), lds,
                     static_cast<hipStream_t>(stream), a);
  const hipError_t le = hipGetLastError();
  return le == hipSuccess ? PE_OK : hip_fail(le, "pe_render");
}

}  // extern "C"
