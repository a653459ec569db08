// tnp_render_raster / tnp_render_shade: an exact integer z-buffer rasteriser
// for polygon soups (include/tropical_hip.h has the contract).  The engine is
// not involved: scratch is allocated per call on the caller's stream and freed.
//
//   k_soup_offsets per polygon: the offsets are checked (soup_check.h; the
//                  front around the checks is soup_host.h's)
//   k_rv_ids       per index: ids checked (nothing is loaded through an id)
//   k_rv_project   per vertex: fp32 projection to 1/16-pixel ints + 20-bit depth
//   k_rv_fan       per polygon: triangle -> polygon map, dropped / degenerate
//   k_rv_small     per triangle: small boxes drawn here, the others flagged
//   scan, k_rv_compact   the flagged triangles as a list
//   k_rv_large     workgroups per listed triangle, 16 x 16 tiles of its box
//   k_rv_resolve   per pixel: polygon id, triangle number, boundary-edge mask
//   k_rv_shade     per output pixel: look-up table, edge colour, box filter
//
// Both coverage paths call tri_pixel() for a pixel and differ only in which
// pixels they visit; every pixel of the clamped box that tri_pixel() accepts
// is visited by either (a skipped tile holds none).
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/tropical_hip_debug.h"
#include "kernels.h"
#include "soup_host.h"

namespace {

constexpr int RV_MAX_DIM = 8192;
constexpr int RV_GUARD = 1 << 18;  // |sx|, |sy| bound (1/16 px)
constexpr int RV_ZMAX = (1 << 20) - 1;
constexpr int RV_SMALL = TNP_RENDER_SMALL_MAX;
constexpr int RV_TILE = 16;           // the workgroup path's tile: 16 x 16 pixels = TNP_BLOCK threads
constexpr unsigned RV_LARGE_GRID = 2048;  // k_rv_large's workgroups (8 per CU)
constexpr unsigned long long RV_BG = ~0ull;
static_assert(RV_TILE * RV_TILE == TNP_BLOCK, "one thread per tile pixel");

int g_path_mode = 0;  // tnp_debug_render_path

// counter block (int64 words)
enum { RC_ERR, RC_NIDX, RC_DROPPED, RC_DEGEN, RC_LARGE, RC_COVERED, RC_N };
// (RC_ERR / RC_NIDX are soup_check.h's two words: the checks are shared with tnp_polygon_report)
static_assert(RC_ERR == SOUP_ERR && RC_NIDX == SOUP_NIDX, "counter layout");

__global__ void __launch_bounds__(TNP_BLOCK)
k_rv_ids(const int64_t* __restrict__ off, int64_t P, const int64_t* __restrict__ idx, int64_t n, int64_t V,
         int64_t* __restrict__ ctr) {
  const int64_t i = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  if (i >= n) return;
  int64_t a, b;
  bool b_ok;
  soup_check_id(off, P, idx, i, V, ctr, a, b, b_ok);
}

struct ViewDev {
  float right[3], up[3], toward[3], center[3];
  float scale, D, h, half_w, half_h;
};

__device__ __forceinline__ float rv_dot(const float* r, const float* d) {
  return __fadd_rn(__fadd_rn(__fmul_rn(r[0], d[0]), __fmul_rn(r[1], d[1])), __fmul_rn(r[2], d[2]));
}

__global__ void __launch_bounds__(TNP_BLOCK)
k_rv_project(const float* __restrict__ xyz, int64_t V, ViewDev vw, int32_t* __restrict__ screen) {
  const int64_t v = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  if (v >= V) return;
  const float d[3] = {__fsub_rn(xyz[3 * v], vw.center[0]), __fsub_rn(xyz[3 * v + 1], vw.center[1]),
                      __fsub_rn(xyz[3 * v + 2], vw.center[2])};
  const float cr = rv_dot(vw.right, d), cu = rv_dot(vw.up, d), ct = rv_dot(vw.toward, d);
  const bool persp = vw.D > 0.f;
  float s = 1.f, q;
  if (persp) {
    s = __fdiv_rn(vw.D, __fsub_rn(vw.D, ct));
    q = __fdiv_rn(__fsub_rn(__fmul_rn(ct, vw.D), __fmul_rn(vw.h, vw.h)), __fmul_rn(vw.h, __fsub_rn(vw.D, ct)));
  } else {
    q = __fdiv_rn(ct, vw.h);
  }
  const float k = __fmul_rn(vw.scale, s);
  const float fx = rintf(__fmul_rn(__fadd_rn(vw.half_w, __fmul_rn(k, cr)), 16.f));
  const float fy = rintf(__fmul_rn(__fsub_rn(vw.half_h, __fmul_rn(k, cu)), 16.f));
  // (the comparisons are written so that a NaN flags)
  const bool ok = fabsf(fx) <= (float)RV_GUARD && fabsf(fy) <= (float)RV_GUARD && q >= -1.f && q <= 1.f &&
                  !(persp && !(ct < vw.D));
  int sx = 0, sy = 0, sz = -1;
  if (ok) {
    sx = (int)fx;
    sy = (int)fy;
    const float z = floorf(__fmul_rn(__fmul_rn(__fsub_rn(1.f, q), 0.5f), 1048576.f));
    sz = min(max((int)z, 0), RV_ZMAX);
  }
  screen[3 * v] = sx;
  screen[3 * v + 1] = sy;
  screen[3 * v + 2] = sz;
}

// ---- the integer triangle ------------------------------------------------------
struct RTri {
  int x0, y0, z0, x1, y1, z1, x2, y2, z2;
  int64_t A2;  // > 0 after setup
};

__device__ __forceinline__ int64_t rv_edge(int ax, int ay, int bx, int by, int px, int py) {
  return (int64_t)(bx - ax) * (int64_t)(py - ay) - (int64_t)(by - ay) * (int64_t)(px - ax);
}
__device__ __forceinline__ bool rv_owns(int dx, int dy) { return dy > 0 || (dy == 0 && dx < 0); }

// false: zero area
__device__ __forceinline__ bool tri_setup(const int32_t* __restrict__ scr, int64_t a, int64_t b, int64_t c, RTri& t) {
  t.x0 = scr[3 * a], t.y0 = scr[3 * a + 1], t.z0 = scr[3 * a + 2];
  t.x1 = scr[3 * b], t.y1 = scr[3 * b + 1], t.z1 = scr[3 * b + 2];
  t.x2 = scr[3 * c], t.y2 = scr[3 * c + 1], t.z2 = scr[3 * c + 2];
  t.A2 = rv_edge(t.x0, t.y0, t.x1, t.y1, t.x2, t.y2);
  if (t.A2 < 0) {
    int q;
    q = t.x1, t.x1 = t.x2, t.x2 = q;
    q = t.y1, t.y1 = t.y2, t.y2 = q;
    q = t.z1, t.z1 = t.z2, t.z2 = q;
    t.A2 = -t.A2;
  }
  return t.A2 != 0;
}

// covered? and the depth.  num < 2^60 and A2 < 2^40, so the quotient is below
// 2^20: the double quotient is off by at most one, which the remainder corrects
__device__ __forceinline__ bool tri_pixel(const RTri& t, int i, int j, unsigned& z) {
  const int px = 16 * i + 8, py = 16 * j + 8;
  const int64_t w0 = rv_edge(t.x1, t.y1, t.x2, t.y2, px, py);
  const int64_t w1 = rv_edge(t.x2, t.y2, t.x0, t.y0, px, py);
  const int64_t w2 = rv_edge(t.x0, t.y0, t.x1, t.y1, px, py);
  if ((w0 | w1 | w2) < 0) return false;
  if (w0 == 0 && !rv_owns(t.x2 - t.x1, t.y2 - t.y1)) return false;
  if (w1 == 0 && !rv_owns(t.x0 - t.x2, t.y0 - t.y2)) return false;
  if (w2 == 0 && !rv_owns(t.x1 - t.x0, t.y1 - t.y0)) return false;
  const int64_t num = w0 * t.z0 + w1 * t.z1 + w2 * t.z2;
  int64_t q = (int64_t)((double)num / (double)t.A2);
  const int64_t r = num - q * t.A2;
  if (r < 0) --q;
  else if (r >= t.A2) ++q;
  z = (unsigned)q;
  return true;
}

// the pixels whose centres lie in the triangle's bounding box, clamped to the
// image: columns [i0, i1], rows [j0, j1] (empty when i1 < i0 or j1 < j0)
__device__ __forceinline__ void tri_box(const RTri& t, int W, int H, int& i0, int& i1, int& j0, int& j1) {
  const int xa = min(t.x0, min(t.x1, t.x2)), xb = max(t.x0, max(t.x1, t.x2));
  const int ya = min(t.y0, min(t.y1, t.y2)), yb = max(t.y0, max(t.y1, t.y2));
  i0 = max((xa + 7) >> 4, 0), i1 = min((xb - 8) >> 4, W - 1);  // (>> of a negative int: arithmetic, floor)
  j0 = max((ya + 7) >> 4, 0), j1 = min((yb - 8) >> 4, H - 1);
}

__device__ __forceinline__ void vis_min(unsigned long long* __restrict__ vis, int64_t at, unsigned z, int64_t T) {
  const unsigned long long key = ((unsigned long long)z << 32) | (unsigned long long)T;
  // (a nearer record already there: the minimum would not change it)
  if (__hip_atomic_load(vis + at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > key) atomicMin(vis + at, key);
}

// triangle T of polygon p: its three index positions' ids
// (the offsets are the scan of the degrees, so polygon p's first triangle is number off[p] - 2 p)
__device__ __forceinline__ void fan_ids(const int64_t* __restrict__ off, const int64_t* __restrict__ idx, int64_t p,
                                        int64_t T, int64_t& a, int64_t& b, int64_t& c) {
  const int64_t base = off[p], t = T - (base - 2 * p);
  a = idx[base], b = idx[base + t + 1], c = idx[base + t + 2];
}

// per polygon: tpoly[T] = p for its triangles; pflag 1: a flagged vertex
// (dropped), 2: every fan triangle has zero area (degenerate), 0: drawn
__global__ void __launch_bounds__(TNP_BLOCK)
k_rv_fan(const int64_t* __restrict__ off, const int64_t* __restrict__ idx, int64_t P,
         const int32_t* __restrict__ scr, int32_t* __restrict__ tpoly, uint8_t* __restrict__ pflag,
         int64_t* __restrict__ ctr) {
  const int64_t p = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  int dropped = 0, degen = 0;
  if (p < P) {
    const int64_t a = off[p], b = off[p + 1], T0 = a - 2 * p;
    bool flagged = false;
    for (int64_t i = a; i < b; ++i) flagged |= scr[3 * idx[i] + 2] < 0;
    bool area = false;
    for (int64_t t = 0; t < b - a - 2; ++t) {
      tpoly[T0 + t] = (int32_t)p;
      if (!flagged && !area) {
        RTri tr;
        area = tri_setup(scr, idx[a], idx[a + t + 1], idx[a + t + 2], tr);
      }
    }
    dropped = flagged, degen = !flagged && !area;
    pflag[p] = flagged ? 1 : (area ? 0 : 2);
  }
  const int wd = tnp::wave_sum(dropped), wg = tnp::wave_sum(degen);
  if (tnp::lane() == 0) {
    if (wd) atomicAdd(reinterpret_cast<unsigned long long*>(ctr + RC_DROPPED), (unsigned long long)wd);
    if (wg) atomicAdd(reinterpret_cast<unsigned long long*>(ctr + RC_DEGEN), (unsigned long long)wg);
  }
}

// mode: 0 by the box, 1 everything here, 2 everything to the list
__global__ void __launch_bounds__(TNP_BLOCK)
k_rv_small(const int64_t* __restrict__ off, const int64_t* __restrict__ idx,
           int64_t nT, const int32_t* __restrict__ scr, const int32_t* __restrict__ tpoly,
           const uint8_t* __restrict__ pflag, int W, int H, int mode, unsigned long long* __restrict__ vis,
           int32_t* __restrict__ islarge) {
  const int64_t T = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  if (T >= nT) return;
  int large = 0;
  const int64_t p = tpoly[T];
  if (pflag[p] == 0) {
    int64_t a, b, c;
    fan_ids(off, idx, p, T, a, b, c);
    RTri t;
    if (tri_setup(scr, a, b, c, t)) {
      int i0, i1, j0, j1;
      tri_box(t, W, H, i0, i1, j0, j1);
      if (i1 >= i0 && j1 >= j0) {
        const bool small = i1 - i0 < RV_SMALL && j1 - j0 < RV_SMALL;
        if (mode == 1 || (mode == 0 && small)) {
          for (int j = j0; j <= j1; ++j)
            for (int i = i0; i <= i1; ++i) {
              unsigned z;
              if (tri_pixel(t, i, j, z)) vis_min(vis, (int64_t)j * W + i, z, T);
            }
        } else {
          large = 1;
        }
      }
    }
  }
  islarge[T] = large;
}

__global__ void __launch_bounds__(TNP_BLOCK)
k_rv_compact(const int32_t* __restrict__ islarge, const int64_t* __restrict__ loff, int64_t nT,
             int32_t* __restrict__ list) {
  const int64_t T = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  if (T < nT && islarge[T]) list[loff[T]] = (int32_t)T;  // loff[T] < the flagged count <= nT
}

// the largest value over the tile's pixel centres of the edge function of a -> b
__device__ __forceinline__ int64_t rv_edge_max(int ax, int ay, int bx, int by, int i0, int i1, int j0, int j1) {
  // e = dx (py - ay) - dy (px - ax): largest at the row end dx's sign picks and the column end -dy's picks
  const int dx = bx - ax, dy = by - ay;
  return rv_edge(ax, ay, bx, by, 16 * (dy > 0 ? i0 : i1) + 8, 16 * (dx > 0 ? j1 : j0) + 8);
}

// A fixed 1-D grid shares the list, whose length n is only known on the
// device: with n >= gridDim.x workgroup b takes triangles b, b + gridDim.x, ...
// whole; with fewer, gridDim.x / n workgroups share each triangle's tiles (so
// one image-sized triangle is spread over the whole grid) and the rest exit
__global__ void __launch_bounds__(TNP_BLOCK)
k_rv_large(const int64_t* __restrict__ off, const int64_t* __restrict__ idx,
           const int32_t* __restrict__ scr, const int32_t* __restrict__ tpoly, const int32_t* __restrict__ list,
           const int64_t* __restrict__ ctr, int W, int H, unsigned long long* __restrict__ vis) {
  const int64_t n = ctr[RC_LARGE];
  if (n == 0) return;
  const int li = threadIdx.x % RV_TILE, lj = threadIdx.x / RV_TILE;
  const int parts = n >= (int64_t)gridDim.x ? 1 : (int)((int64_t)gridDim.x / n);
  const int part = parts == 1 ? 0 : (int)(blockIdx.x / n);
  if (part >= parts) return;
  for (int64_t k = parts == 1 ? blockIdx.x : blockIdx.x % n; k < n; k += gridDim.x) {
    const int64_t T = list[k];
    int64_t a, b, c;
    fan_ids(off, idx, tpoly[T], T, a, b, c);
    RTri t;
    if (!tri_setup(scr, a, b, c, t)) continue;  // (listed triangles have area: block-uniform anyway)
    int i0, i1, j0, j1;
    tri_box(t, W, H, i0, i1, j0, j1);
    if (i1 < i0 || j1 < j0) continue;
    const int ntx = (i1 - i0) / RV_TILE + 1, nty = (j1 - j0) / RV_TILE + 1;
    for (int q = part; q < ntx * nty; q += parts) {
      const int ti0 = i0 + (q % ntx) * RV_TILE, tj0 = j0 + (q / ntx) * RV_TILE;
      const int ti1 = min(ti0 + RV_TILE - 1, i1), tj1 = min(tj0 + RV_TILE - 1, j1);
      // an edge function negative at every centre of the tile: no pixel of it is covered
      if (rv_edge_max(t.x1, t.y1, t.x2, t.y2, ti0, ti1, tj0, tj1) < 0 ||
          rv_edge_max(t.x2, t.y2, t.x0, t.y0, ti0, ti1, tj0, tj1) < 0 ||
          rv_edge_max(t.x0, t.y0, t.x1, t.y1, ti0, ti1, tj0, tj1) < 0)
        continue;
      const int i = ti0 + li, j = tj0 + lj;
      unsigned z;
      if (i <= ti1 && j <= tj1 && tri_pixel(t, i, j, z)) vis_min(vis, (int64_t)j * W + i, z, T);
    }
  }
}

// floor(sqrt(n)), n < 2^40 (exact in double; the loops correct the last unit)
__device__ __forceinline__ int64_t rv_isqrt(int64_t n) {
  int64_t r = (int64_t)sqrt((double)n);
  while (r * r > n) --r;
  while ((r + 1) * (r + 1) <= n) ++r;
  return r;
}

__device__ __forceinline__ bool rv_near_edge(const int32_t* __restrict__ scr, int64_t a, int64_t b, int px, int py,
                                             int hw) {
  const int ax = scr[3 * a], ay = scr[3 * a + 1], bx = scr[3 * b], by = scr[3 * b + 1];
  int64_t w = rv_edge(ax, ay, bx, by, px, py);
  if (w < 0) w = -w;
  const int64_t dx = bx - ax, dy = by - ay;
  return w <= (int64_t)hw * rv_isqrt(dx * dx + dy * dy);
}

__global__ void __launch_bounds__(TNP_BLOCK)
k_rv_resolve(const unsigned long long* __restrict__ vis, int W, int H, const int64_t* __restrict__ off,
             const int64_t* __restrict__ idx, const int32_t* __restrict__ scr,
             const int32_t* __restrict__ tpoly, int hw, int32_t* __restrict__ prim, int32_t* __restrict__ tri,
             uint8_t* __restrict__ edge, int64_t* __restrict__ ctr) {
  const int64_t at = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  int covered = 0;
  if (at < (int64_t)W * H) {
    const unsigned long long key = vis[at];
    int32_t p = -1, T = -1;
    uint8_t e = 0;
    if (key != RV_BG) {
      covered = 1;
      T = (int32_t)(key & 0xffffffffull);
      p = tpoly[T];
      if (edge) {
        const int64_t base = off[p], deg = off[p + 1] - base, t = T - (base - 2 * p);
        const int64_t a = idx[base], b = idx[base + t + 1], c = idx[base + t + 2];
        const int px = 16 * (int)(at % W) + 8, py = 16 * (int)(at / W) + 8;
        e = rv_near_edge(scr, b, c, px, py, hw) || (t == 0 && rv_near_edge(scr, a, b, px, py, hw)) ||
            (t == deg - 3 && rv_near_edge(scr, c, a, px, py, hw));
      }
    }
    prim[at] = p;
    if (tri) tri[at] = T;
    if (edge) edge[at] = e;
  }
  const int w = tnp::wave_sum(covered);
  if (tnp::lane() == 0 && w) atomicAdd(reinterpret_cast<unsigned long long*>(ctr + RC_COVERED), (unsigned long long)w);
}

struct ShadeArgs {
  float vmin, vmax;
  uint8_t edge_rgba[4];
  int W, H, ss;
  int64_t P;
};

// one thread per output pixel
__global__ void __launch_bounds__(TNP_BLOCK)
k_rv_shade(const int32_t* __restrict__ prim, const uint8_t* __restrict__ edge, const float* __restrict__ value,
           const uint8_t* __restrict__ lut, ShadeArgs g, uint8_t* __restrict__ rgba) {
  const int ow = g.W / g.ss, oh = g.H / g.ss;
  const int64_t o = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  if (o >= (int64_t)ow * oh) return;
  const int oi = (int)(o % ow), oj = (int)(o / ow);
  int sum[4] = {0, 0, 0, 0};
  for (int dj = 0; dj < g.ss; ++dj)
    for (int di = 0; di < g.ss; ++di) {
      const int64_t at = (int64_t)(oj * g.ss + dj) * g.W + (oi * g.ss + di);
      const int64_t p = prim[at];
      if (p < 0 || p >= g.P) continue;  // background
      if (edge && edge[at]) {
#pragma unroll
        for (int k = 0; k < 4; ++k) sum[k] += g.edge_rgba[k];
        continue;
      }
      const float f = __fadd_rn(
          __fmul_rn(__fdiv_rn(__fsub_rn(value[p], g.vmin), __fsub_rn(g.vmax, g.vmin)), 255.f), 0.5f);
      const int k = f >= 0.f ? (int)fminf(floorf(f), 255.f) : 0;  // (a NaN: 0)
      sum[0] += lut[3 * k], sum[1] += lut[3 * k + 1], sum[2] += lut[3 * k + 2], sum[3] += 255;
    }
  const int n = g.ss * g.ss;
  uchar4 out;
  out.x = (uint8_t)((sum[0] + n / 2) / n), out.y = (uint8_t)((sum[1] + n / 2) / n);
  out.z = (uint8_t)((sum[2] + n / 2) / n), out.w = (uint8_t)((sum[3] + n / 2) / n);
  reinterpret_cast<uchar4*>(rgba)[o] = out;
}

int rv_view_check(const tnp_render_view* v, ViewDev* out) {
  if (!v) { tnp_set_error("render: null view"); return -1; }
  if (v->width < 1 || v->width > RV_MAX_DIM) {
    tnp_set_error("render: width = %d is outside [1, %d]", (int)v->width, RV_MAX_DIM);
    return -1;
  }
  if (v->height < 1 || v->height > RV_MAX_DIM) {
    tnp_set_error("render: height = %d is outside [1, %d]", (int)v->height, RV_MAX_DIM);
    return -1;
  }
  if (!(v->depth_half > 0.f) || !(v->persp_dist >= 0.f) || !(v->scale == v->scale)) {
    tnp_set_error("render: depth_half = %g (must be > 0), persp_dist = %g (must be >= 0), scale = %g",
                  (double)v->depth_half, (double)v->persp_dist, (double)v->scale);
    return -1;
  }
  memcpy(out->right, v->right, sizeof(out->right));
  memcpy(out->up, v->up, sizeof(out->up));
  memcpy(out->toward, v->toward, sizeof(out->toward));
  memcpy(out->center, v->center, sizeof(out->center));
  out->scale = v->scale, out->D = v->persp_dist, out->h = v->depth_half;
  out->half_w = 0.5f * (float)v->width, out->half_h = 0.5f * (float)v->height;
  return 0;
}

}  // namespace

extern "C" int tnp_debug_render_path(int mode) {
  if (mode < 0 || mode > 2) return -1;
  const int was = g_path_mode;
  g_path_mode = mode;
  return was;
}

extern "C" int tnp_render_raster(const float* d_xyz, int64_t V, const int64_t* d_offsets, const int64_t* d_indices,
                                 int64_t P, const tnp_render_view* view, int32_t edge_half_width, int32_t* d_screen,
                                 int32_t* d_prim, int32_t* d_tri, uint8_t* d_edge, tnp_render_stats* h_stats,
                                 void* stream) {
  const char* who = "render";
  hipStream_t s = (hipStream_t)stream;
  if (!h_stats) { tnp_set_error("render: null stats"); return -1; }
  *h_stats = tnp_render_stats{};
  ViewDev vw;
  if (rv_view_check(view, &vw)) return -1;
  if (edge_half_width < 0 || edge_half_width > 256) {
    tnp_set_error("render: edge_half_width = %d is outside [0, 256]", (int)edge_half_width);
    return -1;
  }
  if (soup_args(who, V, P, true, true, d_xyz, d_offsets, d_indices)) return -1;
  if (!d_prim) { tnp_set_error("render: null array"); return -1; }
  const int W = view->width, H = view->height;
  const int64_t npix = (int64_t)W * H;
  Scratch scr(s, who);
  int32_t* screen = d_screen;
  if (!screen && V > 0) screen = scr.arr<int32_t>(V * 3);
  if (V > 0) {
    if (!screen) return -1;
    SOUP_LAUNCH(k_rv_project, V, d_xyz, V, vw, screen);
  }
  if (P == 0) {
    const FillOp ops[3] = {{d_prim, (uint64_t)npix * 4, 0xFFu}, {d_tri, d_tri ? (uint64_t)npix * 4 : 0, 0xFFu},
                           {d_edge, d_edge ? (uint64_t)npix : 0, 0u}};
    if (launch_fill(ops, 3, s)) return -1;
    TNP_CHECK(hipStreamSynchronize(s));
    return 0;
  }

  int64_t* ctr = nullptr;
  const int64_t n = soup_offsets(who, scr, d_offsets, d_indices, V, P, &ctr, RC_N, s);
  if (n < 0) return -1;
  const int64_t nT = n - 2 * P;  // >= P
  if (nT >= (int64_t)1 << 31) {
    tnp_set_error("render: %lld fan triangles; triangle numbers are held below 2^31", (long long)nT);
    return -1;
  }
  SOUP_LAUNCH(k_rv_ids, n, d_offsets, P, d_indices, n, V, ctr);
  // (independent of the ids: queued behind the check, ahead of its verdict)
  const int64_t lb_words = scan_tiles(nT) + 1;
  uint64_t* lbuf = scr.arr<uint64_t>(lb_words);
  unsigned long long* vis = scr.arr<unsigned long long>(npix);
  if (!lbuf || !vis) return -1;
  TNP_CHECK(hipMemsetAsync(lbuf, 0, (size_t)lb_words * sizeof(uint64_t), s));
  const FillOp clear = {vis, (uint64_t)npix * sizeof(unsigned long long), 0xFFu};
  if (launch_fill(&clear, 1, s)) return -1;
  int64_t h[RC_N];
  if (soup_verdict(who, d_offsets, d_indices, V, ctr, h, 1, s)) return -1;

  // every id is now known to lie in [0, V): from here on ids are followed
  int32_t* tpoly = scr.arr<int32_t>(nT);
  int32_t* islarge = scr.arr<int32_t>(nT);
  int64_t* loff = scr.arr<int64_t>(nT);
  int32_t* list = scr.arr<int32_t>(nT);
  uint8_t* pflag = scr.arr<uint8_t>(P);
  if (!tpoly || !islarge || !loff || !list || !pflag) return -1;
  SOUP_LAUNCH(k_rv_fan, P, d_offsets, d_indices, P, screen, tpoly, pflag, ctr);
  SOUP_LAUNCH(k_rv_small, nT, d_offsets, d_indices, nT, screen, tpoly, pflag, W, H, g_path_mode, vis, islarge);
  if (scan_i32_to_i64(islarge, loff, nT, ctr + RC_LARGE, scan_lb(lbuf), s)) return -1;
  SOUP_LAUNCH(k_rv_compact, nT, islarge, loff, nT, list);
  hipLaunchKernelGGL(k_rv_large, dim3(RV_LARGE_GRID), dim3(TNP_BLOCK), 0, s, d_offsets, d_indices, screen, tpoly, list,
                     ctr, W, H, vis);
  SOUP_LAUNCH(k_rv_resolve, npix, vis, W, H, d_offsets, d_indices, screen, tpoly, (int)edge_half_width, d_prim, d_tri,
              d_edge, ctr);
  TNP_CHECK(hipMemcpyAsync(h, ctr, sizeof(h), hipMemcpyDeviceToHost, s));
  TNP_CHECK(hipStreamSynchronize(s));
  h_stats->n_polygons = P;
  h_stats->n_dropped = h[RC_DROPPED];
  h_stats->n_degenerate = h[RC_DEGEN];
  h_stats->n_drawn = P - h[RC_DROPPED] - h[RC_DEGEN];
  h_stats->n_triangles = nT;
  h_stats->n_large = h[RC_LARGE];
  h_stats->pixels_covered = h[RC_COVERED];
  return 0;
}

extern "C" int tnp_render_shade(const int32_t* d_prim, const uint8_t* d_edge, int32_t width, int32_t height,
                                const float* d_value, int64_t P, float vmin, float vmax, const uint8_t* d_lut,
                                const uint8_t* edge_rgba, int32_t ss, uint8_t* d_rgba, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (width < 1 || width > RV_MAX_DIM || height < 1 || height > RV_MAX_DIM) {
    tnp_set_error("render_shade: raster %d x %d is outside [1, %d]", (int)width, (int)height, RV_MAX_DIM);
    return -1;
  }
  if ((ss != 1 && ss != 2 && ss != 4) || width % ss || height % ss) {
    tnp_set_error("render_shade: ss = %d must be 1, 2 or 4 and divide the raster %d x %d", (int)ss, (int)width,
                  (int)height);
    return -1;
  }
  if (!(vmax > vmin)) {
    tnp_set_error("render_shade: vmin = %g, vmax = %g (vmax must be larger)", (double)vmin, (double)vmax);
    return -1;
  }
  if (P < 0 || !d_prim || !d_lut || !edge_rgba || !d_rgba || (P > 0 && !d_value)) {
    tnp_set_error("render_shade: null array");
    return -1;
  }
  ShadeArgs g;
  g.vmin = vmin, g.vmax = vmax, g.W = width, g.H = height, g.ss = ss, g.P = P;
  memcpy(g.edge_rgba, edge_rgba, 4);
  hipLaunchKernelGGL(k_rv_shade, dim3(tnp_grid((int64_t)(width / ss) * (height / ss))), dim3(TNP_BLOCK), 0, s, d_prim,
                     d_edge, d_value, d_lut, g, d_rgba);
  TNP_CHECK(hipGetLastError());
  return 0;
}
