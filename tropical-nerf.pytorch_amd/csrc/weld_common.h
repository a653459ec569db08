// What tnp_weld_build (weld.hip) and tnp_simplify_build (simplify.hip) share
// beyond topo_common.h: both merge the used vertices of a polygon soup into
// classes with a smallest-id representative (root[v]) and then do the same
// three things with them, so each rule exists once --
//   the used vertices: k_weld_ids, k_weld_box (the finite check, the box)
//   the class means:   class_means (the (representative, id) sort, the
//                      segmented double sums of topo_common.h, k_weld_mean)
//   the drift:         k_weld_shift
//   the rewrite:       Rewrite::count / Rewrite::fill (k_weld_keep ...
//                      k_weld_pinched): every id mapped, a position kept iff
//                      its mapped id differs from its cyclic predecessor's, a
//                      polygon of fewer than 3 kept positions dropped, the
//                      pinched survivors counted
// Included by those two files only (anonymous namespace).
#pragma once
#include <string.h>

#include "topo_common.h"

namespace {

// the counters the rewrite owns (int64 words, zero before), with the drift's
// word in front so that one readback brings all five
enum { RW_SHIFT, RW_KEPT, RW_NPOLY, RW_NIDX, RW_PINCHED, RW_N };

// fp32 <-> uint32 keeping the order (-0 below +0, which no caller tells apart)
__device__ __forceinline__ uint32_t f2ord(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
inline float ord2f(uint32_t o) {
  const uint32_t u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
  float f;
  memcpy(&f, &u, sizeof f);
  return f;
}

__device__ __forceinline__ void count_lanes(bool f, int64_t* word) {
  const uint64_t m = __ballot(f);
  if (tnp::lane() == 0 && m) atomicAdd(reinterpret_cast<unsigned long long*>(word), (unsigned long long)__popcll(m));
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long y = __shfl_xor(v, o, 64);
    v = y > v ? y : v;
  }
  return v;
}

// the squared distance of the definitions: fp32 -> double, every product and
// sum rounded once, left to right
__device__ __forceinline__ double dist2(const float* __restrict__ a, const float* __restrict__ b) {
  const double dx = __dsub_rn((double)a[0], (double)b[0]);
  const double dy = __dsub_rn((double)a[1], (double)b[1]);
  const double dz = __dsub_rn((double)a[2], (double)b[2]);
  return __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
}

__global__ void __launch_bounds__(TNP_BLOCK)
k_weld_ids(const int64_t* __restrict__ off, int64_t P, const int64_t* __restrict__ idx, int64_t n, int64_t V,
           int64_t* __restrict__ ctr, int32_t* __restrict__ used) {
  const int64_t i = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  if (i >= n) return;
  int64_t a, b;
  bool b_ok;
  if (soup_check_id(off, P, idx, i, V, ctr, a, b, b_ok)) used[a] = 1;
}

// per used vertex: the smallest id with a coordinate that is not finite ->
// *bad (all ones before); the box of the finite ones as ordered integers ->
// lo[3] (all ones before), hi[3] (zero before); one atomic per wave and bound
__global__ void __launch_bounds__(TNP_BLOCK)
k_weld_box(const float* __restrict__ xyz, const int32_t* __restrict__ used, int64_t V, int64_t* __restrict__ lo3,
           int64_t* __restrict__ hi3, int64_t* __restrict__ bad1) {
  const int64_t v = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  const bool on = v < V && used[v];
  unsigned long long lo[3] = {~0ull, ~0ull, ~0ull}, hi[3] = {0ull, 0ull, 0ull}, bad = ~0ull;
  if (on) {
    const float* p = xyz + 3 * v;
    if (isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2])) {
#pragma unroll
      for (int q = 0; q < 3; ++q) lo[q] = hi[q] = f2ord(p[q]);
    } else {
      bad = (unsigned long long)v;
    }
  }
  if (!__ballot(on)) return;  // (a whole wave)
  unsigned long long* wl = reinterpret_cast<unsigned long long*>(lo3);
  unsigned long long* wh = reinterpret_cast<unsigned long long*>(hi3);
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const unsigned long long h = wave_max_u64(hi[q]), l = ~wave_max_u64(~lo[q]);
    if (tnp::lane() == 0 && l <= h) {
      atomicMin(wl + q, l);
      atomicMax(wh + q, h);
    }
  }
  bad = ~wave_max_u64(~bad);
  if (tnp::lane() == 0 && bad != ~0ull) atomicMin(reinterpret_cast<unsigned long long*>(bad1), bad);
}

// every member takes its representative's bits; an unused vertex is its own
// representative
__global__ void __launch_bounds__(TNP_BLOCK)
k_weld_first(const float* __restrict__ xyz, const int32_t* __restrict__ root, int64_t V, float* __restrict__ out) {
  const int64_t v = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  if (v >= V) return;
  const float* p = xyz + 3 * (int64_t)root[v];
#pragma unroll
  for (int q = 0; q < 3; ++q) out[3 * v + q] = p[q];
}

__global__ void __launch_bounds__(TNP_BLOCK)
k_weld_mkeys(const int32_t* __restrict__ used, const int64_t* __restrict__ urank, const int32_t* __restrict__ root,
             int64_t V, int64_t U, int shift, uint64_t* __restrict__ keys) {
  const int64_t v = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  if (v >= V || !used[v]) return;
  const int64_t j = urank[v];
  if (j < U) keys[j] = ((uint64_t)root[v] << shift) | (uint64_t)v;
}

// sorted (representative, id) keys: a class starts at its representative
__global__ void __launch_bounds__(TNP_BLOCK)
k_weld_heads(const uint64_t* __restrict__ sk, int64_t U, int shift, int32_t* __restrict__ head) {
  const int64_t j = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  if (j < U) head[j] = (sk[j] >> shift) == (sk[j] & (((uint64_t)1 << shift) - 1));
}

// start[c] of class c (in ascending representative), seg[representative] = c;
// thread 0 closes the starts
__global__ void __launch_bounds__(TNP_BLOCK)
k_weld_starts(const uint64_t* __restrict__ sk, const int32_t* __restrict__ head, const int64_t* __restrict__ hrank,
              int64_t U, int64_t nseg, int shift, int64_t* __restrict__ start, int32_t* __restrict__ seg) {
  const int64_t j = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  if (j == 0) start[nseg] = U;
  if (j >= U || !head[j]) return;
  const int64_t c = hrank[j];
  if (c >= nseg) return;
  start[c] = j;
  seg[sk[j] >> shift] = (int32_t)c;
}

struct VertXYZ {  // the coordinates of vertex v
  const float* xyz;
  __device__ __forceinline__ void operator()(uint64_t v, double* out) const {
    const float* q = xyz + 3 * v;
    out[0] = (double)q[0], out[1] = (double)q[1], out[2] = (double)q[2];
  }
};

// a class of one (an unused vertex too) keeps its bits
__global__ void __launch_bounds__(TNP_BLOCK)
k_weld_mean(const float* __restrict__ xyz, const int32_t* __restrict__ used, const int32_t* __restrict__ root,
            const int* __restrict__ csize, const int32_t* __restrict__ seg, const double* __restrict__ sums,
            int64_t nseg, int64_t V, float* __restrict__ out) {
  const int64_t v = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  if (v >= V) return;
  const int r = root[v];
  const int m = used[v] ? csize[r] : 1;
  const int64_t c = m >= 2 ? seg[r] : 0;
#pragma unroll
  for (int q = 0; q < 3; ++q)
    out[3 * v + q] = (m >= 2 && c < nseg) ? (float)(sums[(int64_t)q * nseg + c] / (double)m) : xyz[3 * v + q];
}

// the largest fp32(sqrt(d2(input, output))) over the used vertices -> *word
// (zero before), an integer maximum over the bit patterns
__global__ void __launch_bounds__(TNP_BLOCK)
k_weld_shift(const float* __restrict__ xyz, const float* __restrict__ out, const int32_t* __restrict__ used, int64_t V,
             int64_t* __restrict__ word) {
  const int64_t v = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  unsigned long long b = 0;
  if (v < V && used[v]) b = __float_as_uint((float)__dsqrt_rn(dist2(xyz + 3 * v, out + 3 * v)));
  b = wave_max_u64(b);
  if (tnp::lane() == 0 && b) atomicMax(reinterpret_cast<unsigned long long*>(word), b);
}

// The class means: out[v] of every member of a class of m >= 2 (csize[root],
// nseg classes in all) is the mean of the class's fp32 coordinates, summed in
// double in the topology's fixed shape over the used vertices in
// (representative, id) order, divided by m once and rounded to fp32 once; any
// other vertex keeps its bits.  nseg_word: a device word the heads' count goes
// to (not read here).
inline int class_means(Scratch& scr, const float* xyz, const int32_t* used, const int64_t* urank, const int32_t* root,
                       const int* csize, int64_t V, int64_t U, int64_t nseg, int64_t* nseg_word, float* out,
                       hipStream_t s) {
  const int shift = bits_for(V), key_bits = 2 * shift;
  const size_t sort_bytes = sort_scratch_bytes(U, key_bits);
  {
    const size_t need = 2 * Scratch::pad(U * sizeof(uint64_t)) + Scratch::pad(sort_bytes) +
                        Scratch::pad(U * sizeof(int32_t)) + Scratch::pad(U * sizeof(int64_t)) +
                        Scratch::pad(((size_t)scan_tiles(U) + 1) * sizeof(uint64_t)) +
                        Scratch::pad((nseg + 1) * sizeof(int64_t)) + Scratch::pad(V * sizeof(int32_t)) +
                        Scratch::pad(3 * U * sizeof(double)) + Scratch::pad(3 * nseg * sizeof(double));
    if (!scr.reserve(need)) return -1;
  }
  uint64_t* ka = scr.arr<uint64_t>(U);
  uint64_t* kb = scr.arr<uint64_t>(U);
  void* sort_scr = scr.get(sort_bytes);
  int32_t* head = scr.arr<int32_t>(U);
  int64_t* hrank = scr.arr<int64_t>(U);
  int64_t* start = scr.arr<int64_t>(nseg + 1);
  int32_t* seg = scr.arr<int32_t>(V);
  double* pieces = scr.arr<double>(3 * U);
  double* sums = scr.arr<double>(3 * nseg);
  if (!ka || !kb || !sort_scr || !head || !hrank || !start || !seg || !pieces || !sums) return -1;
  uint64_t* sk = nullptr;
  SOUP_LAUNCH(k_weld_mkeys, V, used, urank, root, V, U, shift, ka);
  if (sort_keys_u64(ka, kb, U, key_bits, sort_scr, sort_bytes, &sk, s)) return -1;
  SOUP_LAUNCH(k_weld_heads, U, sk, U, shift, head);
  if (scan_flags(scr, head, U, hrank, nseg_word, s)) return -1;
  // (a start the heads do not reach stays inside the pieces)
  TNP_CHECK(hipMemsetAsync(start, 0, (size_t)(nseg + 1) * sizeof(int64_t), s));
  SOUP_LAUNCH(k_weld_starts, U, sk, head, hrank, U, nseg, shift, start, seg);
  hipLaunchKernelGGL((k_seg_pieces<3, VertXYZ>), dim3(tnp_grid(U, SEG)), dim3(TNP_BLOCK), 0, s, sk, U, shift,
                     VertXYZ{xyz}, pieces);
  hipLaunchKernelGGL(k_seg_final<3>, dim3(tnp_grid(nseg, TNP_WAVES)), dim3(TNP_BLOCK), 0, s, start, nseg, U, pieces,
                     sums);
  TNP_CHECK(hipGetLastError());
  SOUP_LAUNCH(k_weld_mean, V, xyz, used, root, csize, seg, sums, nseg, V, out);
  return 0;
}

// keep[i]: the mapped id at i differs from its cyclic predecessor's; keep[n] = 0
__global__ void __launch_bounds__(TNP_BLOCK)
k_weld_keep(const int64_t* __restrict__ off, int64_t P, const int64_t* __restrict__ idx, int64_t n,
            const int32_t* __restrict__ root, int32_t* __restrict__ keep) {
  const int64_t i = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  if (i > n) return;
  if (i == n) { keep[n] = 0; return; }
  const int64_t p = soup_polygon_of(off, P, i);
  const int64_t j = i == off[p] ? off[p + 1] - 1 : i - 1;
  keep[i] = root[idx[i]] != root[idx[j]];
}

__global__ void __launch_bounds__(TNP_BLOCK)
k_weld_degrees(const int64_t* __restrict__ off, int64_t P, const int64_t* __restrict__ krank,
               int32_t* __restrict__ pkeep, int32_t* __restrict__ pdeg) {
  const int64_t p = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  if (p >= P) return;
  const int64_t d = krank[off[p + 1]] - krank[off[p]];
  pkeep[p] = d >= 3;
  pdeg[p] = d >= 3 ? (int32_t)d : 0;
}

// thread 0 closes the offsets (no survivor included)
__global__ void __launch_bounds__(TNP_BLOCK)
k_weld_rows(int64_t P, const int32_t* __restrict__ pkeep, const int64_t* __restrict__ prank,
            const int64_t* __restrict__ poff, int64_t P2, int64_t N2, int64_t* __restrict__ out_off,
            int64_t* __restrict__ source) {
  const int64_t p = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  if (p == 0) out_off[P2] = N2;
  if (p >= P || !pkeep[p]) return;
  const int64_t k = prank[p];
  if (k >= P2) return;
  out_off[k] = poff[p];
  source[k] = p;
}

__global__ void __launch_bounds__(TNP_BLOCK)
k_weld_scatter(const int64_t* __restrict__ off, int64_t P, const int64_t* __restrict__ idx, int64_t n,
               const int32_t* __restrict__ root, const int32_t* __restrict__ keep, const int64_t* __restrict__ krank,
               const int32_t* __restrict__ pkeep, const int64_t* __restrict__ poff, int64_t N2,
               int64_t* __restrict__ out_idx) {
  const int64_t i = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  if (i >= n || !keep[i]) return;
  const int64_t p = soup_polygon_of(off, P, i);
  if (!pkeep[p]) return;
  const int64_t at = poff[p] + (krank[i] - krank[off[p]]);
  if (at < N2) out_idx[at] = root[idx[i]];
}

// an output polygon is pinched when an id occurs twice in it: position t looks
// for its id further on, and the first finder of a polygon sets its flag and
// counts it
__global__ void __launch_bounds__(TNP_BLOCK)
k_weld_pinched(const int64_t* __restrict__ out_off, int64_t P2, const int64_t* __restrict__ out_idx, int64_t N2,
               int* __restrict__ pinched, int64_t* __restrict__ word) {
  const int64_t t = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  bool first = false;
  if (t < N2) {
    const int64_t p = soup_polygon_of(out_off, P2, t), e = out_off[p + 1], a = out_idx[t];
    bool dup = false;
    for (int64_t u = t + 1; u < e && !dup; ++u) dup = out_idx[u] == a;
    first = dup && atomicExch(pinched + p, 1) == 0;
  }
  count_lanes(first, word);
}

// The rewrite of the soup (off, idx; n ids, P polygons) over root[], in two
// halves around the caller's readback of rw (RW_N device words): count queues
// the keep flags, the new degrees and their scans; with P2 = rw[RW_NPOLY] and
// N2 = rw[RW_NIDX] read back and checked by sane(), the caller allocates
// offsets [P2 + 1], indices [N2], source [P2] and fill writes them, with the
// pinched flags of the survivors (scratch, [P2]) and their count in
// rw[RW_PINCHED].
struct Rewrite {
  const int64_t *off, *idx;
  int64_t n, P;
  const int32_t* root;
  int64_t* rw;
  int32_t *keep = nullptr, *pkeep = nullptr, *pdeg = nullptr;
  int64_t *krank = nullptr, *prank = nullptr, *poff = nullptr;
  int* pinched = nullptr;

  static size_t bytes(int64_t n, int64_t P) {
    return Scratch::pad((n + 1) * sizeof(int32_t)) + Scratch::pad((n + 1) * sizeof(int64_t)) +
           2 * Scratch::pad(P * sizeof(int32_t)) + 2 * Scratch::pad(P * sizeof(int64_t)) +
           Scratch::pad(((size_t)scan_tiles(n + 1) + 1) * sizeof(uint64_t)) +
           2 * Scratch::pad(((size_t)scan_tiles(P) + 1) * sizeof(uint64_t));
  }
  int count(Scratch& scr, hipStream_t s) {
    keep = scr.arr<int32_t>(n + 1);
    krank = scr.arr<int64_t>(n + 1);
    pkeep = scr.arr<int32_t>(P);
    pdeg = scr.arr<int32_t>(P);
    prank = scr.arr<int64_t>(P);
    poff = scr.arr<int64_t>(P);
    if (!keep || !krank || !pkeep || !pdeg || !prank || !poff) return -1;
    SOUP_LAUNCH(k_weld_keep, n + 1, off, P, idx, n, root, keep);
    if (scan_flags(scr, keep, n + 1, krank, rw + RW_KEPT, s)) return -1;
    SOUP_LAUNCH(k_weld_degrees, P, off, P, krank, pkeep, pdeg);
    if (scan_flags(scr, pkeep, P, prank, rw + RW_NPOLY, s)) return -1;
    return scan_flags(scr, pdeg, P, poff, rw + RW_NIDX, s);
  }
  // h: the RW_N words as read back
  int sane(const char* who, const int64_t* h) const {
    const int64_t P2 = h[RW_NPOLY], N2 = h[RW_NIDX];
    if (P2 < 0 || P2 > P || N2 < 3 * P2 || N2 > h[RW_KEPT] || h[RW_KEPT] > n) {
      tnp_set_error("%s: %lld polygons of %lld kept with %lld ids of %lld", who, (long long)P2, (long long)P,
                    (long long)N2, (long long)n);
      return -1;
    }
    return 0;
  }
  int fill(Scratch& scr, int64_t P2, int64_t N2, int64_t* out_off, int64_t* out_idx, int64_t* out_src,
           hipStream_t s) {
    SOUP_LAUNCH(k_weld_rows, P, P, pkeep, prank, poff, P2, N2, out_off, out_src);
    if (P2 > 0) {
      pinched = scr.arr<int>(P2);
      if (!pinched) return -1;
      TNP_CHECK(hipMemsetAsync(pinched, 0, (size_t)P2 * sizeof(int), s));
      // (a position the scatter does not reach stays a valid id)
      TNP_CHECK(hipMemsetAsync(out_idx, 0, (size_t)N2 * sizeof(int64_t), s));
      SOUP_LAUNCH(k_weld_scatter, n, off, P, idx, n, root, keep, krank, pkeep, poff, N2, out_idx);
      SOUP_LAUNCH(k_weld_pinched, N2, out_off, P2, out_idx, N2, pinched, rw + RW_PINCHED);
    }
    return 0;
  }
};

}  // namespace
