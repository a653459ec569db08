// The checks every entry point that takes a polygon soup (d_offsets int64
// [P + 1], d_indices int64) makes on the device before anything is read
// through an id, and the edge keys three of them build in the same pass --
// tnp_polygon_report (polygons.hip), tnp_render_raster (render.hip),
// tnp_topology_build (topology.hip), tnp_holes_build (holes.hip),
// tnp_weld_build (weld.hip) and tnp_simplify_build (simplify.hip) share them, so all refuse the same input and name the same first offender.  The
// host side around these kernels is soup_host.h's.
//
// ctr[SOUP_ERR]: the error word, (position << 3) | code under atomicMin, so
// the smallest position wins; SOUP_NONE: no error.  ctr[SOUP_NIDX] = off[P].
#pragma once
#include "kernels.h"

namespace {

enum { SOUP_ERR = 0, SOUP_NIDX = 1 };
enum { SE_OFF0, SE_DECR, SE_SHORT, SE_LONG, SE_ID, SE_EQUAL };
constexpr unsigned long long SOUP_NONE = ~0ull;

__device__ __forceinline__ void soup_fail(int64_t* ctr, int64_t at, int code) {
  atomicMin(reinterpret_cast<unsigned long long*>(ctr + SOUP_ERR), ((unsigned long long)at << 3) | (unsigned)code);
}

// per polygon: offsets[0] == 0, no decrease, 3 <= degree < 2^31; deg[p] (0 for
// a refused polygon) when deg is given
__global__ void __launch_bounds__(TNP_BLOCK)
k_soup_offsets(const int64_t* __restrict__ off, int64_t P, int64_t* __restrict__ ctr, int32_t* __restrict__ deg) {
  const int64_t p = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  if (p == 0) {
    if (off[0] != 0) soup_fail(ctr, 0, SE_OFF0);
    ctr[SOUP_NIDX] = off[P];
  }
  if (p >= P) return;
  const int64_t a = off[p], b = off[p + 1];
  int d = 0;
  if (b < a) soup_fail(ctr, p, SE_DECR);
  else if (b - a < 3) soup_fail(ctr, p, SE_SHORT);
  else if (b - a > 0x7fffffff) soup_fail(ctr, p, SE_LONG);
  else d = (int)(b - a);
  if (deg) deg[p] = d;
}

// the polygon of index position i: the last p in [0, P) with off[p] <= i
// (checked offsets: off[0] == 0, increasing, off[P] > i)
__device__ __forceinline__ int64_t soup_polygon_of(const int64_t* __restrict__ off, int64_t P, int64_t i) {
  int64_t lo = 0, hi = P;
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (off[mid] <= i) lo = mid;
    else hi = mid;
  }
  return lo;
}

// index position i (checked offsets): a = idx[i] must lie in [0, V) and differ
// from b, the next id of its polygon (cyclic).  Nothing is loaded through an
// id.  Returns true when a is valid; b_ok: b lies in [0, V) (b is reported by
// its own thread).
__device__ __forceinline__ bool soup_check_id(const int64_t* __restrict__ off, int64_t P,
                                              const int64_t* __restrict__ idx, int64_t i, int64_t V,
                                              int64_t* __restrict__ ctr, int64_t& a, int64_t& b, bool& b_ok) {
  const int64_t p = soup_polygon_of(off, P, i);
  const int64_t j = i + 1 == off[p + 1] ? off[p] : i + 1;
  a = idx[i], b = idx[j];
  b_ok = b >= 0 && b < V;
  if (a < 0 || a >= V) {
    soup_fail(ctr, i, SE_ID);
    return false;
  }
  if (a == b) soup_fail(ctr, i, SE_EQUAL);
  return true;
}

// one key per index position i: the edge from idx[i] to the next id of its
// polygon (cyclic), (min << 32) | (max << 1) | (from > to); 0 after a failed
// check.  USED: used[a] = 1 for every valid id; POL: pol[i] = the polygon of
// position i.  Stores only -- nothing is loaded through an id.
template <bool USED, bool POL>
__global__ void __launch_bounds__(TNP_BLOCK)
k_soup_edges(const int64_t* __restrict__ off, int64_t P, const int64_t* __restrict__ idx, int64_t n, int64_t V,
             int64_t* __restrict__ ctr, uint64_t* __restrict__ keys, uint8_t* __restrict__ used,
             int32_t* __restrict__ pol) {
  const int64_t i = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  if (i >= n) return;
  int64_t a, b;
  bool b_ok;
  uint64_t key = 0;
  if (soup_check_id(off, P, idx, i, V, ctr, a, b, b_ok)) {
    if (USED) used[a] = 1;
    if (b_ok) {
      const uint64_t lo = (uint64_t)(a < b ? a : b), hi = (uint64_t)(a < b ? b : a);
      key = (lo << 32) | (hi << 1) | (a > b ? 1u : 0u);
    }
  }
  keys[i] = key;
  if (POL) pol[i] = (int32_t)soup_polygon_of(off, P, i);
}

// the failed check of error word w as tnp_last_error(), prefixed `who`; the
// offending values are read back from positions the checks have shown to be
// inside the arrays.  Returns -1.
inline int soup_report_error(const char* who, unsigned long long w, const int64_t* d_off, const int64_t* d_idx,
                             int64_t V, hipStream_t s) {
  const long long at = (long long)(w >> 3);
  const int code = (int)(w & 7);
  int64_t v[2] = {0, 0};
  if (code <= SE_LONG)
    TNP_CHECK(hipMemcpyAsync(v, d_off + at, (code == SE_OFF0 ? 1 : 2) * sizeof(int64_t), hipMemcpyDeviceToHost, s));
  else
    TNP_CHECK(hipMemcpyAsync(v, d_idx + at, sizeof(int64_t), hipMemcpyDeviceToHost, s));
  TNP_CHECK(hipStreamSynchronize(s));
  switch (code) {
    case SE_OFF0: tnp_set_error("%s: offsets[0] = %lld, not 0", who, (long long)v[0]); break;
    case SE_DECR:
      tnp_set_error("%s: offsets decrease at polygon %lld (offsets[%lld] = %lld > offsets[%lld] = %lld)", who, at, at,
                    (long long)v[0], at + 1, (long long)v[1]);
      break;
    case SE_SHORT:
      tnp_set_error("%s: polygon %lld has %lld ids, fewer than 3", who, at, (long long)(v[1] - v[0]));
      break;
    case SE_LONG:
      tnp_set_error("%s: polygon %lld has %lld ids, more than 2^31 - 1", who, at, (long long)(v[1] - v[0]));
      break;
    case SE_ID:
      tnp_set_error("%s: indices[%lld] = %lld is outside [0, %lld)", who, at, (long long)v[0], (long long)V);
      break;
    default:
      tnp_set_error("%s: indices[%lld] = %lld and the next id of its polygon are equal", who, at, (long long)v[0]);
  }
  return -1;
}

}  // namespace
