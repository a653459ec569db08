// What tnp_topology_build (topology.hip), tnp_holes_build (holes.hip) and
// tnp_weld_build (weld.hip; tnp_simplify_build through weld_common.h) share beyond soup_host.h: the lock-free union-find,
// the per-class wave reductions, the boundary graph's classes (one union per
// edge used once, the root flags and their scan) and the segmented double
// sums.  Included by those files only (anonymous namespace).
#pragma once
#include "kernels.h"
#include "soup_host.h"
#include "step.h"

namespace {

// counter block (int64 words); the first two are soup_check.h's
enum { TC_ERR, TC_NIDX, TC_C, TC_L, TC_B, TC_N };
static_assert(TC_ERR == SOUP_ERR && TC_NIDX == SOUP_NIDX, "counter layout");
constexpr int SEG = TNP_BLOCK;  // positions per piece block of the segmented sums

__device__ __forceinline__ int ld_i32(const int* p) {
  return __hip_atomic_load(const_cast<int*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Union-find over ids [0, n): parent[x] <= x always (a root is only ever
// hooked under a smaller root), so every chain ends and a root is the
// smallest member of its class.
// find with path halving: a non-root's parent is replaced by its grandparent.
// Any ancestor is a valid parent and a non-root never becomes a root again,
// so the plain relaxed stores race harmlessly with each other and cannot
// collide with a hook (the CAS below expects parent[x] == x).
__device__ __forceinline__ int uf_find(int* parent, int x) {
  while (true) {
    const int p = ld_i32(parent + x);
    if (p == x) return x;
    const int g = ld_i32(parent + p);
    if (g == p) return p;
    __hip_atomic_store(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    x = g;
  }
}

// hook the larger root under the smaller; a lost race (the larger is no
// longer a root) is retried from its new root -- no thread waits for another
__device__ __forceinline__ void uf_union(int* parent, int a, int b) {
  a = uf_find(parent, a);
  b = uf_find(parent, b);
  while (a != b) {
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = atomicCAS(parent + a, a, b);
    if (old == a) return;
    a = uf_find(parent, old);
    b = uf_find(parent, b);
  }
}

// Integer adds into per-class counters.  The active lanes of a wave are taken
// class by class: f(in, c0, leader) runs once per distinct class c0 among
// them, `in` marking its lanes, and reduces over them before one lane issues
// the atomic.  One giant component is the common case: one round and one
// atomic per wave, where every lane would otherwise hit the same word; a wave
// that also holds a few floaters takes a round for each.  The loop is
// wave-uniform; every lane of the wave must call it.
template <class F>
__device__ __forceinline__ void wave_classes(bool active, int c, F&& f) {
  uint64_t todo = __ballot(active);
  while (todo) {
    const int leader = __builtin_ctzll(todo);
    const int c0 = __shfl(c, leader, 64);
    const bool in = active && c == c0;
    f(in, c0, leader);
    todo &= ~__ballot(in);
  }
}
__device__ __forceinline__ void class_add(bool in, int leader, int64_t* row, int c0, int64_t v) {
  const int64_t s = tnp::wave_sum(in ? v : (int64_t)0);
  if (tnp::lane() == leader && s)
    atomicAdd(reinterpret_cast<unsigned long long*>(row + c0), (unsigned long long)s);
}

__global__ void __launch_bounds__(TNP_BLOCK) k_iota(int* __restrict__ a, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  if (i < n) a[i] = (int)i;
}

// sorted keys: position i is an edge used exactly once
__device__ __forceinline__ bool lone_run(const uint64_t* __restrict__ sk, int64_t n, int64_t i) {
  const uint64_t x = sk[i] >> 1;
  return (i == 0 || (sk[i - 1] >> 1) != x) && (i + 1 == n || (sk[i + 1] >> 1) != x);
}

// one union per boundary edge; bdeg[v]: boundary edges at v; their number -> ctr[TC_B]
__global__ void __launch_bounds__(TNP_BLOCK)
k_boundary_union(const uint64_t* __restrict__ sk, int64_t n, int* vparent, int* __restrict__ bdeg,
                 int64_t* __restrict__ ctr) {
  const int64_t i = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  const bool lone = i < n && lone_run(sk, n, i);
  if (lone) {
    const int a = (int)(sk[i] >> 32), b = (int)((sk[i] >> 1) & 0x7fffffffu);
    uf_union(vparent, a, b);
    atomicAdd(bdeg + a, 1);
    atomicAdd(bdeg + b, 1);
  }
  const uint64_t m = __ballot(lone);
  if (tnp::lane() == 0 && m)
    atomicAdd(reinterpret_cast<unsigned long long*>(ctr + TC_B), (unsigned long long)__popcll(m));
}

// flag[i] = i is a root (and, with deg, carries at least one boundary edge)
__global__ void __launch_bounds__(TNP_BLOCK)
k_flag_roots(const int* __restrict__ parent, const int* __restrict__ deg, int64_t n, int32_t* __restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  if (i < n) flag[i] = parent[i] == (int)i && (!deg || deg[i] > 0);
}

// Segmented double sums, first level: the sorted positions in blocks of SEG.
// A piece is a maximal run of one class inside a block; its sum is stored at
// the position of its first member.  A block of one class and SEG members is
// summed by the fixed xor tree, any other piece left to right by its first
// thread: the shape depends on the keys alone.
template <int NV, class F>
__global__ void __launch_bounds__(TNP_BLOCK)
k_seg_pieces(const uint64_t* __restrict__ k, int64_t n, int shift, F vals, double* __restrict__ ps) {
  __shared__ uint64_t lc[SEG];
  __shared__ double lv[NV][SEG];
  __shared__ double lw[NV][TNP_WAVES];
  const int t = threadIdx.x;
  const int64_t j0 = (int64_t)blockIdx.x * SEG, j = j0 + t;
  const bool active = j < n;
  double v[NV];
#pragma unroll
  for (int q = 0; q < NV; ++q) v[q] = 0.0;
  uint64_t c = ~0ull;
  if (active) {
    c = k[j] >> shift;
    vals(k[j] & ((1ull << shift) - 1ull), v);
  }
  lc[t] = c;
#pragma unroll
  for (int q = 0; q < NV; ++q) lv[q][t] = v[q];
  __syncthreads();
  const bool whole = __syncthreads_and(active && c == lc[0]);
  if (whole) {
#pragma unroll
    for (int q = 0; q < NV; ++q) {
      double s = v[q];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
      if (tnp::lane() == 0) lw[q][tnp::wave()] = s;
    }
    __syncthreads();
    if (t == 0) {
#pragma unroll
      for (int q = 0; q < NV; ++q) {
        double s = lw[q][0];
#pragma unroll
        for (int w = 1; w < TNP_WAVES; ++w) s += lw[q][w];
        ps[(int64_t)q * n + j0] = s;
      }
    }
    return;
  }
  if (active && (t == 0 || lc[t - 1] != c)) {
    for (int e = t + 1; e < SEG && lc[e] == c; ++e) {
#pragma unroll
      for (int q = 0; q < NV; ++q) v[q] += lv[q][e];
    }
#pragma unroll
    for (int q = 0; q < NV; ++q) ps[(int64_t)q * n + j] = v[q];
  }
}

// second level, one wave per class: its pieces start at start[c] and at the
// multiples of SEG inside (start[c], start[c + 1]); lane l adds pieces l,
// l + 64, ... in order, then the xor tree.  out[q * nseg + c].
template <int NV>
__global__ void __launch_bounds__(TNP_BLOCK)
k_seg_final(const int64_t* __restrict__ start, int64_t nseg, int64_t n, const double* __restrict__ ps,
            double* __restrict__ out) {
  const int64_t c = (int64_t)blockIdx.x * TNP_WAVES + tnp::wave();
  if (c >= nseg) return;  // (a whole wave)
  const int64_t s = start[c], e = start[c + 1];
  const int64_t b0 = s / SEG, np = e > s ? (e - 1) / SEG - b0 + 1 : 0;
  double v[NV];
#pragma unroll
  for (int q = 0; q < NV; ++q) v[q] = 0.0;
  for (int64_t r = tnp::lane(); r < np; r += 64) {
    const int64_t at = r == 0 ? s : (b0 + r) * SEG;
#pragma unroll
    for (int q = 0; q < NV; ++q) v[q] += ps[(int64_t)q * n + at];
  }
#pragma unroll
  for (int q = 0; q < NV; ++q) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[q] += __shfl_xor(v[q], o, 64);
    if (tnp::lane() == 0) out[(int64_t)q * nseg + c] = v[q];
  }
}

// The boundary graph's classes over the sorted keys sk: vparent (any
// contents) becomes the union-find of the vertices joined by an edge used
// once, bdeg (zeroed by the caller) their boundary degrees, vrank the number
// of the class of every root that carries a boundary edge -- the loop numbers
// -- with their count in ctr[TC_L] and the edges' in ctr[TC_B] (both zero
// before).  Nothing is read back here.
int boundary_classes(Scratch& scr, const uint64_t* sk, int64_t n, int64_t V, int* vparent, int* bdeg, int32_t* vflag,
                     int64_t* vrank, int64_t* ctr, hipStream_t s) {
  SOUP_LAUNCH(k_iota, V, vparent, V);
  SOUP_LAUNCH(k_boundary_union, n, sk, n, vparent, bdeg, ctr);
  SOUP_LAUNCH(k_flag_roots, V, vparent, bdeg, V, vflag);
  return scan_flags(scr, vflag, V, vrank, ctr + TC_L, s);
}

}  // namespace
