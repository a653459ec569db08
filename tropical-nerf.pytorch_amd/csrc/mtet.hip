// Marching tetrahedra (tropical/utils/mtet.py of the reference, a kaolin
// derivative) on gfx950: the mesh of `python -m tropical.stanford.evaluate
// -t mtet`.  Three calls, the outputs allocated by the caller in between:
//
//   tnp_mt_classify  one thread per tet: range check of the four ids, the
//                    orientation flip (written back to the caller's tets),
//                    one case byte per tet, and per tile of 256 tets the
//                    counts (crossed edges, 1-triangle tets, 2-triangle
//                    tets), scanned over the tiles
//   tnp_mt_edges     every valid tet appends the keys lo << nb | hi of its
//                    crossed edges at its scanned offset (no atomics: the
//                    buffer is the same from run to run); radix sort on the
//                    2 nb significant bits; rocPRIM unique (head flags +
//                    scan) leaves the vertex list, numbered by the
//                    lexicographic rank of (lo, hi)
//   tnp_mt_emit      vertices from the unique keys (five individually
//                    rounded fp32 ops, no fma); faces by a binary search of
//                    every corner's edge key in the unique keys, written at
//                    the scanned (1-triangle, then 2-triangle) offsets
//
// Modelled traffic: classify reads 32 B of ids and gathers 64 B (4 sdf + 12
// coordinates, L2 hits on a grid) per tet and writes 1 B (+ 16 B where it
// flips); the key pass reads 1 B per tet and 32 B + 8 B per key for the valid
// ones; the sort moves 16 B per key and 8-bit digit pass; emit reads 1 B per
// tet, 32 B per valid tet and ~log2(V) L2-resident probes per corner, and
// writes 24 B + 8 B per face and 12 B + 16 B per vertex.
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_select.hpp>

#include <algorithm>

#include "common.h"
#include "step.h"

namespace {

// triangles of a case (bit i: corner i of the flipped tet is inside, sdf > 0)
// as tet edges, numbered (0,1) (0,2) (0,3) (1,2) (1,3) (2,3)
__constant__ int8_t c_mt_tri[16][6] = {
    {-1, -1, -1, -1, -1, -1}, {1, 0, 2, -1, -1, -1}, {4, 0, 3, -1, -1, -1}, {1, 4, 2, 1, 3, 4},
    {3, 1, 5, -1, -1, -1},    {2, 3, 0, 2, 5, 3},    {1, 4, 0, 1, 5, 4},    {4, 2, 5, -1, -1, -1},
    {4, 5, 2, -1, -1, -1},    {4, 1, 0, 4, 5, 1},    {3, 2, 0, 3, 5, 2},    {1, 3, 5, -1, -1, -1},
    {4, 1, 2, 4, 3, 1},       {3, 0, 4, -1, -1, -1}, {2, 0, 1, -1, -1, -1}, {-1, -1, -1, -1, -1, -1}};

// per-tile counts and their scan: crossed-edge keys, 1- and 2-triangle tets
struct Cnt3 {
  int64_t e, n1, n2;
};
struct Cnt3Plus {
  __host__ __device__ Cnt3 operator()(const Cnt3& a, const Cnt3& b) const {
    return Cnt3{a.e + b.e, a.n1 + b.n1, a.n2 + b.n2};
  }
};

// corners inside -> triangles (0, 1 or 2) and crossed edges (0, 3 or 4)
__device__ __forceinline__ int mt_tris(int c) {
  const int p = __popc(c);
  return p == 2 ? 2 : ((p == 1 || p == 3) ? 1 : 0);
}
__device__ __forceinline__ int mt_edges(int c) {
  const int n = mt_tris(c);
  return n ? n + 2 : 0;
}

struct Tet {
  int64_t id[4];
};
// two 16-B loads per lane (the caller guarantees 16-B alignment)
__device__ __forceinline__ Tet tet_load(const int64_t* tets, int64_t t) {
  const longlong2* p = reinterpret_cast<const longlong2*>(tets) + 2 * t;
  const longlong2 a = p[0], b = p[1];
  return Tet{{a.x, a.y, b.x, b.y}};
}

__device__ __forceinline__ uint64_t edge_key(int64_t a, int64_t b, int nb) {
  const uint64_t lo = (uint64_t)(a < b ? a : b), hi = (uint64_t)(a < b ? b : a);
  return (lo << nb) | hi;
}

__global__ void __launch_bounds__(TNP_BLOCK)
k_mt_classify(const float* __restrict__ V, const float* __restrict__ sdf, int64_t N,
              int64_t* __restrict__ tets, int64_t T, uint8_t* __restrict__ cs, Cnt3* __restrict__ tile,
              int64_t* __restrict__ err) {
  __shared__ int lds[TNP_WAVES];
  const int64_t t = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  int c = 0;
  bool bad = false;
  if (t < T) {
    Tet q = tet_load(tets, t);
    // every id is checked before any gather
#pragma unroll
    for (int i = 0; i < 4; ++i) bad |= (uint64_t)q.id[i] >= (uint64_t)N;
    if (!bad) {
      float s[4], p[4][3];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        s[i] = sdf[q.id[i]];
#pragma unroll
        for (int d = 0; d < 3; ++d) p[i][d] = V[3 * q.id[i] + d];
      }
      // sign of det[(b - a), (c - a), (d - a)] in double
      double e[3][3];
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int d = 0; d < 3; ++d) e[i][d] = (double)p[i + 1][d] - (double)p[0][d];
      const double det = e[0][0] * (e[1][1] * e[2][2] - e[1][2] * e[2][1]) -
                         e[0][1] * (e[1][0] * e[2][2] - e[1][2] * e[2][0]) +
                         e[0][2] * (e[1][0] * e[2][1] - e[1][1] * e[2][0]);
      if (det < 0.0) {  // swap the first two ids, in the caller's buffer
        reinterpret_cast<longlong2*>(tets)[2 * t] = make_longlong2(q.id[1], q.id[0]);
        const float x = s[0];
        s[0] = s[1];
        s[1] = x;
      }
      c = (int)(s[0] > 0.f) | ((int)(s[1] > 0.f) << 1) | ((int)(s[2] > 0.f) << 2) |
          ((int)(s[3] > 0.f) << 3);
    }
    cs[t] = (uint8_t)c;
  }
  const int n = mt_tris(c);
  // edges <= 1024, tets <= 256 per tile: one packed block sum
  const int packed = tnp::wave_sum(mt_edges(c) | ((n == 1) << 12) | ((n == 2) << 22));
  if (tnp::lane() == 0) lds[tnp::wave()] = packed;
  if (__ballot(bad) && tnp::lane() == 0) tnp::or_sticky(err, 1ull);
  __syncthreads();
  if (threadIdx.x == 0) {
    int sum = 0;
#pragma unroll
    for (int w = 0; w < TNP_WAVES; ++w) sum += lds[w];
    tile[blockIdx.x] = Cnt3{sum & 0xFFF, (sum >> 12) & 0x3FF, (sum >> 22) & 0x3FF};
  }
}

__global__ void __launch_bounds__(TNP_BLOCK)
k_mt_keys(const int64_t* __restrict__ tets, int64_t T, const uint8_t* __restrict__ cs,
          const Cnt3* __restrict__ tile, int nb, uint64_t* __restrict__ keys) {
  __shared__ int64_t lds[TNP_WAVES];
  const int64_t t = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  const int c = t < T ? cs[t] : 0;
  const int ne = mt_edges(c);
  int64_t total;
  const int64_t rank = tnp::block_scan_excl((int64_t)ne, lds, total);
  if (!ne) return;
  const Tet q = tet_load(tets, t);
  constexpr int EI[6] = {0, 0, 0, 1, 1, 2}, EJ[6] = {1, 2, 3, 2, 3, 3};
  uint64_t* o = keys + tile[blockIdx.x].e + rank;
#pragma unroll
  for (int e = 0; e < 6; ++e)
    if (((c >> EI[e]) ^ (c >> EJ[e])) & 1) *o++ = edge_key(q.id[EI[e]], q.id[EJ[e]], nb);
}

__global__ void __launch_bounds__(TNP_BLOCK)
k_mt_verts(const uint64_t* __restrict__ ukeys, int64_t nV, int nb, const float* __restrict__ V,
           const float* __restrict__ sdf, float* __restrict__ verts, int64_t* __restrict__ interp) {
  const int64_t i = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  if (i >= nV) return;
  const uint64_t k = ukeys[i];
  const int64_t a = (int64_t)(k >> nb), b = (int64_t)(k & ((1ull << nb) - 1ull));
  const float sa = sdf[a], sb = sdf[b];
  float pa[3], pb[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    pa[d] = V[3 * a + d];
    pb[d] = V[3 * b + d];
  }
  // [s_a, -s_b] flipped over their sum; each op rounded on its own
  const float n = -sb;
  const float den = __fadd_rn(sa, n);
  const float w0 = __fdiv_rn(n, den), w1 = __fdiv_rn(sa, den);
#pragma unroll
  for (int d = 0; d < 3; ++d) verts[3 * i + d] = __fadd_rn(__fmul_rn(pa[d], w0), __fmul_rn(pb[d], w1));
  reinterpret_cast<longlong2*>(interp)[i] = make_longlong2(a, b);
}

// rank of key k in the sorted unique keys (k is one of them)
__device__ __forceinline__ int64_t key_rank(const uint64_t* __restrict__ u, int64_t n, uint64_t k) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (u[mid] < k) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__global__ void __launch_bounds__(TNP_BLOCK)
k_mt_faces(const int64_t* __restrict__ tets, int64_t T, const uint8_t* __restrict__ cs,
           const Cnt3* __restrict__ tile, const uint64_t* __restrict__ ukeys, int64_t nV, int nb,
           int64_t n_one, int64_t* __restrict__ faces, int64_t* __restrict__ tet_idx) {
  __shared__ int64_t lds[TNP_WAVES];
  const int64_t t = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  const int c = t < T ? cs[t] : 0;
  const int nt = mt_tris(c);
  int64_t total;
  // 1-triangle rank in the low half, 2-triangle rank in the high half
  const int64_t rank =
      tnp::block_scan_excl((int64_t)(nt == 1) | ((int64_t)(nt == 2) << 32), lds, total);
  if (!nt) return;
  const Tet q = tet_load(tets, t);
  constexpr int EI[6] = {0, 0, 0, 1, 1, 2}, EJ[6] = {1, 2, 3, 2, 3, 3};
  int64_t vid[6];
#pragma unroll
  for (int e = 0; e < 6; ++e) {
    vid[e] = -1;
    if (((c >> EI[e]) ^ (c >> EJ[e])) & 1) vid[e] = key_rank(ukeys, nV, edge_key(q.id[EI[e]], q.id[EJ[e]], nb));
  }
  const Cnt3 base = tile[blockIdx.x];
  const int64_t f = nt == 1 ? base.n1 + (rank & 0xFFFFFFFFll) : n_one + 2 * (base.n2 + (rank >> 32));
  for (int k = 0; k < 3 * nt; ++k) {
    const int e = c_mt_tri[c][k];
    int64_t v = vid[0];
#pragma unroll
    for (int j = 1; j < 6; ++j) v = e == j ? vid[j] : v;
    faces[3 * f + k] = v;
  }
  tet_idx[f] = t;
  if (nt == 2) tet_idx[f + 1] = t;
}

int64_t mt_tiles(int64_t T) { return (T + TNP_BLOCK - 1) / TNP_BLOCK; }
int mt_bits(int64_t N) {
  int nb = 1;
  while ((1ll << nb) < N) ++nb;
  return nb;
}

}  // namespace

extern "C" int tnp_mt_classify(const float* d_vertices, const float* d_sdf, int64_t n_points,
                               int64_t* d_tets, int64_t n_tets, uint8_t* d_case, int64_t* d_tile,
                               int64_t* n_keys, int64_t* n_one, int64_t* n_two, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  *n_keys = *n_one = *n_two = 0;
  if (n_points < 0 || n_points >= (1ll << 31)) { tnp_set_error("marching tetrahedra: %lld points (needs < 2^31)", (long long)n_points); return -1; }
  if (n_tets < 0 || mt_tiles(n_tets) >= (1ll << 31)) { tnp_set_error("marching tetrahedra: %lld tets", (long long)n_tets); return -1; }
  if (n_tets == 0) return 0;
  const int64_t nt = mt_tiles(n_tets);
  Cnt3* tile = reinterpret_cast<Cnt3*>(d_tile);
  int64_t* err = d_tile + 3 * (nt + 1);
  // the scan's unused last input, the error flag and the unique count
  TNP_CHECK(hipMemsetAsync(tile + nt, 0, sizeof(Cnt3) + 2 * sizeof(int64_t), s));
  hipLaunchKernelGGL(k_mt_classify, dim3((unsigned)nt), dim3(TNP_BLOCK), 0, s, d_vertices, d_sdf, n_points,
                     d_tets, n_tets, d_case, tile, err);
  TNP_CHECK(hipGetLastError());
  size_t tmp = 0;
  TNP_CHECK(rocprim::exclusive_scan(nullptr, tmp, tile, tile, Cnt3{0, 0, 0}, (size_t)(nt + 1), Cnt3Plus(), s));
  void* scratch = nullptr;
  TNP_CHECK(hipMallocAsync(&scratch, std::max<size_t>(tmp, 16), s));
  hipError_t e = rocprim::exclusive_scan(scratch, tmp, tile, tile, Cnt3{0, 0, 0}, (size_t)(nt + 1), Cnt3Plus(), s);
  TNP_CHECK(hipFreeAsync(scratch, s));
  TNP_CHECK(e);
  int64_t host[4];  // totals, then the error flag
  TNP_CHECK(hipMemcpyAsync(host, tile + nt, sizeof(host), hipMemcpyDeviceToHost, s));
  TNP_CHECK(hipStreamSynchronize(s));
  if (host[3]) {
    tnp_set_error("marching tetrahedra: a tet index is outside [0, %lld)", (long long)n_points);
    return 1;
  }
  *n_keys = host[0];
  *n_one = host[1];
  *n_two = host[2];
  return 0;
}

extern "C" int tnp_mt_edges(const int64_t* d_tets, int64_t n_tets, int64_t n_points,
                            const uint8_t* d_case, int64_t* d_tile, int64_t n_keys, uint64_t* d_keys,
                            int64_t* n_verts, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  *n_verts = 0;
  if (n_tets <= 0 || n_keys <= 0) return 0;
  const int64_t nt = mt_tiles(n_tets);
  const int nb = mt_bits(n_points);
  hipLaunchKernelGGL(k_mt_keys, dim3((unsigned)nt), dim3(TNP_BLOCK), 0, s, d_tets, n_tets, d_case,
                     reinterpret_cast<const Cnt3*>(d_tile), nb, d_keys);
  TNP_CHECK(hipGetLastError());
  int64_t* d_count = d_tile + 3 * (nt + 1) + 1;
  uint64_t* cur = nullptr;
  size_t ubytes = 0;
  TNP_CHECK(rocprim::unique(nullptr, ubytes, d_keys, d_keys, d_count, (size_t)n_keys,
                            rocprim::equal_to<uint64_t>(), s));
  const size_t sbytes = sort_scratch_bytes(n_keys, 2 * nb);
  const size_t bytes = std::max<size_t>(std::max(ubytes, sbytes), 16);
  void* scratch = nullptr;
  TNP_CHECK(hipMallocAsync(&scratch, bytes, s));
  int rc = sort_keys_u64(d_keys, d_keys + n_keys, n_keys, 2 * nb, scratch, sbytes, &cur, s);
  uint64_t* other = cur == d_keys ? d_keys + n_keys : d_keys;
  hipError_t e = hipSuccess;
  if (rc == 0)
    e = rocprim::unique(scratch, ubytes, cur, other, d_count, (size_t)n_keys, rocprim::equal_to<uint64_t>(), s);
  TNP_CHECK(hipFreeAsync(scratch, s));
  if (rc) return rc;
  TNP_CHECK(e);
  int64_t nv = 0;
  TNP_CHECK(hipMemcpyAsync(&nv, d_count, sizeof(int64_t), hipMemcpyDeviceToHost, s));
  TNP_CHECK(hipStreamSynchronize(s));
  if (nv < 0 || nv > n_keys) { tnp_set_error("marching tetrahedra: unique edge count %lld of %lld keys", (long long)nv, (long long)n_keys); return -1; }
  // the unique keys end in d_keys[0, nv)
  if (other != d_keys && nv > 0)
    TNP_CHECK(hipMemcpyAsync(d_keys, other, (size_t)nv * sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
  *n_verts = nv;
  return 0;
}

extern "C" int tnp_mt_emit(const float* d_vertices, const float* d_sdf, int64_t n_points,
                           const int64_t* d_tets, int64_t n_tets, const uint8_t* d_case,
                           const int64_t* d_tile, const uint64_t* d_keys, int64_t n_verts, int64_t n_one,
                           float* d_verts, int64_t* d_interp, int64_t* d_faces, int64_t* d_tet_idx,
                           void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (n_tets <= 0 || n_verts <= 0) return 0;
  const int nb = mt_bits(n_points);
  hipLaunchKernelGGL(k_mt_verts, dim3(tnp_grid(n_verts)), dim3(TNP_BLOCK), 0, s, d_keys, n_verts, nb,
                     d_vertices, d_sdf, d_verts, d_interp);
  hipLaunchKernelGGL(k_mt_faces, dim3((unsigned)mt_tiles(n_tets)), dim3(TNP_BLOCK), 0, s, d_tets, n_tets,
                     d_case, reinterpret_cast<const Cnt3*>(d_tile), d_keys, n_verts, nb, n_one, d_faces,
                     d_tet_idx);
  TNP_CHECK(hipGetLastError());
  return 0;
}
