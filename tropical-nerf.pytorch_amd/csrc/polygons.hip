// tnp_polygon_report: closedness, orientation and planarity of a polygon soup
// (include/tropical_hip.h has the definitions).  The engine is not involved:
// scratch is allocated per call on the caller's stream and freed.
//
//   k_soup_offsets  per polygon: the offsets are checked, degrees written
//   k_poly_edges    per index: ids checked, one directed-edge key and one
//                   used-vertex flag written (stores only -- nothing is loaded
//                   through an id here)
//   sort_keys_u64   the keys, on the bits the ids need
//   k_edge_runs     run lengths of equal undirected edges -> five counters
//   k_poly_geom     per polygon: fp32 Newell area and planarity deviation;
//                   reads the error word first and does nothing after a
//                   failed check, so no coordinate is loaded through a bad id
//   k_area_total    the per-workgroup area partials, summed in a fixed order
#include <string.h>

#include <algorithm>
#include <vector>

#include "faces.h"
#include "kernels.h"
#include "poly_geom.h"
#include "soup_check.h"
#include "step.h"

namespace {

// counter block (int64 words)
enum { PC_ERR, PC_NIDX, PC_MAXDEG, PC_VUSED, PC_EDGES, PC_BOUND, PC_MANI, PC_NONM, PC_MISO, PC_DEV, PC_AREA, PC_N };
// (the error word, the offsets kernel and the id check are soup_check.h's: PC_ERR / PC_NIDX are its two words)
static_assert(PC_ERR == SOUP_ERR && PC_NIDX == SOUP_NIDX, "counter layout");

// one key per index position i: the edge from idx[i] to the next id of its
// polygon (cyclic), (min << 32) | (max << 1) | (from > to)
__global__ void __launch_bounds__(TNP_BLOCK)
k_poly_edges(const int64_t* __restrict__ off, int64_t P, const int64_t* __restrict__ idx, int64_t n, int64_t V,
             int64_t* __restrict__ ctr, uint8_t* __restrict__ used, uint64_t* __restrict__ keys) {
  const int64_t i = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  if (i >= n) return;
  int64_t a, b;
  bool b_ok;
  uint64_t key = 0;
  if (soup_check_id(off, P, idx, i, V, ctr, a, b, b_ok)) {
    used[a] = 1;
    if (b_ok) {
      const uint64_t lo = (uint64_t)(a < b ? a : b), hi = (uint64_t)(a < b ? b : a);
      key = (lo << 32) | (hi << 1) | (a > b ? 1u : 0u);
    }
  }
  keys[i] = key;
}

// sorted keys: a run of equal key >> 1 is one undirected edge used run-length
// times.  The run's first key classifies it from the two keys after it (the
// classes are 1, 2, more).  Few workgroups that loop; the five counts are
// reduced per workgroup in LDS and leave it as one integer atomic each.
__global__ void __launch_bounds__(TNP_BLOCK)
k_edge_runs(const uint64_t* __restrict__ k, int64_t n, int64_t* __restrict__ ctr) {
  __shared__ int lds[5];
  if (threadIdx.x < 5) lds[threadIdx.x] = 0;
  __syncthreads();
  int c[5] = {0, 0, 0, 0, 0};  // edges, boundary, manifold, non-manifold, misoriented
  for (int64_t i = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * TNP_BLOCK) {
    const uint64_t x = k[i];
    if (i > 0 && (k[i - 1] >> 1) == (x >> 1)) continue;
    const bool two = i + 1 < n && (k[i + 1] >> 1) == (x >> 1);
    const bool more = two && i + 2 < n && (k[i + 2] >> 1) == (x >> 1);
    c[0] += 1;
    c[1] += !two;
    c[2] += two && !more;
    c[3] += more;
    c[4] += two && !more && ((k[i + 1] ^ x) & 1) == 0;
  }
#pragma unroll
  for (int q = 0; q < 5; ++q) {
    const int w = tnp::wave_sum(c[q]);
    if (tnp::lane() == 0 && w) atomicAdd(&lds[q], w);
  }
  __syncthreads();
  if (threadIdx.x < 5 && lds[threadIdx.x])
    atomicAdd(reinterpret_cast<unsigned long long*>(ctr + PC_EDGES + threadIdx.x),
              (unsigned long long)lds[threadIdx.x]);
}

// fp32 Newell about the members' mean c: N = 1/2 sum (p_i - c) x (p_i+1 - c),
// area |N|, dev = max |(p_i - c) . N| / |N| (0 when |N| = 0).  One thread per
// polygon walks its members in order (poly_geom.h newell_area).  The areas
// leave the workgroup as one double partial, reduced in a fixed order;
// dev >= 0, so its bits order as integers.
__global__ void __launch_bounds__(TNP_BLOCK)
k_poly_geom(const float* __restrict__ xyz, const int64_t* __restrict__ off, const int64_t* __restrict__ idx,
            int64_t P, int64_t* __restrict__ ctr, float* __restrict__ area, float* __restrict__ dev,
            double* __restrict__ partial) {
  __shared__ double lds_a[TNP_WAVES];
  __shared__ float lds_d[TNP_WAVES];
  if (__hip_atomic_load(reinterpret_cast<unsigned long long*>(ctr + PC_ERR), __ATOMIC_RELAXED,
                        __HIP_MEMORY_SCOPE_AGENT) != SOUP_NONE)
    return;  // (every thread: a failed check)
  const int64_t p = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  float A = 0.f, D = 0.f;
  if (p < P) {
    const int64_t a = off[p], b = off[p + 1];
    float c[3], N[3];
    A = newell_area(xyz, idx, a, b, c, N);
    if (A > 0.f) {
      for (int64_t i = a; i < b; ++i) {
        const float* q = xyz + 3 * idx[i];
        D = fmaxf(D, fabsf((q[0] - c[0]) * N[0] + (q[1] - c[1]) * N[1] + (q[2] - c[2]) * N[2]));
      }
      D /= A;
    }
    if (area) area[p] = A;
    if (dev) dev[p] = D;
  }
  double sa = (double)A;
  float sd = D;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sa += __shfl_xor(sa, o, 64);
    sd = fmaxf(sd, __shfl_xor(sd, o, 64));
  }
  if (tnp::lane() == 0) {
    lds_a[tnp::wave()] = sa;
    lds_d[tnp::wave()] = sd;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = lds_a[0];
    float d = lds_d[0];
#pragma unroll
    for (int w = 1; w < TNP_WAVES; ++w) {
      t += lds_a[w];
      d = fmaxf(d, lds_d[w]);
    }
    partial[blockIdx.x] = t;
    if (d > 0.f)
      atomicMax(reinterpret_cast<unsigned long long*>(ctr + PC_DEV), (unsigned long long)__float_as_uint(d));
  }
}

// one workgroup: thread t adds partials t, t + 256, ... in order, then the
// same tree as above -- the same bits for the same input, whatever ran before
__global__ void __launch_bounds__(TNP_BLOCK)
k_area_total(const double* __restrict__ partial, int64_t n, int64_t* __restrict__ ctr) {
  __shared__ double lds[TNP_WAVES];
  if (__hip_atomic_load(reinterpret_cast<unsigned long long*>(ctr + PC_ERR), __ATOMIC_RELAXED,
                        __HIP_MEMORY_SCOPE_AGENT) != SOUP_NONE)
    return;
  double t = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += TNP_BLOCK) t += partial[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
  if (tnp::lane() == 0) lds[tnp::wave()] = t;
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = lds[0];
#pragma unroll
    for (int w = 1; w < TNP_WAVES; ++w) a += lds[w];
    *reinterpret_cast<double*>(ctr + PC_AREA) = a;
  }
}

// device scratch of one call, freed on the stream on every way out
struct Scratch {
  hipStream_t s;
  std::vector<void*> p;
  explicit Scratch(hipStream_t st) : s(st) {}
  ~Scratch() {
    for (void* q : p) (void)hipFreeAsync(q, s);
  }
  void* get(size_t bytes) {
    void* q = nullptr;
    if (hipMallocAsync(&q, bytes < 256 ? 256 : bytes, s) != hipSuccess) {
      tnp_set_error("polygon_report: hipMallocAsync of %zu bytes failed", bytes);
      return nullptr;
    }
    p.push_back(q);
    return q;
  }
};

}  // namespace

extern "C" int tnp_polygon_report(const float* d_xyz, int64_t V, const int64_t* d_offsets, const int64_t* d_indices,
                                  int64_t P, tnp_polygon_stats* h_out, float* d_area, float* d_dev, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!h_out) { tnp_set_error("polygon_report: null stats"); return -1; }
  *h_out = tnp_polygon_stats{};
  if (P < 0 || V < 0) { tnp_set_error("polygon_report: P = %lld, V = %lld", (long long)P, (long long)V); return -1; }
  if (V >= (int64_t)1 << 31) {
    tnp_set_error("polygon_report: V = %lld vertices; the edge keys hold ids below 2^31", (long long)V);
    return -1;
  }
  if (P == 0) return 0;
  if (!d_offsets || !d_indices || (V > 0 && !d_xyz)) { tnp_set_error("polygon_report: null array"); return -1; }
  Scratch scr(s);
  int64_t* ctr = static_cast<int64_t*>(scr.get(PC_N * sizeof(int64_t)));
  int32_t* deg = static_cast<int32_t*>(scr.get(P * sizeof(int32_t)));
  if (!ctr || !deg) return -1;
  int64_t h[PC_N];
  for (int i = 0; i < PC_N; ++i) h[i] = 0;
  h[PC_ERR] = (int64_t)SOUP_NONE;
  TNP_CHECK(hipMemcpyAsync(ctr, h, sizeof(h), hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_soup_offsets, dim3(tnp_grid(P)), dim3(TNP_BLOCK), 0, s, d_offsets, P, ctr, deg);
  TNP_CHECK(hipGetLastError());
  TNP_CHECK(hipMemcpyAsync(h, ctr, 2 * sizeof(int64_t), hipMemcpyDeviceToHost, s));
  TNP_CHECK(hipStreamSynchronize(s));
  if ((unsigned long long)h[PC_ERR] != SOUP_NONE)
    return soup_report_error("polygon_report", (unsigned long long)h[PC_ERR], d_offsets, d_indices, V, s);
  const int64_t n = h[PC_NIDX];  // >= 3 P: every offset is now known to lie in [0, n]

  int bits = 1;
  while (((int64_t)1 << bits) < V) ++bits;
  const int key_bits = 32 + bits;  // min in [32, 32 + bits), max << 1 | direction below
  const size_t sort_bytes = sort_scratch_bytes(n, key_bits);
  const int64_t nblk = tnp_grid(P);
  uint64_t* ka = static_cast<uint64_t*>(scr.get(n * sizeof(uint64_t)));
  uint64_t* kb = static_cast<uint64_t*>(scr.get(n * sizeof(uint64_t)));
  void* sort_scr = scr.get(sort_bytes);
  uint8_t* used = static_cast<uint8_t*>(scr.get((size_t)(V > 16 ? V : 16)));
  double* partial = static_cast<double*>(scr.get(nblk * sizeof(double)));
  if (!ka || !kb || !sort_scr || !used || !partial) return -1;
  TNP_CHECK(hipMemsetAsync(used, 0, (size_t)(V > 16 ? V : 16), s));
  hipLaunchKernelGGL(k_poly_edges, dim3(tnp_grid(n)), dim3(TNP_BLOCK), 0, s, d_offsets, P, d_indices, n, V, ctr,
                     used, ka);
  TNP_CHECK(hipGetLastError());
  uint64_t* sorted = nullptr;
  if (sort_keys_u64(ka, kb, n, key_bits, sort_scr, sort_bytes, &sorted, s)) return -1;
  hipLaunchKernelGGL(k_edge_runs, dim3(std::min<unsigned>(tnp_grid(n), 256u)), dim3(TNP_BLOCK), 0, s, sorted, n, ctr);
  TNP_CHECK(hipGetLastError());
  if (launch_count_flags(used, V, ctr, PC_VUSED, s)) return -1;
  if (launch_max_i32(deg, P, ctr + PC_MAXDEG, s)) return -1;
  hipLaunchKernelGGL(k_poly_geom, dim3((unsigned)nblk), dim3(TNP_BLOCK), 0, s, d_xyz, d_offsets, d_indices, P, ctr,
                     d_area, d_dev, partial);
  hipLaunchKernelGGL(k_area_total, dim3(1), dim3(TNP_BLOCK), 0, s, partial, nblk, ctr);
  TNP_CHECK(hipGetLastError());
  TNP_CHECK(hipMemcpyAsync(h, ctr, sizeof(h), hipMemcpyDeviceToHost, s));
  TNP_CHECK(hipStreamSynchronize(s));
  if ((unsigned long long)h[PC_ERR] != SOUP_NONE)
    return soup_report_error("polygon_report", (unsigned long long)h[PC_ERR], d_offsets, d_indices, V, s);
  h_out->n_polygons = P;
  h_out->n_indices = n;
  h_out->max_degree = h[PC_MAXDEG];
  h_out->n_vertices_used = h[PC_VUSED];
  h_out->n_edges = h[PC_EDGES];
  h_out->e_boundary = h[PC_BOUND];
  h_out->e_manifold = h[PC_MANI];
  h_out->e_nonmanifold = h[PC_NONM];
  h_out->e_misoriented = h[PC_MISO];
  h_out->euler = h_out->n_vertices_used - h_out->n_edges + h_out->n_polygons;
  memcpy(&h_out->area, &h[PC_AREA], sizeof(double));
  const uint32_t db = (uint32_t)h[PC_DEV];
  memcpy(&h_out->max_dev, &db, sizeof(float));
  return 0;
}
