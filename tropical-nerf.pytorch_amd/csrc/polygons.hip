// tnp_polygon_report: closedness, orientation and planarity of a polygon soup
// (include/tropical_hip.h has the definitions).  The engine is not involved:
// scratch is allocated per call on the caller's stream and freed.
//
//   k_soup_offsets  per polygon: the offsets are checked, degrees written
//   k_soup_edges    per index: ids checked, one directed-edge key and one
//                   used-vertex flag written (soup_check.h; the front around
//                   both is soup_host.h's)
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
#include "soup_host.h"
#include "step.h"

namespace {

// counter block (int64 words)
enum { PC_ERR, PC_NIDX, PC_MAXDEG, PC_VUSED, PC_EDGES, PC_BOUND, PC_MANI, PC_NONM, PC_MISO, PC_DEV, PC_AREA, PC_N };
// (the error word, the offsets kernel and the id check are soup_check.h's: PC_ERR / PC_NIDX are its two words)
static_assert(PC_ERR == SOUP_ERR && PC_NIDX == SOUP_NIDX, "counter layout");

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

}  // namespace

extern "C" int tnp_polygon_report(const float* d_xyz, int64_t V, const int64_t* d_offsets, const int64_t* d_indices,
                                  int64_t P, tnp_polygon_stats* h_out, float* d_area, float* d_dev, void* stream) {
  const char* who = "polygon_report";
  hipStream_t s = (hipStream_t)stream;
  if (!h_out) { tnp_set_error("polygon_report: null stats"); return -1; }
  *h_out = tnp_polygon_stats{};
  if (soup_args(who, V, P, false, P > 0, d_xyz, d_offsets, d_indices)) return -1;
  if (P == 0) return 0;
  Scratch scr(s, who);
  int64_t* ctr = nullptr;
  int32_t* deg = scr.arr<int32_t>(P);
  if (!deg) return -1;
  const int64_t n = soup_offsets(who, scr, d_offsets, d_indices, V, P, &ctr, PC_N, s, deg);
  if (n < 0) return -1;

  const int key_bits = 32 + bits_for(V);  // min in [32, 32 + bits), max << 1 | direction below
  const size_t sort_bytes = sort_scratch_bytes(n, key_bits);
  const int64_t nblk = tnp_grid(P);
  uint64_t* ka = scr.arr<uint64_t>(n);
  uint64_t* kb = scr.arr<uint64_t>(n);
  void* sort_scr = scr.get(sort_bytes);
  uint8_t* used = scr.arr<uint8_t>(V > 16 ? V : 16);
  double* partial = scr.arr<double>(nblk);
  if (!ka || !kb || !sort_scr || !used || !partial) return -1;
  TNP_CHECK(hipMemsetAsync(used, 0, (size_t)(V > 16 ? V : 16), s));
  SOUP_LAUNCH((k_soup_edges<true, false>), n, d_offsets, P, d_indices, n, V, ctr, ka, used, (int32_t*)nullptr);
  uint64_t* sorted = nullptr;
  if (sort_keys_u64(ka, kb, n, key_bits, sort_scr, sort_bytes, &sorted, s)) return -1;
  hipLaunchKernelGGL(k_edge_runs, dim3(std::min<unsigned>(tnp_grid(n), 256u)), dim3(TNP_BLOCK), 0, s, sorted, n, ctr);
  TNP_CHECK(hipGetLastError());
  if (launch_count_flags(used, V, ctr, PC_VUSED, s)) return -1;
  if (launch_max_i32(deg, P, ctr + PC_MAXDEG, s)) return -1;
  SOUP_LAUNCH(k_poly_geom, P, d_xyz, d_offsets, d_indices, P, ctr, d_area, d_dev, partial);
  hipLaunchKernelGGL(k_area_total, dim3(1), dim3(TNP_BLOCK), 0, s, partial, nblk, ctr);
  TNP_CHECK(hipGetLastError());
  int64_t h[PC_N];
  if (soup_verdict(who, d_offsets, d_indices, V, ctr, h, PC_N, s)) return -1;
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
