// tnp_topology_*: connected components and boundary loops of a polygon soup
// (include/tropical_hip.h has the definitions).  The engine is not involved:
// scratch is allocated per build on the caller's stream and freed; the handle
// keeps the three result tables.
//
//   k_soup_offsets, k_soup_edges   (soup_check.h, behind soup_host.h's front)
//                     the offsets checked; per index: ids checked, one
//                     directed-edge key (the report's) and its polygon written
//   sort_pairs_u64    (key, polygon) on the bits the ids need
//   k_union_edges     lock-free union-find over the polygons: every use of an
//                     undirected edge is united with the use before it in the
//                     sorted run (the same classes as uniting each with the
//                     run's first, and no walk back to find it).  connect = 1:
//                     k_vertex_owner (the smallest polygon at each vertex) and
//                     k_union_vertices instead
//   k_boundary_union  the same union-find over the vertices, one union per
//                     edge used once; boundary degrees
//   k_flag_roots, scan_i32_to_i64 (x 2)   hooks go to the smaller id, so a
//                     root is its class's smallest member: the exclusive scan
//                     of the root flags ranks the classes canonically
//   k_labels          the flatten pass: label[p] = rank[find(p)]
//   k_comp_polys      per polygon: degree and box into its component (integer
//                     atomics, one per wave and label present in it), fp32
//                     area and double fan determinant stored
//   k_edge_stats      per sorted run: the report's five classes per component
//   k_vertex_keys, sort_keys_u64, k_key_runs     distinct (label, vertex)
//   k_poly_keys, sort_keys_u64, k_seg_starts     the polygons in (label, p)
//                     order; a component's segment gives n_polygons
//   k_seg_pieces, k_seg_final   the doubles, reduced in a shape fixed by the
//                     input (no float atomics)
//   k_loop_verts, k_loop_keys, sort_keys_u64, k_seg_starts, k_seg_pieces,
//   k_seg_final       the loops' counts and lengths the same way
//   k_comp_rows, k_loop_rows    the tables
// The number of launches is fixed (it does not depend on the graph), and no
// kernel waits for another workgroup: a failed hook is retried from the new
// root.  The union-find, the boundary graph's classes and the segmented sums
// are topo_common.h's, shared with holes.hip.  tnp_topology_build is its
// stages in order, one function each, with the build's state in a TopoBuild.
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/tropical_hip_debug.h"
#include "kernels.h"
#include "poly_geom.h"
#include "topo_common.h"

struct tnp_topology {
  int device = 0;
  int32_t* label = nullptr;
  tnp_component* comps = nullptr;
  tnp_boundary_loop* loops = nullptr;
  int64_t P = 0, C = 0, L = 0;
  bool timed = false;
  int n_ms = 0;
  double ms[TNP_TOPOLOGY_STAGES] = {};
};

namespace {

// per-component int64 columns, per-loop int64 columns
enum { CK_FIRST, CK_NIDX, CK_NVERT, CK_EDGES, CK_BOUND, CK_MANI, CK_NONM, CK_MISO, CK_N };
enum { LK_FIRST, LK_NVERT, LK_NONSIMPLE, LK_N };

// fp32 <-> a uint32 that orders the same way (for integer atomicMin / atomicMax)
__device__ __forceinline__ uint32_t f32_ord(float f) {
  const uint32_t b = __float_as_uint(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float ord_f32(uint32_t o) {
  return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

__global__ void __launch_bounds__(TNP_BLOCK)
k_union_edges(const uint64_t* __restrict__ sk, const int32_t* __restrict__ sp, int64_t n, int* parent) {
  const int64_t i = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  if (i < 1 || i >= n) return;
  if ((sk[i] >> 1) == (sk[i - 1] >> 1)) uf_union(parent, sp[i], sp[i - 1]);
}

// connect = 1 (checked ids): the smallest polygon at each vertex, then every
// polygon united with the owner of each of its vertices
__global__ void __launch_bounds__(TNP_BLOCK)
k_vertex_owner(const int64_t* __restrict__ off, int64_t P, const int64_t* __restrict__ idx, int64_t n,
               unsigned* __restrict__ vown) {
  const int64_t i = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  if (i >= n) return;
  atomicMin(vown + idx[i], (unsigned)soup_polygon_of(off, P, i));
}
__global__ void __launch_bounds__(TNP_BLOCK)
k_union_vertices(const int64_t* __restrict__ off, int64_t P, const int64_t* __restrict__ idx, int64_t n,
                 const unsigned* __restrict__ vown, int* parent) {
  const int64_t i = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  if (i >= n) return;
  uf_union(parent, (int)soup_polygon_of(off, P, i), (int)vown[idx[i]]);
}

// the flatten pass: every polygon takes the rank of its root
__global__ void __launch_bounds__(TNP_BLOCK)
k_labels(int* parent, const int64_t* __restrict__ rank, int64_t P, int32_t* __restrict__ label,
         int64_t* __restrict__ cnt, int64_t C) {
  const int64_t p = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  if (p >= P) return;
  const int r = uf_find(parent, (int)p);
  const int32_t c = (int32_t)rank[r];
  label[p] = c;
  if (r == (int)p) cnt[CK_FIRST * C + c] = p;
}

// per polygon: its degree and its vertices' box into its component; its fp32
// area (the report's) and the double fan determinant, by polygon id
__global__ void __launch_bounds__(TNP_BLOCK)
k_comp_polys(const float* __restrict__ xyz, const int64_t* __restrict__ off, const int64_t* __restrict__ idx,
             int64_t P, const int32_t* __restrict__ label, int64_t* __restrict__ cnt, uint32_t* __restrict__ box,
             int64_t C, double* __restrict__ parea, double* __restrict__ pdet) {
  const int64_t p = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  const bool active = p < P;
  int c = 0;
  int64_t deg = 0;
  uint32_t lo[3] = {~0u, ~0u, ~0u}, hi[3] = {0u, 0u, 0u};
  if (active) {
    c = label[p];
    const int64_t a = off[p], b = off[p + 1];
    deg = b - a;
    for (int64_t i = a; i < b; ++i) {
      const float* q = xyz + 3 * idx[i];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const uint32_t o = f32_ord(q[k]);
        lo[k] = o < lo[k] ? o : lo[k];
        hi[k] = o > hi[k] ? o : hi[k];
      }
    }
    float cm[3], N[3];
    parea[p] = (double)newell_area(xyz, idx, a, b, cm, N);
    const float* q0 = xyz + 3 * idx[a];
    const double p0[3] = {(double)q0[0], (double)q0[1], (double)q0[2]};
    double det = 0.0;
    for (int64_t i = a + 1; i + 1 < b; ++i) {
      const float* q1 = xyz + 3 * idx[i];
      const float* q2 = xyz + 3 * idx[i + 1];
      const double u[3] = {(double)q1[0], (double)q1[1], (double)q1[2]};
      const double v[3] = {(double)q2[0], (double)q2[1], (double)q2[2]};
      det += p0[0] * (u[1] * v[2] - u[2] * v[1]) + p0[1] * (u[2] * v[0] - u[0] * v[2]) +
             p0[2] * (u[0] * v[1] - u[1] * v[0]);
    }
    pdet[p] = det;
  }
  wave_classes(active, c, [&](bool in, int c0, int leader) {
    class_add(in, leader, cnt + CK_NIDX * C, c0, deg);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      uint32_t l = in ? lo[k] : ~0u, h = in ? hi[k] : 0u;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const uint32_t l2 = __shfl_xor(l, o, 64), h2 = __shfl_xor(h, o, 64);
        l = l2 < l ? l2 : l;
        h = h2 > h ? h2 : h;
      }
      if (tnp::lane() == leader) {
        atomicMin(box + (int64_t)k * C + c0, l);
        atomicMax(box + (int64_t)(3 + k) * C + c0, h);
      }
    }
  });
}

// sorted (key, polygon): the first use of every undirected edge classifies it
// as k_edge_runs of polygons.hip does, into the component of its polygon
__global__ void __launch_bounds__(TNP_BLOCK)
k_edge_stats(const uint64_t* __restrict__ k, const int32_t* __restrict__ sp, int64_t n,
             const int32_t* __restrict__ label, int64_t* __restrict__ cnt, int64_t C) {
  const int64_t i = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  bool head = false, two = false, more = false, miso = false;
  int c = 0;
  if (i < n) {
    const uint64_t x = k[i];
    head = i == 0 || (k[i - 1] >> 1) != (x >> 1);
    if (head) {
      two = i + 1 < n && (k[i + 1] >> 1) == (x >> 1);
      more = two && i + 2 < n && (k[i + 2] >> 1) == (x >> 1);
      miso = two && !more && ((k[i + 1] ^ x) & 1) == 0;
      c = label[sp[i]];
    }
  }
  wave_classes(head, c, [&](bool in, int c0, int leader) {
    class_add(in, leader, cnt + CK_EDGES * C, c0, 1);
    class_add(in, leader, cnt + CK_BOUND * C, c0, !two);
    class_add(in, leader, cnt + CK_MANI * C, c0, two && !more);
    class_add(in, leader, cnt + CK_NONM * C, c0, more);
    class_add(in, leader, cnt + CK_MISO * C, c0, miso);
  });
}

// (label << vbits) | vertex of every index position
__global__ void __launch_bounds__(TNP_BLOCK)
k_vertex_keys(const int64_t* __restrict__ off, int64_t P, const int64_t* __restrict__ idx, int64_t n,
              const int32_t* __restrict__ label, int vbits, uint64_t* __restrict__ keys) {
  const int64_t i = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  if (i < n) keys[i] = ((uint64_t)label[soup_polygon_of(off, P, i)] << vbits) | (uint64_t)idx[i];
}

// sorted keys: every distinct key adds one to the counter of its class key >> shift
__global__ void __launch_bounds__(TNP_BLOCK)
k_key_runs(const uint64_t* __restrict__ k, int64_t n, int shift, int64_t* __restrict__ row) {
  const int64_t i = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  const bool head = i < n && (i == 0 || k[i - 1] != k[i]);
  const int c = head ? (int)(k[i] >> shift) : 0;
  wave_classes(head, c, [&](bool in, int c0, int leader) { class_add(in, leader, row, c0, 1); });
}

__global__ void __launch_bounds__(TNP_BLOCK)
k_poly_keys(const int32_t* __restrict__ label, int64_t P, int pbits, uint64_t* __restrict__ keys) {
  const int64_t p = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  if (p < P) keys[p] = ((uint64_t)label[p] << pbits) | (uint64_t)p;
}

// sorted keys (class << shift | member), every class present: start[c] = the
// first position of class c, start[nseg] = n
__global__ void __launch_bounds__(TNP_BLOCK)
k_seg_starts(const uint64_t* __restrict__ k, int64_t n, int shift, int64_t nseg, int64_t* __restrict__ start) {
  const int64_t j = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  if (j == 0) start[nseg] = n;
  if (j >= n) return;
  const uint64_t c = k[j] >> shift;
  if (j == 0 || (k[j - 1] >> shift) != c) start[c] = j;
}

// the values the segmented sums add, by the member bits of a key
struct PolyVals {  // a polygon's area and fan determinant
  const double* area;
  const double* det;
  __device__ __forceinline__ void operator()(uint64_t p, double* out) const {
    out[0] = area[p];
    out[1] = det[p];
  }
};
struct EdgeLength {  // the length of the edge at sorted position i
  const uint64_t* sk;
  const float* xyz;
  __device__ __forceinline__ void operator()(uint64_t i, double* out) const {
    const float* a = xyz + 3 * (sk[i] >> 32);
    const float* b = xyz + 3 * ((sk[i] >> 1) & 0x7fffffffu);
    const double dx = (double)b[0] - (double)a[0], dy = (double)b[1] - (double)a[1], dz = (double)b[2] - (double)a[2];
    out[0] = sqrt(dx * dx + dy * dy + dz * dz);
  }
};

// per boundary vertex: its loop's vertex count, first vertex, simplicity
__global__ void __launch_bounds__(TNP_BLOCK)
k_loop_verts(int* vparent, const int* __restrict__ bdeg, const int64_t* __restrict__ vrank, int64_t V,
             int64_t* __restrict__ lcnt, int64_t L) {
  const int64_t v = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  const bool active = v < V && bdeg[v] > 0;
  int l = 0;
  if (active) {
    const int r = uf_find(vparent, (int)v);
    l = (int)vrank[r];
    if (r == (int)v) lcnt[LK_FIRST * L + l] = v;
    if (bdeg[v] != 2) lcnt[LK_NONSIMPLE * L + l] = 1;
  }
  wave_classes(active, l,
               [&](bool in, int c0, int leader) { class_add(in, leader, lcnt + LK_NVERT * L, c0, 1); });
}

// (loop << nbits) | sorted position of every boundary edge, appended in any
// order (the keys are distinct: the sort fixes the order); cur zeroed
__global__ void __launch_bounds__(TNP_BLOCK)
k_loop_keys(const uint64_t* __restrict__ sk, int64_t n, int* vparent, const int64_t* __restrict__ vrank, int nbits,
            uint64_t* __restrict__ keys, int64_t B, unsigned long long* __restrict__ cur) {
  const int64_t i = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  const bool lone = i < n && lone_run(sk, n, i);
  const uint64_t m = __ballot(lone);
  if (!m) return;
  unsigned long long base = 0;
  if (tnp::lane() == 0) base = atomicAdd(cur, (unsigned long long)__popcll(m));
  base = __shfl(base, 0, 64);
  if (lone) {
    const int64_t at = (int64_t)base + tnp::mbcnt(m);
    const uint64_t l = (uint64_t)vrank[uf_find(vparent, (int)(sk[i] >> 32))];
    if (at < B) keys[at] = (l << nbits) | (uint64_t)i;
  }
}

__global__ void __launch_bounds__(TNP_BLOCK)
k_comp_rows(int64_t C, const int64_t* __restrict__ cnt, const int64_t* __restrict__ start,
            const uint32_t* __restrict__ box, const double* __restrict__ sums, tnp_component* __restrict__ out) {
  const int64_t c = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  if (c >= C) return;
  tnp_component r;
  r.first_polygon = cnt[CK_FIRST * C + c];
  r.n_polygons = start[c + 1] - start[c];
  r.n_indices = cnt[CK_NIDX * C + c];
  r.n_vertices = cnt[CK_NVERT * C + c];
  r.n_edges = cnt[CK_EDGES * C + c];
  r.e_boundary = cnt[CK_BOUND * C + c];
  r.e_manifold = cnt[CK_MANI * C + c];
  r.e_nonmanifold = cnt[CK_NONM * C + c];
  r.e_misoriented = cnt[CK_MISO * C + c];
  r.euler = r.n_vertices - r.n_edges + r.n_polygons;
  r.area = sums[c];
  r.volume = sums[C + c] / 6.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    r.lo[k] = ord_f32(box[(int64_t)k * C + c]);
    r.hi[k] = ord_f32(box[(int64_t)(3 + k) * C + c]);
  }
  out[c] = r;
}

// lkeys: the sorted loop keys (a loop's first key is its smallest edge)
__global__ void __launch_bounds__(TNP_BLOCK)
k_loop_rows(int64_t L, const int64_t* __restrict__ lcnt, const int64_t* __restrict__ lstart,
            const uint64_t* __restrict__ lkeys, int nbits, const int32_t* __restrict__ sp,
            const int32_t* __restrict__ label, const double* __restrict__ length,
            tnp_boundary_loop* __restrict__ out) {
  const int64_t l = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  if (l >= L) return;
  tnp_boundary_loop r;
  r.first_vertex = lcnt[LK_FIRST * L + l];
  r.n_edges = lstart[l + 1] - lstart[l];
  r.n_vertices = lcnt[LK_NVERT * L + l];
  r.component = label[sp[lkeys[lstart[l]] & ((1ull << nbits) - 1ull)]];
  r.length = length[l];
  r.simple = lcnt[LK_NONSIMPLE * L + l] == 0;
  r.reserved = 0;
  out[l] = r;
}

void drop_tables(tnp_topology* t) {
  if (t->label) (void)hipFree(t->label);
  if (t->comps) (void)hipFree(t->comps);
  if (t->loops) (void)hipFree(t->loops);
  t->label = nullptr, t->comps = nullptr, t->loops = nullptr;
  t->P = t->C = t->L = 0;
}

// the state of one build, handed from stage to stage
struct TopoBuild {
  tnp_topology* t;
  const float* xyz;
  int64_t V;
  const int64_t *off, *idx;
  int64_t P;
  int connect;
  hipStream_t s;
  Scratch scr;
  Stages st;
  int64_t* ctr = nullptr;
  int64_t n = 0, C = 0, L = 0, B = 0;
  int vbits = 0, pbits = 0, nbits = 0, cbits = 0, lbits = 0;
  uint64_t *sk = nullptr, *spare = nullptr;  // the sorted keys; n words free once they are sorted
  int32_t* sp = nullptr;                     // the sorted keys' polygons
  int *parent = nullptr, *vparent = nullptr, *bdeg = nullptr;
  int64_t *prank = nullptr, *vrank = nullptr;
  int64_t *cnt = nullptr, *cstart = nullptr;
  uint32_t* box = nullptr;
  double *csum = nullptr, *parea = nullptr, *pdet = nullptr, *pieces = nullptr;
  size_t vsort_bytes = 0, psort_bytes = 0, lsort_bytes = 0;
  int edges(), classes(), tables(), components(), loops();  // the stages, in order
};

// stages check_edges, edge_sort
int TopoBuild::edges() {
  n = soup_offsets("topology", scr, off, idx, V, P, &ctr, TC_N, s);
  if (n < 0) return -1;
  vbits = bits_for(V), pbits = bits_for(P), nbits = bits_for(n);
  const int key_bits = 32 + vbits;
  const size_t pair_bytes = sort_pairs_u64_scratch_bytes(n, key_bits);
  {  // everything up to the class counts
    const size_t scan_words = (size_t)scan_tiles(P) + (size_t)scan_tiles(V) + 2;
    const size_t need = 2 * Scratch::pad(n * sizeof(uint64_t)) + 2 * Scratch::pad(n * sizeof(int32_t)) +
                        Scratch::pad(pair_bytes) + 2 * Scratch::pad(P * sizeof(int32_t)) +
                        Scratch::pad(P * sizeof(int64_t)) + 4 * Scratch::pad(V * sizeof(int32_t)) +
                        Scratch::pad(V * sizeof(int64_t)) + 2 * Scratch::pad(scan_words * sizeof(uint64_t));
    if (!scr.reserve(need)) return -1;
  }
  uint64_t* ka = scr.arr<uint64_t>(n);
  uint64_t* kb = scr.arr<uint64_t>(n);
  int32_t* pa = scr.arr<int32_t>(n);
  int32_t* pb = scr.arr<int32_t>(n);
  void* pair_scr = scr.get(pair_bytes);
  if (!ka || !kb || !pa || !pb || !pair_scr) return -1;
  SOUP_LAUNCH((k_soup_edges<false, true>), n, off, P, idx, n, V, ctr, ka, (uint8_t*)nullptr, pa);
  // the ids are read through from here on: the check's verdict first
  int64_t h[1];
  if (soup_verdict("topology", off, idx, V, ctr, h, 1, s)) return -1;
  st.mark();
  if (sort_pairs_u64(ka, kb, pa, pb, n, key_bits, pair_scr, pair_bytes, &sk, &sp, s)) return -1;
  spare = sk == ka ? kb : ka;
  st.mark();
  return 0;
}

// stages label_polygons, label_boundary: the classes and their counts C, L, B
int TopoBuild::classes() {
  parent = scr.arr<int>(P);
  int32_t* pflag = scr.arr<int32_t>(P);
  prank = scr.arr<int64_t>(P);
  if (!parent || !pflag || !prank) return -1;
  SOUP_LAUNCH(k_iota, P, parent, P);
  if (connect == 0) {
    SOUP_LAUNCH(k_union_edges, n, sk, sp, n, parent);
  } else {
    unsigned* vown = scr.arr<unsigned>(V);
    if (!vown) return -1;
    TNP_CHECK(hipMemsetAsync(vown, 0xFF, (size_t)V * sizeof(unsigned), s));
    SOUP_LAUNCH(k_vertex_owner, n, off, P, idx, n, vown);
    SOUP_LAUNCH(k_union_vertices, n, off, P, idx, n, vown, parent);
  }
  SOUP_LAUNCH(k_flag_roots, P, parent, (const int*)nullptr, P, pflag);
  if (scan_flags(scr, pflag, P, prank, ctr + TC_C, s)) return -1;
  st.mark();

  vparent = scr.arr<int>(V);
  bdeg = scr.arr<int>(V);
  int32_t* vflag = scr.arr<int32_t>(V);
  vrank = scr.arr<int64_t>(V);
  if (!vparent || !bdeg || !vflag || !vrank) return -1;
  TNP_CHECK(hipMemsetAsync(bdeg, 0, (size_t)(V > 0 ? V : 1) * sizeof(int), s));
  if (boundary_classes(scr, sk, n, V, vparent, bdeg, vflag, vrank, ctr, s)) return -1;
  int64_t h[TC_N];
  TNP_CHECK(hipMemcpyAsync(h, ctr, sizeof(h), hipMemcpyDeviceToHost, s));
  TNP_CHECK(hipStreamSynchronize(s));
  st.mark();
  C = h[TC_C], L = h[TC_L], B = h[TC_B];
  if (C < 1 || C > P || L < 0 || L > B) {
    tnp_set_error("topology: %lld components of %lld polygons, %lld loops of %lld boundary edges",
                  (long long)C, (long long)P, (long long)L, (long long)B);
    return -1;
  }
  cbits = bits_for(C), lbits = bits_for(L);
  if (lbits + nbits > 64) { tnp_set_error("topology: %lld loops over %lld indices do not fit a key", (long long)L, (long long)n); return -1; }
  return 0;
}

// stage tables_alloc: the handle's tables, the second scratch block, the per-component accumulators cleared
int TopoBuild::tables() {
  TNP_CHECK(hipMalloc(&t->label, (size_t)P * sizeof(int32_t)));
  TNP_CHECK(hipMalloc(&t->comps, (size_t)C * sizeof(tnp_component)));
  if (L > 0) TNP_CHECK(hipMalloc(&t->loops, (size_t)L * sizeof(tnp_boundary_loop)));
  vsort_bytes = sort_scratch_bytes(n, vbits + cbits);
  psort_bytes = sort_scratch_bytes(P, pbits + cbits);
  lsort_bytes = L > 0 ? sort_scratch_bytes(B, lbits + nbits) : 0;
  {  // everything after the class counts
    const size_t need = Scratch::pad(CK_N * C * sizeof(int64_t)) + Scratch::pad(6 * C * sizeof(uint32_t)) +
                        Scratch::pad((C + 1) * sizeof(int64_t)) + Scratch::pad(2 * C * sizeof(double)) +
                        2 * Scratch::pad(P * sizeof(double)) + Scratch::pad(2 * std::max(P, B) * sizeof(double)) +
                        Scratch::pad(n * sizeof(uint64_t)) + Scratch::pad(vsort_bytes) +
                        2 * Scratch::pad(P * sizeof(uint64_t)) + Scratch::pad(psort_bytes) +
                        Scratch::pad(LK_N * L * sizeof(int64_t)) + Scratch::pad((L + 1) * sizeof(int64_t)) +
                        Scratch::pad(L * sizeof(double)) + 2 * Scratch::pad(B * sizeof(uint64_t)) +
                        Scratch::pad(lsort_bytes) + Scratch::pad(sizeof(unsigned long long));
    if (!scr.reserve(need)) return -1;
  }
  cnt = scr.arr<int64_t>(CK_N * C);
  box = scr.arr<uint32_t>(6 * C);
  cstart = scr.arr<int64_t>(C + 1);
  csum = scr.arr<double>(2 * C);
  parea = scr.arr<double>(P);
  pdet = scr.arr<double>(P);
  pieces = scr.arr<double>(2 * std::max(P, B));
  if (!cnt || !box || !cstart || !csum || !parea || !pdet || !pieces) return -1;
  FillOp ops[3] = {{cnt, (uint64_t)(CK_N * C) * sizeof(int64_t), 0u},
                   {box, (uint64_t)(3 * C) * sizeof(uint32_t), 0xFFu},
                   {box + 3 * C, (uint64_t)(3 * C) * sizeof(uint32_t), 0u}};
  if (launch_fill(ops, 3, s)) return -1;
  st.mark();
  return 0;
}

// stages component_counts, vertex_sort, polygon_order, geometry: the labels and the component rows
int TopoBuild::components() {
  SOUP_LAUNCH(k_labels, P, parent, prank, P, t->label, cnt, C);
  SOUP_LAUNCH(k_comp_polys, P, xyz, off, idx, P, t->label, cnt, box, C, parea, pdet);
  SOUP_LAUNCH(k_edge_stats, n, sk, sp, n, t->label, cnt, C);
  st.mark();

  {  // distinct (label, vertex)
    uint64_t* va = spare;
    uint64_t* vb = scr.arr<uint64_t>(n);
    void* sscr = scr.get(vsort_bytes);
    if (!vb || !sscr) return -1;
    SOUP_LAUNCH(k_vertex_keys, n, off, P, idx, n, t->label, vbits, va);
    uint64_t* sv = nullptr;
    if (sort_keys_u64(va, vb, n, vbits + cbits, sscr, vsort_bytes, &sv, s)) return -1;
    SOUP_LAUNCH(k_key_runs, n, sv, n, vbits, cnt + CK_NVERT * C);
  }
  st.mark();

  // the polygons in (label, p) order
  uint64_t* spk = nullptr;
  uint64_t* qa = scr.arr<uint64_t>(P);
  uint64_t* qb = scr.arr<uint64_t>(P);
  void* sscr = scr.get(psort_bytes);
  if (!qa || !qb || !sscr) return -1;
  SOUP_LAUNCH(k_poly_keys, P, t->label, P, pbits, qa);
  if (sort_keys_u64(qa, qb, P, pbits + cbits, sscr, psort_bytes, &spk, s)) return -1;
  SOUP_LAUNCH(k_seg_starts, P, spk, P, pbits, C, cstart);
  st.mark();

  // area, volume
  hipLaunchKernelGGL((k_seg_pieces<2, PolyVals>), dim3(tnp_grid(P, SEG)), dim3(TNP_BLOCK), 0, s, spk, P, pbits,
                     PolyVals{parea, pdet}, pieces);
  hipLaunchKernelGGL(k_seg_final<2>, dim3(tnp_grid(C, TNP_WAVES)), dim3(TNP_BLOCK), 0, s, cstart, C, P, pieces,
                     csum);
  TNP_CHECK(hipGetLastError());
  SOUP_LAUNCH(k_comp_rows, C, C, cnt, cstart, box, csum, t->comps);
  st.mark();
  return 0;
}

// stage loops: the loop rows
int TopoBuild::loops() {
  if (L > 0) {
    int64_t* lcnt = scr.arr<int64_t>(LK_N * L);
    int64_t* lstart = scr.arr<int64_t>(L + 1);
    double* llen = scr.arr<double>(L);
    uint64_t* la = scr.arr<uint64_t>(B);
    uint64_t* lb = scr.arr<uint64_t>(B);
    void* sscr = scr.get(lsort_bytes);
    unsigned long long* cur = scr.arr<unsigned long long>(1);
    if (!lcnt || !lstart || !llen || !la || !lb || !sscr || !cur) return -1;
    TNP_CHECK(hipMemsetAsync(lcnt, 0, (size_t)(LK_N * L) * sizeof(int64_t), s));
    TNP_CHECK(hipMemsetAsync(cur, 0, sizeof(unsigned long long), s));
    SOUP_LAUNCH(k_loop_verts, V, vparent, bdeg, vrank, V, lcnt, L);
    SOUP_LAUNCH(k_loop_keys, n, sk, n, vparent, vrank, nbits, la, B, cur);
    uint64_t* sl = nullptr;
    if (sort_keys_u64(la, lb, B, lbits + nbits, sscr, lsort_bytes, &sl, s)) return -1;
    SOUP_LAUNCH(k_seg_starts, B, sl, B, nbits, L, lstart);
    hipLaunchKernelGGL((k_seg_pieces<1, EdgeLength>), dim3(tnp_grid(B, SEG)), dim3(TNP_BLOCK), 0, s, sl, B, nbits,
                       EdgeLength{sk, xyz}, pieces);
    hipLaunchKernelGGL(k_seg_final<1>, dim3(tnp_grid(L, TNP_WAVES)), dim3(TNP_BLOCK), 0, s, lstart, L, B, pieces,
                       llen);
    TNP_CHECK(hipGetLastError());
    SOUP_LAUNCH(k_loop_rows, L, L, lcnt, lstart, sl, nbits, sp, t->label, llen, t->loops);
  }
  st.mark();
  return 0;
}

}  // namespace

extern "C" int tnp_topology_create(tnp_topology** out, int device) { return handle_create("topology", out, device); }

extern "C" void tnp_topology_destroy(tnp_topology* t) { handle_destroy(t, drop_tables); }

extern "C" int tnp_debug_topology_stages(tnp_topology* t, int enable, double* ms, int n) {
  return handle_stages("topology", t, enable, ms, n);
}

extern "C" int tnp_topology_build(tnp_topology* t, const float* d_xyz, int64_t V, const int64_t* d_offsets,
                                  const int64_t* d_indices, int64_t P, int connect, int64_t* n_components,
                                  int64_t* n_loops, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (n_components) *n_components = 0;
  if (n_loops) *n_loops = 0;
  if (handle_use("topology", t)) return -1;
  TNP_CHECK(hipStreamSynchronize(s));  // (an earlier export may still read the tables)
  drop_tables(t);
  t->n_ms = 0;
  if (connect != 0 && connect != 1) { tnp_set_error("topology: connect = %d (0: edge, 1: vertex)", connect); return -1; }
  if (soup_args("topology", V, P, true, P > 0, d_xyz, d_offsets, d_indices)) return -1;
  if (P == 0) return 0;
  TopoBuild b{t, d_xyz, V, d_offsets, d_indices, P, connect, s, Scratch(s, "topology"), Stages(t->timed, s)};
  b.st.mark();
  if (b.edges() || b.classes() || b.tables() || b.components() || b.loops()) return -1;
  TNP_CHECK(hipStreamSynchronize(s));
  t->P = P, t->C = b.C, t->L = b.L;
  handle_keep_ms(t, b.st);
  if (n_components) *n_components = b.C;
  if (n_loops) *n_loops = b.L;
  return 0;
}

extern "C" int tnp_topology_export(tnp_topology* t, int32_t* d_label, tnp_component* d_components,
                                   tnp_boundary_loop* d_loops, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (handle_use("topology", t)) return -1;
  if (d_label && t->P > 0)
    TNP_CHECK(hipMemcpyAsync(d_label, t->label, (size_t)t->P * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
  if (d_components && t->C > 0)
    TNP_CHECK(hipMemcpyAsync(d_components, t->comps, (size_t)t->C * sizeof(tnp_component), hipMemcpyDeviceToDevice, s));
  if (d_loops && t->L > 0)
    TNP_CHECK(hipMemcpyAsync(d_loops, t->loops, (size_t)t->L * sizeof(tnp_boundary_loop), hipMemcpyDeviceToDevice, s));
  return 0;
}
