// tnp_weld_*: the near-coincident vertices of a polygon soup welded by single
// linkage, and the soup rewritten over the clusters' representatives
// (include/tropical_hip.h has the definitions).  The front is soup_host.h's,
// the union-find and the segmented double sums are topo_common.h's, the used
// vertices, the class means, the drift and the rewrite are weld_common.h's
// (tnp_simplify_build shares them); tnp_weld_build is its stages in order, one
// function each, with the state in a WeldBuild.
//
//   k_soup_offsets, k_weld_ids   the soup's checks; used[v] = 1 per valid id
//   k_weld_box, scan             per used vertex: the finite check (the smallest
//                     offending id by an integer atomic), the bounding box (fp32
//                     as ordered integers, one atomic per wave and bound); the
//                     used vertices' ranks and their number
//   k_weld_cells      one (cell key, id) pair per used vertex, in id order
//   sort_pairs_u64    by cell key on the bits three cell coordinates need
//                     (stable: a cell's ids ascend)
//   k_weld_search     one thread per sorted pair: the 3 x 3 columns of cells
//                     about its own, each a contiguous key range found by a
//                     binary search of the sorted keys; the predicate on every
//                     candidate of a larger id, one uf_union per close pair,
//                     the pairs counted once (one atomic per wave)
//   k_weld_map, k_weld_roots   map[v] = uf_find(v); the classes' sizes by
//                     integer atomics; classes, clusters, the largest
//   k_weld_first      mode 0: every member takes its representative's bits
//   mode 1: k_weld_mkeys (representative << shift | id), sort_keys_u64,
//                     k_weld_heads + scan + k_weld_starts (a class starts at
//                     its representative), k_seg_pieces / k_seg_final (the
//                     coordinate sums in double, in the topology's fixed
//                     shape), k_weld_mean
//   k_weld_shift      max_shift: an integer maximum over fp32 bit patterns
//   k_weld_keep, scan per index: mapped id differs from its cyclic predecessor's
//   k_weld_degrees, scan (x 2)   the new degrees, the survivors, their offsets
//   k_weld_rows, k_weld_scatter  offsets, source and indices of the output
//   k_weld_pinched    per output position: the same id later in its polygon
//                     (the first finder of a polygon counts it)
// The number of launches is fixed; no kernel waits for another workgroup.
#include <math.h>
#include <string.h>

#include "../../include/tropical_hip_debug.h"
#include "kernels.h"
#include "weld_common.h"

struct tnp_weld {
  int device = 0;
  int64_t* map = nullptr;      // [V]
  float* xyz = nullptr;        // [V x 3]
  int64_t* offsets = nullptr;  // [P' + 1]
  int64_t* indices = nullptr;  // [n_indices]
  int64_t* source = nullptr;   // [P']
  int64_t V = 0;
  tnp_weld_stats st = {};
  bool timed = false;
  int n_ms = 0;
  double ms[TNP_WELD_STAGES] = {};
};

namespace {

// the counters of a build (int64 words, a block of their own behind the
// front's two): WC_BAD, WC_LO* start at all ones, the others at zero;
// WC_SHIFT .. WC_PINCHED are weld_common.h's RW_* words
enum { WC_BAD, WC_LOX, WC_LOY, WC_LOZ, WC_HIX, WC_HIY, WC_HIZ, WC_NUSED, WC_PAIRS, WC_CLASSES, WC_CLUSTERS,
       WC_LARGEST, WC_SHIFT, WC_KEPT, WC_NPOLY, WC_NIDX, WC_PINCHED, WC_NSEG, WC_N };
static_assert(WC_KEPT == WC_SHIFT + RW_KEPT && WC_NPOLY == WC_SHIFT + RW_NPOLY && WC_NIDX == WC_SHIFT + RW_NIDX &&
              WC_PINCHED == WC_SHIFT + RW_PINCHED, "counter layout");

constexpr int CELL_BITS = 21;          // three cell coordinates fill 63 key bits
constexpr double CELL_SLACK = 0x1p-10;  // h >= tol (1 + slack): DESIGN 7h

struct Grid {
  double lo[3], h;
  int bits;  // per cell coordinate
};

// the cell coordinate: monotone in x (a rounded difference, a rounded quotient,
// floor, clamp)
__device__ __forceinline__ int64_t cell_of(const Grid& g, int q, float x) {
  const double u = floor(((double)x - g.lo[q]) / g.h);
  const double top = (double)(((int64_t)1 << g.bits) - 1);
  return (int64_t)(u < 0.0 ? 0.0 : u > top ? top : u);
}

__global__ void __launch_bounds__(TNP_BLOCK)
k_weld_cells(const float* __restrict__ xyz, const int32_t* __restrict__ used, const int64_t* __restrict__ urank,
             int64_t V, int64_t U, Grid g, uint64_t* __restrict__ keys, int32_t* __restrict__ ids) {
  const int64_t v = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  if (v >= V || !used[v]) return;
  const int64_t j = urank[v];
  if (j >= U) return;
  const float* p = xyz + 3 * v;
  keys[j] = ((uint64_t)cell_of(g, 0, p[0]) << (2 * g.bits)) | ((uint64_t)cell_of(g, 1, p[1]) << g.bits) |
            (uint64_t)cell_of(g, 2, p[2]);
  ids[j] = (int32_t)v;
}

// the first position in [0, n) whose key is >= x
__device__ __forceinline__ int64_t lower_bound(const uint64_t* __restrict__ k, int64_t n, uint64_t x) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (k[mid] < x) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__global__ void __launch_bounds__(TNP_BLOCK)
k_weld_search(const uint64_t* __restrict__ keys, const int32_t* __restrict__ ids, int64_t U,
              const float* __restrict__ xyz, int64_t V, int bits, double tol2, int* parent,
              int64_t* __restrict__ wc) {
  const int64_t j = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  int64_t pairs = 0;
  if (j < U) {
    const int v = ids[j];
    const uint64_t key = keys[j], m = ((uint64_t)1 << bits) - 1;
    const int64_t cx = (int64_t)(key >> (2 * bits)), cy = (int64_t)((key >> bits) & m), cz = (int64_t)(key & m);
    const float p[3] = {xyz[3 * (int64_t)v], xyz[3 * (int64_t)v + 1], xyz[3 * (int64_t)v + 2]};
    const int64_t z0 = cz > 0 ? cz - 1 : 0, z1 = cz < (int64_t)m ? cz + 1 : (int64_t)m;
    for (int64_t x = cx - 1; x <= cx + 1; ++x) {
      if (x < 0 || x > (int64_t)m) continue;
      for (int64_t y = cy - 1; y <= cy + 1; ++y) {
        if (y < 0 || y > (int64_t)m) continue;
        // the cells (x, y, z0 .. z1) are one run of the sorted keys
        const uint64_t base = ((uint64_t)x << (2 * bits)) | ((uint64_t)y << bits);
        const uint64_t k1 = base | (uint64_t)z1;
        for (int64_t e = lower_bound(keys, U, base | (uint64_t)z0); e < U && keys[e] <= k1; ++e) {
          const int w = ids[e];
          if (w <= v || w >= V) continue;  // (each pair by its smaller id)
          if (dist2(p, xyz + 3 * (int64_t)w) <= tol2) {
            uf_union(parent, v, w);
            ++pairs;
          }
        }
      }
    }
  }
  pairs = tnp::wave_sum(pairs);
  if (tnp::lane() == 0 && pairs)
    atomicAdd(reinterpret_cast<unsigned long long*>(wc + WC_PAIRS), (unsigned long long)pairs);
}

// map[v] and root[v] = the class's smallest id; csize[root] += 1 per used member
__global__ void __launch_bounds__(TNP_BLOCK)
k_weld_map(int* parent, const int32_t* __restrict__ used, int64_t V, int64_t* __restrict__ map,
           int32_t* __restrict__ root, int* __restrict__ csize) {
  const int64_t v = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  if (v >= V) return;
  const int r = uf_find(parent, (int)v);
  map[v] = r;
  root[v] = r;
  if (used && used[v]) atomicAdd(csize + r, 1);
}

__global__ void __launch_bounds__(TNP_BLOCK)
k_weld_roots(const int32_t* __restrict__ root, const int32_t* __restrict__ used, const int* __restrict__ csize,
             int64_t V, int64_t* __restrict__ wc) {
  const int64_t v = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  const bool cls = v < V && used[v] && root[v] == (int)v;
  const int m = cls ? csize[v] : 0;
  count_lanes(cls, wc + WC_CLASSES);
  count_lanes(m >= 2, wc + WC_CLUSTERS);
  const unsigned long long mx = wave_max_u64((unsigned long long)m);
  if (tnp::lane() == 0 && mx) atomicMax(reinterpret_cast<unsigned long long*>(wc + WC_LARGEST), mx);
}

void drop_weld(tnp_weld* h) {
  void* all[] = {h->map, h->xyz, h->offsets, h->indices, h->source};
  for (void* p : all)
    if (p) (void)hipFree(p);
  h->map = h->offsets = h->indices = h->source = nullptr;
  h->xyz = nullptr;
  h->V = 0;
  h->st = tnp_weld_stats{};
}

// the state of one build, handed from stage to stage
struct WeldBuild {
  tnp_weld* h;
  const float* xyz;
  int64_t V;
  const int64_t *off, *idx;
  int64_t P;
  double tol;
  int mode;
  hipStream_t s;
  Scratch scr;
  Stages st;
  int64_t *ctr = nullptr, *wc = nullptr;
  int64_t c[WC_N] = {};  // the counters as last read back
  int64_t n = 0, U = 0;
  Grid g = {};
  int32_t *used = nullptr, *root = nullptr, *ids = nullptr;
  int64_t* urank = nullptr;
  uint64_t* keys = nullptr;
  int *parent = nullptr, *csize = nullptr;
  tnp_weld_stats ws = {};
  int read_counters();
  int used_box(), cells(), sort_cells(), search(), clusters(), positions(), rewrite();  // the stages, in order
};

int WeldBuild::read_counters() {
  TNP_CHECK(hipMemcpyAsync(c, wc, sizeof(c), hipMemcpyDeviceToHost, s));
  TNP_CHECK(hipStreamSynchronize(s));
  return 0;
}

// stage check_used: the front, the used flags and ranks, the finite check, the box
int WeldBuild::used_box() {
  n = soup_offsets("weld", scr, off, idx, V, P, &ctr, 2, s);
  if (n < 0) return -1;
  {  // everything up to the search
    const size_t need = Scratch::pad(WC_N * sizeof(int64_t)) + 4 * Scratch::pad(V * sizeof(int32_t)) +
                        Scratch::pad(V * sizeof(int64_t)) +
                        Scratch::pad(((size_t)scan_tiles(V) + 1) * sizeof(uint64_t));
    if (!scr.reserve(need)) return -1;
  }
  wc = scr.arr<int64_t>(WC_N);
  used = scr.arr<int32_t>(V);
  root = scr.arr<int32_t>(V);
  parent = scr.arr<int>(V);
  csize = scr.arr<int>(V);
  urank = scr.arr<int64_t>(V);
  if (!wc || !used || !root || !parent || !csize || !urank) return -1;
  for (int i = 0; i < WC_N; ++i) c[i] = (i == WC_BAD || (i >= WC_LOX && i <= WC_LOZ)) ? -1 : 0;
  TNP_CHECK(hipMemcpyAsync(wc, c, sizeof(c), hipMemcpyHostToDevice, s));
  const uint64_t vb = (uint64_t)(V > 0 ? V : 1) * sizeof(int32_t);
  FillOp ops[2] = {{used, vb, 0u}, {csize, vb, 0u}};
  if (launch_fill(ops, 2, s)) return -1;
  SOUP_LAUNCH(k_weld_ids, n, off, P, idx, n, V, ctr, used);
  int64_t front[1];
  if (soup_verdict("weld", off, idx, V, ctr, front, 1, s)) return -1;
  SOUP_LAUNCH(k_weld_box, V, xyz, used, V, wc + WC_LOX, wc + WC_HIX, wc + WC_BAD);
  if (scan_flags(scr, used, V, urank, wc + WC_NUSED, s)) return -1;
  if (read_counters()) return -1;
  st.mark();
  if (c[WC_BAD] != -1) {
    tnp_set_error("weld: vertex %lld has a coordinate that is not finite", (long long)c[WC_BAD]);
    return -1;
  }
  U = c[WC_NUSED];
  if (U < 1 || U > V || U > n) { tnp_set_error("weld: %lld used vertices of %lld", (long long)U, (long long)V); return -1; }
  ws.n_used = U;
  return 0;
}

// stage grid_keys: h = max(tol (1 + slack), largest extent / 2^CELL_BITS), any
// positive h when both are 0; the key takes the bits the cells present need
int WeldBuild::cells() {
  double ext = 0.0;
  for (int q = 0; q < 3; ++q) {
    g.lo[q] = (double)ord2f((uint32_t)c[WC_LOX + q]);
    const double e = (double)ord2f((uint32_t)c[WC_HIX + q]) - g.lo[q];
    ext = e > ext ? e : ext;
  }
  g.h = fmax(tol * (1.0 + CELL_SLACK), ext / (double)((int64_t)1 << CELL_BITS));
  if (!(g.h > 0.0)) g.h = 1.0;
  const double cells_d = floor(ext / g.h) + 2.0;  // (one more than the largest coordinate can reach)
  g.bits = cells_d >= (double)((int64_t)1 << CELL_BITS) ? CELL_BITS : bits_for((int64_t)cells_d);
  keys = scr.arr<uint64_t>(U);
  ids = scr.arr<int32_t>(U);
  if (!keys || !ids) return -1;
  SOUP_LAUNCH(k_weld_cells, V, xyz, used, urank, V, U, g, keys, ids);
  st.mark();
  return 0;
}

// stage cell_sort
int WeldBuild::sort_cells() {
  const int key_bits = 3 * g.bits;
  const size_t sort_bytes = sort_pairs_u64_scratch_bytes(U, key_bits);
  uint64_t* kb = scr.arr<uint64_t>(U);
  int32_t* vb = scr.arr<int32_t>(U);
  void* sort_scr = scr.get(sort_bytes);
  if (!kb || !vb || !sort_scr) return -1;
  if (sort_pairs_u64(keys, kb, ids, vb, U, key_bits, sort_scr, sort_bytes, &keys, &ids, s)) return -1;
  st.mark();
  return 0;
}

// stage search: the close pairs and their unions
int WeldBuild::search() {
  SOUP_LAUNCH(k_iota, V, parent, V);
  SOUP_LAUNCH(k_weld_search, U, keys, ids, U, xyz, V, g.bits, tol * tol, parent, wc);
  st.mark();
  return 0;
}

// stage clusters: the map, the classes' sizes and their counts
int WeldBuild::clusters() {
  TNP_CHECK(hipMalloc(&h->map, (size_t)V * sizeof(int64_t)));
  TNP_CHECK(hipMalloc(&h->xyz, (size_t)V * 3 * sizeof(float)));
  SOUP_LAUNCH(k_weld_map, V, parent, used, V, h->map, root, csize);
  SOUP_LAUNCH(k_weld_roots, V, root, used, csize, V, wc);
  if (read_counters()) return -1;
  st.mark();
  ws.n_pairs = c[WC_PAIRS], ws.n_clusters = c[WC_CLUSTERS], ws.n_merged = U - c[WC_CLASSES];
  ws.max_cluster = c[WC_LARGEST];
  if (c[WC_CLASSES] < 1 || c[WC_CLASSES] > U || ws.n_clusters > c[WC_CLASSES] || ws.max_cluster > U) {
    tnp_set_error("weld: %lld classes of %lld used vertices", (long long)c[WC_CLASSES], (long long)U);
    return -1;
  }
  return 0;
}

// stage positions
int WeldBuild::positions() {
  if (mode == 0 || ws.n_clusters == 0) {
    SOUP_LAUNCH(k_weld_first, V, xyz, root, V, h->xyz);
  } else {
    if (class_means(scr, xyz, used, urank, root, csize, V, U, c[WC_CLASSES], wc + WC_NSEG, h->xyz, s)) return -1;
  }
  SOUP_LAUNCH(k_weld_shift, V, xyz, h->xyz, used, V, wc + WC_SHIFT);
  st.mark();
  return 0;
}

// stage rewrite: the keep flags, the new degrees, the survivors and the output soup
int WeldBuild::rewrite() {
  if (!scr.reserve(Rewrite::bytes(n, P))) return -1;
  Rewrite rw{off, idx, n, P, root, wc + WC_SHIFT};
  if (rw.count(scr, s) || read_counters() || rw.sane("weld", c + WC_SHIFT)) return -1;
  const int64_t P2 = c[WC_NPOLY], N2 = c[WC_NIDX];
  TNP_CHECK(hipMalloc(&h->offsets, (size_t)(P2 + 1) * sizeof(int64_t)));
  if (P2 > 0) {
    TNP_CHECK(hipMalloc(&h->indices, (size_t)N2 * sizeof(int64_t)));
    TNP_CHECK(hipMalloc(&h->source, (size_t)P2 * sizeof(int64_t)));
  }
  if (rw.fill(scr, P2, N2, h->offsets, h->indices, h->source, s)) return -1;
  if (read_counters()) return -1;
  st.mark();
  ws.n_polygons = P2, ws.n_indices = N2, ws.n_dropped_polygons = P - P2, ws.n_pinched = c[WC_PINCHED];
  const uint32_t sb = (uint32_t)c[WC_SHIFT];
  memcpy(&ws.max_shift, &sb, sizeof sb);
  return 0;
}

// P = 0: every vertex is unused -- the identity map, the input's bits, no polygon
int weld_empty(tnp_weld* h, const float* xyz, int64_t V, hipStream_t s) {
  TNP_CHECK(hipMalloc(&h->offsets, sizeof(int64_t)));
  TNP_CHECK(hipMemsetAsync(h->offsets, 0, sizeof(int64_t), s));
  if (V > 0) {
    Scratch scr(s, "weld");
    int* parent = scr.arr<int>(V);
    int32_t* root = scr.arr<int32_t>(V);
    if (!parent || !root) return -1;
    TNP_CHECK(hipMalloc(&h->map, (size_t)V * sizeof(int64_t)));
    TNP_CHECK(hipMalloc(&h->xyz, (size_t)V * 3 * sizeof(float)));
    SOUP_LAUNCH(k_iota, V, parent, V);
    SOUP_LAUNCH(k_weld_map, V, parent, (const int32_t*)nullptr, V, h->map, root, (int*)nullptr);
    TNP_CHECK(hipMemcpyAsync(h->xyz, xyz, (size_t)V * 3 * sizeof(float), hipMemcpyDeviceToDevice, s));
    TNP_CHECK(hipStreamSynchronize(s));  // (the scratch is freed on the way out)
  }
  TNP_CHECK(hipStreamSynchronize(s));
  return 0;
}

}  // namespace

extern "C" int tnp_weld_create(tnp_weld** out, int device) { return handle_create("weld", out, device); }

extern "C" void tnp_weld_destroy(tnp_weld* w) { handle_destroy(w, drop_weld); }

extern "C" int tnp_debug_weld_stages(tnp_weld* w, int enable, double* ms, int n) {
  return handle_stages("weld", w, enable, ms, n);
}

extern "C" int tnp_weld_build(tnp_weld* w, const float* d_xyz, int64_t V, const int64_t* d_offsets,
                              const int64_t* d_indices, int64_t P, float tol, int mode, tnp_weld_stats* h_stats,
                              void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (h_stats) *h_stats = tnp_weld_stats{};
  if (handle_use("weld", w)) return -1;
  TNP_CHECK(hipStreamSynchronize(s));  // (an earlier export may still read the result)
  drop_weld(w);
  w->n_ms = 0;
  if (!(tol >= 0.f) || !isfinite(tol)) { tnp_set_error("weld: tol = %g (finite, >= 0)", (double)tol); return -1; }
  if (mode != 0 && mode != 1) { tnp_set_error("weld: mode = %d (0: first, 1: mean)", mode); return -1; }
  if (soup_args("weld", V, P, true, true, d_xyz, d_offsets, d_indices)) return -1;
  w->V = V;
  if (P == 0) {
    if (weld_empty(w, d_xyz, V, s)) { drop_weld(w); return -1; }
    return 0;
  }
  WeldBuild b{w, d_xyz, V, d_offsets, d_indices, P, (double)tol, mode, s, Scratch(s, "weld"), Stages(w->timed, s)};
  b.st.mark();
  if (b.used_box() || b.cells() || b.sort_cells() || b.search() || b.clusters() || b.positions() || b.rewrite()) {
    (void)hipStreamSynchronize(s);
    drop_weld(w);
    return -1;
  }
  TNP_CHECK(hipStreamSynchronize(s));  // (the last stage's event)
  handle_keep_ms(w, b.st);
  w->st = b.ws;
  if (h_stats) *h_stats = b.ws;
  return 0;
}

extern "C" int tnp_weld_export(tnp_weld* w, int64_t* d_map, float* d_xyz_out, int64_t* d_offsets, int64_t* d_indices,
                               int64_t* d_source, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (handle_use("weld", w)) return -1;
  const int64_t V = w->V, P2 = w->st.n_polygons, N2 = w->st.n_indices;
  if (d_map && w->map) TNP_CHECK(hipMemcpyAsync(d_map, w->map, (size_t)V * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
  if (d_xyz_out && w->xyz)
    TNP_CHECK(hipMemcpyAsync(d_xyz_out, w->xyz, (size_t)V * 3 * sizeof(float), hipMemcpyDeviceToDevice, s));
  if (d_offsets) {
    if (w->offsets)
      TNP_CHECK(hipMemcpyAsync(d_offsets, w->offsets, (size_t)(P2 + 1) * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
    else
      TNP_CHECK(hipMemsetAsync(d_offsets, 0, sizeof(int64_t), s));  // (no build: [0])
  }
  if (d_indices && N2 > 0)
    TNP_CHECK(hipMemcpyAsync(d_indices, w->indices, (size_t)N2 * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
  if (d_source && P2 > 0)
    TNP_CHECK(hipMemcpyAsync(d_source, w->source, (size_t)P2 * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
  return 0;
}
