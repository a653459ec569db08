// tnp_simplify_*: the used vertices of a polygon soup clustered by the cells of
// a uniform grid, the soup rewritten over the cells' representatives and its
// duplicate polygons removed (include/tropical_hip.h has the definitions).
// The front is soup_host.h's; the used vertices, the class means, the drift
// and the rewrite are weld_common.h's, shared with tnp_weld_build, so each
// rule exists once.  tnp_simplify_build is its stages in order, one function
// each, with the state in a SimplifyBuild.
//
//   k_soup_offsets, k_weld_ids, k_weld_box, scan   as weld's check_used
//   k_simp_cells      one (cell key, id) pair per used vertex, in id order;
//                     the cell coordinate is floor of one rounded difference
//                     over one rounded quotient, unclamped (the host has
//                     refused a grid of more than 2^21 cells on an axis)
//   sort_pairs_u64    by cell key (stable: a cell's ids ascend, so a class is
//                     a run of equal keys and its first id is its smallest)
//   k_simp_heads, scan, k_simp_starts, k_simp_classes   a class starts where
//                     the key changes; map[v] = root[v] = the id at its start;
//                     the classes' sizes; their number (the scan's total) and
//                     the largest (one atomic per wave)
//   mode 0: class_means (weld's mode-1 rule: the (representative, id) sort, the
//                     fixed-shape double sums, one division, one rounding)
//   mode 1: class_means into a scratch copy, then k_simp_d2 (d2 to the mean, an
//                     integer minimum per class over its bit pattern),
//                     k_simp_pick (an integer minimum over the ids that reach
//                     it), k_simp_take (every member takes that member's bits)
//   k_weld_shift      max_shift
//   Rewrite           weld's rewrite, into scratch
//   k_simp_canon      per surviving polygon: the smallest rotation of its id
//                     sequence and of the reversed sequence, a 64-bit hash of
//                     each canonical form
//   sort_pairs_u64    (hash of the forward form, polygon), stable
//   k_simp_dups       per polygon: the run of its forward hash, and of its
//                     reversed form's hash, searched in the sorted keys; the
//                     earlier members compared id by id -- duplicate, folded;
//                     the hash only buckets, the comparison decides
//   scan (x 2), k_simp_rows, k_simp_copy   the output soup
// The number of launches is fixed; no kernel waits for another workgroup.
#include <math.h>
#include <string.h>

#include "../../include/tropical_hip_debug.h"
#include "kernels.h"
#include "weld_common.h"

struct tnp_simplify {
  int device = 0;
  int64_t* map = nullptr;      // [V]
  float* xyz = nullptr;        // [V x 3]
  int64_t* offsets = nullptr;  // [P' + 1]
  int64_t* indices = nullptr;  // [n_indices]
  int64_t* source = nullptr;   // [P']
  int64_t V = 0;
  tnp_simplify_stats st = {};
  bool timed = false;
  int n_ms = 0;
  double ms[TNP_SIMPLIFY_STAGES] = {};
};

namespace {

// the counters of a build (int64 words): SC_BAD, SC_LO* start at all ones, the
// others at zero; SC_SHIFT .. SC_PINCHED are weld_common.h's RW_* words
enum { SC_BAD, SC_LOX, SC_LOY, SC_LOZ, SC_HIX, SC_HIY, SC_HIZ, SC_NUSED, SC_NCELLS, SC_LARGEST, SC_NSEG,
       SC_SHIFT, SC_KEPT, SC_NPOLY, SC_NIDX, SC_PINCHED, SC_NPOLY2, SC_NIDX2, SC_FOLDED, SC_PINCHED2, SC_N };
static_assert(SC_KEPT == SC_SHIFT + RW_KEPT && SC_NPOLY == SC_SHIFT + RW_NPOLY && SC_NIDX == SC_SHIFT + RW_NIDX &&
              SC_PINCHED == SC_SHIFT + RW_PINCHED, "counter layout");

constexpr int CELL_BITS = 21;  // three cell coordinates fill 63 key bits

struct Grid {
  double lo[3], h;
  int bits;  // per cell coordinate
};

// the cell coordinate of the definitions, on the device and (for the box's
// upper corner) on the host: one rounded difference, one rounded quotient,
// nothing to fuse; monotone in x
__host__ __device__ __forceinline__ double cell_coord(double x, double lo, double h) { return floor((x - lo) / h); }

__global__ void __launch_bounds__(TNP_BLOCK)
k_simp_cells(const float* __restrict__ xyz, const int32_t* __restrict__ used, const int64_t* __restrict__ urank,
             int64_t V, int64_t U, Grid g, uint64_t* __restrict__ keys, int32_t* __restrict__ ids) {
  const int64_t v = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  if (v >= V || !used[v]) return;
  const int64_t j = urank[v];
  if (j >= U) return;
  const float* p = xyz + 3 * v;
  const uint64_t m = ((uint64_t)1 << g.bits) - 1;  // (never cuts: lo <= x <= hi, and hi's coordinate fits)
  uint64_t c[3];
#pragma unroll
  for (int q = 0; q < 3; ++q) c[q] = (uint64_t)(int64_t)cell_coord((double)p[q], g.lo[q], g.h) & m;
  keys[j] = (c[0] << (2 * g.bits)) | (c[1] << g.bits) | c[2];
  ids[j] = (int32_t)v;
}

// map[v] = root[v] = v: an unused vertex is a class of its own
__global__ void __launch_bounds__(TNP_BLOCK)
k_simp_identity(int64_t V, int64_t* __restrict__ map, int32_t* __restrict__ root) {
  const int64_t v = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  if (v >= V) return;
  map[v] = v;
  if (root) root[v] = (int32_t)v;
}

__global__ void __launch_bounds__(TNP_BLOCK)
k_simp_heads(const uint64_t* __restrict__ sk, int64_t U, int32_t* __restrict__ head) {
  const int64_t j = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  if (j < U) head[j] = j == 0 || sk[j] != sk[j - 1];
}

// cstart[c] of class c, in key order
__global__ void __launch_bounds__(TNP_BLOCK)
k_simp_starts(const int32_t* __restrict__ head, const int64_t* __restrict__ hrank, int64_t U,
              int64_t* __restrict__ cstart) {
  const int64_t j = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  if (j < U && head[j]) cstart[hrank[j]] = j;  // (hrank[j] <= j < U)
}

// every member's representative; the class's last member stores its size
__global__ void __launch_bounds__(TNP_BLOCK)
k_simp_classes(const int32_t* __restrict__ ids, const int32_t* __restrict__ head, const int64_t* __restrict__ hrank,
               const int64_t* __restrict__ cstart, int64_t U, int64_t V, int64_t* __restrict__ map,
               int32_t* __restrict__ root, int* __restrict__ csize, int64_t* __restrict__ wc) {
  const int64_t j = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  unsigned long long m = 0;
  if (j < U) {
    const int64_t j0 = cstart[hrank[j] + head[j] - 1];
    const int v = ids[j], r = (j0 >= 0 && j0 <= j) ? ids[j0] : v;
    if (v >= 0 && v < V && r >= 0 && r < V) {
      map[v] = r;
      root[v] = r;
      if (j + 1 == U || head[j + 1]) {
        csize[r] = (int)(j + 1 - j0);
        m = (unsigned long long)(j + 1 - j0);
      }
    }
  }
  m = wave_max_u64(m);
  if (tnp::lane() == 0 && m) atomicMax(reinterpret_cast<unsigned long long*>(wc + SC_LARGEST), m);
}

// mode 1: best[r] = the smallest d2(member, mean) of class r, as the bit
// pattern of a double that is never negative
__global__ void __launch_bounds__(TNP_BLOCK)
k_simp_d2(const float* __restrict__ xyz, const float* __restrict__ mean, const int32_t* __restrict__ used,
          const int32_t* __restrict__ root, int64_t V, unsigned long long* __restrict__ best) {
  const int64_t v = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  if (v >= V || !used[v]) return;
  atomicMin(best + root[v], (unsigned long long)__double_as_longlong(dist2(xyz + 3 * v, mean + 3 * v)));
}

// bestid[r] = the smallest id that reaches best[r]
__global__ void __launch_bounds__(TNP_BLOCK)
k_simp_pick(const float* __restrict__ xyz, const float* __restrict__ mean, const int32_t* __restrict__ used,
            const int32_t* __restrict__ root, int64_t V, const unsigned long long* __restrict__ best,
            unsigned int* __restrict__ bestid) {
  const int64_t v = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  if (v >= V || !used[v]) return;
  const int r = root[v];
  if ((unsigned long long)__double_as_longlong(dist2(xyz + 3 * v, mean + 3 * v)) == best[r])
    atomicMin(bestid + r, (unsigned int)v);
}

__global__ void __launch_bounds__(TNP_BLOCK)
k_simp_take(const float* __restrict__ xyz, const int32_t* __restrict__ used, const int32_t* __restrict__ root,
            const unsigned int* __restrict__ bestid, int64_t V, float* __restrict__ out) {
  const int64_t v = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  if (v >= V) return;
  int64_t w = v;
  if (used[v]) {
    const unsigned int b = bestid[root[v]];
    if ((int64_t)b < V) w = b;
  }
#pragma unroll
  for (int q = 0; q < 3; ++q) out[3 * v + q] = xyz[3 * w + q];
}

// ---- the duplicates ----
// element t of rotation r of a polygon's ids (d of them at a), forward or reversed
template <bool REV>
__device__ __forceinline__ int64_t rot_at(const int64_t* __restrict__ a, int d, int r, int t) {
  int e = r + t;
  e = e >= d ? e - d : e;
  return a[REV ? d - 1 - e : e];
}

// the start of the lexicographically smallest rotation (the first such start)
template <bool REV>
__device__ __forceinline__ int min_rotation(const int64_t* __restrict__ a, int d) {
  int best = 0;
  for (int r = 1; r < d; ++r) {
    for (int t = 0; t < d; ++t) {
      const int64_t x = rot_at<REV>(a, d, r, t), y = rot_at<REV>(a, d, best, t);
      if (x != y) {
        if (x < y) best = r;
        break;
      }
    }
  }
  return best;
}

__device__ __forceinline__ uint64_t mix64(uint64_t x) {
  x ^= x >> 30;
  x *= 0xbf58476d1ce4e5b9ull;
  x ^= x >> 27;
  x *= 0x94d049bb133111ebull;
  return x ^ (x >> 31);
}

template <bool REV>
__device__ __forceinline__ uint64_t canon_hash(const int64_t* __restrict__ a, int d, int r) {
  uint64_t h = mix64((uint64_t)d + 0x9e3779b97f4a7c15ull);
  for (int t = 0; t < d; ++t) h = mix64(h ^ (uint64_t)rot_at<REV>(a, d, r, t)) + 0x9e3779b97f4a7c15ull;
  return h;
}

// per surviving polygon: rot[p], rrot[p], the hashes of both canonical forms; pol[p] = p
__global__ void __launch_bounds__(TNP_BLOCK)
k_simp_canon(const int64_t* __restrict__ off, int64_t P2, const int64_t* __restrict__ idx,
             int32_t* __restrict__ rot, int32_t* __restrict__ rrot, uint64_t* __restrict__ hf,
             uint64_t* __restrict__ hr, uint64_t* __restrict__ keys, int32_t* __restrict__ pol) {
  const int64_t p = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  if (p >= P2) return;
  const int64_t* a = idx + off[p];
  const int d = (int)(off[p + 1] - off[p]);
  const int r = min_rotation<false>(a, d), rr = min_rotation<true>(a, d);
  rot[p] = r, rrot[p] = rr;
  const uint64_t h = canon_hash<false>(a, d, r);
  hf[p] = keys[p] = h;
  hr[p] = canon_hash<true>(a, d, rr);
  pol[p] = (int32_t)p;
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

// does polygon p's canonical form (REV: of its reversed sequence) equal the
// forward canonical form of an earlier polygon of the run of hash h
template <bool REV>
__device__ __forceinline__ bool earlier_equal(const int64_t* __restrict__ off, const int64_t* __restrict__ idx,
                                              const int32_t* __restrict__ rot, const uint64_t* __restrict__ sk,
                                              const int32_t* __restrict__ sv, int64_t P2, int64_t p, int r,
                                              uint64_t h) {
  const int64_t* a = idx + off[p];
  const int d = (int)(off[p + 1] - off[p]);
  for (int64_t j = lower_bound(sk, P2, h); j < P2 && sk[j] == h; ++j) {
    const int64_t q = sv[j];
    if (q >= p) break;  // (the sort is stable: a run's polygons ascend)
    if (q < 0 || off[q + 1] - off[q] != d) continue;
    const int64_t* b = idx + off[q];
    const int rq = rot[q];
    bool same = true;
    for (int t = 0; t < d && same; ++t) same = rot_at<REV>(a, d, r, t) == rot_at<false>(b, d, rq, t);
    if (same) return true;
  }
  return false;
}

__global__ void __launch_bounds__(TNP_BLOCK)
k_simp_dups(const int64_t* __restrict__ off, int64_t P2, const int64_t* __restrict__ idx,
            const int32_t* __restrict__ rot, const int32_t* __restrict__ rrot, const uint64_t* __restrict__ hf,
            const uint64_t* __restrict__ hr, const uint64_t* __restrict__ sk, const int32_t* __restrict__ sv,
            const int* __restrict__ pinched, int32_t* __restrict__ keep, int32_t* __restrict__ deg,
            int64_t* __restrict__ wc) {
  const int64_t p = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  bool kept = false, folded = false;
  if (p < P2) {
    kept = !earlier_equal<false>(off, idx, rot, sk, sv, P2, p, rot[p], hf[p]);
    folded = kept && earlier_equal<true>(off, idx, rot, sk, sv, P2, p, rrot[p], hr[p]);
    keep[p] = kept;
    deg[p] = kept ? (int32_t)(off[p + 1] - off[p]) : 0;
  }
  count_lanes(folded, wc + SC_FOLDED);
  count_lanes(kept && pinched[p], wc + SC_PINCHED2);
}

// thread 0 closes the offsets
__global__ void __launch_bounds__(TNP_BLOCK)
k_simp_rows(int64_t P2, const int32_t* __restrict__ keep, const int64_t* __restrict__ rank,
            const int64_t* __restrict__ noff, const int64_t* __restrict__ src, int64_t P3, int64_t N3,
            int64_t* __restrict__ out_off, int64_t* __restrict__ source) {
  const int64_t p = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  if (p == 0) out_off[P3] = N3;
  if (p >= P2 || !keep[p]) return;
  const int64_t k = rank[p];
  if (k >= P3) return;
  out_off[k] = noff[p];
  source[k] = src[p];
}

__global__ void __launch_bounds__(TNP_BLOCK)
k_simp_copy(const int64_t* __restrict__ off, int64_t P2, const int64_t* __restrict__ idx, int64_t N2,
            const int32_t* __restrict__ keep, const int64_t* __restrict__ noff, int64_t N3,
            int64_t* __restrict__ out_idx) {
  const int64_t i = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  if (i >= N2) return;
  const int64_t p = soup_polygon_of(off, P2, i);
  if (!keep[p]) return;
  const int64_t at = noff[p] + (i - off[p]);
  if (at < N3) out_idx[at] = idx[i];
}

void drop_simplify(tnp_simplify* h) {
  void* all[] = {h->map, h->xyz, h->offsets, h->indices, h->source};
  for (void* p : all)
    if (p) (void)hipFree(p);
  h->map = h->offsets = h->indices = h->source = nullptr;
  h->xyz = nullptr;
  h->V = 0;
  h->st = tnp_simplify_stats{};
}

// the state of one build, handed from stage to stage
struct SimplifyBuild {
  tnp_simplify* h;
  const float* xyz;
  int64_t V;
  const int64_t *off, *idx;
  int64_t P;
  double cell;
  int mode;
  hipStream_t s;
  Scratch scr;
  Stages st;
  int64_t *ctr = nullptr, *wc = nullptr;
  int64_t c[SC_N] = {};  // the counters as last read back
  int64_t n = 0, U = 0;
  Grid g = {};
  int32_t *used = nullptr, *root = nullptr, *ids = nullptr;
  int64_t* urank = nullptr;
  uint64_t* keys = nullptr;
  int* csize = nullptr;
  int64_t *off2 = nullptr, *idx2 = nullptr, *src2 = nullptr;  // the rewritten soup, before the duplicates go
  int* pinched = nullptr;
  tnp_simplify_stats ss = {};
  int read_counters();
  // the stages, in order
  int used_box(), cells(), sort_cells(), classes(), positions(), rewrite(), duplicates();
};

int SimplifyBuild::read_counters() {
  TNP_CHECK(hipMemcpyAsync(c, wc, sizeof(c), hipMemcpyDeviceToHost, s));
  TNP_CHECK(hipStreamSynchronize(s));
  return 0;
}

// stage check_used: the front, the used flags and ranks, the finite check, the box
int SimplifyBuild::used_box() {
  n = soup_offsets("simplify", scr, off, idx, V, P, &ctr, 2, s);
  if (n < 0) return -1;
  const int64_t Ub = V < n ? V : n;  // U is at most this
  {  // everything up to the classes
    const size_t need = Scratch::pad(SC_N * sizeof(int64_t)) + 3 * Scratch::pad(V * sizeof(int32_t)) +
                        Scratch::pad(V * sizeof(int64_t)) +
                        2 * Scratch::pad(((size_t)scan_tiles(V) + 1) * sizeof(uint64_t)) +
                        2 * Scratch::pad(Ub * sizeof(uint64_t)) + 3 * Scratch::pad(Ub * sizeof(int32_t)) +
                        2 * Scratch::pad((Ub + 1) * sizeof(int64_t)) +
                        Scratch::pad(sort_pairs_u64_scratch_bytes(Ub, 3 * CELL_BITS));
    if (!scr.reserve(need)) return -1;
  }
  wc = scr.arr<int64_t>(SC_N);
  used = scr.arr<int32_t>(V);
  root = scr.arr<int32_t>(V);
  csize = scr.arr<int>(V);
  urank = scr.arr<int64_t>(V);
  if (!wc || !used || !root || !csize || !urank) return -1;
  for (int i = 0; i < SC_N; ++i) c[i] = (i == SC_BAD || (i >= SC_LOX && i <= SC_LOZ)) ? -1 : 0;
  TNP_CHECK(hipMemcpyAsync(wc, c, sizeof(c), hipMemcpyHostToDevice, s));
  const uint64_t vb = (uint64_t)(V > 0 ? V : 1) * sizeof(int32_t);
  FillOp ops[2] = {{used, vb, 0u}, {csize, vb, 0u}};
  if (launch_fill(ops, 2, s)) return -1;
  SOUP_LAUNCH(k_weld_ids, n, off, P, idx, n, V, ctr, used);
  int64_t front[1];
  if (soup_verdict("simplify", off, idx, V, ctr, front, 1, s)) return -1;
  SOUP_LAUNCH(k_weld_box, V, xyz, used, V, wc + SC_LOX, wc + SC_HIX, wc + SC_BAD);
  if (scan_flags(scr, used, V, urank, wc + SC_NUSED, s)) return -1;
  if (read_counters()) return -1;
  st.mark();
  if (c[SC_BAD] != -1) {
    tnp_set_error("simplify: vertex %lld has a coordinate that is not finite", (long long)c[SC_BAD]);
    return -1;
  }
  U = c[SC_NUSED];
  if (U < 1 || U > V || U > n) {
    tnp_set_error("simplify: %lld used vertices of %lld", (long long)U, (long long)V);
    return -1;
  }
  ss.n_used = U;
  return 0;
}

// stage grid_keys: lo = the box's lower corner; an axis of more than
// 2^CELL_BITS cells is refused; the key takes the bits the cells present need
int SimplifyBuild::cells() {
  g.h = cell;
  double most = 1.0;
  for (int q = 0; q < 3; ++q) {
    g.lo[q] = (double)ord2f((uint32_t)c[SC_LOX + q]);
    // (the cell coordinate is monotone in x: the upper corner's is the largest)
    const double cnt = cell_coord((double)ord2f((uint32_t)c[SC_HIX + q]), g.lo[q], g.h) + 1.0;
    if (!(cnt <= (double)((int64_t)1 << CELL_BITS))) {
      tnp_set_error("simplify: axis %c needs %.0f cells of %g, more than 2^%d", "xyz"[q], cnt, cell, CELL_BITS);
      return -1;
    }
    most = cnt > most ? cnt : most;
  }
  g.bits = bits_for((int64_t)most);
  keys = scr.arr<uint64_t>(U);
  ids = scr.arr<int32_t>(U);
  if (!keys || !ids) return -1;
  SOUP_LAUNCH(k_simp_cells, V, xyz, used, urank, V, U, g, keys, ids);
  st.mark();
  return 0;
}

// stage cell_sort
int SimplifyBuild::sort_cells() {
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

// stage classes: the heads, the map, the sizes, the counts
int SimplifyBuild::classes() {
  int32_t* head = scr.arr<int32_t>(U);
  int64_t* hrank = scr.arr<int64_t>(U + 1);
  int64_t* cstart = scr.arr<int64_t>(U + 1);
  if (!head || !hrank || !cstart) return -1;
  TNP_CHECK(hipMalloc(&h->map, (size_t)V * sizeof(int64_t)));
  TNP_CHECK(hipMalloc(&h->xyz, (size_t)V * 3 * sizeof(float)));
  SOUP_LAUNCH(k_simp_identity, V, V, h->map, root);
  SOUP_LAUNCH(k_simp_heads, U, keys, U, head);
  if (scan_flags(scr, head, U, hrank, wc + SC_NCELLS, s)) return -1;
  // (a start the heads do not reach stays inside the sorted pairs)
  TNP_CHECK(hipMemsetAsync(cstart, 0, (size_t)(U + 1) * sizeof(int64_t), s));
  SOUP_LAUNCH(k_simp_starts, U, head, hrank, U, cstart);
  SOUP_LAUNCH(k_simp_classes, U, ids, head, hrank, cstart, U, V, h->map, root, csize, wc);
  if (read_counters()) return -1;
  st.mark();
  ss.n_cells = c[SC_NCELLS], ss.max_cell = c[SC_LARGEST];
  if (ss.n_cells < 1 || ss.n_cells > U || ss.max_cell < 1 || ss.max_cell > U) {
    tnp_set_error("simplify: %lld cells of %lld used vertices", (long long)ss.n_cells, (long long)U);
    return -1;
  }
  return 0;
}

// stage positions
int SimplifyBuild::positions() {
  if (ss.max_cell == 1) {  // (every class is one vertex: its own bits)
    SOUP_LAUNCH(k_weld_first, V, xyz, root, V, h->xyz);
  } else if (mode == 0) {
    if (class_means(scr, xyz, used, urank, root, csize, V, U, ss.n_cells, wc + SC_NSEG, h->xyz, s)) return -1;
  } else {
    if (!scr.reserve(Scratch::pad(3 * V * sizeof(float)) + Scratch::pad(V * sizeof(uint64_t)) +
                     Scratch::pad(V * sizeof(unsigned int))))
      return -1;
    float* mean = scr.arr<float>(3 * V);
    unsigned long long* best = scr.arr<unsigned long long>(V);
    unsigned int* bestid = scr.arr<unsigned int>(V);
    if (!mean || !best || !bestid) return -1;
    FillOp ops[2] = {{best, (uint64_t)V * sizeof(unsigned long long), 0xffu},
                     {bestid, (uint64_t)V * sizeof(unsigned int), 0xffu}};
    if (launch_fill(ops, 2, s)) return -1;
    if (class_means(scr, xyz, used, urank, root, csize, V, U, ss.n_cells, wc + SC_NSEG, mean, s)) return -1;
    SOUP_LAUNCH(k_simp_d2, V, xyz, mean, used, root, V, best);
    SOUP_LAUNCH(k_simp_pick, V, xyz, mean, used, root, V, best, bestid);
    SOUP_LAUNCH(k_simp_take, V, xyz, used, root, bestid, V, h->xyz);
  }
  SOUP_LAUNCH(k_weld_shift, V, xyz, h->xyz, used, V, wc + SC_SHIFT);
  st.mark();
  return 0;
}

// stage rewrite: weld's, into scratch
int SimplifyBuild::rewrite() {
  // this stage's arrays and the next one's, P and n bounding what survives
  const size_t sort_bytes = sort_pairs_u64_scratch_bytes(P, 64);
  {
    const size_t need = Rewrite::bytes(n, P) + 3 * Scratch::pad((P + 1) * sizeof(int64_t)) +
                        Scratch::pad(n * sizeof(int64_t)) + 5 * Scratch::pad(P * sizeof(int32_t)) +
                        4 * Scratch::pad(P * sizeof(uint64_t)) + Scratch::pad(sort_bytes) +
                        2 * Scratch::pad(P * sizeof(int32_t)) + 2 * Scratch::pad(P * sizeof(int64_t)) +
                        2 * Scratch::pad(((size_t)scan_tiles(P) + 1) * sizeof(uint64_t));
    if (!scr.reserve(need)) return -1;
  }
  Rewrite rw{off, idx, n, P, root, wc + SC_SHIFT};
  if (rw.count(scr, s) || read_counters() || rw.sane("simplify", c + SC_SHIFT)) return -1;
  const int64_t P2 = c[SC_NPOLY], N2 = c[SC_NIDX];
  off2 = scr.arr<int64_t>(P2 + 1);
  idx2 = scr.arr<int64_t>(N2);
  src2 = scr.arr<int64_t>(P2);
  if (!off2 || !idx2 || !src2) return -1;
  if (rw.fill(scr, P2, N2, off2, idx2, src2, s)) return -1;
  pinched = rw.pinched;
  st.mark();
  return 0;
}

// stage duplicates: the canonical forms, their buckets, the exact comparison, the output soup
int SimplifyBuild::duplicates() {
  const int64_t P2 = c[SC_NPOLY], N2 = c[SC_NIDX];
  int64_t P3 = 0, N3 = 0;
  int32_t *keep = nullptr;
  int64_t *rank = nullptr, *noff = nullptr;
  if (P2 > 0) {
    const size_t sort_bytes = sort_pairs_u64_scratch_bytes(P2, 64);
    int32_t* rot = scr.arr<int32_t>(P2);
    int32_t* rrot = scr.arr<int32_t>(P2);
    uint64_t* hf = scr.arr<uint64_t>(P2);
    uint64_t* hr = scr.arr<uint64_t>(P2);
    uint64_t* ka = scr.arr<uint64_t>(P2);
    uint64_t* kb = scr.arr<uint64_t>(P2);
    int32_t* va = scr.arr<int32_t>(P2);
    int32_t* vb = scr.arr<int32_t>(P2);
    void* sort_scr = scr.get(sort_bytes);
    keep = scr.arr<int32_t>(P2);
    int32_t* deg = scr.arr<int32_t>(P2);
    rank = scr.arr<int64_t>(P2);
    noff = scr.arr<int64_t>(P2);
    if (!rot || !rrot || !hf || !hr || !ka || !kb || !va || !vb || !sort_scr || !keep || !deg || !rank || !noff)
      return -1;
    uint64_t* sk = nullptr;
    int32_t* sv = nullptr;
    SOUP_LAUNCH(k_simp_canon, P2, off2, P2, idx2, rot, rrot, hf, hr, ka, va);
    if (sort_pairs_u64(ka, kb, va, vb, P2, 64, sort_scr, sort_bytes, &sk, &sv, s)) return -1;
    SOUP_LAUNCH(k_simp_dups, P2, off2, P2, idx2, rot, rrot, hf, hr, sk, sv, pinched, keep, deg, wc);
    if (scan_flags(scr, keep, P2, rank, wc + SC_NPOLY2, s)) return -1;
    if (scan_flags(scr, deg, P2, noff, wc + SC_NIDX2, s)) return -1;
    if (read_counters()) return -1;
    P3 = c[SC_NPOLY2], N3 = c[SC_NIDX2];
    if (P3 < 1 || P3 > P2 || N3 < 3 * P3 || N3 > N2 || c[SC_FOLDED] > P3 || c[SC_PINCHED2] > c[SC_PINCHED]) {
      tnp_set_error("simplify: %lld polygons of %lld kept with %lld ids of %lld", (long long)P3, (long long)P2,
                    (long long)N3, (long long)N2);
      return -1;
    }
  }
  TNP_CHECK(hipMalloc(&h->offsets, (size_t)(P3 + 1) * sizeof(int64_t)));
  if (P3 > 0) {
    TNP_CHECK(hipMalloc(&h->indices, (size_t)N3 * sizeof(int64_t)));
    TNP_CHECK(hipMalloc(&h->source, (size_t)P3 * sizeof(int64_t)));
    // (a position the copy does not reach stays a valid id)
    TNP_CHECK(hipMemsetAsync(h->indices, 0, (size_t)N3 * sizeof(int64_t), s));
    SOUP_LAUNCH(k_simp_rows, P2, P2, keep, rank, noff, src2, P3, N3, h->offsets, h->source);
    SOUP_LAUNCH(k_simp_copy, N2, off2, P2, idx2, N2, keep, noff, N3, h->indices);
  } else {
    TNP_CHECK(hipMemsetAsync(h->offsets, 0, sizeof(int64_t), s));
  }
  st.mark();
  ss.n_polygons = P3, ss.n_indices = N3, ss.n_dropped_polygons = P - P2, ss.n_duplicate_polygons = P2 - P3;
  ss.n_folded = P2 > 0 ? c[SC_FOLDED] : 0, ss.n_pinched = P2 > 0 ? c[SC_PINCHED2] : 0;
  const uint32_t sb = (uint32_t)c[SC_SHIFT];
  memcpy(&ss.max_shift, &sb, sizeof sb);
  return 0;
}

// P = 0: every vertex is unused -- the identity map, the input's bits, no polygon
int simplify_empty(tnp_simplify* h, const float* xyz, int64_t V, hipStream_t s) {
  TNP_CHECK(hipMalloc(&h->offsets, sizeof(int64_t)));
  TNP_CHECK(hipMemsetAsync(h->offsets, 0, sizeof(int64_t), s));
  if (V > 0) {
    TNP_CHECK(hipMalloc(&h->map, (size_t)V * sizeof(int64_t)));
    TNP_CHECK(hipMalloc(&h->xyz, (size_t)V * 3 * sizeof(float)));
    SOUP_LAUNCH(k_simp_identity, V, V, h->map, (int32_t*)nullptr);
    TNP_CHECK(hipMemcpyAsync(h->xyz, xyz, (size_t)V * 3 * sizeof(float), hipMemcpyDeviceToDevice, s));
  }
  TNP_CHECK(hipStreamSynchronize(s));
  return 0;
}

}  // namespace

extern "C" int tnp_simplify_create(tnp_simplify** out, int device) { return handle_create("simplify", out, device); }

extern "C" void tnp_simplify_destroy(tnp_simplify* h) { handle_destroy(h, drop_simplify); }

extern "C" int tnp_debug_simplify_stages(tnp_simplify* h, int enable, double* ms, int n) {
  return handle_stages("simplify", h, enable, ms, n);
}

extern "C" int tnp_simplify_build(tnp_simplify* h, const float* d_xyz, int64_t V, const int64_t* d_offsets,
                                  const int64_t* d_indices, int64_t P, float cell, int mode,
                                  tnp_simplify_stats* h_stats, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (h_stats) *h_stats = tnp_simplify_stats{};
  if (handle_use("simplify", h)) return -1;
  TNP_CHECK(hipStreamSynchronize(s));  // (an earlier export may still read the result)
  drop_simplify(h);
  h->n_ms = 0;
  if (!(cell > 0.f) || !isfinite(cell)) { tnp_set_error("simplify: cell = %g (finite, > 0)", (double)cell); return -1; }
  if (mode != 0 && mode != 1) { tnp_set_error("simplify: mode = %d (0: mean, 1: nearest)", mode); return -1; }
  if (soup_args("simplify", V, P, true, true, d_xyz, d_offsets, d_indices)) return -1;
  h->V = V;
  if (P == 0) {
    if (simplify_empty(h, d_xyz, V, s)) { drop_simplify(h); return -1; }
    return 0;
  }
  SimplifyBuild b{h, d_xyz, V, d_offsets, d_indices, P, (double)cell, mode, s, Scratch(s, "simplify"),
                  Stages(h->timed, s)};
  b.st.mark();
  if (b.used_box() || b.cells() || b.sort_cells() || b.classes() || b.positions() || b.rewrite() || b.duplicates()) {
    (void)hipStreamSynchronize(s);
    drop_simplify(h);
    return -1;
  }
  TNP_CHECK(hipStreamSynchronize(s));  // (the last stage's event; the scratch is freed behind it)
  handle_keep_ms(h, b.st);
  h->st = b.ss;
  if (h_stats) *h_stats = b.ss;
  return 0;
}

extern "C" int tnp_simplify_export(tnp_simplify* h, int64_t* d_map, float* d_xyz_out, int64_t* d_offsets,
                                   int64_t* d_indices, int64_t* d_source, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (handle_use("simplify", h)) return -1;
  const int64_t V = h->V, P2 = h->st.n_polygons, N2 = h->st.n_indices;
  if (d_map && h->map) TNP_CHECK(hipMemcpyAsync(d_map, h->map, (size_t)V * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
  if (d_xyz_out && h->xyz)
    TNP_CHECK(hipMemcpyAsync(d_xyz_out, h->xyz, (size_t)V * 3 * sizeof(float), hipMemcpyDeviceToDevice, s));
  if (d_offsets) {
    if (h->offsets)
      TNP_CHECK(hipMemcpyAsync(d_offsets, h->offsets, (size_t)(P2 + 1) * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
    else
      TNP_CHECK(hipMemsetAsync(d_offsets, 0, sizeof(int64_t), s));  // (no build: [0])
  }
  if (d_indices && N2 > 0)
    TNP_CHECK(hipMemcpyAsync(d_indices, h->indices, (size_t)N2 * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
  if (d_source && P2 > 0)
    TNP_CHECK(hipMemcpyAsync(d_source, h->source, (size_t)P2 * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
  return 0;
}
