// tnp_holes_*: the boundary loops of a polygon soup as ordered cycles, and the
// caps that close them (include/tropical_hip.h has the definitions).  The
// front half is the topology's (soup_host.h's front, topo_common.h's
// boundary_classes), so the loops get the same numbers; tnp_holes_build is
// its stages in order, one function each, with the state in a HolesBuild.
//
//   k_soup_offsets, k_soup_edges    the soup's checks, one directed-edge key
//                     per index (no polygon: the direction is the key's bit 0)
//   sort_keys_u64     the keys on the bits the ids need
//   boundary_classes  the loops and their numbers
//   k_cap_edges       per edge used once, a -> b in its polygon: succ[b] = a,
//                     kept as pred[a] = b, which is what the ranking follows
//                     (a plain store: a vertex of a loop that is capped is
//                     the head of one reversed edge and the tail of one, and
//                     no other loop's pred is read), and the out-degree of b
//                     by an integer atomic
//   k_hole_verts      per boundary vertex: its loop, the loop's first vertex,
//                     edge count (the out-degrees add up to it) and flags
//                     (a vertex with other than 2 boundary edges; one that is
//                     not the tail of exactly one reversed edge -- its
//                     in-degree is then not 1 either), one atomic per wave
//                     and loop present in it
//   k_hole_status     per loop: status, the capped loops' flags and lengths
//   scan (x 3)        cycle numbers, cycle offsets, ranks among the star cycles
//   k_cycle_rows      cycle_loop, cycle_offsets, the star ranks
//   k_flag_cverts, scan, k_rank_init   the capped loops' vertices compacted;
//                     one word (pointer : 32 | distance : 32) each, toward
//                     the loop's first vertex along pred
//   k_rank_round      pointer doubling, ceil(log2(longest capped loop)) rounds
//                     ping-ponged between two arrays
//   k_cycle_scatter   cycle_vertices[offset + distance] = vertex
// tnp_holes_caps: mode 0 copies the cycles; mode 1 is k_star_caps (the
// triangles, and one key per cycle position), k_seg_pieces / k_seg_final (the
// coordinate sums in double, in the topology's fixed shape) and k_star_centres.
// The number of launches is fixed but for the doubling rounds; no thread
// follows a chain of successors, and no kernel waits for another workgroup.
#include <string.h>

#include "../../include/tropical_hip_debug.h"
#include "kernels.h"
#include "topo_common.h"

struct tnp_holes {
  int device = 0;
  int32_t* status = nullptr;        // [L]
  int64_t* cycle_loop = nullptr;    // [K]
  int64_t* cycle_offsets = nullptr; // [K + 1]
  int64_t* cycle_star = nullptr;    // [K]: the rank among the cycles of 4 or more edges
  int64_t* cycle_vertices = nullptr;  // [M]
  int64_t V = 0, n_star = 0;
  tnp_hole_stats st = {};
  bool timed = false;
  int n_ms = 0;
  double ms[TNP_HOLES_STAGES] = {};
};

namespace {

enum { HF_NONSIMPLE = 1, HF_UNORIENTED = 2 };
// the counters of a build after the topology's (int64 words)
enum { HC_CAPPED = TC_N, HC_NIDX, HC_NSTAR, HC_NCV, HC_NONSIMPLE, HC_UNORIENTED, HC_TOOLONG, HC_NTRI, HC_LONGEST, HC_N };

__global__ void __launch_bounds__(TNP_BLOCK)
k_cap_edges(const uint64_t* __restrict__ sk, int64_t n, int* __restrict__ pred, int* __restrict__ outd) {
  const int64_t i = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  if (i >= n || !lone_run(sk, n, i)) return;
  const uint64_t x = sk[i];
  const int lo = (int)(x >> 32), hi = (int)((x >> 1) & 0x7fffffffu);
  const int from = (x & 1) ? hi : lo, to = (x & 1) ? lo : hi;  // the polygon's direction
  pred[from] = to;
  atomicAdd(outd + to, 1);
}

__global__ void __launch_bounds__(TNP_BLOCK)
k_hole_verts(int* vparent, const int* __restrict__ bdeg, const int* __restrict__ outd,
             const int64_t* __restrict__ vrank, int64_t V, int32_t* __restrict__ vloop, int64_t* __restrict__ lfirst,
             int64_t* __restrict__ ledges, int* __restrict__ lflags) {
  const int64_t v = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  const bool active = v < V && bdeg[v] > 0;
  int l = 0, od = 0, bits = 0;
  if (active) {
    const int r = uf_find(vparent, (int)v);
    l = (int)vrank[r];
    vloop[v] = l;
    if (r == (int)v) lfirst[l] = v;
    od = outd[v];
    bits = (bdeg[v] != 2 ? HF_NONSIMPLE : 0) | (od != 1 ? HF_UNORIENTED : 0);
  }
  wave_classes(active, l, [&](bool in, int c0, int leader) {
    class_add(in, leader, ledges, c0, od);
    const int b = (__ballot(in && (bits & HF_NONSIMPLE)) ? HF_NONSIMPLE : 0) |
                  (__ballot(in && (bits & HF_UNORIENTED)) ? HF_UNORIENTED : 0);
    if (tnp::lane() == leader && b) atomicOr(lflags + c0, b);
  });
}

__device__ __forceinline__ void count_lanes(bool f, int64_t* word) {
  const uint64_t m = __ballot(f);
  if (tnp::lane() == 0 && m) atomicAdd(reinterpret_cast<unsigned long long*>(word), (unsigned long long)__popcll(m));
}

__global__ void __launch_bounds__(TNP_BLOCK)
k_hole_status(int64_t L, const int64_t* __restrict__ ledges, const int* __restrict__ lflags, int64_t max_edges,
              int32_t* __restrict__ status, int32_t* __restrict__ capflag, int32_t* __restrict__ lenflag,
              int32_t* __restrict__ starflag, int64_t* __restrict__ ctr) {
  const int64_t l = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  int st = -1;
  int64_t m = 0;
  if (l < L) {
    const int f = lflags[l];
    m = ledges[l];
    st = (f & HF_NONSIMPLE) ? TNP_HOLE_NONSIMPLE
         : (f & HF_UNORIENTED) ? TNP_HOLE_UNORIENTED
         : (max_edges > 0 && m > max_edges) ? TNP_HOLE_TOO_LONG : TNP_HOLE_CAPPED;
    const bool cap = st == TNP_HOLE_CAPPED;
    status[l] = st;
    capflag[l] = cap;
    lenflag[l] = cap ? (int32_t)m : 0;
    starflag[l] = cap && m >= 4;
  }
  const bool cap = st == TNP_HOLE_CAPPED;
  count_lanes(st == TNP_HOLE_NONSIMPLE, ctr + HC_NONSIMPLE);
  count_lanes(st == TNP_HOLE_UNORIENTED, ctr + HC_UNORIENTED);
  count_lanes(st == TNP_HOLE_TOO_LONG, ctr + HC_TOOLONG);
  count_lanes(cap && m == 3, ctr + HC_NTRI);
  unsigned long long mx = cap ? (unsigned long long)m : 0ull;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long y = __shfl_xor(mx, o, 64);
    mx = y > mx ? y : mx;
  }
  if (tnp::lane() == 0 && mx) atomicMax(reinterpret_cast<unsigned long long*>(ctr + HC_LONGEST), mx);
}

// thread 0 closes the offsets (L = 0 included)
__global__ void __launch_bounds__(TNP_BLOCK)
k_cycle_rows(int64_t L, const int32_t* __restrict__ capflag, const int64_t* __restrict__ crank,
             const int64_t* __restrict__ loff, const int64_t* __restrict__ srank, int64_t K, int64_t M,
             int64_t* __restrict__ cycle_loop, int64_t* __restrict__ cycle_offsets, int64_t* __restrict__ cycle_star) {
  const int64_t l = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  if (l == 0) cycle_offsets[K] = M;
  if (l >= L || !capflag[l]) return;
  const int64_t k = crank[l];
  if (k >= K) return;
  cycle_loop[k] = l;
  cycle_offsets[k] = loff[l];
  cycle_star[k] = srank[l];
}

__global__ void __launch_bounds__(TNP_BLOCK)
k_flag_cverts(int64_t V, const int* __restrict__ bdeg, const int32_t* __restrict__ vloop,
              const int32_t* __restrict__ capflag, int32_t* __restrict__ flag) {
  const int64_t v = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  if (v < V) flag[v] = bdeg[v] > 0 && capflag[vloop[v]];
}

// compact position j of vertex v; the loop's first vertex points at itself
// with distance 0, every other vertex at its predecessor with distance 1
__global__ void __launch_bounds__(TNP_BLOCK)
k_rank_init(int64_t V, const int32_t* __restrict__ flag, const int64_t* __restrict__ cpos,
            const int* __restrict__ pred, const int32_t* __restrict__ vloop, const int64_t* __restrict__ lfirst,
            int64_t M, int32_t* __restrict__ cvert, uint64_t* __restrict__ w) {
  const int64_t v = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  if (v >= V || !flag[v]) return;
  const int64_t j = cpos[v];
  if (j >= M) return;
  cvert[j] = (int32_t)v;
  const bool head = lfirst[vloop[v]] == v;
  int64_t p = head ? j : cpos[pred[v]];
  if (p < 0 || p >= M) p = j;  // (never: pred[v] lies in the same capped loop)
  w[j] = ((uint64_t)p << 32) | (head ? 0u : 1u);
}

__global__ void __launch_bounds__(TNP_BLOCK)
k_rank_round(const uint64_t* __restrict__ a, uint64_t* __restrict__ b, int64_t M) {
  const int64_t j = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  if (j >= M) return;
  const uint64_t w = a[j], w2 = a[w >> 32];
  b[j] = (w2 & 0xffffffff00000000ull) | (uint64_t)((uint32_t)w + (uint32_t)w2);
}

__global__ void __launch_bounds__(TNP_BLOCK)
k_cycle_scatter(int64_t M, const uint64_t* __restrict__ w, const int32_t* __restrict__ cvert,
                const int32_t* __restrict__ vloop, const int64_t* __restrict__ loff,
                const int64_t* __restrict__ ledges, int64_t* __restrict__ cycle_vertices) {
  const int64_t j = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  if (j >= M) return;
  const int v = cvert[j], l = vloop[v];
  const int64_t r = (int64_t)(uint32_t)w[j];
  if (r < ledges[l]) cycle_vertices[loff[l] + r] = v;
}

// the last k in [0, K) with coff[k] <= j  (coff[0] == 0, increasing, coff[K] > j)
__device__ __forceinline__ int64_t cycle_of(const int64_t* __restrict__ coff, int64_t K, int64_t j) {
  int64_t lo = 0, hi = K;
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (coff[mid] <= j) lo = mid;
    else hi = mid;
  }
  return lo;
}

// per cycle position j: its star triangle (a 3-cycle: its own triangle, by
// its first position) and the key (cycle << shift) | j of the centre sums.
// T triangles in all; thread 0 closes the offsets (M = 0 included).
__global__ void __launch_bounds__(TNP_BLOCK)
k_star_caps(int64_t M, int64_t K, const int64_t* __restrict__ coff, const int64_t* __restrict__ cstar,
            const int64_t* __restrict__ cv, int64_t V, int64_t T, int shift, int64_t* __restrict__ cap_off,
            int64_t* __restrict__ cap_idx, uint64_t* __restrict__ keys) {
  const int64_t j = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  if (j == 0) cap_off[T] = 3 * T;
  if (j >= M) return;
  const int64_t k = cycle_of(coff, K, j);
  const int64_t a = coff[k], m = coff[k + 1] - a, i = j - a, s = cstar[k];
  keys[j] = ((uint64_t)k << shift) | (uint64_t)j;
  const int64_t tb = a - 2 * (k - s);  // the triangles of the cycles before k
  if (m == 3 && i > 0) return;
  const int64_t t = tb + (m == 3 ? 0 : i);
  if (t >= T) return;
  cap_off[t] = 3 * t;
  cap_idx[3 * t] = cv[a + i];
  cap_idx[3 * t + 1] = cv[a + (i + 1 == m ? 0 : i + 1)];
  cap_idx[3 * t + 2] = m == 3 ? cv[a + 2] : V + s;
}

struct CycleXYZ {  // the coordinates of the vertex at cycle position j
  const int64_t* cv;
  const float* xyz;
  __device__ __forceinline__ void operator()(uint64_t j, double* out) const {
    const float* q = xyz + 3 * cv[j];
    out[0] = (double)q[0], out[1] = (double)q[1], out[2] = (double)q[2];
  }
};

__global__ void __launch_bounds__(TNP_BLOCK)
k_star_centres(int64_t K, const int64_t* __restrict__ coff, const int64_t* __restrict__ cstar,
               const double* __restrict__ sums, int64_t n_star, float* __restrict__ out) {
  const int64_t k = (int64_t)blockIdx.x * TNP_BLOCK + threadIdx.x;
  if (k >= K) return;
  const int64_t m = coff[k + 1] - coff[k], s = cstar[k];
  if (m < 4 || s >= n_star) return;
#pragma unroll
  for (int q = 0; q < 3; ++q) out[3 * s + q] = (float)(sums[(int64_t)q * K + k] / (double)m);
}

void drop_cycles(tnp_holes* h) {
  void* all[] = {h->status, h->cycle_loop, h->cycle_offsets, h->cycle_star, h->cycle_vertices};
  for (void* p : all)
    if (p) (void)hipFree(p);
  h->status = nullptr, h->cycle_loop = h->cycle_offsets = h->cycle_star = h->cycle_vertices = nullptr;
  h->V = h->n_star = 0;
  h->st = tnp_hole_stats{};
}

// the state of one build, handed from stage to stage
struct HolesBuild {
  tnp_holes* h;
  int64_t V;
  const int64_t *off, *idx;
  int64_t P, max_edges;
  hipStream_t s;
  Scratch scr;
  Stages st;
  int64_t* ctr = nullptr;
  int64_t c[HC_N] = {};  // the counters as last read back
  int64_t n = 0, L = 0, B = 0, K = 0, M = 0;
  uint64_t* sk = nullptr;
  int *vparent = nullptr, *bdeg = nullptr, *outd = nullptr, *pred = nullptr;
  int32_t *vflag = nullptr, *vloop = nullptr, *capflag = nullptr;
  int64_t *vrank = nullptr, *cpos = nullptr, *lfirst = nullptr, *ledges = nullptr, *crank = nullptr, *loff = nullptr,
          *srank = nullptr;
  tnp_hole_stats hs = {};
  int edges(), loops(), status(), cycles();  // the stages, in order
};

// stages check_edges, edge_sort
int HolesBuild::edges() {
  n = soup_offsets("holes", scr, off, idx, V, P, &ctr, HC_N, s);
  if (n < 0) return -1;
  const int key_bits = 32 + bits_for(V);
  const size_t sort_bytes = sort_scratch_bytes(n, key_bits);
  {  // everything up to the loop count
    const size_t need = 2 * Scratch::pad(n * sizeof(uint64_t)) + Scratch::pad(sort_bytes) +
                        6 * Scratch::pad(V * sizeof(int32_t)) + 2 * Scratch::pad(V * sizeof(int64_t)) +
                        2 * Scratch::pad(((size_t)scan_tiles(V) + 1) * sizeof(uint64_t));
    if (!scr.reserve(need)) return -1;
  }
  uint64_t* ka = scr.arr<uint64_t>(n);
  uint64_t* kb = scr.arr<uint64_t>(n);
  void* sort_scr = scr.get(sort_bytes);
  if (!ka || !kb || !sort_scr) return -1;
  SOUP_LAUNCH((k_soup_edges<false, false>), n, off, P, idx, n, V, ctr, ka, (uint8_t*)nullptr, (int32_t*)nullptr);
  if (soup_verdict("holes", off, idx, V, ctr, c, 1, s)) return -1;
  st.mark();
  if (sort_keys_u64(ka, kb, n, key_bits, sort_scr, sort_bytes, &sk, s)) return -1;
  st.mark();
  return 0;
}

// stage label_boundary: the boundary graph's classes (the topology's loop
// numbers) -> L, B; the reversed boundary edges
int HolesBuild::loops() {
  vparent = scr.arr<int>(V);
  bdeg = scr.arr<int>(V);
  outd = scr.arr<int>(V);
  pred = scr.arr<int>(V);
  vflag = scr.arr<int32_t>(V);
  vloop = scr.arr<int32_t>(V);
  vrank = scr.arr<int64_t>(V);
  cpos = scr.arr<int64_t>(V);
  if (!vparent || !bdeg || !outd || !pred || !vflag || !vloop || !vrank || !cpos) return -1;
  const uint64_t vb = (uint64_t)(V > 0 ? V : 1) * sizeof(int);
  FillOp ops[3] = {{bdeg, vb, 0u}, {outd, vb, 0u}, {vloop, vb, 0u}};  // (vloop: a valid loop for every vertex)
  if (launch_fill(ops, 3, s)) return -1;
  if (boundary_classes(scr, sk, n, V, vparent, bdeg, vflag, vrank, ctr, s)) return -1;
  SOUP_LAUNCH(k_cap_edges, n, sk, n, pred, outd);
  TNP_CHECK(hipMemcpyAsync(c, ctr, (TC_B + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, s));
  TNP_CHECK(hipStreamSynchronize(s));
  st.mark();
  L = c[TC_L], B = c[TC_B];
  if (L < 0 || L > B || L > V) {
    tnp_set_error("holes: %lld loops of %lld boundary edges", (long long)L, (long long)B);
    return -1;
  }
  hs.n_loops = L;
  return 0;
}

// stage status (L > 0): every loop's status, the cycles' numbers and offsets -> K, M, the stats
int HolesBuild::status() {
  TNP_CHECK(hipMalloc(&h->status, (size_t)L * sizeof(int32_t)));
  {
    const size_t need = 2 * Scratch::pad(L * sizeof(int64_t)) + 4 * Scratch::pad(L * sizeof(int32_t)) +
                        3 * Scratch::pad(L * sizeof(int64_t)) +
                        3 * Scratch::pad(((size_t)scan_tiles(L) + 1) * sizeof(uint64_t));
    if (!scr.reserve(need)) return -1;
  }
  lfirst = scr.arr<int64_t>(L);
  ledges = scr.arr<int64_t>(L);
  int* lflags = scr.arr<int>(L);
  capflag = scr.arr<int32_t>(L);
  int32_t* lenflag = scr.arr<int32_t>(L);
  int32_t* starflag = scr.arr<int32_t>(L);
  crank = scr.arr<int64_t>(L);
  loff = scr.arr<int64_t>(L);
  srank = scr.arr<int64_t>(L);
  if (!lfirst || !ledges || !lflags || !capflag || !lenflag || !starflag || !crank || !loff || !srank)
    return -1;
  FillOp ops[2] = {{ledges, (uint64_t)L * sizeof(int64_t), 0u}, {lflags, (uint64_t)L * sizeof(int), 0u}};
  if (launch_fill(ops, 2, s)) return -1;
  SOUP_LAUNCH(k_hole_verts, V, vparent, bdeg, outd, vrank, V, vloop, lfirst, ledges, lflags);
  SOUP_LAUNCH(k_hole_status, L, L, ledges, lflags, max_edges, h->status, capflag, lenflag, starflag, ctr);
  if (scan_flags(scr, capflag, L, crank, ctr + HC_CAPPED, s)) return -1;
  if (scan_flags(scr, lenflag, L, loff, ctr + HC_NIDX, s)) return -1;
  if (scan_flags(scr, starflag, L, srank, ctr + HC_NSTAR, s)) return -1;
  TNP_CHECK(hipMemcpyAsync(c, ctr, sizeof(c), hipMemcpyDeviceToHost, s));
  TNP_CHECK(hipStreamSynchronize(s));
  st.mark();
  K = c[HC_CAPPED], M = c[HC_NIDX];
  hs.n_capped = K, hs.n_nonsimple = c[HC_NONSIMPLE], hs.n_unoriented = c[HC_UNORIENTED], hs.n_too_long = c[HC_TOOLONG];
  hs.n_cycle_indices = M, hs.n_triangles = c[HC_NTRI], hs.longest_capped = c[HC_LONGEST];
  if (K < 0 || K > L || M < 3 * K || M > B || M > V || c[HC_NSTAR] != K - hs.n_triangles ||
      hs.longest_capped > M || K + hs.n_nonsimple + hs.n_unoriented + hs.n_too_long != L) {
    tnp_set_error("holes: %lld capped loops of %lld with %lld edges of %lld", (long long)K, (long long)L,
                  (long long)M, (long long)B);
    return -1;
  }
  return 0;
}

// stages compact, rank, scatter: the capped loops' vertices, ranked and scattered into the cycles
int HolesBuild::cycles() {
  TNP_CHECK(hipMalloc(&h->cycle_offsets, (size_t)(K + 1) * sizeof(int64_t)));
  if (K > 0) {
    TNP_CHECK(hipMalloc(&h->cycle_loop, (size_t)K * sizeof(int64_t)));
    TNP_CHECK(hipMalloc(&h->cycle_star, (size_t)K * sizeof(int64_t)));
    TNP_CHECK(hipMalloc(&h->cycle_vertices, (size_t)M * sizeof(int64_t)));
  }
  SOUP_LAUNCH(k_cycle_rows, L, L, capflag, crank, loff, srank, K, M, h->cycle_loop, h->cycle_offsets,
              h->cycle_star);
  if (K > 0) {
    {
      const size_t need = Scratch::pad(M * sizeof(int32_t)) + 2 * Scratch::pad(M * sizeof(uint64_t)) +
                          Scratch::pad(((size_t)scan_tiles(V) + 1) * sizeof(uint64_t));
      if (!scr.reserve(need)) return -1;
    }
    int32_t* cvert = scr.arr<int32_t>(M);
    uint64_t* wa = scr.arr<uint64_t>(M);
    uint64_t* wb = scr.arr<uint64_t>(M);
    if (!cvert || !wa || !wb) return -1;
    SOUP_LAUNCH(k_flag_cverts, V, V, bdeg, vloop, capflag, vflag);
    if (scan_flags(scr, vflag, V, cpos, ctr + HC_NCV, s)) return -1;
    // (a position the ranking does not reach stays a valid self pointer)
    TNP_CHECK(hipMemsetAsync(wa, 0, (size_t)M * sizeof(uint64_t), s));
    TNP_CHECK(hipMemsetAsync(cvert, 0, (size_t)M * sizeof(int32_t), s));
    SOUP_LAUNCH(k_rank_init, V, V, vflag, cpos, pred, vloop, lfirst, M, cvert, wa);
    st.mark();
    int rounds = 0;
    while (((int64_t)1 << rounds) < hs.longest_capped) ++rounds;
    for (int r = 0; r < rounds; ++r) {
      SOUP_LAUNCH(k_rank_round, M, wa, wb, M);
      uint64_t* t = wa;
      wa = wb, wb = t;
    }
    st.mark();
    SOUP_LAUNCH(k_cycle_scatter, M, M, wa, cvert, vloop, loff, ledges, h->cycle_vertices);
  } else {
    st.mark();
    st.mark();
  }
  st.mark();
  return 0;
}

}  // namespace

extern "C" int tnp_holes_create(tnp_holes** out, int device) { return handle_create("holes", out, device); }

extern "C" void tnp_holes_destroy(tnp_holes* h) { handle_destroy(h, drop_cycles); }

extern "C" int tnp_debug_holes_stages(tnp_holes* h, int enable, double* ms, int n) {
  return handle_stages("holes", h, enable, ms, n);
}

extern "C" int tnp_holes_build(tnp_holes* h, int64_t V, const int64_t* d_offsets, const int64_t* d_indices, int64_t P,
                               int64_t max_edges, tnp_hole_stats* h_stats, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (h_stats) *h_stats = tnp_hole_stats{};
  if (handle_use("holes", h)) return -1;
  TNP_CHECK(hipStreamSynchronize(s));  // (an earlier export may still read the cycles)
  drop_cycles(h);
  h->n_ms = 0;
  if (max_edges < 0) { tnp_set_error("holes: max_edges = %lld (0: no limit)", (long long)max_edges); return -1; }
  if (soup_args("holes", V, P, true, false, nullptr, d_offsets, d_indices)) return -1;
  h->V = V;
  if (P == 0) return 0;
  HolesBuild b{h, V, d_offsets, d_indices, P, max_edges, s, Scratch(s, "holes"), Stages(h->timed, s)};
  b.st.mark();
  if (b.edges() || b.loops()) return -1;
  if (b.L > 0) {
    if (b.status() || b.cycles()) return -1;
    TNP_CHECK(hipStreamSynchronize(s));
    h->n_star = b.K - b.hs.n_triangles;
    handle_keep_ms(h, b.st);
  }
  h->st = b.hs;
  if (h_stats) *h_stats = b.hs;
  return 0;
}

extern "C" int tnp_holes_export(tnp_holes* h, int32_t* d_status, int64_t* d_cycle_loop, int64_t* d_cycle_offsets,
                                int64_t* d_cycle_vertices, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (handle_use("holes", h)) return -1;
  const int64_t L = h->st.n_loops, K = h->st.n_capped, M = h->st.n_cycle_indices;
  if (d_status && L > 0)
    TNP_CHECK(hipMemcpyAsync(d_status, h->status, (size_t)L * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
  if (d_cycle_loop && K > 0)
    TNP_CHECK(hipMemcpyAsync(d_cycle_loop, h->cycle_loop, (size_t)K * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
  if (d_cycle_offsets) {
    if (h->cycle_offsets)
      TNP_CHECK(hipMemcpyAsync(d_cycle_offsets, h->cycle_offsets, (size_t)(K + 1) * sizeof(int64_t),
                               hipMemcpyDeviceToDevice, s));
    else
      TNP_CHECK(hipMemsetAsync(d_cycle_offsets, 0, sizeof(int64_t), s));  // (no loops: [0])
  }
  if (d_cycle_vertices && M > 0)
    TNP_CHECK(hipMemcpyAsync(d_cycle_vertices, h->cycle_vertices, (size_t)M * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
  return 0;
}

extern "C" int tnp_holes_caps(tnp_holes* h, int mode, const float* d_xyz, int64_t* d_cap_offsets,
                              int64_t* d_cap_indices, float* d_new_xyz, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (handle_use("holes", h)) return -1;
  if (mode != 0 && mode != 1) { tnp_set_error("holes: mode = %d (0: polygon, 1: star)", mode); return -1; }
  if (mode == 0) return tnp_holes_export(h, nullptr, nullptr, d_cap_offsets, d_cap_indices, stream);
  const int64_t K = h->st.n_capped, M = h->st.n_cycle_indices, nt = h->st.n_triangles;
  const int64_t T = nt + (M - 3 * nt);
  if (!d_cap_offsets || (T > 0 && !d_cap_indices) || (h->n_star > 0 && (!d_xyz || !d_new_xyz))) {
    tnp_set_error("holes: null array");
    return -1;
  }
  if (K == 0) {
    TNP_CHECK(hipMemsetAsync(d_cap_offsets, 0, sizeof(int64_t), s));
    return 0;
  }
  Scratch scr(s, "holes");
  const int shift = bits_for(M);
  if (shift + bits_for(K) > 64) { tnp_set_error("holes: %lld cycles over %lld indices do not fit a key", (long long)K, (long long)M); return -1; }
  if (!scr.reserve(Scratch::pad(M * sizeof(uint64_t)) + Scratch::pad(3 * M * sizeof(double)) +
                   Scratch::pad(3 * K * sizeof(double))))
    return -1;
  uint64_t* keys = scr.arr<uint64_t>(M);
  double* pieces = scr.arr<double>(3 * M);
  double* sums = scr.arr<double>(3 * K);
  if (!keys || !pieces || !sums) return -1;
  SOUP_LAUNCH(k_star_caps, M, M, K, h->cycle_offsets, h->cycle_star, h->cycle_vertices, h->V, T, shift, d_cap_offsets,
              d_cap_indices, keys);
  if (h->n_star > 0) {
    hipLaunchKernelGGL((k_seg_pieces<3, CycleXYZ>), dim3(tnp_grid(M, SEG)), dim3(TNP_BLOCK), 0, s, keys, M, shift,
                       CycleXYZ{h->cycle_vertices, d_xyz}, pieces);
    hipLaunchKernelGGL(k_seg_final<3>, dim3(tnp_grid(K, TNP_WAVES)), dim3(TNP_BLOCK), 0, s, h->cycle_offsets, K, M,
                       pieces, sums);
    TNP_CHECK(hipGetLastError());
    SOUP_LAUNCH(k_star_centres, K, K, h->cycle_offsets, h->cycle_star, sums, h->n_star, d_new_xyz);
  }
  TNP_CHECK(hipStreamSynchronize(s));  // (the scratch is freed on the way out)
  return 0;
}
