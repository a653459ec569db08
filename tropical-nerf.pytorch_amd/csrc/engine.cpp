// Host side of the extraction engine: device-resident complex, buffer
// management and the per-step launch sequence (C ABI in
// include/tropical_hip.h).  One engine = one device = one HIP stream per
// call; all scratch is stream-ordered (hipMallocAsync) and reused across
// steps.  Host syncs per active step: split count, hit count, cell entries,
// pair count, final sizes (each one pinned readback of the counter block).
// This file: the engine's state and what every phase uses (buffers, counter
// readback, kernel timer, look-back state, masks, compaction), the nets, and
// load / export / surface.  The step is in engine_step.cpp, the curve branch
// in engine_curve.cpp, the lattice and skeleton loaders in
// engine_skeleton.cpp, faces and polygons in engine_faces.cpp, the debug
// entry points in engine_debug.cpp; engine.h is what they share.
#include "engine.h"

namespace tnp_host {
thread_local std::string g_err;
}
using namespace tnp_host;

void tnp_set_error(const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
}

extern "C" const char* tnp_last_error(void) { return g_err.c_str(); }
extern "C" int tnp_abi_version(void) { return TNP_ABI_VERSION; }
extern "C" int tnp_device_count(int* n) {
  TNP_CHECK(hipGetDeviceCount(n));
  return 0;
}

// ---------------------------------------------------------------------------
// small utility kernels (layout conversion)
// ---------------------------------------------------------------------------
namespace {

__global__ void k_i64_to_i32(const int64_t* __restrict__ in, int32_t* __restrict__ out, int64_t n) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = (int32_t)in[i];
}
__global__ void k_i32_to_i64(const int32_t* __restrict__ in, int64_t* __restrict__ out, int64_t n) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = in[i];
}
// row-major [n][K] <-> plane-major [K][ld]
__global__ void k_rows_to_planes(const float* __restrict__ in, int64_t n, int K, float* __restrict__ out,
                                 int64_t ld) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  for (int p = 0; p < K; ++p) out[(int64_t)p * ld + i] = in[i * K + p];
}
__global__ void k_planes_to_rows(const float* __restrict__ in, int64_t ld, int64_t n, int K,
                                 float* __restrict__ out) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  for (int p = 0; p < K; ++p) out[i * K + p] = in[(int64_t)p * ld + i];
}

}  // namespace

// ---------------------------------------------------------------------------
// buffers
// ---------------------------------------------------------------------------
namespace tnp_host {

// the capacity buf_ensure grows a buffer of `have` bytes to for a request of
// `bytes`: geometric (x1.5), in whole 256-B units
size_t buf_grow_bytes(size_t have, size_t bytes) {
  const size_t nb = std::max(bytes, have + have / 2);
  return std::max<size_t>((nb + 255) & ~size_t(255), 256);
}

// the connect phase's key capacity (keys) for a step of M members, given the
// key buffer's current size: XS_N equal per-XCD regions.  The capacity the
// buffer already holds is rounded DOWN to the regions (so it never asks for
// more than the buffer has -- round 4's 1.5x-per-step growth to 44 GB came
// from rounding it up); only the floor of 4 M + 1024 keys is rounded up.
int64_t connect_key_cap(size_t have_bytes, int64_t M, int xs_n) {
  const int64_t have = (int64_t)(have_bytes / sizeof(uint64_t)) / xs_n * xs_n;
  const int64_t floor = (4 * M + 1024 + xs_n - 1) / xs_n * xs_n;
  return std::max(have, floor);
}

int buf_ensure(Buf& b, size_t bytes, hipStream_t s, bool keep) {
  if (bytes <= b.bytes && b.p) return 0;
  const size_t nb = buf_grow_bytes(b.bytes, bytes);
  void* p = nullptr;
  if (hipMallocAsync(&p, nb, s) != hipSuccess) {
    size_t fr = 0, tot = 0;
    (void)hipMemGetInfo(&fr, &tot);
    tnp_set_error("hipMallocAsync of %zu bytes (buffer of %zu, %zu requested): out of memory, %zu of %zu free",
                  nb, b.bytes, bytes, fr, tot);
    return -1;
  }
  if (keep && b.p && b.bytes) TNP_CHECK(hipMemcpyAsync(p, b.p, b.bytes, hipMemcpyDeviceToDevice, s));
  if (b.p) TNP_CHECK(hipFreeAsync(b.p, s));
  b.p = p;
  b.bytes = nb;
  return 0;
}
static void buf_free(Buf& b, hipStream_t s) {
  if (b.p) (void)hipFreeAsync(b.p, s);
  b.p = nullptr;
  b.bytes = 0;
}

// counter readback: k_publish writes the block into host-mapped memory and
// the host spins on its sequence word (measured on MI355X: 9.9 us per round
// trip against 15.7 us for a copy + stream synchronise); after 2 ms of
// spinning (long kernels) it blocks in the stream synchronise instead
// vpart != null: the published CTR_V (and CTR_E when ne > 0) are the sums of
// vpart[nv] / epart[ne] (the deferred live counts), not the device words
// (post_ctr enqueues the publish, wait_ctr takes it: work enqueued between
// the two runs on the GPU while the counters travel to the host)
int post_ctr(tnp_engine* e, hipStream_t s, int64_t* seq_out, const int64_t* vpart, int nv, const int64_t* epart,
             int ne, bool clear) {
  const int64_t seq = ++e->pub_seq;
  if (vpart ? launch_publish_sums(P<int64_t>(e->ctr), e->h_map_dev, seq, vpart, nv, epart, ne, s)
            : launch_publish(P<int64_t>(e->ctr), e->h_map_dev, seq, s, clear))
    return -1;
  e->ctr_zero = clear && !vpart;
  *seq_out = seq;
  return 0;
}
int wait_ctr(tnp_engine* e, hipStream_t s, int64_t seq) {
  volatile int64_t* flag = e->h_map + 31;
  const auto t0 = std::chrono::steady_clock::now();
  int n = 0;
  while (*flag != seq) {
    if ((++n & 255) == 0 &&
        std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) {
      TNP_CHECK(hipStreamSynchronize(s));
      if (*flag != seq) { tnp_set_error("counter readback: no publish after the stream drained"); return -1; }
      break;
    }
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  memcpy(e->h_ctr, (const void*)e->h_map, CTR_N * sizeof(int64_t));
  return 0;
}
int read_ctr(tnp_engine* e, hipStream_t s, const int64_t* vpart, int nv, const int64_t* epart, int ne,
             bool clear) {
  int64_t seq = 0;
  return post_ctr(e, s, &seq, vpart, nv, epart, ne, clear) || wait_ctr(e, s, seq) ? -1 : 0;
}

// the deferred live counts arrived (V_live, E_live; E_live < 0: unchanged)
void apply_counts(tnp_engine* e, int64_t V_live, int64_t E_live) {
  e->V_live = V_live;
  if (e->pend_lz_n > 0) e->E_live = E_live;
  if (e->pend_st) {
    e->pend_st->V_out = e->V_live;
    e->pend_st->E_out = e->E_live;
  }
  e->cnt_pending = false;
  e->pend_lz_n = 0;
  e->pend_st = nullptr;
}

// the deferred counts now, by the counting pass (a split without hit
// workers, the end of the run loop, any other caller); the counter words
// CTR_V / CTR_E are still zero from the last split's reset
int resolve_counts(tnp_engine* e, hipStream_t s) {
  if (!e->cnt_pending) return 0;
  int64_t* ctr = P<int64_t>(e->ctr);
  if (launch_count_flags(P<uint8_t>(e->live), e->V, ctr, CTR_V, s, e->pend_lz_n ? P<int64_t>(e->lzpart) : nullptr,
                         (int)e->pend_lz_n, CTR_E))
    return -1;
  if (read_ctr(e, s)) return -1;
  apply_counts(e, e->h_ctr[CTR_V], e->h_ctr[CTR_E]);
  return 0;
}

// ---- per-kernel HIP-event timer (bench.py's roofline leg) -----------------
int ktimer_begin(tnp_engine* e, const char* name, double bytes, hipStream_t s) {
  if (!e->kt_on) return -1;
  KRec r;
  r.name = name;
  r.bytes = bytes;
  if (hipEventCreate(&r.a) != hipSuccess || hipEventCreate(&r.b) != hipSuccess) return -1;
  (void)hipEventRecord(r.a, s);
  e->kt.push_back(r);
  return (int)e->kt.size() - 1;
}
// bytes of the encoding tables (2 fp32 features per entry)
double table_bytes(const NetDev& n) {
  double b = 0;
  for (int l = 0; l < n.n_levels; ++l) b += 8.0 * n.sizes[l];
  return b;
}
// modelled bytes of the last timed launch, when they depend on its result
void ktimer_set_bytes(tnp_engine* e, double bytes) {
  if (e->kt_on && !e->kt.empty()) e->kt.back().bytes = bytes;
}
// ... of the latest timed launch named `name` (counts read back later)
void ktimer_set_bytes(tnp_engine* e, const char* name, double bytes) {
  if (!e->kt_on) return;
  for (size_t i = e->kt.size(); i-- > 0;)
    if (strcmp(e->kt[i].name, name) == 0) {
      e->kt[i].bytes = bytes;
      return;
    }
}
void ktimer_end(tnp_engine* e, int t, hipStream_t s) {
  if (t >= 0) (void)hipEventRecord(e->kt[t].b, s);
}

// look-back state `w` for a single-pass launch of `tiles` tiles (common.h TnpLB)
// (`ticketed` false: the kernel numbers tiles by blockIdx and takes no ticket)
int lb_begin(tnp_engine* e, int64_t tiles, hipStream_t s, TnpLB* out, int w, bool ticketed) {
  Buf& b = e->lb[w];
  size_t need = (size_t)(tiles + 1) * sizeof(uint64_t);
  if (need > b.bytes || !b.p) {
    if (buf_ensure(b, std::max(need, (size_t)64 << 10), s)) return -1;
    TNP_CHECK(hipMemsetAsync(b.p, 0, b.bytes, s));  // flag 0: no record
    e->lb_tickets[w] = 0;
  }
  e->lb_epoch[w] = (e->lb_epoch[w] + 1) & 0x3FFFFFu;
  if (e->lb_epoch[w] == 0) {  // wrapped: clear records that could carry a reused epoch
    TNP_CHECK(hipMemsetAsync(b.p, 0, b.bytes, s));
    e->lb_tickets[w] = 0;
    e->lb_epoch[w] = 1;
  }
  out->ticket = static_cast<unsigned long long*>(b.p);
  out->st = static_cast<uint64_t*>(b.p) + 1;
  out->tbase = e->lb_tickets[w];
  out->epoch = e->lb_epoch[w];
  out->spin = e->lb_spin;
  if (!e->lbrc.p) {
    if (buf_ensure(e->lbrc, sizeof(uint64_t), s)) return -1;
    TNP_CHECK(hipMemsetAsync(e->lbrc.p, 0, sizeof(uint64_t), s));
  }
  out->rc = static_cast<unsigned long long*>(e->lbrc.p);
  if (ticketed) e->lb_tickets[w] += (uint64_t)tiles;
  return 0;
}

int scan_counts(tnp_engine* e, const int32_t* in, int64_t* out, int64_t n, int slot, hipStream_t s) {
  TnpLB lb;
  if (n > 0 && lb_begin(e, scan_tiles(n), s, &lb, 0, false)) return -1;
  TIMED("scan", 12.0 * n, scan_i32_to_i64(in, out, n, P<int64_t>(e->ctr) + slot, lb, s));
  return 0;
}

// grow a vertex set to `rows` keeping [0, keep_rows)
int vset_ensure(tnp_engine* e, VSet& v, int64_t rows, int64_t keep_rows, hipStream_t s) {
  if (rows <= v.cap && v.K == e->K) return 0;
  // another net: nothing of the old set is kept, and its capacity is no
  // growth history (alternating nets must not compound the 1.5x)
  const bool same = v.K == e->K;
  if (!same) keep_rows = 0;
  int64_t nc = same ? std::max<int64_t>(rows, v.cap + v.cap / 2) : rows;
  nc = (nc + 255) / 256 * 256;
  VSet n;
  n.cap = nc;
  n.K = e->K;
  if (buf_ensure(n.xyz, nc * 3 * sizeof(float), s)) return -1;
  if (buf_ensure(n.pre, (size_t)nc * e->K * sizeof(float), s)) return -1;
  const int64_t kb = 8 * e->kw;  // bytes per key
  if (buf_ensure(n.grid, nc * sizeof(uint64_t), s)) return -1;
  if (buf_ensure(n.pz, nc * 2 * kb, s)) return -1;
  if (keep_rows > 0 && v.cap > 0) {
    TNP_CHECK(hipMemcpyAsync(n.xyz.p, v.xyz.p, keep_rows * 3 * sizeof(float), hipMemcpyDeviceToDevice, s));
    TNP_CHECK(hipMemcpy2DAsync(n.pre.p, nc * sizeof(float), v.pre.p, v.cap * sizeof(float),
                               keep_rows * sizeof(float), e->K, hipMemcpyDeviceToDevice, s));
    TNP_CHECK(hipMemcpyAsync(n.grid.p, v.grid.p, keep_rows * 8, hipMemcpyDeviceToDevice, s));
    TNP_CHECK(hipMemcpyAsync(n.pz.p, v.pz.p, keep_rows * 2 * kb, hipMemcpyDeviceToDevice, s));
  }
  buf_free(v.xyz, s);
  buf_free(v.pre, s);
  buf_free(v.grid, s);
  buf_free(v.pz, s);
  v = n;
  return 0;
}

static int keys_for(tnp_engine* e, VSet& v, int64_t from, int64_t n, hipStream_t s) {
  return launch_keys(e->net, P<float>(v.xyz) + 3 * from, P<float>(v.pre) + from, v.cap, n, e->K,
                     VP(v, e->kw, from), VZ(v, e->kw, from), P<uint64_t>(v.grid) + from, s,
                     VP(v, e->kw, from));
}

// live flags of slots [from, from + n) := 1 (kept capacity: earlier flags stay)
int set_alive(tnp_engine* e, int64_t from, int64_t n, hipStream_t s) {
  if (buf_ensure(e->live, std::max<int64_t>(from + n, 16), s, true)) return -1;
  const FillOp f{P<uint8_t>(e->live) + from, (uint64_t)std::max<int64_t>(n, 0), 1};
  if (launch_fill(&f, 1, s)) return -1;
  return 0;
}

// a freshly loaded complex: every slot live, ids dense, edge masks to compute
int reset_live(tnp_engine* e, hipStream_t s, bool edges_changed) {
  if (edges_changed) e->masks_valid = false;
  e->rows_valid = false;  // (load, lattice, skeleton, surface, a compaction: other vertex ids)
  e->valid = true;
  e->dirty = false;
  e->V_live = e->V;
  return set_alive(e, 0, e->V, s);
}

// the cell grouping runs on spatial buckets (bucket.hip) unless the grid is
// too fine for them or TNP_RADIX_CELLS=1; *bg: their geometry
void span_all(tnp_engine* e) {
  for (int d = 0; d < 3; ++d) e->sp_lo[d] = 0, e->sp_hi[d] = -1;
}
// the span's mark planes along each axis (the whole axis where not narrowed)
void span_of(const tnp_engine* e, int lo[3], int hi[3]) {
  for (int d = 0; d < 3; ++d) {
    const bool set = e->sp_hi[d] >= e->sp_lo[d];
    lo[d] = set ? e->sp_lo[d] : 0;
    hi[d] = set ? e->sp_hi[d] : e->net.n_marks - 1;
  }
}
bool uses_buckets(const tnp_engine* e, BucketGeom* bg) {
  if (e->kw != 1) return false;  // two-word keys: the radix path's 48-B records
  int lo[3], hi[3];
  span_of(e, lo, hi);
  return !e->radix_cells && bucket_geometry(e->net.n_marks, lo, hi, bg) == 0;
}

// split-eps mode: subpoly's eps argument differs from Net.eps (tnp_engine_set_eps)
bool eps2(const tnp_engine* e) { return e->net.eps_s != e->net.eps; }

// the cache planes a flat step at plane idx stores for its new vertices:
// those a later step, the surface (plane K - 1) or an export can read.  In the
// hot loop that is planes > idx (the step's pruning moves valid_from to
// idx + 1; the last plane always) -- not [valid_from, idx], dead the moment
// the step ends (up to 15 of 33 planes a split at 128^3).  A caller that
// hands outputs_ back (keep_all) or the split-eps mode keeps every plane.
int new_keep_from(const tnp_engine* e, int idx) {
  if (e->keep_all || eps2(e)) return e->valid_from;
  return std::max(e->valid_from, std::min(idx + 1, e->K - 1));
}

// per-edge high plane and first split plane (>= from) from the endpoint
// keys; ctr != null: the OR of the first split planes -> ctr[CTR_ACTIVE]
int compute_masks(tnp_engine* e, int from, int64_t* ctr, hipStream_t s) {
  const int64_t E1 = std::max<int64_t>(e->E, 1);
  if (buf_ensure(e->edm, E1 * sizeof(uint8_t), s)) return -1;
  if (buf_ensure(e->eef, E1 * sizeof(uint8_t), s)) return -1;
  TIMED("edge_masks", 42.0 * e->E,
        launch_edge_masks(P<int32_t>(e->edges), e->E, P<uint64_t>(e->cur.pz), P<uint8_t>(e->edm),
                          P<uint8_t>(e->eef), from, e->K - 1, e->cnt_pending || e->E != e->E_live, ctr, s));
  if (eps2(e)) {
    // first split planes at subpoly's eps from the cached planes (the mode
    // keeps them all): they replace the Net.eps ones and their OR
    if (e->valid_from > from) {
      tnp_set_error("split-eps masks from plane %d: planes below %d were dropped", from, e->valid_from);
      return -1;
    }
    if (ctr) TNP_CHECK(hipMemsetAsync(ctr + CTR_ACTIVE, 0, sizeof(int64_t), s));
    TIMED("edge_masks", 8.0 * e->E,
          launch_ef_cache(P<int32_t>(e->edges), e->E, P<uint8_t>(e->edm), P<uint8_t>(e->eef),
                          P<float>(e->cur.pre), e->cur.cap, from, e->K, e->net.eps_s, ctr, s));
  }
  e->masks_valid = true;
  e->mask_from = from;
  return 0;
}

// the masks a step at plane idx can use: the stored first split planes were
// taken from mask_from, so they are the ones of idx unless a plane in
// [mask_from, idx) still splits some edge (a step the caller skipped) --
// then they are recomputed from idx.  Returns 1 if recomputed (the OR of
// the first planes is then in ctr[CTR_ACTIVE], ctr zeroed by the caller).
// the active-plane word of the planes [lo, hi) (planes >= 63 share bit 63)
static uint64_t act_range(int lo, int hi) {
  uint64_t m = 0;
  for (int p = lo; p < hi && p < 63; ++p) m |= 1ull << p;
  if (hi > 63 && hi > lo) m |= 1ull << 63;
  return m;
}

int ensure_masks(tnp_engine* e, int idx, hipStream_t s) {
  if (e->masks_valid && idx >= e->mask_from && (e->act_bits & act_range(e->mask_from, idx)) == 0) return 0;
  return compute_masks(e, idx, P<int64_t>(e->ctr), s) ? -1 : 1;
}

// drop the lazily deleted edges, live ones in order (the compacting prune
// keeping every live edge: idx = -1)
static int compact_edges(tnp_engine* e, hipStream_t s) {
  if (e->E == e->E_live) return 0;
  const int64_t E = e->E, E1 = std::max<int64_t>(E, 1);
  if (buf_ensure(e->edges_alt, E1 * 2 * sizeof(int32_t), s)) return -1;
  if (buf_ensure(e->edm_alt, E1 * sizeof(uint8_t), s)) return -1;
  if (buf_ensure(e->eef_alt, E1 * sizeof(uint8_t), s)) return -1;
  TnpLB lb;
  if (lb_begin(e, lb_tiles(E), s, &lb, 0, false)) return -1;
  TIMED("compact_edges", 12.0 * E,
        launch_prune_lb(P<int32_t>(e->edges), E, nullptr, 0, e->V, nullptr, 0, 0, -1, e->K - 1,
                        P<uint64_t>(e->cur.pz), P<uint8_t>(e->edm), P<uint8_t>(e->eef), P<int32_t>(e->edges_alt),
                        P<uint8_t>(e->edm_alt), P<uint8_t>(e->eef_alt), P<uint8_t>(e->live), P<int64_t>(e->ctr),
                        lb, s));
  std::swap(e->edges, e->edges_alt);
  std::swap(e->edm, e->edm_alt);
  std::swap(e->eef, e->eef_alt);
  if (read_ctr(e, s)) return -1;
  if (e->h_ctr[CTR_E] != e->E_live) {
    tnp_set_error("edge compaction: %lld live edges, %lld expected", (long long)e->h_ctr[CTR_E],
                  (long long)e->E_live);
    return -1;
  }
  e->E = e->E_live;
  return 0;
}

// renumber the live slots densely (the reference's per-step compaction,
// subpoly.py:266-277, done once): scan of the live flags, gather of the
// vertex rows (planes >= valid_from), edge remap
int compact_now(tnp_engine* e, hipStream_t s) {
  if (e->cnt_pending) {  // (run_steps resolves them on every exit; V_live / E_live would read stale)
    tnp_set_error("compaction with the live counts of the last step still pending");
    return -1;
  }
  if (compact_edges(e, s)) return -1;
  if (!e->dirty) return 0;
  const int64_t NV = e->V;
  if (buf_ensure(e->nid, std::max<int64_t>(NV, 1) * sizeof(int64_t), s)) return -1;
  if (buf_ensure(e->used, std::max<int64_t>(NV, 1) * sizeof(int32_t), s)) return -1;
  if (launch_widen_flags(P<uint8_t>(e->live), NV, P<int32_t>(e->used), s)) return -1;
  if (scan_counts(e, P<int32_t>(e->used), P<int64_t>(e->nid), NV, CTR_AUX, s)) return -1;
  if (vset_ensure(e, e->alt, NV, 0, s)) return -1;
  VSet& c = e->cur;
  VSet& a = e->alt;
  TIMED("gather_vertices", 4.0 * NV + 2.0 * (12 + 4.0 * (e->K - e->valid_from) + 24) * e->V_live,
        launch_gather_vertices(P<int32_t>(e->used), P<int64_t>(e->nid), NV, e->K, e->valid_from,
                               P<float>(c.xyz), P<float>(c.pre), c.cap, VP(c, e->kw),
                               VZ(c, e->kw), P<uint64_t>(c.grid), P<float>(a.xyz),
                               P<float>(a.pre), a.cap, VP(a, e->kw), VZ(a, e->kw),
                               P<uint64_t>(a.grid), P<uint64_t>(a.pz), s));
  TIMED("remap_edges", 32.0 * e->E, launch_remap_edges(P<int32_t>(e->edges), e->E, P<int64_t>(e->nid), s));
  if (read_ctr(e, s)) return -1;
  const int64_t V2 = e->h_ctr[CTR_AUX];
  if (V2 != e->V_live) {
    tnp_set_error("compaction: %lld live slots, %lld expected", (long long)V2, (long long)e->V_live);
    return -1;
  }
  std::swap(e->cur, e->alt);
  e->V = V2;
  return reset_live(e, s, false);  // same edges, same order: masks stay valid
}

int require_valid(const tnp_engine* e, const char* what) {
  if (e->valid) return 0;
  tnp_set_error("%s: no consistent complex (none loaded, or a failed step left it half-updated); "
                "load one first (tnp_engine_load / lattice / skeleton)", what);
  return -1;
}

}  // namespace tnp_host

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
extern "C" int tnp_engine_create(tnp_engine** out, int device) {
  TNP_CHECK(hipSetDevice(device));
  tnp_engine* e = new tnp_engine();
  e->device = device;
  if (const char* lim = getenv("TNP_MAX_PAIR_TESTS")) e->max_pair_tests = atoll(lim);
  if (const char* rc = getenv("TNP_RADIX_CELLS")) e->radix_cells = atoi(rc) != 0;
  if (const char* lr = getenv("TNP_LDS_RECORDS")) e->lds_records = atoi(lr) != 0;
  if (const char* sp = getenv("TNP_LB_SPIN")) e->lb_spin = atoi(sp);
  if (const char* ef = getenv("TNP_EARLY_FWD")) e->early_forward = atoi(ef) != 0;
  if (const char* eb = getenv("TNP_EARLY_BOUND")) e->early_bound_splits = atoi(eb) != 0;
  if (const char* sr = getenv("TNP_SORT_RUN")) e->sort_run = atoi(sr);
  if (hipHostMalloc((void**)&e->h_ctr, CTR_N * sizeof(int64_t), hipHostMallocDefault) != hipSuccess ||
      hipHostMalloc((void**)&e->h_map, 32 * sizeof(int64_t), hipHostMallocMapped | hipHostMallocCoherent) !=
          hipSuccess ||
      hipHostGetDevicePointer((void**)&e->h_map_dev, e->h_map, 0) != hipSuccess) {
    if (e->h_ctr) (void)hipHostFree(e->h_ctr);
    if (e->h_map) (void)hipHostFree(e->h_map);
    delete e;
    tnp_set_error("hipHostMalloc failed");
    return -1;
  }
  memset((void*)e->h_map, 0, 32 * sizeof(int64_t));
  *out = e;
  return 0;
}

// every device buffer the engine owns (destroy, tnp_engine_scratch_bytes)
template <typename F>
static void for_each_buf(tnp_engine* e, F&& f) {
  for (VSet* v : {&e->cur, &e->alt})
    for (Buf* b : {&v->xyz, &v->pre, &v->grid, &v->pz}) f(*b);
  Buf* bufs[] = {&e->edges, &e->edges_alt, &e->blk, &e->blkoff, &e->sa, &e->sb,
                 &e->stage, &e->shared, &e->members, &e->pcn, &e->pent, &e->rstart,
                 &e->ent_v, &e->ents, &e->pcell, &e->ptoff, &e->bcell,
                 &e->ckeys_a, &e->ckeys_b, &e->sort_scr, &e->flags, &e->used, &e->nid,
                 &e->ctr, &e->tri, &e->faces, &e->lb[0], &e->lb[1], &e->edm, &e->eef,
                 &e->edm_alt, &e->eef_alt, &e->live, &e->tied_table, &e->xs, &e->lbrc, &e->lzpart,
                 &e->kse_pz, &e->kse_grid, &e->sk_gload, &e->sk_gmax, &e->sents, &e->sents2,
                 &e->spcnt, &e->spoff, &e->part, &e->ekey_a, &e->ekey_b, &e->eval_b, &e->sort_scr2,
                 &e->hpart};
  for (Buf* b : bufs) f(*b);
  for (Buf& b : e->fscr2) f(b);
  for (Buf& b : e->bk) f(b);
  for (Buf& b : e->cv) f(b);
}

extern "C" void tnp_engine_destroy(tnp_engine* e) {
  if (!e) return;
  (void)hipSetDevice(e->device);
  (void)hipDeviceSynchronize();
  hipStream_t s = 0;
  for_each_buf(e, [&](Buf& b) { buf_free(b, s); });
  (void)hipDeviceSynchronize();
  if (e->h_ctr) (void)hipHostFree(e->h_ctr);
  delete e;
}

extern "C" int tnp_engine_scratch_bytes(tnp_engine* e, int64_t* bytes, int64_t* buffers, int64_t* key_bytes) {
  if (!e || !bytes) { tnp_set_error("tnp_engine_scratch_bytes: null argument"); return -1; }
  int64_t tot = 0, n = 0;
  for_each_buf(e, [&](Buf& b) { tot += (int64_t)b.bytes; n += b.p != nullptr; });
  *bytes = tot;
  if (buffers) *buffers = n;
  if (key_bytes) *key_bytes = (int64_t)e->ckeys_a.bytes;
  return 0;
}

namespace tnp_host {

NetDev to_dev(const tnp_net* n) {
  NetDev d{};
  for (int l = 0; l < TNP_MAX_LEVELS; ++l) {
    d.scales[l] = n->scales[l];
    d.res[l] = n->res[l];
    d.sizes[l] = n->sizes[l];
    d.offsets[l] = n->offsets[l];
    d.dense[l] = n->dense[l];
  }
  d.table = n->d_table;
  d.weights = n->d_weights;
  d.marks = n->d_marks;
  d.n_levels = n->n_levels;
  d.num_layers = n->num_layers;
  d.num_hidden = n->num_hidden;
  d.n_marks = n->n_marks;
  d.eps = n->eps;
  d.eps_s = n->eps;
  return d;
}

int check_net(const tnp_net* n) {
  if (!n) { tnp_set_error("null net"); return -1; }
  if (n->n_features != 2) { tnp_set_error("n_features must be 2"); return -1; }
  NetDev d = to_dev(n);
  if (!net_supported(d)) {
    tnp_set_error("net shape (levels=%d, layers=%d, hidden=%d) not instantiated", n->n_levels,
                  n->num_layers, n->num_hidden);
    return -1;
  }
  if (net_K(d) > 127) { tnp_set_error("more than 127 planes (two-word sign keys)"); return -1; }
  return 0;
}

}  // namespace tnp_host

// Levels with the same fp32 scale, resolution, table size and addressing
// (e.g. the synthetic lattice nets, r_min == r_max) share corner weights and
// hash indices: the engine keeps a level-interleaved copy of the table so a
// corner is one 16-B gather for two levels (net_device.h encode_tied).
static bool levels_tied(const tnp_net* n) {
  if (n->n_levels < 2 || n->n_levels % 2 != 0 || getenv("TNP_NO_TIED")) return false;
  for (int l = 1; l < n->n_levels; ++l)
    if (memcmp(&n->scales[l], &n->scales[0], sizeof(float)) != 0 || n->res[l] != n->res[0] ||
        n->sizes[l] != n->sizes[0] || n->dense[l] != n->dense[0])
      return false;
  return true;
}

extern "C" int tnp_engine_set_net(tnp_engine* e, const tnp_net* n) {
  if (check_net(n)) return -1;
  TNP_CHECK(hipSetDevice(e->device));
  e->rows_valid = false;
  e->net = to_dev(n);
  if (levels_tied(n)) {
    const int L = n->n_levels;
    const size_t entry = 2 * sizeof(float);
    if (buf_ensure(e->tied_table, (size_t)n->sizes[0] * L * entry, 0)) return -1;
    for (int l = 0; l < L; ++l)
      TNP_CHECK(hipMemcpy2DAsync(static_cast<char*>(e->tied_table.p) + l * entry, L * entry,
                                 n->d_table + 2 * (size_t)n->offsets[l], entry, entry, n->sizes[0],
                                 hipMemcpyDeviceToDevice, 0));
    TNP_CHECK(hipStreamSynchronize(0));
    e->net.table = P<float>(e->tied_table);
    e->net.tied = 1;
  }
  const int K = net_K(e->net);
  if (e->has_net && K != e->K) {
    // the resident complex's cache has the old net's planes (vset_ensure
    // reallocates the vertex sets for the new K): load a complex again
    e->valid = false;
    e->pend_idx = -1;
  }
  e->K = K;
  e->kw = net_kw(e->net);
  e->has_net = true;
  return 0;
}

extern "C" int tnp_forward(const tnp_net* n, const float* xyz, int64_t N, float* pre, int64_t ld,
                           float* out2, void* stream) {
  if (check_net(n)) return -1;
  return launch_forward(to_dev(n), xyz, N, pre, ld, 1, (hipStream_t)stream, out2);
}
extern "C" int tnp_encode(const tnp_net* n, const float* x01, int64_t N, float* out, void* stream) {
  if (check_net(n)) return -1;
  return launch_encode(to_dev(n), x01, N, out, (hipStream_t)stream);
}
extern "C" int tnp_forward_grouped(const tnp_net* n, const float* xyz, int64_t N, float* pre,
                                   int64_t ld, float* out2, void* stream) {
  if (check_net(n)) return -1;
  return launch_forward(to_dev(n), xyz, N, pre, ld, 8, (hipStream_t)stream, out2);
}
extern "C" int tnp_region(const tnp_net* n, const float* xyz, const float* pre, int64_t ld,
                          int64_t N, float eps, int64_t* m, int64_t* off, void* stream) {
  if (check_net(n)) return -1;
  return launch_region(to_dev(n), xyz, pre, ld, N, eps, m, off, (hipStream_t)stream);
}
extern "C" int tnp_sdf_grad(const tnp_net* n, const float* xyz, int64_t N, float* sdf, float* grad,
                            void* stream) {
  if (check_net(n)) return -1;
  return launch_sdf_grad(to_dev(n), xyz, N, sdf, grad, (hipStream_t)stream);
}

extern "C" int tnp_sdf_train_grad(const tnp_net* n, const float* xyz, const float* gt, int64_t N, float clamp_t,
                                  float eik_w, int64_t eik_batch, float* d_grad_table, float* d_grad_weights,
                                  double* d_stats, void* stream) {
  if (check_net(n)) return -1;
  if (N < 0 || !d_grad_table || !d_grad_weights || !d_stats) { tnp_set_error("sdf_train_grad: bad arguments"); return -1; }
  return launch_train_grad(to_dev(n), xyz, gt, N, clamp_t, eik_w, eik_batch > 0 ? eik_batch : N, d_grad_table, d_grad_weights, d_stats,
                           (hipStream_t)stream);
}

extern "C" int tnp_sdf_vjp(const tnp_net* n, const float* xyz, const float* gout, int64_t N, float* d_grad_table,
                           float* d_grad_weights, void* stream) {
  if (check_net(n)) return -1;
  if (N < 0 || !gout || !d_grad_table || !d_grad_weights) { tnp_set_error("sdf_vjp: bad arguments"); return -1; }
  return launch_sdf_vjp(to_dev(n), xyz, gout, N, d_grad_table, d_grad_weights, (hipStream_t)stream);
}

extern "C" int tnp_normal_vjp(const tnp_net* n, const float* xyz, const float* gJ, int64_t N, float* d_grad_table,
                              float* d_grad_weights, float* d_grad_x, void* stream) {
  if (check_net(n)) return -1;
  if (N < 0 || !gJ || !d_grad_table || !d_grad_weights) { tnp_set_error("normal_vjp: bad arguments"); return -1; }
  return launch_normal_vjp(to_dev(n), xyz, gJ, N, d_grad_table, d_grad_weights, d_grad_x, (hipStream_t)stream);
}

extern "C" int tnp_forward_vjp(const tnp_net* n, const float* xyz, int64_t N, const float* d_gpre, int64_t ld,
                               const float* d_gout, float* d_grad_table, float* d_grad_weights, float* d_grad_x,
                               void* stream) {
  if (check_net(n)) return -1;
  if (N < 0 || (!d_gpre && !d_gout) || (d_gpre && ld < N) || !d_grad_table || !d_grad_weights) {
    tnp_set_error("forward_vjp: bad arguments");
    return -1;
  }
  return launch_forward_vjp(to_dev(n), xyz, N, d_gpre, ld, d_gout, d_grad_table, d_grad_weights, d_grad_x,
                            (hipStream_t)stream);
}

extern "C" int tnp_mesh_signed_distance(const float* d_V, int64_t nV, const int32_t* d_F, int64_t nF,
                                        const float* d_p, int64_t n, float* d_work, float* d_dist, void* stream) {
  if (n < 0) { tnp_set_error("mesh_signed_distance: n < 0"); return -1; }
  return launch_mesh_sd(d_V, nV, d_F, nF, d_p, n, d_work, d_dist, (hipStream_t)stream);
}

static int set_edges_i64(tnp_engine* e, const int64_t* d_edges, int64_t E, hipStream_t s) {
  if (buf_ensure(e->edges, std::max<int64_t>(E, 1) * 2 * sizeof(int32_t), s)) return -1;
  if (E > 0)
    hipLaunchKernelGGL(k_i64_to_i32, dim3(tnp_grid(2 * E)), dim3(TNP_BLOCK), 0, s, d_edges,
                       P<int32_t>(e->edges), 2 * E);
  TNP_CHECK(hipGetLastError());
  e->E = E;
  e->E_live = E;
  return 0;
}

extern "C" int tnp_engine_load(tnp_engine* e, const float* d_xyz, int64_t V, const int64_t* d_edges,
                               int64_t E, const float* d_pre, int keep_all, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  e->rows_valid = false;
  if (!e->has_net) { tnp_set_error("engine has no net"); return -1; }
  TNP_CHECK(hipSetDevice(e->device));
  span_all(e);  // anywhere (tnp_engine_set_span narrows it)
  if (buf_ensure(e->ctr, CTR_CLEAR_BYTES, s)) return -1;
  if (vset_ensure(e, e->cur, std::max<int64_t>(V, 1), 0, s)) return -1;
  if (V > 0)
    TNP_CHECK(hipMemcpyAsync(e->cur.xyz.p, d_xyz, V * 3 * sizeof(float), hipMemcpyDeviceToDevice, s));
  if (set_edges_i64(e, d_edges, E, s)) return -1;
  if (d_pre) {
    if (V > 0)
      hipLaunchKernelGGL(k_rows_to_planes, dim3(tnp_grid(V)), dim3(TNP_BLOCK), 0, s, d_pre, V, e->K,
                         P<float>(e->cur.pre), e->cur.cap);
    TNP_CHECK(hipGetLastError());
  } else {
    if (launch_forward(e->net, P<float>(e->cur.xyz), V, P<float>(e->cur.pre), e->cur.cap, 1, s, nullptr,
                       VP(e->cur, e->kw), VZ(e->cur, e->kw), P<uint64_t>(e->cur.grid),
                       P<uint64_t>(e->cur.pz)))
      return -1;
  }
  if (d_pre && keys_for(e, e->cur, 0, V, s)) return -1;
  e->V = V;
  e->keep_all = keep_all;
  e->valid_from = 0;
  e->pend_idx = -1;
  return reset_live(e, s);
}

extern "C" int tnp_engine_sizes(tnp_engine* e, int64_t* V, int64_t* E) {
  if (e->cnt_pending) {  // (never a silent 0 from a deferred count)
    tnp_set_error("tnp_engine_sizes: the live counts of the last step are still pending");
    return -1;
  }
  *V = e->V_live;
  *E = e->E_live;
  return 0;
}

extern "C" int tnp_engine_active_planes(tnp_engine* e, int from, uint64_t* mask, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  TNP_CHECK(hipSetDevice(e->device));
  if (require_valid(e, "active_planes")) return -1;
  if (buf_ensure(e->ctr, CTR_CLEAR_BYTES, s)) return -1;
  TNP_CHECK(hipMemsetAsync(P<int64_t>(e->ctr) + CTR_ACTIVE, 0, sizeof(int64_t), s));
  // the per-edge masks are (re)computed here and the OR of their first split
  // planes taken in the same pass: the planes the next steps must visit
  if (compute_masks(e, from, P<int64_t>(e->ctr), s)) return -1;
  if (read_ctr(e, s)) return -1;
  *mask = (uint64_t)e->h_ctr[CTR_ACTIVE];
  e->act_bits = *mask;
  return 0;
}

extern "C" int tnp_engine_export(tnp_engine* e, float* d_xyz, int64_t* d_edges, float* d_pre,
                                 void* stream) {
  hipStream_t s = (hipStream_t)stream;
  TNP_CHECK(hipSetDevice(e->device));
  if (require_valid(e, "export")) return -1;
  if (compact_now(e, s)) return -1;
  if (d_xyz && e->V > 0)
    TNP_CHECK(hipMemcpyAsync(d_xyz, e->cur.xyz.p, e->V * 3 * sizeof(float), hipMemcpyDeviceToDevice, s));
  if (d_edges && e->E > 0)
    hipLaunchKernelGGL(k_i32_to_i64, dim3(tnp_grid(2 * e->E)), dim3(TNP_BLOCK), 0, s,
                       P<int32_t>(e->edges), d_edges, 2 * e->E);
  if (d_pre && e->V > 0) {
    if (e->valid_from != 0) {
      tnp_set_error("cached planes below %d were dropped (load with keep_all_planes=1)", e->valid_from);
      return -1;
    }
    hipLaunchKernelGGL(k_planes_to_rows, dim3(tnp_grid(e->V)), dim3(TNP_BLOCK), 0, s,
                       P<float>(e->cur.pre), e->cur.cap, e->V, e->K, d_pre);
  }
  TNP_CHECK(hipGetLastError());
  return 0;
}

// extract_skeleton (subpoly.py:556-581)
extern "C" int tnp_engine_surface(tnp_engine* e, void* stream, int64_t* V_out, int64_t* E_out) {
  hipStream_t s = (hipStream_t)stream;
  TNP_CHECK(hipSetDevice(e->device));
  e->rows_valid = false;
  if (require_valid(e, "surface")) return -1;
  if (compact_now(e, s)) return -1;
  const int64_t V = e->V, E = e->E;
  VSet& c = e->cur;
  const float* col = P<float>(c.pre) + (int64_t)(e->K - 1) * c.cap;
  if (buf_ensure(e->used, std::max<int64_t>(V, 1) * sizeof(int32_t), s)) return -1;
  if (buf_ensure(e->flags, std::max<int64_t>(V, 1) * sizeof(int32_t), s)) return -1;
  if (buf_ensure(e->nid, std::max<int64_t>(V, 1) * sizeof(int64_t), s)) return -1;
  TNP_CHECK(hipMemsetAsync(e->ctr.p, 0, CTR_CLEAR_BYTES, s));
  int32_t* on = P<int32_t>(e->flags);
  if (launch_surface_flags(P<float>(c.xyz), col, V, e->net.eps_s, on, s)) return -1;
  if (scan_counts(e, on, P<int64_t>(e->nid), V, CTR_AUX, s)) return -1;
  if (read_ctr(e, s)) return -1;
  if (e->h_ctr[CTR_AUX] < 3) {
    e->V = 0;
    e->E = 0;
    e->E_live = 0;
    *V_out = 0;
    *E_out = 0;
    return reset_live(e, s);
  }
  int64_t nt = step_tiles(E);
  if (buf_ensure(e->blk, (nt + 1) * sizeof(int32_t), s)) return -1;
  if (buf_ensure(e->blkoff, (nt + 1) * sizeof(int64_t), s)) return -1;
  if (buf_ensure(e->edges_alt, std::max<int64_t>(E, 1) * 2 * sizeof(int32_t), s)) return -1;
  const FillOp fu{e->used.p, (uint64_t)V * sizeof(int32_t), 0};
  if (launch_fill(&fu, 1, s)) return -1;
  if (launch_surface_edges(P<int32_t>(e->edges), E, on, P<int32_t>(e->blk), nullptr, 0, nullptr,
                           nullptr, s))
    return -1;
  if (scan_counts(e, P<int32_t>(e->blk), P<int64_t>(e->blkoff), nt, CTR_E, s)) return -1;
  if (launch_surface_edges(P<int32_t>(e->edges), E, on, nullptr, P<int64_t>(e->blkoff), 1,
                           P<int32_t>(e->edges_alt), P<int32_t>(e->used), s))
    return -1;
  if (scan_counts(e, P<int32_t>(e->used), P<int64_t>(e->nid), V, CTR_V, s)) return -1;
  if (vset_ensure(e, e->alt, V, 0, s)) return -1;
  VSet& a = e->alt;
  int keep_from = e->valid_from;
  if (launch_gather_vertices(P<int32_t>(e->used), P<int64_t>(e->nid), V, e->K, keep_from,
                             P<float>(c.xyz), P<float>(c.pre), c.cap, VP(c, e->kw),
                             VZ(c, e->kw), P<uint64_t>(c.grid), P<float>(a.xyz),
                             P<float>(a.pre), a.cap, VP(a, e->kw), VZ(a, e->kw),
                             P<uint64_t>(a.grid), P<uint64_t>(a.pz), s))
    return -1;
  if (read_ctr(e, s)) return -1;
  int64_t E2 = e->h_ctr[CTR_E], V2 = e->h_ctr[CTR_V];
  if (launch_remap_edges(P<int32_t>(e->edges_alt), E2, P<int64_t>(e->nid), s)) return -1;
  std::swap(e->cur, e->alt);
  std::swap(e->edges, e->edges_alt);
  e->V = V2;
  e->E = E2;
  e->E_live = E2;
  *V_out = V2;
  *E_out = E2;
  return reset_live(e, s);
}

// ---------------------------------------------------------------------------
// the step's mode: shards, curve branch, strict filter, the shards' collective
// ---------------------------------------------------------------------------
extern "C" int tnp_engine_set_shards(tnp_engine* e, int world) {
  e->shards = world < 1 ? 1 : world;
  return 0;
}

extern "C" int tnp_engine_set_curve(tnp_engine* e, int on) {
  e->curve = on ? 1 : 0;
  return 0;
}

extern "C" int tnp_engine_set_strict(tnp_engine* e, int on) {
  e->strict = on ? 1 : 0;
  return 0;
}

extern "C" int tnp_engine_set_collective(tnp_engine* e, tnp_collective_fn fn, void* ctx) {
  e->coll_fn = fn;
  e->coll_ctx = ctx;
  return 0;
}

// ---------------------------------------------------------------------------
// slab boundary + kernel timer controls
// ---------------------------------------------------------------------------
extern "C" int tnp_engine_set_owned(tnp_engine* e, int lo, int hi) {
  e->own = OwnBox{{lo, 1, 1}, {hi, 0, 0}};
  return 0;
}

extern "C" int tnp_engine_set_owned_box(tnp_engine* e, const int32_t* lo3, const int32_t* hi3) {
  for (int d = 0; d < 3; ++d) e->own.lo[d] = lo3[d], e->own.hi[d] = hi3[d];
  return 0;
}

extern "C" int tnp_engine_set_eps(tnp_engine* e, float eps) {
  if (!e->has_net) { tnp_set_error("engine has no net"); return -1; }
  if (!(eps > 0.f)) { tnp_set_error("eps must be positive (got %g)", (double)eps); return -1; }
  e->rows_valid = false;
  if (eps != e->net.eps_s) {
    e->net.eps_s = eps;
    e->masks_valid = false;  // first split planes at the new eps
  }
  return 0;
}

extern "C" int tnp_engine_set_span(tnp_engine* e, const int32_t* lo3, const int32_t* hi3) {
  for (int d = 0; d < 3; ++d)
    if (hi3[d] >= lo3[d] && (lo3[d] < 0 || (e->has_net && hi3[d] >= e->net.n_marks))) {
      tnp_set_error("bad span: axis %d marks [%d, %d]", d, lo3[d], hi3[d]);
      return -1;
    }
  for (int d = 0; d < 3; ++d) e->sp_lo[d] = lo3[d], e->sp_hi[d] = hi3[d];
  return 0;
}

extern "C" int tnp_engine_set_xspan(tnp_engine* e, int x0, int x1) {
  const int32_t lo[3] = {x0, 0, 0}, hi[3] = {x1, -1, -1};
  return tnp_engine_set_span(e, lo, hi);
}

extern "C" int tnp_engine_kernel_timer(tnp_engine* e, int on, void* stream, int32_t* n_kernels) {
  hipStream_t s = (hipStream_t)stream;
  TNP_CHECK(hipSetDevice(e->device));
  *n_kernels = 0;
  if (on) {
    e->kt.clear();
    e->kt_on = true;
    return 0;
  }
  e->kt_on = false;
  TNP_CHECK(hipStreamSynchronize(s));
  e->kt_names.clear();
  e->kt_ms.clear();
  e->kt_bytes.clear();
  e->kt_n.clear();
  for (KRec& r : e->kt) {
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, r.a, r.b);
    (void)hipEventDestroy(r.a);
    (void)hipEventDestroy(r.b);
    size_t i = 0;
    for (; i < e->kt_names.size(); ++i)
      if (e->kt_names[i] == r.name) break;
    if (i == e->kt_names.size()) {
      e->kt_names.push_back(r.name);
      e->kt_ms.push_back(0);
      e->kt_bytes.push_back(0);
      e->kt_n.push_back(0);
    }
    e->kt_ms[i] += ms;
    e->kt_bytes[i] += r.bytes;
    e->kt_n[i] += 1;
  }
  e->kt.clear();
  *n_kernels = (int32_t)e->kt_names.size();
  return 0;
}

extern "C" int tnp_engine_kernel_stat(tnp_engine* e, int i, char* name, int cap, double* ms,
                                      int64_t* launches, double* bytes) {
  if (i < 0 || i >= (int)e->kt_names.size()) { tnp_set_error("kernel stat %d out of range", i); return -1; }
  snprintf(name, cap, "%s", e->kt_names[i].c_str());
  *ms = e->kt_ms[i];
  *launches = e->kt_n[i];
  *bytes = e->kt_bytes[i];
  return 0;
}
