// The host side every entry point that takes a polygon soup shares --
// tnp_polygon_report (polygons.hip), tnp_render_raster (render.hip),
// tnp_topology_build (topology.hip), tnp_holes_build (holes.hip),
// tnp_weld_build (weld.hip), tnp_simplify_build (simplify.hip): the argument refusals, the per-call scratch, the two halves of the check front around
// soup_check.h's kernels, the stand-alone scan, the stage events and the
// handle boilerplate.  A new consumer starts from soup_args, soup_offsets and
// soup_verdict and follows no id before the verdict.  Included by those six
// files only, the last four through topo_common.h (anonymous namespace).
#pragma once
#include <vector>

#include "kernels.h"
#include "soup_check.h"

namespace {

#define SOUP_LAUNCH(kernel, count, ...)                                                              \
  do {                                                                                                \
    hipLaunchKernelGGL(kernel, dim3(tnp_grid(count)), dim3(TNP_BLOCK), 0, s, __VA_ARGS__);           \
    TNP_CHECK(hipGetLastError());                                                                     \
  } while (0)

// the refusals of the arguments alone; p_ids: polygon numbers are held in 32
// bits too, xyz_needed: the coordinates are read
inline int soup_args(const char* who, int64_t V, int64_t P, bool p_ids, bool xyz_needed, const float* d_xyz,
                     const int64_t* d_offsets, const int64_t* d_indices) {
  if (P < 0 || V < 0) { tnp_set_error("%s: P = %lld, V = %lld", who, (long long)P, (long long)V); return -1; }
  if (V >= (int64_t)1 << 31) {
    tnp_set_error("%s: V = %lld vertices; ids are held below 2^31", who, (long long)V);
    return -1;
  }
  if (p_ids && P >= (int64_t)1 << 31) {
    tnp_set_error("%s: P = %lld polygons; ids are held below 2^31", who, (long long)P);
    return -1;
  }
  if ((P > 0 && (!d_offsets || !d_indices)) || (xyz_needed && V > 0 && !d_xyz)) {
    tnp_set_error("%s: null array", who);
    return -1;
  }
  return 0;
}

// device scratch of one call, freed on the stream on every way out: one
// stream-ordered allocation per array, unless the caller reserves a block
// first and the arrays are carved out of it (a stream-ordered allocation that
// the pool cannot serve from memory it still holds costs more than most of the
// kernels of a build, and a build has some forty arrays).  An array that does
// not fit the block gets an allocation of its own.
struct Scratch {
  hipStream_t s;
  const char* who;
  std::vector<void*> p;
  char* cur = nullptr;
  size_t left = 0;
  Scratch(hipStream_t st, const char* w) : s(st), who(w) {}
  Scratch(const Scratch&) = delete;
  ~Scratch() {
    for (void* q : p) (void)hipFreeAsync(q, s);
  }
  static size_t pad(size_t bytes) { return ((bytes < 256 ? 256 : bytes) + 255) / 256 * 256; }
  bool reserve(size_t bytes) {
    cur = nullptr, left = 0;
    void* q = alloc(bytes);
    if (!q) return false;
    cur = static_cast<char*>(q), left = pad(bytes);
    return true;
  }
  void* get(size_t bytes) {
    const size_t b = pad(bytes);
    if (b <= left) {
      void* q = cur;
      cur += b, left -= b;
      return q;
    }
    return alloc(bytes);
  }
  void* alloc(size_t bytes) {
    void* q = nullptr;
    if (hipMallocAsync(&q, bytes < 256 ? 256 : bytes, s) != hipSuccess) {
      tnp_set_error("%s: hipMallocAsync of %zu bytes failed", who, bytes);
      return nullptr;
    }
    p.push_back(q);
    return q;
  }
  template <typename T>
  T* arr(int64_t n) { return static_cast<T*>(get((size_t)(n > 0 ? n : 1) * sizeof(T))); }
};

// The check front, first half: the counter block (n_words int64 words, zero
// but for the error word) is allocated, the offsets are checked (deg as
// k_soup_offsets takes it) and read back.  Returns n = offsets[P] >= 3 P --
// every offset is then known to lie in [0, n] -- or -1 with the error set.
constexpr int SOUP_CTR_MAX = 16;
inline int64_t soup_offsets(const char* who, Scratch& scr, const int64_t* d_offsets, const int64_t* d_indices,
                            int64_t V, int64_t P, int64_t** ctr, int n_words, hipStream_t s, int32_t* deg = nullptr) {
  int64_t h[SOUP_CTR_MAX] = {};
  h[SOUP_ERR] = (int64_t)SOUP_NONE;
  if (n_words > SOUP_CTR_MAX || !(*ctr = scr.arr<int64_t>(n_words))) return -1;
  TNP_CHECK(hipMemcpyAsync(*ctr, h, n_words * sizeof(int64_t), hipMemcpyHostToDevice, s));
  SOUP_LAUNCH(k_soup_offsets, P, d_offsets, P, *ctr, deg);
  TNP_CHECK(hipMemcpyAsync(h, *ctr, 2 * sizeof(int64_t), hipMemcpyDeviceToHost, s));
  TNP_CHECK(hipStreamSynchronize(s));
  if ((unsigned long long)h[SOUP_ERR] != SOUP_NONE)
    return soup_report_error(who, (unsigned long long)h[SOUP_ERR], d_offsets, d_indices, V, s);
  return h[SOUP_NIDX];
}

// second half, behind the caller's id check (k_soup_edges, the rasteriser's k_rv_ids) and
// whatever it queues that follows no id: the first n_words counters are read
// back into h and the verdict reported.  0: every id lies in [0, V).
inline int soup_verdict(const char* who, const int64_t* d_offsets, const int64_t* d_indices, int64_t V,
                        const int64_t* ctr, int64_t* h, int n_words, hipStream_t s) {
  TNP_CHECK(hipMemcpyAsync(h, ctr, n_words * sizeof(int64_t), hipMemcpyDeviceToHost, s));
  TNP_CHECK(hipStreamSynchronize(s));
  if ((unsigned long long)h[SOUP_ERR] != SOUP_NONE)
    return soup_report_error(who, (unsigned long long)h[SOUP_ERR], d_offsets, d_indices, V, s);
  return 0;
}

// look-back state of one stand-alone scan launch over buf, scan_tiles(n) + 1
// words zeroed once; a fresh epoch per launch (common.h TnpLB; ticket-free,
// so no ticket base)
inline TnpLB scan_lb(uint64_t* buf, uint32_t epoch = 1) {
  TnpLB lb{};
  lb.ticket = reinterpret_cast<unsigned long long*>(buf);
  lb.st = buf + 1;
  lb.tbase = 0;
  lb.epoch = epoch;
  lb.spin = -1;
  lb.rc = nullptr;
  return lb;
}

// rank = the exclusive scan of flag, its sum -> *total (device)
inline int scan_flags(Scratch& scr, const int32_t* flag, int64_t n, int64_t* rank, int64_t* total, hipStream_t s) {
  const size_t words = (size_t)scan_tiles(n) + 1;
  uint64_t* buf = scr.arr<uint64_t>((int64_t)words);
  if (!buf) return -1;
  TNP_CHECK(hipMemsetAsync(buf, 0, words * sizeof(uint64_t), s));
  return scan_i32_to_i64(flag, rank, n, total, scan_lb(buf), s);
}

inline int bits_for(int64_t n) {  // the smallest b >= 1 with 2^b >= n
  int b = 1;
  while (((int64_t)1 << b) < n) ++b;
  return b;
}

// the stage events of a timed build
struct Stages {
  bool on;
  hipStream_t s;
  std::vector<hipEvent_t> ev;
  Stages(bool o, hipStream_t st) : on(o), s(st) {}
  Stages(const Stages&) = delete;
  ~Stages() {
    for (hipEvent_t e : ev) (void)hipEventDestroy(e);
  }
  void mark() {
    if (!on) return;
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) { on = false; return; }
    (void)hipEventRecord(e, s);
    ev.push_back(e);
  }
};

// ---- the handles (tnp_topology, tnp_holes, tnp_weld, tnp_simplify): H has device, timed, n_ms and
// ms[N]; drop(h) frees what the last build left ----
template <class H>
int handle_create(const char* who, H** out, int device) {
  if (!out) { tnp_set_error("%s: null handle pointer", who); return -1; }
  TNP_CHECK(hipSetDevice(device));
  *out = new H();
  (*out)->device = device;
  return 0;
}

template <class H, class Drop>
void handle_destroy(H* h, Drop drop) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  drop(h);
  delete h;
}

// a call on the handle: its device is made current
template <class H>
int handle_use(const char* who, H* h) {
  if (!h) { tnp_set_error("%s: null handle", who); return -1; }
  TNP_CHECK(hipSetDevice(h->device));
  return 0;
}

// tnp_debug_*_stages
template <class H>
int handle_stages(const char* who, H* h, int enable, double* ms, int n) {
  constexpr int N = sizeof(H::ms) / sizeof(double);
  if (!h) { tnp_set_error("%s: null handle", who); return -1; }
  h->timed = enable != 0;
  if (ms)
    for (int i = 0; i < n && i < N; ++i) ms[i] = i < h->n_ms ? h->ms[i] : 0.0;
  return N;
}

// the stage times of a finished build, when every mark was recorded
template <class H>
void handle_keep_ms(H* h, const Stages& st) {
  constexpr int N = sizeof(H::ms) / sizeof(double);
  if (!st.on || (int)st.ev.size() != N + 1) return;
  for (int i = 0; i < N; ++i) {
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, st.ev[i], st.ev[i + 1]);
    h->ms[i] = (double)ms;
  }
  h->n_ms = N;
}

}  // namespace
