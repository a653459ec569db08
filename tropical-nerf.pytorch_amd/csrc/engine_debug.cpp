// The engine's debug entry points (include/tropical_hip_debug.h): what the
// tests read or force that the extraction itself never needs.
#include "engine.h"

using namespace tnp_host;

extern "C" int tnp_engine_debug_vertex_capacity(tnp_engine* e, int64_t* rows, int64_t* early_redo) {
  if (!e || !rows || !early_redo) { tnp_set_error("tnp_engine_debug_vertex_capacity: null argument"); return -1; }
  *rows = e->cur.cap;
  *early_redo = e->n_early_redo;
  return 0;
}

extern "C" int tnp_debug_buf_growth(int64_t have_bytes, int64_t request_bytes, int64_t members, int xs_n,
                                    int64_t* grown_bytes, int64_t* key_cap) {
  if (have_bytes < 0 || request_bytes < 0 || members < 0 || xs_n < 1 || xs_n > 63) {
    tnp_set_error("tnp_debug_buf_growth: bad argument");
    return -1;
  }
  if (grown_bytes) *grown_bytes = (int64_t)buf_grow_bytes((size_t)have_bytes, (size_t)request_bytes);
  if (key_cap) *key_cap = connect_key_cap((size_t)have_bytes, members, xs_n);
  return 0;
}

// diagnostics of the ticket-free look-back (common.h lb_prefix_rc): the poll
// count before a waiting wave recomputes an unpublished predecessor (< 0: the
// kernels' defaults; 0 forces the recompute on every unpublished one), and
// the number of recomputes since the last reset
extern "C" int tnp_engine_debug_set_lb_spin(tnp_engine* e, int spin) {
  e->lb_spin = spin;
  return 0;
}
extern "C" int tnp_engine_debug_set_lds_records(tnp_engine* e, int on) {
  e->lds_records = on != 0;
  return 0;
}
extern "C" int tnp_engine_debug_lb_recomputes(tnp_engine* e, int64_t* n, int reset, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  TNP_CHECK(hipSetDevice(e->device));
  *n = 0;
  if (!e->lbrc.p) return 0;
  uint64_t v = 0;
  TNP_CHECK(hipMemcpyAsync(&v, e->lbrc.p, sizeof(v), hipMemcpyDeviceToHost, s));
  TNP_CHECK(hipStreamSynchronize(s));
  if (reset) TNP_CHECK(hipMemsetAsync(e->lbrc.p, 0, sizeof(uint64_t), s));
  *n = (int64_t)v;
  return 0;
}
// the count scan on its own, as scan_counts runs it: chain 0 of the engine's
// look-back buffer, its epoch and lb_spin; the total comes back to the host
extern "C" int tnp_engine_debug_scan(tnp_engine* e, const int32_t* d_in, int64_t n, int64_t* d_out,
                                     int64_t* h_total, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!e || !h_total || n < 0 || (n > 0 && (!d_in || !d_out))) {
    tnp_set_error("tnp_engine_debug_scan: bad argument");
    return -1;
  }
  TNP_CHECK(hipSetDevice(e->device));
  int64_t* tot = nullptr;
  TNP_CHECK(hipMalloc(&tot, sizeof(int64_t)));
  TnpLB lb{};
  int rc = (n > 0 && lb_begin(e, scan_tiles(n), s, &lb, 0, false)) ? -1 : 0;
  if (rc == 0) rc = scan_i32_to_i64(d_in, d_out, n, tot, lb, s);
  if (rc == 0 && hipMemcpyAsync(h_total, tot, sizeof(int64_t), hipMemcpyDeviceToHost, s) != hipSuccess) {
    tnp_set_error("tnp_engine_debug_scan: total readback failed");
    rc = -1;
  }
  if (hipStreamSynchronize(s) != hipSuccess && rc == 0) {
    tnp_set_error("tnp_engine_debug_scan: stream synchronise failed");
    rc = -1;
  }
  (void)hipFree(tot);
  return rc;
}
// a look-back chain's launch epoch (lb_begin): read, and with set >= 0
// overwritten -- the host field only, the records in memory stay
extern "C" int tnp_engine_debug_lb_epoch(tnp_engine* e, int chain, int64_t set, int64_t* h_epoch) {
  if (!e || chain < 0 || chain > 1 || set > 0x3FFFFF) {
    tnp_set_error("tnp_engine_debug_lb_epoch: bad argument");
    return -1;
  }
  if (h_epoch) *h_epoch = (int64_t)e->lb_epoch[chain];
  if (set >= 0) e->lb_epoch[chain] = (uint32_t)set;
  return 0;
}

// debugging aid: the gradient-descent fallback on arbitrary rows
// (tropical_hip_debug.h; checked against the oracle's descent)
extern "C" int tnp_debug_descend(const tnp_net* n, const float* d_ends, float* d_x, const int32_t* d_plane,
                                 int64_t N, int idx, float eps, int iters, float* d_d0, float* d_d1, int per_thread,
                                 void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (check_net(n)) return -1;
  if (N <= 0) return 0;
  if (N > (1 << 20)) { tnp_set_error("debug_descend: at most 2^20 rows"); return -1; }
  NetDev net = to_dev(n);
  // the engine's operands for rows of a made-up complex: vertices 2r, 2r + 1
  // are the ends of split r, which is curve row r and descending row r
  std::vector<int32_t> h(4 * N);
  for (int64_t r = 0; r < N; ++r) {
    h[r] = (int32_t)(2 * r);          // sa
    h[N + r] = (int32_t)(2 * r + 1);  // sb
    h[2 * N + r] = (int32_t)r;        // crow
    h[3 * N + r] = (int32_t)r;        // glist
  }
  int32_t* d = nullptr;
  unsigned long long* conv = nullptr;
  TNP_CHECK(hipMalloc(&d, 4 * N * sizeof(int32_t)));
  TNP_CHECK(hipMalloc(&conv, 8 * sizeof(unsigned long long)));
  int rc = hipMemcpyAsync(d, h.data(), 4 * N * sizeof(int32_t), hipMemcpyHostToDevice, s) == hipSuccess ? 0 : -1;
  if (rc == 0) {
    const char* prev = getenv("TNP_DESCEND_THREAD");
    std::string keep = prev ? prev : "";
    setenv("TNP_DESCEND_THREAD", per_thread ? "1" : "0", 1);
    rc = launch_descend(net, N, d + 3 * N, d + 2 * N, d, d + N, d_ends, d_plane, idx, eps, iters, 0, d_x, d_d0,
                        d_d1, conv, s);
    if (prev) setenv("TNP_DESCEND_THREAD", keep.c_str(), 1);
    else unsetenv("TNP_DESCEND_THREAD");
  }
  if (hipStreamSynchronize(s) != hipSuccess && rc == 0) {
    tnp_set_error("debug_descend: stream synchronise failed");
    rc = -1;
  }
  (void)hipFree(d);
  (void)hipFree(conv);
  return rc;
}
