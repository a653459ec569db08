// Host side of the curve branch (force=False, kernels in curve.hip) and the
// shards' collective it takes its whole-batch decisions with.
#include "engine.h"

using namespace tnp_host;

// ---------------------------------------------------------------------------
// curve path, phase 1 (subpoly.py:120-177, 204-207): correct the new vertices
// of non-axis-aligned split edges to the trilinear intersection, with the
// gradient-descent fallback; leaves per-split strict-filter inputs in cinfo.
// ---------------------------------------------------------------------------
namespace tnp_host {

// the shards' reduction of n words (tnp_engine_set_collective); one shard:
// none.  Every call carries one more word, this shard's failure flag
// (coll_fail), reduced with the same op: a shard that failed between two
// collectives joins the next one with the flag set, and every shard then
// fails at that same call -- none is left blocked in a collective its peer
// never reaches.
int coll(tnp_engine* e, int64_t* v, int n, int op) {
  if (e->shards <= 1) return 0;
  if (!e->coll_fn) {
    tnp_set_error("curve path on %d shards: no collective for its whole-complex decisions "
                  "(tnp_engine_set_collective)", e->shards);
    return -1;
  }
  const bool all_ones = op == TNP_COLL_AND;  // AND: "no failure" is all ones
  std::vector<int64_t> w(v, v + n);
  w.push_back(e->coll_err ? (all_ones ? 0 : 1) : (all_ones ? -1 : 0));
  if (e->coll_fn(w.data(), n + 1, op, e->coll_ctx) != 0) {
    tnp_set_error("the shards' collective failed");
    return -1;
  }
  if (all_ones ? w[n] != -1 : w[n] != 0) {
    if (!e->coll_err) tnp_set_error("a peer shard failed in this sharded step (its own error names the cause)");
    e->coll_err = false;
    return -1;
  }
  std::copy(w.begin(), w.begin() + n, v);
  return 0;
}

// this shard failed before the step's next collective (n words, op): join
// it with the failure flag set, keep this shard's own error message
int coll_fail(tnp_engine* e, int n, int op) {
  if (e->shards <= 1 || !e->coll_fn) return -1;
  const std::string msg = g_err;
  std::vector<int64_t> v(n, op == TNP_COLL_AND ? -1 : 0);
  e->coll_err = true;
  (void)coll(e, v.data(), n, op);
  e->coll_err = false;
  g_err = msg;
  return -1;
}

// curve path, phase 1 (subpoly.py:120-177, subpoly_debug.py:121-165).  On
// shards (e->shards > 1) every shard calls it for every split step, S == 0
// included, and takes the batch's decisions with the others: the curve rows'
// and descent rows' totals (MKL's row-count schedules of the corner, point
// and descent launches follow the whole batch) and the descent's stop (the
// AND of the shards' per-iteration convergence words).
// A sharded curve step whose batch -- the shards' total rows of one of its
// forwards -- is 2..15 rows on a 32-wide net: MKL's 32-input FOLD schedule
// of the 2-output layer depends on each row's parity in the WHOLE batch
// (net_device.h neuron_mode), the shards number their rows locally, and the
// batch's row order across shards is not defined.  Refused instead of left
// to halo_check; every shard sees the same total after the
// same collective, so every shard refuses at the same point.
int fold32_sharded(const tnp_engine* e, int64_t rows, const char* what, int idx) {
  if (e->shards > 1 && e->net.num_hidden == 32 && rows >= 2 && rows <= 15) {
    tnp_set_error("plane %d: a sharded curve step of %lld %s on a 32-wide net (MKL's 2..15-row FOLD schedule "
                  "depends on each row's parity in the whole batch, which the shards do not share); run it "
                  "unsharded", idx, (long long)rows, what);
    return -1;
  }
  return 0;
}

int curve_correct(tnp_engine* e, int idx, int64_t S, hipStream_t s) {
  const float eps = e->net.eps_s;  // subpoly_'s eps (subpoly.py:120-177)
  const int K = e->K;
  Buf* cv = e->cv;
  int64_t* ctr = P<int64_t>(e->ctr);
  const int32_t* sa = P<int32_t>(e->sa);
  const int32_t* sb = P<int32_t>(e->sb);
  float* xyz = P<float>(e->cur.xyz);
  // (sharded: a segment that fails joins the step's next collective with the
  // failure flag, coll_fail, so every shard stops at the same call)
  int64_t B = 0;
  auto seg_flags = [&]() -> int {
  if (S > 0) {
    if (buf_ensure(cv[CV_CFLAG], S * sizeof(int32_t), s)) return -1;
    if (buf_ensure(cv[CV_COFF], S * sizeof(int64_t), s)) return -1;
    if (buf_ensure(cv[CV_CINFO], S * sizeof(int32_t), s)) return -1;
    const FillOp f{cv[CV_CINFO].p, (uint64_t)S * sizeof(int32_t), 0};
    if (launch_fill(&f, 1, s)) return -1;
    TIMED("curve_flags", 32.0 * S,
          launch_curve_flags(sa, sb, S, xyz, eps, P<int32_t>(cv[CV_CFLAG]), s));
    if (scan_counts(e, P<int32_t>(cv[CV_CFLAG]), P<int64_t>(cv[CV_COFF]), S, CTR_B, s)) return -1;
    if (read_ctr(e, s)) return -1;
    B = e->h_ctr[CTR_B];
  }
  return 0;
  };
  if (seg_flags()) return coll_fail(e, 1, TNP_COLL_SUM);
  const bool sh = e->shards > 1;
  int64_t Bg = B;  // the batch's curve rows (r_edges, subpoly.py:120)
  if (coll(e, &Bg, 1, TNP_COLL_SUM)) return -1;
  if (Bg == 0) return 0;
  if (fold32_sharded(e, Bg, "curve rows", idx)) return -1;
  NetDev ns = e->net;  // sharded: the schedules of the whole batch
  int64_t G = 0;
  int32_t* crow = nullptr;
  int32_t* plane = nullptr;
  float* ints = nullptr;
  float* d0s = nullptr;
  float* d1s = nullptr;
  auto seg_rows = [&]() -> int {
  if (B > 0) {
  if (buf_ensure(cv[CV_CROW], B * sizeof(int32_t), s)) return -1;
  if (buf_ensure(cv[CV_CORNERS], 24 * B * sizeof(float), s)) return -1;
  if (buf_ensure(cv[CV_PLANE], B * sizeof(int32_t), s)) return -1;
  if (buf_ensure(cv[CV_STAGE_C], (size_t)8 * B * K * sizeof(float), s)) return -1;
  if (buf_ensure(cv[CV_INTS], 3 * B * sizeof(float), s)) return -1;
  if (buf_ensure(cv[CV_INTS0], 3 * B * sizeof(float), s)) return -1;
  if (buf_ensure(cv[CV_PTS], 3 * B * sizeof(float), s)) return -1;
  if (buf_ensure(cv[CV_STAGE_P], (size_t)B * K * sizeof(float), s)) return -1;
  for (int k : {CV_D0, CV_D1, CV_GG, CV_GD}) if (buf_ensure(cv[k], B * 4, s)) return -1;
  if (buf_ensure(cv[CV_GOFF], B * sizeof(int64_t), s)) return -1;
  crow = P<int32_t>(cv[CV_CROW]);
  plane = P<int32_t>(cv[CV_PLANE]);
  ints = P<float>(cv[CV_INTS]);
  d0s = P<float>(cv[CV_D0]);
  d1s = P<float>(cv[CV_D1]);
  if (launch_curve_rows(P<int32_t>(cv[CV_CFLAG]), P<int64_t>(cv[CV_COFF]), S, crow, s)) return -1;
  TIMED("curve_corners", 8.0 * B * 12 + 24.0 * B,
        launch_curve_corners(crow, B, sa, sb, xyz, VZ(e->cur, e->kw), P<uint64_t>(e->cur.grid), idx,
                             P<float>(cv[CV_CORNERS]), plane, ctr, e->kw, s));
  if (sh) ns.sched_rows = 8 * Bg;
  TIMED("curve_forward", 8.0 * B * (12 + 4.0 * K),
        launch_forward(ns, P<float>(cv[CV_CORNERS]), 8 * B, P<float>(cv[CV_STAGE_C]), 8 * B, 8, s));
  TIMED("curve_solve", 64.0 * B + 24.0 * B,
        launch_curve_solve(B, P<float>(cv[CV_STAGE_C]), 8 * B, plane, idx, crow, sa, sb, xyz, ints,
                           P<float>(cv[CV_PTS]), s));
  if (sh) ns.sched_rows = Bg;
  TIMED("curve_forward", B * (12 + 4.0 * K),
        launch_forward(ns, P<float>(cv[CV_PTS]), B, P<float>(cv[CV_STAGE_P]), B, 1, s));
  if (launch_curve_dnew(B, P<float>(cv[CV_STAGE_P]), B, plane, idx, ints, eps, d0s, d1s,
                        P<int32_t>(cv[CV_GG]), P<int32_t>(cv[CV_GD]), s)) return -1;
  if (scan_counts(e, P<int32_t>(cv[CV_GD]), P<int64_t>(cv[CV_GOFF]), B, CTR_G, s)) return -1;
  if (read_ctr(e, s)) return -1;
  if (e->h_ctr[CTR_NOPLANE] & 2) {
    tnp_set_error("curve path, plane %d: a split edge's endpoints share fewer than two zero columns (the "
                  "reference's check_new_vertices_on_two_planes then fails: AttributeError, "
                  "subpoly_debug.py:96-104)", idx);
    return -1;
  }
  if (e->h_ctr[CTR_NOPLANE]) {
    tnp_set_error("curve path: a split edge shares no plane below %d (the reference prints it and "
                  "exit()s, subpoly.py:141-148)", idx);
    return -1;
  }
  G = e->h_ctr[CTR_G];
  }  // B > 0
  return 0;
  };
  if (seg_rows()) return coll_fail(e, 1, TNP_COLL_SUM);
  int64_t Gg = G;  // the batch's descent rows
  if (coll(e, &Gg, 1, TNP_COLL_SUM)) return -1;
  if (fold32_sharded(e, Gg, "descent rows", idx)) return -1;
  if (Gg > 0) {
    if (sh) ns.sched_rows = Gg;
    uint64_t h_conv[8] = {~0ull, ~0ull, ~0ull, ~0ull, ~0ull, ~0ull, ~0ull, ~0ull};  // (no rows: converged)
    int32_t* glist = nullptr;
    unsigned long long* conv = nullptr;
    auto seg_desc = [&]() -> int {
    if (G > 0) {
      if (buf_ensure(cv[CV_GLIST], G * sizeof(int32_t), s)) return -1;
      if (buf_ensure(cv[CV_CONV], 8 * sizeof(uint64_t), s)) return -1;
      glist = P<int32_t>(cv[CV_GLIST]);
      conv = P<unsigned long long>(cv[CV_CONV]);
      if (launch_gd_rows(P<int32_t>(cv[CV_GD]), P<int64_t>(cv[CV_GOFF]), B, glist, s)) return -1;
      TNP_CHECK(hipMemcpyAsync(cv[CV_INTS0].p, ints, 3 * B * sizeof(float), hipMemcpyDeviceToDevice, s));
      TNP_CHECK(hipMemsetAsync(conv, 0xFF, 8 * sizeof(uint64_t), s));
      TIMED("descend", 0.0,
            launch_descend(ns, G, glist, crow, sa, sb, xyz, plane, idx, eps, e->gd_iters, 1, ints,
                           d0s, d1s, conv, s));
      TNP_CHECK(hipMemcpyAsync(h_conv, conv, sizeof(h_conv), hipMemcpyDeviceToHost, s));
      TNP_CHECK(hipStreamSynchronize(s));
    }
    return 0;
    };
    if (seg_desc()) return coll_fail(e, 8, TNP_COLL_AND);
    // the loop of subpoly_debug.py:141 stops when EVERY row of the batch met
    // both planes: the AND of the shards' per-iteration words
    if (coll(e, reinterpret_cast<int64_t*>(h_conv), 8, TNP_COLL_AND)) return -1;
    int stop = -1;  // first iteration after which every row met both planes (the replay below
                    // fails towards the step's next collective, the strict flag's OR)
    for (int i = 0; i < e->gd_iters && stop < 0; ++i)
      if ((h_conv[i >> 6] >> (i & 63)) & 1) stop = i;
    auto seg_replay = [&]() -> int {
    if (G > 0 && stop >= 0 && stop + 1 < e->gd_iters) {
      // the loop ends after iteration `stop`: replay
      TNP_CHECK(hipMemcpyAsync(ints, cv[CV_INTS0].p, 3 * B * sizeof(float), hipMemcpyDeviceToDevice, s));
      TIMED("descend", 0.0,
            launch_descend(ns, G, glist, crow, sa, sb, xyz, plane, idx, eps, stop + 1, 0, ints,
                           d0s, d1s, conv, s));
    }
    return 0;
    };
    if (seg_replay()) return coll_fail(e, 1, TNP_COLL_OR);
  }
  auto seg_apply = [&]() -> int {
  if (B > 0)
    TIMED("curve_apply", 60.0 * B,
          launch_curve_apply(B, crow, sa, sb, xyz, e->V, ints, d0s, P<int32_t>(cv[CV_GG]), eps,
                             P<int32_t>(cv[CV_CINFO]), ctr, s));
  return 0;
  };
  if (seg_apply()) return coll_fail(e, 1, TNP_COLL_OR);
  return 0;
}

// curve path, phase 2 (subpoly_debug.py:234-271): strict filter after the
// override; surviving splits get consecutive ids in edge order and rewire
// their edges (masked_scatter_ of the filtered mask, subpoly.py:201-212).
int curve_filter(tnp_engine* e, int idx, int override_, hipStream_t s, int64_t* S_out) {
  const int64_t S = e->pend_S, V = e->V;
  const int K = e->K;
  Buf* cv = e->cv;
  if (S == 0) { *S_out = 0; return 0; }
  if (buf_ensure(cv[CV_KEEP], S * sizeof(int32_t), s)) return -1;
  if (buf_ensure(cv[CV_NID], S * sizeof(int64_t), s)) return -1;
  if (launch_strict_keep(S, P<int32_t>(cv[CV_CINFO]), P<float>(e->stage), idx, override_,
                         P<uint64_t>(e->shared), e->net.eps_s, e->pend_tight, e->strict, P<int32_t>(cv[CV_KEEP]),
                         e->kw, s))
    return -1;
  if (scan_counts(e, P<int32_t>(cv[CV_KEEP]), P<int64_t>(cv[CV_NID]), S, CTR_KEEP, s)) return -1;
  if (read_ctr(e, s)) return -1;
  const int64_t S2 = e->h_ctr[CTR_KEEP];
  const int64_t n = std::max<int64_t>(S2, 1);
  if (buf_ensure(cv[CV_SA2], n * sizeof(int32_t), s)) return -1;
  if (buf_ensure(cv[CV_SB2], n * sizeof(int32_t), s)) return -1;
  if (buf_ensure(cv[CV_SHARED2], n * sizeof(uint64_t) * e->kw, s)) return -1;
  if (buf_ensure(cv[CV_STAGE2], (size_t)n * K * sizeof(float), s)) return -1;
  if (buf_ensure(cv[CV_XYZ2], 3 * n * sizeof(float), s)) return -1;
  if (buf_ensure(cv[CV_GRID2], n * sizeof(uint64_t), s)) return -1;
  TIMED("compact_splits", (16.0 + 8.0 * K + 40.0) * S,
        launch_compact_splits(S, K, P<int32_t>(cv[CV_KEEP]), P<int64_t>(cv[CV_NID]),
                              P<int32_t>(cv[CV_EIDX]), V, P<int32_t>(e->sa), P<int32_t>(e->sb),
                              P<uint64_t>(e->shared), P<float>(e->stage), P<float>(e->cur.xyz),
                              P<uint64_t>(e->cur.grid), S2, P<int32_t>(cv[CV_SA2]),
                              P<int32_t>(cv[CV_SB2]), P<uint64_t>(cv[CV_SHARED2]),
                              P<float>(cv[CV_STAGE2]), P<float>(cv[CV_XYZ2]),
                              P<uint64_t>(cv[CV_GRID2]), P<int32_t>(e->edges), e->kw, s));
  if (S2 > 0) {
    TNP_CHECK(hipMemcpyAsync(P<float>(e->cur.xyz) + 3 * V, cv[CV_XYZ2].p, 3 * S2 * sizeof(float),
                             hipMemcpyDeviceToDevice, s));
    TNP_CHECK(hipMemcpyAsync(P<uint64_t>(e->cur.grid) + V, cv[CV_GRID2].p, S2 * sizeof(uint64_t),
                             hipMemcpyDeviceToDevice, s));
  }
  std::swap(e->sa, cv[CV_SA2]);
  std::swap(e->sb, cv[CV_SB2]);
  std::swap(e->shared, cv[CV_SHARED2]);
  std::swap(e->stage, cv[CV_STAGE2]);
  e->pend_S = S2;
  *S_out = S2;
  return 0;
}

}  // namespace tnp_host

extern "C" int tnp_engine_split_keep(tnp_engine* e, int32_t* d_keep, int64_t n, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  TNP_CHECK(hipSetDevice(e->device));
  if (!e->curve || n <= 0) return 0;
  if (e->cv[CV_KEEP].bytes < (size_t)n * sizeof(int32_t)) {
    tnp_set_error("split_keep: no strict filter ran for %lld splits", (long long)n);
    return -1;
  }
  TNP_CHECK(hipMemcpyAsync(d_keep, e->cv[CV_KEEP].p, n * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
  return 0;
}
