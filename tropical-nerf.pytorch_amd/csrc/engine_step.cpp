// One step of the hyperplane loop on the host: tnp_engine_split and its
// stages, tnp_engine_finish and its phases, and the loop itself
// (tnp_engine_run_steps).  Kernels in step.hip, bucket.hip, sort.hip.
#include "engine.h"

using namespace tnp_host;

// the flat step's new vertices: split points + forward + failover test +
// keys in one pass, straight into the cache (k_forward_new).  n < 0: S is
// still on the device (launched right behind the split, before the host
// reads S back: the readback's round trip overlaps this kernel), -n bounds
// it and sizes the vertex set and the shared-plane words.
static int64_t early_bound(const tnp_engine* e) {
  if (!e->early_bound_splits) return e->E;
  return std::min<int64_t>(e->E, e->max_split_seen + e->max_split_seen / 4 + 4096);
}

static int flat_forward_new(tnp_engine* e, int idx, int64_t n, hipStream_t s) {
  const int64_t bound = n >= 0 ? n : -n;
  if (vset_ensure(e, e->cur, e->V + bound, e->V, s)) return -1;
  if (buf_ensure(e->shared, bound * sizeof(uint64_t) * e->kw, s)) return -1;
  const float* col = P<float>(e->cur.pre) + (int64_t)idx * e->cur.cap;  // (after any move)
  e->pend_keep = new_keep_from(e, idx);
  // compulsory bytes per split: reads 8 B endpoint ids, 24 B endpoint
  // coordinates, 8 B endpoint plane values, 16 B endpoint zero keys; writes
  // 12 B coordinates, the cache planes >= keep_from, 32 B keys (pz: pos and
  // zero, the only copy since round 6; grid; shared); plus the encoding
  // tables once per launch (the 8
  // corners x L levels gathers are cache traffic).  (n < 0: set once S is known)
  TIMED("forward_new",
        (8.0 + 24.0 + 8.0 + 16.0 + 12.0 + 4.0 * (e->K - e->pend_keep) + 32.0) * std::max<int64_t>(n, 0) +
            table_bytes(e->net),
        launch_forward_new(e->net, P<float>(e->cur.xyz) + 3 * e->V, n, P<float>(e->cur.pre), e->cur.cap, e->V,
                           e->pend_keep, P<int32_t>(e->sa), P<int32_t>(e->sb), idx, e->own,
                           VP(e->cur, e->kw), VZ(e->cur, e->kw), P<uint64_t>(e->cur.grid),
                           P<uint64_t>(e->shared), P<int64_t>(e->ctr), P<uint64_t>(e->cur.pz), col, s));
  return 0;
}

// what the stages of one tnp_engine_split share (built by the driver)
struct SplitStep {
  int idx;
  float eps;       // subpoly_'s eps: hits, split point, failover
  int64_t S, Sg;   // this shard's splits; the whole batch's (ccoll: the shards' total)
  bool early_fwd;  // k_forward_new already launched (device S)
  // curve branch on shards: the new vertices' forward follows the schedule of
  // the whole batch, and every shard joins the branch's decisions (curve_correct)
  bool ccoll;
  int32_t* fail;   // out: the failover flag (-1: left on the device)
};

// 1. the split, the plane's hit vertices and (flat path) the early forward
static int split_edges(tnp_engine* e, SplitStep& p, hipStream_t s) {
  const int idx = p.idx;
  const float eps = p.eps;
  const float* col = P<float>(e->cur.pre) + (int64_t)idx * e->cur.cap;
  int64_t& S = p.S;
  bool& early_fwd = p.early_fwd;
  // the last step's deferred live counts ride in this split's hit workers
  // (the flat bucket path); otherwise they are counted now, before the reset
  BucketGeom bgs{};
  const bool fused_hits = !e->curve && e->V > 0 && e->E > 0 && uses_buckets(e, &bgs);
  if (e->cnt_pending && !fused_hits && resolve_counts(e, s)) return -1;
  const bool take_counts = e->cnt_pending;
  if (!(e->in_run && e->ctr_zero)) TNP_CHECK(hipMemsetAsync(e->ctr.p, 0, CTR_CLEAR_BYTES, s));
  e->ctr_zero = false;
  if (e->E > 0) {
    // single pass; the id buffers hold the upper bound E (capacity is kept)
    if (buf_ensure(e->sa, e->E * sizeof(int32_t), s)) return -1;
    if (buf_ensure(e->sb, e->E * sizeof(int32_t), s)) return -1;
    if (e->curve && buf_ensure(e->cv[CV_EIDX], e->E * sizeof(int32_t), s)) return -1;
    const int fresh = ensure_masks(e, idx, s);
    if (fresh < 0) return -1;
    TnpLB lb;
    if (lb_begin(e, split_tiles(e->E), s, &lb, 0, false)) return -1;
    // flat path: the plane's hit vertices are found with the split (they
    // read only the cached column and the live flags), so one readback
    // returns S and H.  The bucket path reads them at members[E, E + H)
    // (S <= E) and they ride in the split's own dispatch; the radix path
    // wants them after the S new members (members[S, S + H)): launched
    // behind the split, which writes S
    const bool flat_hits = !e->curve && e->V > 0;
    if (flat_hits && buf_ensure(e->members, (e->E + e->V) * sizeof(int32_t), s)) return -1;
    if (take_counts && buf_ensure(e->hpart, HIT_WORKERS_MAX * sizeof(int64_t), s)) return -1;
    const HitArgs ha{col, P<uint8_t>(e->live), e->V, eps, P<int32_t>(e->members) + e->E,
                     take_counts ? P<int64_t>(e->hpart) : nullptr};
    // algorithmic bytes: 1 B first split plane per edge (+ 5 B per vertex
    // slot for fused hits); per split 8 B endpoints, 4 B rewired id, 1 B
    // stale mask (set once S is known)
    TIMED("split", 1.0 * e->E + (fused_hits ? 5.0 * e->V : 0.0),
          launch_split_lb(P<int32_t>(e->edges), e->E, P<uint8_t>(e->eef), P<uint8_t>(e->edm), idx,
                          e->V, P<int32_t>(e->sa), P<int32_t>(e->sb), P<int64_t>(e->ctr),
                          e->curve ? P<int32_t>(e->cv[CV_EIDX]) : nullptr, lb, s, fused_hits ? &ha : nullptr));
    if (flat_hits && !fused_hits)
      TIMED("hits", 5.0 * e->V,
            launch_hits(col, P<uint8_t>(e->live), e->V, eps, P<int32_t>(e->members), -1,
                        P<int64_t>(e->ctr), s));
    e->pend_hits = flat_hits;
    e->pend_hoff = fused_hits ? e->E : -1;
    // flat path: the new vertices' forward goes behind the split now, sized
    // by the bound S <= E, so the GPU runs it while S travels to the host
    early_fwd = !e->curve && e->early_forward;
    const int64_t eb = early_fwd ? early_bound(e) : 0;
    int64_t seq = 0;
    if (take_counts ? post_ctr(e, s, &seq, P<int64_t>(e->hpart), split_hit_workers(e->V),
                               e->pend_lz_n ? P<int64_t>(e->lzpart) : nullptr, (int)e->pend_lz_n)
                    : post_ctr(e, s, &seq))
      return -1;
    if (early_fwd && flat_forward_new(e, idx, -eb, s)) return -1;
    if (wait_ctr(e, s, seq)) return -1;
    if (take_counts) apply_counts(e, e->h_ctr[CTR_V], e->h_ctr[CTR_E]);
    S = e->h_ctr[CTR_S];
    e->max_split_seen = std::max(e->max_split_seen, S);
    if (early_fwd && S > eb) {
      // more splits than the early launch's bound: it processed rows [0, eb)
      // only; the whole forward runs again once S is known (the same values;
      // the failover OR is idempotent, the halo count is recounted)
      early_fwd = false;
      e->n_early_redo++;
      TNP_CHECK(hipMemsetAsync(P<int64_t>(e->ctr) + CTR_DUP, 0, sizeof(int64_t), s));
    }
    if (fresh) e->act_bits = (uint64_t)e->h_ctr[CTR_ACTIVE];
    if (e->h_ctr[CTR_MISSED]) {  // ensure_masks keeps this from happening
      tnp_set_error("plane %d: an edge's first split plane lies below the step (stale edge masks)", idx);
      return -1;
    }
    ktimer_set_bytes(e, "split", 1.0 * e->E + 13.0 * S + (e->pend_hoff >= 0 ? 5.0 * e->V : 0.0));
  }
  if (e->V + S >= (int64_t)INT32_MAX) {
    // slots (dead ones included: compaction is lazy) are int32 ids in sa/sb,
    // members, edges and the packed pair keys
    tnp_set_error("plane %d: %lld vertex slots + %lld splits exceed the int32 slot range", idx,
                  (long long)e->V, (long long)S);
    return -1;
  }
  return 0;
}

// 2. room for the S new vertices; curve branch: their split points
static int split_new_vertices(tnp_engine* e, const SplitStep& p, hipStream_t s) {
  const int64_t S = p.S;
  if (vset_ensure(e, e->cur, e->V + S, e->V, s)) return -1;
  const float* col = P<float>(e->cur.pre) + (int64_t)p.idx * e->cur.cap;  // may have moved
  if (e->curve)
    TIMED("new_vertices", 52.0 * S,
          launch_new_vertices(P<int32_t>(e->sa), P<int32_t>(e->sb), S, col, p.eps, P<float>(e->cur.xyz),
                              e->V, s));
  return 0;
}

// 3. the new vertices' forward and failover test (flat path: one kernel)
static int split_forward(tnp_engine* e, const SplitStep& p, hipStream_t s) {
  const int idx = p.idx;
  const int64_t S = p.S;
  e->pend_fused = !e->curve;
  if (e->pend_fused) {
    if (p.early_fwd)  // (launched behind the split; its modelled bytes now)
      ktimer_set_bytes(e, "forward_new",
                       (8.0 + 24.0 + 8.0 + 16.0 + 12.0 + 4.0 * (e->K - e->pend_keep) + 32.0) * S +
                           table_bytes(e->net));
    else if (flat_forward_new(e, idx, S, s))
      return -1;
  } else {
    if (buf_ensure(e->shared, S * sizeof(uint64_t) * e->kw, s)) return -1;
    if (buf_ensure(e->stage, (size_t)S * e->K * sizeof(float), s)) return -1;
    NetDev nf = e->net;
    if (p.ccoll) nf.sched_rows = p.Sg;
    TIMED("forward", (12.0 + 4.0 * e->K) * S,
          launch_forward(nf, P<float>(e->cur.xyz) + 3 * e->V, S, P<float>(e->stage), S, 1, s));
    // grid words of the new vertices (coordinates are final; the failover
    // test of a shard reads them: only owned vertices vote)
    if (launch_keys(e->net, P<float>(e->cur.xyz) + 3 * e->V, P<float>(e->stage), S, S, 0,
                    VP(e->cur, e->kw, e->V), VZ(e->cur, e->kw, e->V), P<uint64_t>(e->cur.grid) + e->V, s,
                    VP(e->cur, e->kw, e->V)))
      return -1;
    TIMED("fail_check", 48.0 * S,
          launch_fail_check(P<int32_t>(e->sa), P<int32_t>(e->sb), S, idx, VZ(e->cur, e->kw),
                            P<float>(e->stage), p.eps, P<uint64_t>(e->shared), P<int64_t>(e->ctr),
                            P<uint64_t>(e->cur.grid) + e->V, e->own, e->kw, s));
  }
  if (e->curve || e->shards > 1) {
    // the host takes the global override decision (all-reduce) / the curve
    // filter needs it: read it back
    if (read_ctr(e, s)) return -1;
    *p.fail = e->h_ctr[CTR_FAIL] ? 1 : 0;
  } else {
    *p.fail = -1;  // single device: the finish kernels read it in place
  }
  return 0;
}

// The stages in order, each followed by the collective its failure joins: on
// a sharded curve step (ccoll) a shard that fails between two collectives
// enters the next one with its failure flag (coll_fail), or its peers would
// block there.  Stages 1 and 2 join the next one-word TNP_COLL_SUM (the split
// count's, then curve_correct's first), stage 3 the strict flag's TNP_COLL_OR.
extern "C" int tnp_engine_split(tnp_engine* e, int idx, void* stream, int64_t* S_out, int32_t* fail) {
  hipStream_t s = (hipStream_t)stream;
  TNP_CHECK(hipSetDevice(e->device));
  e->rows_valid = false;
  if (idx < e->valid_from || idx >= e->K) {
    tnp_set_error("plane %d not cached (valid from %d)", idx, e->valid_from);
    return -1;
  }
  if (require_valid(e, "split")) return -1;
  e->valid = false;  // until this split has completed
  SplitStep p{idx, e->net.eps_s, 0, 0, false, e->curve && e->shards > 1, fail};
  const auto failed = [&](int op) { return p.ccoll ? coll_fail(e, 1, op) : -1; };
  e->pend_hits = false;
  if (split_edges(e, p, s)) return failed(TNP_COLL_SUM);
  *fail = 0;
  const int64_t S = p.S;
  p.Sg = S;
  if (p.ccoll && coll(e, &p.Sg, 1, TNP_COLL_SUM)) return -1;
  if (p.ccoll && fold32_sharded(e, p.Sg, "splits", idx)) return -1;
  if (p.ccoll && S == 0 && p.Sg > 0 && curve_correct(e, idx, 0, s)) return -1;
  if (S > 0) {
    if (split_new_vertices(e, p, s)) return failed(TNP_COLL_SUM);
    if (e->curve && curve_correct(e, idx, S, s)) return -1;
    if (split_forward(e, p, s)) return failed(TNP_COLL_OR);
  }
  e->pend_dup = S > 0 ? e->h_ctr[CTR_DUP] : 0;
  e->pend_tight = (S > 0 && e->curve) ? (int)e->h_ctr[CTR_TIGHT] : 0;
  if (p.ccoll && p.Sg > 0) {  // the strict filter's flag is the batch's (subpoly_debug.py:253-257)
    int64_t t = e->pend_tight;
    if (coll(e, &t, 1, TNP_COLL_OR)) return -1;
    e->pend_tight = t != 0;
  }
  *S_out = S;
  e->pend_idx = idx;
  e->pend_S = S;
  e->valid = true;
  return 0;
}

// what the phases of one tnp_engine_finish share (built by the driver)
struct FinishStep {
  int idx, prune, override_;
  int64_t V, E, S, NV;  // vertex slots, edge slots, kept splits, V + S
  int64_t E_live;       // live edges on entry
  // set by finish_members: members, the bounds of their cell entries and
  // pair cells, k_connect's chunk-table capacity
  int64_t M, TB, RC, bcap;
  int nb;               // bits of a vertex slot in a connecting-edge key
  BucketGeom bg;
  bool buckets, hits_done;
  int64_t hoff;
  // out: hit members, cell entries, kept connecting edges; the workgroup
  // parts of the in-stream part-A prune; the prune is the lazy one
  int64_t H, T, X;
  int part_a;
  bool lazy;
  // out (finish_prune): the state the driver commits
  int64_t V_out, E_out, E_live_out;
  int next_valid;
  bool defer;  // the live counts left to the next split (tnp_engine_run_steps)
};

// 1. override + keys of the new vertices (flat bucket path: the override
//    runs inside the bucket count, finish_buckets)
static int finish_new_keys(tnp_engine* e, const FinishStep& f, hipStream_t s) {
  if (e->pend_fused && f.buckets) return 0;
  const int64_t V = f.V, S = f.S;
  const int override_ = f.override_, K = e->K;
  VSet& c = e->cur;
  int64_t* ctr = P<int64_t>(e->ctr);
  uint64_t* pos = VP(c, e->kw);
  uint64_t* zero = VZ(c, e->kw);
  if (e->pend_fused) {
    TIMED("override_new", 8.0 * S,
          launch_override_new(S, override_, P<uint64_t>(e->shared), P<float>(c.pre), c.cap,
                              e->pend_keep, V, pos, zero, ctr, P<uint64_t>(c.pz), e->kw, s));
  } else {
    TIMED("finalize_new", (8.0 + 4.0 * K + 4.0 * (K - e->valid_from) + 16.0) * S,
          launch_finalize_new(S, K, override_, P<uint64_t>(e->shared), P<float>(e->stage), e->net.eps,
                              P<float>(c.pre), c.cap, e->valid_from, V, pos, zero, ctr,
                              P<uint64_t>(c.pz), e->kw, s));
  }
  return 0;
}

// 2. members = new vertices ++ live hit vertices (any order); the bucket
//    path reads the new vertices as slots V.. without a list.  Sets M, TB, RC
//    and bcap, and sizes the buffers of the members' cell entries
static int finish_members(tnp_engine* e, FinishStep& f, hipStream_t s) {
  const int64_t V = f.V, S = f.S, NV = f.NV;
  const bool hits_done = f.hits_done, buckets = f.buckets;
  const float* col = P<float>(e->cur.pre) + (int64_t)f.idx * e->cur.cap;
  int64_t* ctr = P<int64_t>(e->ctr);
  if (buf_ensure(e->members, std::max<int64_t>(NV, 1) * sizeof(int32_t), s, hits_done)) return -1;
  if (hits_done) {
    if (!buckets && launch_new_members(P<int32_t>(e->members), S, V, s)) return -1;
  } else {
    TIMED("hits", 5.0 * V + 4.0 * S,
          launch_hits(col, P<uint8_t>(e->live), V, e->net.eps_s, P<int32_t>(e->members), S, ctr, s));
  }
  if (e->net.n_marks + 2 > 1023) {  // connect packs cell coordinates in 10 bits each
    tnp_set_error("more than 1021 marks per axis");
    return -1;
  }
  // the live member count sizes the span pass and its scan (V counts every
  // slot, live or dead: sizing by it would scan ~V elements per step)
  if (!hits_done && read_ctr(e, s)) return -1;  // else: H came back with S
  const int64_t M = S + e->h_ctr[CTR_H];
  // a member spans <= 8 cells (2 per axis when on a mark plane): entry
  // buffers take the bound 8 M, so nothing waits for the entry count T
  const int64_t TB = std::max<int64_t>(8 * M, 1);
  const int64_t RC = TB / 2 + 1;  // a pair cell holds >= 2 entries
  f.M = M;
  f.TB = TB;
  f.RC = RC;
  if (buf_ensure(e->ents, TB * cell_ent_bytes(e->kw), s)) return -1;
  if (buf_ensure(e->pcell, RC * sizeof(int32_t), s)) return -1;
  if (buf_ensure(e->pent, RC * sizeof(int32_t), s)) return -1;
  if (buf_ensure(e->pcn, RC * sizeof(int32_t), s)) return -1;
  if (buf_ensure(e->ptoff, RC * sizeof(int64_t), s)) return -1;
  // k_connect's chunk table: its capacity is kept across steps (grown on
  // overflow and redone); the bucket path fills it in its pair-cell gather
  f.bcap = std::max<int64_t>(e->bcell.bytes / sizeof(int32_t), 4096);
  if (buf_ensure(e->bcell, f.bcap * sizeof(int32_t), s)) return -1;
  return 0;
}

// 3. bucket members by grid cell (dense cell grid over the marks): one
//    (cell, member) entry per spanned cell.
//    Spatial buckets, every count on the device (bucket.hip)
static int finish_buckets(tnp_engine* e, const FinishStep& f, hipStream_t s) {
  const int idx = f.idx, prune = f.prune, override_ = f.override_;
  const int64_t V = f.V, S = f.S, NV = f.NV, M = f.M, TB = f.TB, hoff = f.hoff;
  const BucketGeom& bg = f.bg;
  const int NB = bg.NB;
  VSet& c = e->cur;
  int64_t* ctr = P<int64_t>(e->ctr);
  uint64_t* pos = VP(c, e->kw);
  uint64_t* zero = VZ(c, e->kw);
  uint64_t* grid = P<uint64_t>(c.grid);
  void* const bk0 = e->bk[BK_CNT].p;
  void* const bk1 = e->bk[BK_CUR].p;
  if (buf_ensure(e->bk[BK_CNT], (NB + 1) * sizeof(int32_t), s)) return -1;  // counts (+1: read in pairs)
  if (buf_ensure(e->bk[BK_CUR], NB * sizeof(int32_t), s)) return -1;        // cursors
  if (e->bk[BK_CNT].p != bk0 || e->bk[BK_CUR].p != bk1) e->bk_clean = false;     // fresh memory
  if (buf_ensure(e->bk[BK_BASE], (NB + 1) * sizeof(int64_t), s)) return -1;  // bases
  // block parts: one per workgroup of the member passes (the grid is at least
  // FUSE_MAX_BLOCKS = 512 when the live-flag zeroing rides along)
  if (buf_ensure(e->bk[BK_PART], (std::max<int64_t>(bucket_member_blocks(M), 512) + 2) * sizeof(int64_t), s))
    return -1;
  if (buf_ensure(e->sents, TB * sizeof(uint64_t), s)) return -1;
  // a pruning step recomputes the live flags: zeroed by the bucket count
  // (after the hit pass read them), re-marked by the prune
  if (prune && buf_ensure(e->live, std::max<int64_t>(NV + 4, 16), s)) return -1;
  NewOverride nov{override_, P<uint64_t>(e->shared), P<float>(c.pre), c.cap, e->pend_keep, pos, zero,
                  P<uint64_t>(c.pz)};
  TIMED("bucket_entries", 16.0 * M,  // + 8 B per entry, set once T is known
        // (member m >= S is members[m]: the hits sit at hoff >= S when the split found them)
        launch_bucket_entries(P<int32_t>(e->members) + (hoff >= 0 ? hoff - S : 0), S, V, M, grid, zero, idx, bg,
                              P<int32_t>(e->bk[BK_CNT]), P<int32_t>(e->bk[BK_CUR]), P<int64_t>(e->bk[BK_BASE]),
                              P<int64_t>(e->bk[BK_PART]), P<uint64_t>(e->sents), e->bk_clean,
                              prune ? P<uint8_t>(e->live) : nullptr, NV, e->pend_fused ? &nov : nullptr,
                              ctr, s));
  e->bk_clean = false;  // until the grouping's pair-cell gather has reset the counters
  if (bg.sub) {
    // two-level geometry: the 16^3-cell buckets split into their 8^3-cell
    // octants (the grouping's buckets); the refine resets the counters
    if (buf_ensure(e->bk[BK_OBASE], ((int64_t)bg.NG + 1) * sizeof(int64_t), s)) return -1;
    if (buf_ensure(e->sents2, TB * sizeof(uint64_t), s)) return -1;
    TIMED("bucket_refine", 24.0 * M,  // 8 B read twice + 8 B written per entry (set once T is known)
          launch_bucket_refine(bg, P<int64_t>(e->bk[BK_BASE]), P<uint64_t>(e->sents), P<int64_t>(e->bk[BK_OBASE]),
                               P<uint64_t>(e->sents2), P<int32_t>(e->bk[BK_CNT]), P<int32_t>(e->bk[BK_CUR]), s));
  }
  return 0;
}

// 3. (fallback) the entries radix-sorted by cell: grids finer than the bucket
//    geometry, TNP_RADIX_CELLS=1
static int finish_radix_cells(tnp_engine* e, FinishStep& f, hipStream_t s) {
  const int idx = f.idx;
  const int64_t S = f.S, M = f.M, TB = f.TB;
  int64_t& H = f.H;
  int64_t& T = f.T;
  const int NC = e->net.n_marks + 2;
  const int64_t ncell = (int64_t)NC * NC * NC;
  VSet& c = e->cur;
  int64_t* ctr = P<int64_t>(e->ctr);
  uint64_t* zero = VZ(c, e->kw);
  uint64_t* grid = P<uint64_t>(c.grid);
  if (buf_ensure(e->spcnt, std::max<int64_t>(M, 1) * sizeof(int32_t), s)) return -1;
  if (buf_ensure(e->spoff, std::max<int64_t>(M, 1) * sizeof(int64_t), s)) return -1;
  if (buf_ensure(e->part, (int64_t)(tnp_grid(M) + 1) * sizeof(int64_t), s)) return -1;
  TIMED("span_count", 28.0 * M,
        launch_span_count(P<int32_t>(e->members), S, M, grid, zero, idx, P<int32_t>(e->spcnt),
                          P<int64_t>(e->part), ctr, e->kw, s));
  if (scan_counts(e, P<int32_t>(e->spcnt), P<int64_t>(e->spoff), M, CTR_T, s)) return -1;
  if (buf_ensure(e->ekey_a, TB * sizeof(uint32_t), s)) return -1;
  if (buf_ensure(e->ent_v, TB * sizeof(int32_t), s)) return -1;
  if (buf_ensure(e->ekey_b, TB * sizeof(uint32_t), s)) return -1;
  if (buf_ensure(e->eval_b, TB * sizeof(int32_t), s)) return -1;
  TIMED("span_emit", 28.0 * M,
        launch_span_emit(P<int32_t>(e->members), S, M, grid, NC, P<int64_t>(e->spoff),
                         P<uint32_t>(e->ekey_a), P<int32_t>(e->ent_v), ctr, s));
  if (read_ctr(e, s)) return -1;
  if (e->h_ctr[CTR_K0]) {
    // the reference builds torch.cartesian_prod() of zero tensors (subpoly.py:317)
    tnp_set_error("meshgrid expects a non-empty TensorList (a region row without zeros, plane %d)", idx);
    return -1;
  }
  H = e->h_ctr[CTR_H];
  T = e->h_ctr[CTR_T];
  const int64_t T1 = std::max<int64_t>(T, 1);
  ktimer_set_bytes(e, 20.0 * M + 8.0 * T);  // span_emit's bytes, known only now
  int cbits = 1;
  while (cbits < 32 && (1ll << cbits) < ncell) ++cbits;
  uint32_t* skey = nullptr;
  int32_t* sval = nullptr;
  {
    size_t need = sort_pairs_scratch_bytes(T, cbits);
    if (buf_ensure(e->sort_scr2, std::max<size_t>(need, 16), s)) return -1;
    TIMED("cell_sort", 16.0 * T * ((cbits + 7) / 8),
          sort_pairs_u32(P<uint32_t>(e->ekey_a), P<uint32_t>(e->ekey_b), P<int32_t>(e->ent_v),
                         P<int32_t>(e->eval_b), T, cbits, e->sort_scr2.p, e->sort_scr2.bytes, &skey,
                         &sval, s));
  }
  // cells holding member pairs straight from the runs of the sorted keys
  // (compacted, with their flattened pair space offsets; total = tests)
  {
    if (buf_ensure(e->rstart, (T1 + 1) * sizeof(int32_t), s)) return -1;
    if (T > 0) {
      TnpLB la, lr, lp;
      if (lb_begin(e, run_tiles(T), s, &la, 0)) return -1;
      TIMED("run_starts", 8.0 * T,
            launch_run_starts(skey, T, P<int32_t>(e->rstart), ctr, la, s));
      const int64_t pt = pair_run_tiles(T);
      if (lb_begin(e, pt, s, &lr, 0) || lb_begin(e, pt, s, &lp, 1)) return -1;
      TIMED("pair_cells", 0.0,
            launch_pair_runs(skey, P<int32_t>(e->rstart), T, P<int32_t>(e->pcell), P<int32_t>(e->pent),
                             P<int32_t>(e->pcn), P<int64_t>(e->ptoff), ctr, lr, lp, s));
    }
  }
  TIMED("entry_keys", 52.0 * T,
        launch_entry_keys(sval, skey, NC, T, grid, P<uint64_t>(c.pz), e->ents.p, e->kw, s));
  return 0;
}

// the counters one connect attempt published: the bucket path's entry
// errors and counts, the pair tests TT and the kept keys X
static int connect_counts(tnp_engine* e, FinishStep& f, int64_t* TT_out) {
  const int idx = f.idx;
  const int64_t M = f.M;
  const BucketGeom& bg = f.bg;
  int64_t& H = f.H;
  int64_t& T = f.T;
  int64_t& X = f.X;
  if (f.buckets) {
    int sp0[3], sp1[3];
    span_of(e, sp0, sp1);
    // the atomically allocated pair-cell list: cells | pairs << 24
    e->h_ctr[CTR_R] = e->h_ctr[CTR_PCK] & (PCK_CELLS - 1);
    e->h_ctr[CTR_TESTS] = e->h_ctr[CTR_PCK] >> 24;
    if (e->h_ctr[CTR_K0] & 2) {
      tnp_set_error("plane %d: a vertex outside the mark planes [%d, %d] x [%d, %d] x [%d, %d] the engine "
                    "was given (tnp_engine_set_span)", idx, sp0[0], sp1[0], sp0[1], sp1[1], sp0[2], sp1[2]);
      return -1;
    }
    if (e->h_ctr[CTR_K0]) {
      // the reference builds torch.cartesian_prod() of zero tensors (subpoly.py:317)
      tnp_set_error("meshgrid expects a non-empty TensorList (a region row without zeros, plane %d)",
                    idx);
      return -1;
    }
    H = e->h_ctr[CTR_H];
    T = e->h_ctr[CTR_T];
    // entries: written once by the scatter; the grouping reads them, gathers
    // 16 B of member keys and writes the 32 B record; the window pass reads
    // every record (once, algorithmically) and writes the kept keys
    ktimer_set_bytes(e, "bucket_entries", 16.0 * M + 8.0 * T);
    if (bg.sub) ktimer_set_bytes(e, "bucket_refine", 24.0 * T);
    // the window pass re-reads the records the same workgroup just wrote
    // (cache traffic): its compulsory bytes are the kept keys.  LDS-record
    // path: 8 B entry word + 16 B member keys + 4 + 4 B cell order (written,
    // read back) per entry, records in memory only for k_connect's cells
    // (not counted: an understatement)
    ktimer_set_bytes(e, "bucket_group", (e->lds_records ? 32.0 : 56.0) * T + 8.0 * e->h_ctr[CTR_XK]);
  }
  const int64_t TT = e->h_ctr[CTR_TESTS];
  X = e->h_ctr[CTR_XK];
  ktimer_set_bytes(e, 32.0 * TT + 8.0 * T);  // known only now
  if (e->h_ctr[CTR_BIG] || TT > e->max_pair_tests) {
    // one linear region holding ~sqrt(2*tests) vertices: the reference would
    // materialise every in-region pair (subpoly.py:505-518) and run out of
    // memory long before; refuse instead of grinding for hours
    tnp_set_error("degenerate complex at plane %d: %lld in-cell vertex pairs exceed the limit %lld "
                  "(TNP_MAX_PAIR_TESTS)", idx, (long long)TT, (long long)e->max_pair_tests);
    return -1;
  }
  *TT_out = TT;
  return 0;
}

// 4. connecting edges: test every in-cell member pair once, append the
//    emitted ones, radix-sort them (lexicographic c_new, subpoly.py:243-244).
//    The pair count stays on the device; the chunk table and the key buffer
//    keep their capacity across steps and grow (then redo) on overflow.
static int finish_connect(tnp_engine* e, FinishStep& f, hipStream_t s) {
  const int idx = f.idx, prune = f.prune, nb = f.nb, K = e->K;
  const int64_t V = f.V, E = f.E, S = f.S, NV = f.NV, M = f.M, TB = f.TB, RC = f.RC;
  const BucketGeom& bg = f.bg;
  const bool buckets = f.buckets;
  const int NC = e->net.n_marks + 2;
  int64_t bcap = f.bcap;
  int64_t& X = f.X;
  VSet& c = e->cur;
  int64_t* ctr = P<int64_t>(e->ctr);
  // connecting edges this step's pruning drops are never appended (sorted,
  // re-tested): keep_edge() depends on the endpoints only
  const uint64_t cfmask = prune ? prune_mask(idx, K - 1) : 0ull;
  // the kept keys go to XS_N per-XCD regions of cap / XS_N keys (step.h) on
  // grids of many bucket workgroups; small grids count in ctr directly
  const int NG = buckets ? bg.NG : 0;  // grouping workgroups
  const bool shard = !buckets || NG > 512;
  if (shard && buf_ensure(e->xs, XS_WORDS * sizeof(int64_t), s)) return -1;
  int64_t* const xs = shard ? P<int64_t>(e->xs) : nullptr;
  // small bucket grids: per-bucket statistics rows (plain stores) that the
  // connect kernel sums, instead of counter-block atomics from every bucket
  if (buckets && !shard && buf_ensure(e->bk[BK_STAT], (int64_t)NG * 4 * sizeof(int64_t), s)) return -1;
  int64_t* const bstat = (buckets && !shard) ? P<int64_t>(e->bk[BK_STAT]) : nullptr;
  int64_t cap = connect_key_cap(e->ckeys_a.bytes, M, XS_N);
  int64_t TT = 0;
  bool chunks_ok = false;  // (radix path) the chunk table matches the pair cells
  // lazy edge deletion (k_prune_lazy) unless the list is mostly dead edges
  // already: then the compacting prune drops them (and this step's)
  // (split-eps mode: always lazy -- its first split planes are recomputed
  // over the edge slots in place, k_ef_cache)
  const bool lazy = prune && (eps2(e) || (E - f.E_live) <= f.E_live);
  // the lazy prune's old edges and e_new need no connecting edge: they are
  // pruned while the connect counts travel to the host (slots [0, E + S)),
  // c_new after the sort (part A's workgroup parts first in lzpart)
  const bool early_prune = lazy && buckets && e->early_forward && !eps2(e) && !e->curve && e->masks_valid;
  int part_a = 0;
  const int64_t ES = E + S;
  // part A (slots [0, E + S)) reads the edge slots, their bytes, the keys of
  // the new vertices (forward_new; their override came with the bucket
  // count) and writes the slots' bytes, e_new and the live flags the bucket
  // count zeroed -- nothing the grouping, the connect, the key sort or their
  // counters touch.  So it is enqueued behind the connect's counter publish
  // and runs while the counts travel to the host
  if (early_prune) {
    if (buf_ensure(e->live, std::max<int64_t>(NV + 4, 16), s)) return -1;  // (+4: word atomics)
    if (buf_ensure(e->edges, std::max<int64_t>(ES, 1) * 2 * sizeof(int32_t), s, true)) return -1;
    if (buf_ensure(e->edm, std::max<int64_t>(ES, 1) * sizeof(uint8_t), s, true)) return -1;
    if (buf_ensure(e->eef, std::max<int64_t>(ES, 1) * sizeof(uint8_t), s, true)) return -1;
    part_a = prune_lazy_blocks(ES);
    if (buf_ensure(e->lzpart, part_a * sizeof(int64_t), s)) return -1;
  }
  for (int attempt = 0; attempt < 3; ++attempt) {
    if (buf_ensure(e->ckeys_a, std::max<int64_t>(cap, 1) * sizeof(uint64_t), s)) return -1;
    if (attempt > 0) {  // the split zeroed the whole counter block
      TNP_CHECK(hipMemsetAsync(ctr + CTR_X, 0, sizeof(int64_t), s));
      TNP_CHECK(hipMemsetAsync(ctr + CTR_XK, 0, sizeof(int64_t), s));
      TNP_CHECK(hipMemsetAsync(ctr + CTR_P, 0, 2 * sizeof(int64_t), s));  // CTR_P, CTR_COMPAT
      TNP_CHECK(hipMemsetAsync(ctr + CTR_BOVF, 0, sizeof(int64_t), s));
      TNP_CHECK(hipMemsetAsync(ctr + CTR_PCK, 0, sizeof(int64_t), s));
      TNP_CHECK(hipMemsetAsync(ctr + CTR_SPAIRS, 0, sizeof(int64_t), s));
    }
    // the shards are left zero by k_keys_finish; cleared here after an
    // aborted step or on fresh memory
    if (shard && !e->xs_clean) TNP_CHECK(hipMemsetAsync(e->xs.p, 0, XS_WORDS * sizeof(int64_t), s));
    if (shard) e->xs_clean = false;
    if (buckets) {
      // in-bucket grouping + the window pass over each bucket (cells of <=
      // WCELL members) + pair-cell lists and k_connect's chunk table (bcap)
      if (buf_ensure(e->bcell, bcap * sizeof(int32_t), s)) return -1;
      const ConnectWin cw{idx, nb, cfmask, P<uint64_t>(e->ckeys_a), cap, xs, bstat,
                          packed_ok(idx, K) ? 1 : 0};
      // the LDS-record path's cell-order scratch (TNP_LDS_RECORDS=0: off)
      const bool lrec = e->lds_records;
      if (lrec && buf_ensure(e->bk[BK_EWORD], TB * sizeof(uint64_t), s)) return -1;  // (entry words)
      TIMED("bucket_group", 0.0,
            launch_bucket_pairs(bg, P<int64_t>(e->bk[bg.sub ? BK_OBASE : BK_BASE]), P<uint64_t>(bg.sub ? e->sents2 : e->sents),
                                P<uint64_t>(c.pz), P<CellEnt>(e->ents), P<int32_t>(e->pcell),
                                P<int32_t>(e->pent), P<int32_t>(e->pcn), P<int64_t>(e->ptoff),
                                P<int32_t>(e->bcell), bcap, P<int32_t>(e->bk[BK_CNT]), P<int32_t>(e->bk[BK_CUR]),
                                cw, lrec ? P<uint64_t>(e->bk[BK_EWORD]) : nullptr, ctr, s));
      e->bk_clean = true;
    } else if (!chunks_ok) {
      if (buf_ensure(e->bcell, bcap * sizeof(int32_t), s)) return -1;
      if (launch_chunk_cells(P<int64_t>(e->ptoff), P<int32_t>(e->pcn), RC,
                             P<int32_t>(e->bcell), bcap, ctr, s)) return -1;
    }
    // cells above WCELL members: the flattened pair space (every cell on the
    // radix path); the others: the window pass
    TIMED("connect", 0.0,
          launch_connect(P<int64_t>(e->ptoff), P<int32_t>(e->pcell), P<int32_t>(e->pcn),
                         P<int32_t>(e->pent), NC, e->max_pair_tests, P<int32_t>(e->bcell),
                         e->ents.p, idx, nb, prune ? K - 1 : -1, e->kw, P<uint64_t>(e->ckeys_a), cap, xs, ctr, s,
                         bstat, NG));
    if (shard) {
      if (launch_keys_finish(xs, cap, ctr, s)) return -1;
      e->xs_clean = true;
    }
    int64_t seq = 0;
    if (post_ctr(e, s, &seq)) return -1;
    if (early_prune && attempt == 0) {  // (a redone connect leaves part A as it is)
      TIMED("prune", 1.0 * E + 36.0 * S,
            launch_prune_lazy(P<int32_t>(e->edges), E, P<int32_t>(e->sb), S, V, nullptr, nb, 0, idx, K - 1,
                              P<uint64_t>(c.pz), P<uint8_t>(e->edm), P<uint8_t>(e->eef), P<uint8_t>(e->live),
                              P<int64_t>(e->lzpart), ctr, s, 0, ES));
    }
    if (wait_ctr(e, s, seq)) return -1;
    if (connect_counts(e, f, &TT)) return -1;
    if (e->h_ctr[CTR_BOVF]) {  // chunk table too small: grow, remap, redo
      bcap = connect_chunks(TT) + 1;
      chunks_ok = false;
      continue;
    }
    chunks_ok = true;
    if (X <= cap) break;
    cap = (X + XS_N - 1) / XS_N * XS_N;  // appended beyond the buffer: grow and redo
  }
  if (e->h_ctr[CTR_BOVF] || X > cap) { tnp_set_error("connect: capacity retry failed"); return -1; }
  if (e->h_ctr[CTR_COMPAT] == 0 && e->shards <= 1) {
    // every region has a single member: extract_every_valid_edge cats an
    // empty list (subpoly.py:505-513)
    tnp_set_error("torch.cat(): expected a non-empty list of Tensors (no region with two vertices, plane %d)", idx);
    return -1;
  }
  if (buf_ensure(e->ckeys_b, std::max<int64_t>(X, 1) * sizeof(uint64_t), s)) return -1;
  // sharded: the regions concatenated (a, per-XCD -> b), then sorted (b <-> a)
  uint64_t* kin = P<uint64_t>(e->ckeys_a);
  uint64_t* kalt = P<uint64_t>(e->ckeys_b);
  if (shard) {
    TIMED("keys_compact", 16.0 * X, launch_keys_compact(kin, cap, xs, X, kalt, s));
    std::swap(kin, kalt);
  }
  {
    size_t need = sort_lex_scratch_bytes(X, nb, e->sort_run);
    if (buf_ensure(e->sort_scr, std::max<size_t>(need, 16), s)) return -1;
    TIMED("pair_sort", 16.0 * X * ((2 * nb + 7) / 8),
          sort_keys_lex(kin, kalt, X, nb, e->sort_run, e->sort_scr.p, e->sort_scr.bytes, &e->ckeys, s));
  }
  f.part_a = part_a;
  f.lazy = lazy;
  return 0;
}

// 5. pruning over [edges; e_new; c_new] + vertex compaction: the lazy prune
//    (what part A left of it), the compacting prune, the last plane's
//    compaction behind lazily deleted edges, or the plain concatenation
static int finish_prune(tnp_engine* e, FinishStep& f, hipStream_t s) {
  const int idx = f.idx, prune = f.prune, nb = f.nb, part_a = f.part_a, K = e->K;
  const int64_t V = f.V, E = f.E, S = f.S, NV = f.NV, X = f.X, E_live_in = f.E_live;
  const bool buckets = f.buckets, lazy = f.lazy;
  VSet& c = e->cur;
  int64_t* ctr = P<int64_t>(e->ctr);
  uint64_t* pos = VP(c, e->kw);
  uint64_t* zero = VZ(c, e->kw);
  const int64_t N = E + S + X;
  int64_t nt = step_tiles(N);
  if (buf_ensure(e->blk, (nt + 1) * sizeof(int32_t), s)) return -1;
  if (buf_ensure(e->blkoff, (nt + 1) * sizeof(int64_t), s)) return -1;
  // ctr[CTR_ACTIVE] and ctr[CTR_V] are still zero from the split's reset
  const int32_t* eg = P<int32_t>(e->edges);
  int64_t V2 = NV, E2 = N, E2_live = N;
  bool defer = false;  // the live counts left to the next split (tnp_engine_run_steps)
  int next_valid = e->valid_from;
  bool swap_edges = true;
  if (prune) {
    // live flags recomputed from the kept edges; no vertex moves (lazy
    // compaction): the distinct flagged count is the reference's V'
    if (buf_ensure(e->live, std::max<int64_t>(NV + 4, 16), s)) return -1;  // +4: word atomics
    if (!buckets) TNP_CHECK(hipMemsetAsync(e->live.p, 0, NV, s));  // else zeroed by the bucket count
    // (word-atomic live counting inside the prune measured slower than the
    // counting pass even at bunny scale: 0.25 vs 0.13 + 0.07 ms per subpoly,
    // and was removed)
    // the run loop leaves the live counts to the next split's hit workers
    // (not in the kernel-timer pass: the prune's modelled bytes want them)
    BucketGeom bgd{};
    defer = e->defer_counts && !e->kt_on && !e->curve && !eps2(e) && uses_buckets(e, &bgd);
    // (curve path: recomputed after the rewiring, first split planes above idx)
    if (!e->masks_valid && compute_masks(e, idx + 1, nullptr, s)) return -1;
    const int64_t N1 = std::max<int64_t>(N, 1);
    if (lazy) {
      // in place: the slots grow to N (kept contents), nothing is compacted
      if (buf_ensure(e->edges, N1 * 2 * sizeof(int32_t), s, true)) return -1;
      if (buf_ensure(e->edm, N1 * sizeof(uint8_t), s, true)) return -1;
      if (buf_ensure(e->eef, N1 * sizeof(uint8_t), s, true)) return -1;
      // old edges: 1 B high plane (+ 1 B first split plane, 8 B ids when
      // kept); e_new / c_new: 4 / 8 B ids + 32 B endpoint keys, 10 B written
      // (part_a > 0: the old edges and e_new were pruned behind the connect)
      const int64_t i0 = part_a ? E + S : 0;
      const int nparts = part_a + prune_lazy_blocks(N - i0);
      if (buf_ensure(e->lzpart, nparts * sizeof(int64_t), s, part_a > 0)) return -1;
      TIMED("prune", part_a ? 40.0 * X : 1.0 * E + 36.0 * S + 40.0 * X,
            launch_prune_lazy(P<int32_t>(e->edges), E, P<int32_t>(e->sb), S, V, e->ckeys, nb, X, idx, K - 1,
                              P<uint64_t>(c.pz), P<uint8_t>(e->edm), P<uint8_t>(e->eef), P<uint8_t>(e->live),
                              P<int64_t>(e->lzpart) + part_a, ctr, s, i0, N));
      if (eps2(e)) {  // the first split planes at subpoly's eps, and their OR
        TNP_CHECK(hipMemsetAsync(ctr + CTR_ACTIVE, 0, sizeof(int64_t), s));
        TIMED("edge_masks", 8.0 * N,
              launch_ef_cache(P<int32_t>(e->edges), N, P<uint8_t>(e->edm), P<uint8_t>(e->eef), P<float>(c.pre),
                              c.cap, idx + 1, K, e->net.eps_s, ctr, s));
      }
      if (defer)
        e->pend_lz_n = nparts;
      else
        TIMED("count_live", 1.0 * NV,
              launch_count_flags(P<uint8_t>(e->live), NV, ctr, CTR_V, s, P<int64_t>(e->lzpart), nparts, CTR_E));
      swap_edges = false;
    } else {
      if (buf_ensure(e->edges_alt, N1 * 2 * sizeof(int32_t), s)) return -1;
      if (buf_ensure(e->edm_alt, N1 * sizeof(uint8_t), s)) return -1;
      if (buf_ensure(e->eef_alt, N1 * sizeof(uint8_t), s)) return -1;
      TnpLB lb;
      if (lb_begin(e, lb_tiles(N), s, &lb, 0, false)) return -1;
      // old edges: 8 B ids + 1 B high plane + 1 B first split plane read; e_new /
      // c_new: 4 / 8 B ids + 32 B endpoint keys; kept edges: 10 B written + 2 B flags
      TIMED("prune", 10.0 * E + 36.0 * S + 40.0 * X,
            launch_prune_lb(eg, E, P<int32_t>(e->sb), S, V, e->ckeys, nb, X, idx, K - 1,
                            P<uint64_t>(c.pz), P<uint8_t>(e->edm), P<uint8_t>(e->eef),
                            P<int32_t>(e->edges_alt), P<uint8_t>(e->edm_alt), P<uint8_t>(e->eef_alt),
                            P<uint8_t>(e->live), ctr, lb, s));
      std::swap(e->edm, e->edm_alt);
      std::swap(e->eef, e->eef_alt);
      if (defer)
        e->pend_lz_n = 0;  // (E_live: the compacting prune's own count, read back below)
      else
        TIMED("count_live", 1.0 * NV, launch_count_flags(P<uint8_t>(e->live), NV, ctr, CTR_V, s));
    }
    next_valid = (e->keep_all || eps2(e)) ? 0 : std::min(idx + 1, K - 1);
    if (read_ctr(e, s, nullptr, 0, nullptr, 0, e->in_run)) return -1;
    E2_live = (defer && lazy) ? E_live_in : e->h_ctr[CTR_E];  // (deferred: set by apply_counts)
    E2 = lazy ? N : E2_live;
    ktimer_set_bytes(e, "prune", lazy ? 1.0 * E + 36.0 * S + 40.0 * X + 9.0 * E2_live
                                      : 10.0 * E + 36.0 * S + 40.0 * X + 12.0 * E2_live);
    V2 = e->h_ctr[CTR_V];
    // the kept edges' first split planes are above idx now
    e->mask_from = idx + 1;
    e->act_bits = (uint64_t)e->h_ctr[CTR_ACTIVE];
    e->dirty = true;
  } else if (E != E_live_in) {
    // the last plane (no pruning) behind lazily deleted edges: the
    // concatenation drops them (the compacting prune keeping every live edge)
    const int64_t N1 = std::max<int64_t>(N, 1);
    if (buf_ensure(e->edges_alt, N1 * 2 * sizeof(int32_t), s)) return -1;
    if (buf_ensure(e->edm_alt, N1 * sizeof(uint8_t), s)) return -1;
    if (buf_ensure(e->eef_alt, N1 * sizeof(uint8_t), s)) return -1;
    // (the live flags grow to the new slots first: the pass marks endpoints)
    if (set_alive(e, V, S, s)) return -1;
    TnpLB lb;
    if (lb_begin(e, lb_tiles(N), s, &lb, 0, false)) return -1;
    if (launch_prune_lb(eg, E, P<int32_t>(e->sb), S, V, e->ckeys, nb, X, -1, K - 1, P<uint64_t>(c.pz),
                        P<uint8_t>(e->edm), P<uint8_t>(e->eef), P<int32_t>(e->edges_alt),
                        P<uint8_t>(e->edm_alt), P<uint8_t>(e->eef_alt), P<uint8_t>(e->live), ctr, lb, s))
      return -1;
    std::swap(e->edm, e->edm_alt);
    std::swap(e->eef, e->eef_alt);
    V2 = e->V_live + S;
    e->masks_valid = false;
    if (read_ctr(e, s)) return -1;
    E2 = E2_live = e->h_ctr[CTR_E];
  } else {
    if (buf_ensure(e->edges_alt, std::max<int64_t>(N, 1) * 2 * sizeof(int32_t), s)) return -1;
    if (launch_prune(true, eg, E, P<int32_t>(e->sb), S, V, e->ckeys, nb, X, idx, 0, K - 1, pos, zero, nullptr, nullptr,
                     P<int32_t>(e->edges_alt), nullptr, ctr, s))
      return -1;
    if (set_alive(e, V, S, s)) return -1;
    V2 = e->V_live + S;
    e->masks_valid = false;  // the concatenated edge list carries no masks
    if (read_ctr(e, s)) return -1;
  }
  if (swap_edges) std::swap(e->edges, e->edges_alt);
  f.V_out = V2;
  f.E_out = E2;
  f.E_live_out = E2_live;
  f.next_valid = next_valid;
  f.defer = defer;
  return 0;
}

extern "C" int tnp_engine_finish(tnp_engine* e, int idx, int prune, int override_, void* stream,
                                 tnp_step_stats* st) {
  hipStream_t s = (hipStream_t)stream;
  e->rows_valid = false;
  TNP_CHECK(hipSetDevice(e->device));
  if (e->pend_idx != idx) { tnp_set_error("finish(%d) without split(%d)", idx, idx); return -1; }
  if (require_valid(e, "finish")) return -1;
  if (e->cnt_pending) {  // (the split resolves them; a finish never sees them pending)
    tnp_set_error("finish(%d): live counts of the last step still pending", idx);
    return -1;
  }
  e->pend_idx = -1;
  e->valid = false;  // until this step has completed
  FinishStep f{};
  f.idx = idx;
  f.prune = prune;
  f.override_ = override_;
  f.hits_done = e->pend_hits;
  f.hoff = f.hits_done ? e->pend_hoff : -1;
  e->pend_hits = false;
  int64_t S_kept = e->pend_S;
  if (e->curve) {
    if (curve_filter(e, idx, override_, s, &S_kept)) return -1;
    e->masks_valid = false;  // the filter rewired the kept split edges
    // the kept splits another shard owns (read back with the connect
    // counters; the split's CTR_DUP count is the flat path's)
    TNP_CHECK(hipMemsetAsync(P<int64_t>(e->ctr) + CTR_DUP, 0, sizeof(int64_t), s));
    if (launch_count_unowned(P<uint64_t>(e->cur.grid) + e->V, S_kept, e->own, P<int64_t>(e->ctr), s))
      return -1;
  }
  f.V = e->V;
  f.E = e->E;
  f.S = S_kept;
  f.NV = f.V + f.S;
  f.E_live = e->E_live;
  f.buckets = uses_buckets(e, &f.bg);
  f.nb = 1;
  while (f.nb < 31 && (1ll << f.nb) < f.NV) ++f.nb;
  if (finish_new_keys(e, f, s) || finish_members(e, f, s)) return -1;
  if (f.buckets ? finish_buckets(e, f, s) : finish_radix_cells(e, f, s)) return -1;
  if (finish_connect(e, f, s) || finish_prune(e, f, s)) return -1;
  // the new vertices hold planes >= pend_keep only: valid_from never claims
  // the planes below (a step order that could read them needs keep_all)
  if (e->pend_fused) f.next_valid = std::max(f.next_valid, e->pend_keep);
  const int64_t V_in_live = e->V_live;
  e->V = f.NV;  // slots
  e->V_live = f.V_out;
  e->E = f.E_out;
  e->E_live = f.E_live_out;
  e->valid_from = f.next_valid;
  if (f.defer) {  // V_live (and the lazy prune's E_live) arrive with the next split
    e->cnt_pending = true;
    e->pend_st = st;
  }
  if (st) {
    st->idx = idx;
    st->V_in = V_in_live;
    st->E_in = f.E_live;
    st->S = f.S;
    st->H = f.H;
    st->X = e->h_ctr[CTR_X];  // all connecting edges (X kept ones were appended)
    st->V_out = f.V_out;
    st->E_out = f.E_live_out;
    st->A = e->h_ctr[CTR_A];
    st->P = e->h_ctr[CTR_P];
    st->pair_tests = (e->h_ctr[CTR_PCK] ? (e->h_ctr[CTR_PCK] >> 24) : e->h_ctr[CTR_TESTS]) + e->h_ctr[CTR_SPAIRS];
    st->override_applied = override_ < 0 ? (e->h_ctr[CTR_FAIL] != 0) : override_;
    st->next_active = (uint64_t)e->h_ctr[CTR_ACTIVE];
    st->S_dup = e->curve ? e->h_ctr[CTR_DUP] : e->pend_dup;
    st->T = f.T;
  }
  e->valid = true;
  return 0;
}

// the hyperplane loop of subpoly.py:58-69 on one device, in the library:
// the same split / finish calls the Python driver makes per step, without a
// host-language round trip per step (bunny-scale steps are tens of us)
extern "C" int tnp_engine_run_steps(tnp_engine* e, void* stream, tnp_step_stats* stats, int max_stats,
                                    int* n_steps) {
  *n_steps = 0;
  e->rows_valid = false;
  if (e->shards > 1) {
    tnp_set_error("run_steps: a sharded engine takes its global decisions between split and finish");
    return -1;
  }
  uint64_t mask = 0;
  if (tnp_engine_active_planes(e, 0, &mask, stream)) return -1;
  const int K = e->K;
  // a pruning step's live counts are taken by the next split (deferred);
  // every exit path below resolves the last ones
  tnp_step_stats spare{};
  auto done = [&](int rc) -> int {
    e->in_run = false;
    e->ctr_zero = false;
    e->defer_counts = false;
    if (resolve_counts(e, (hipStream_t)stream)) rc = -1;
    e->pend_st = nullptr;
    return rc;
  };
  e->defer_counts = true;
  e->in_run = true;
  e->ctr_zero = false;
  for (int idx = 0; idx < K; ++idx) {
    if (!tnp::act_test(mask, idx)) continue;
    int64_t S = 0;
    int32_t fail = 0;
    if (tnp_engine_split(e, idx, stream, &S, &fail)) return done(-1);
    if (S == 0) continue;
    const int prune = idx < K - 1;  // the last plane never prunes
    tnp_step_stats* st = *n_steps < max_stats ? &stats[*n_steps] : &spare;
    *st = tnp_step_stats{};
    if (tnp_engine_finish(e, idx, prune, fail, stream, st)) return done(-1);
    ++*n_steps;
    // (planes >= 63 share bit 63: after such a step only the next-active word counts)
    if (prune) mask = idx >= 62 ? ((mask & ((1ull << 63) - 1ull)) | st->next_active)
                                : ((mask & ((2ull << idx) - 1ull)) | st->next_active);
  }
  return done(0);
}
