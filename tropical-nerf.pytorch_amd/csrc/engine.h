// What the host files of the extraction engine share (engine.cpp and the
// engine_*.cpp pieces): the buffer types, the engine's state and the helpers
// that more than one piece calls.  Internal, not installed.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/tropical_hip.h"
#include "../../include/tropical_hip_debug.h"
#include "common.h"
#include "kernels.h"
#include "step.h"

// ---------------------------------------------------------------------------
// buffers
// ---------------------------------------------------------------------------
struct Buf {
  void* p = nullptr;
  size_t bytes = 0;
};

template <typename T>
static T* P(Buf& b) { return static_cast<T*>(b.p); }

struct VSet {
  Buf xyz, pre, grid;
  // the vertex keys, (pos, zero) interleaved: 2 kw words per vertex, one
  // gather for both; the kernels' pos / zero arrays are views of it (VP / VZ,
  // common.h vkey_load)
  Buf pz;
  int64_t cap = 0;  // rows; pre leading dimension == cap
  int K = 0;        // planes the pre buffer holds (the engine is reused across nets)
};
// the pos / zero key views of a vertex set from vertex `from` on
static uint64_t* VP(VSet& v, int kw, int64_t from = 0) { return static_cast<uint64_t*>(v.pz.p) + 2 * kw * from; }
static uint64_t* VZ(VSet& v, int kw, int64_t from = 0) { return VP(v, kw, from) + kw; }

struct KRec {
  const char* name;
  double bytes;
  hipEvent_t a, b;
};

// curve-path scratch (force=False branch, curve.hip)
enum {
  CV_EIDX, CV_CFLAG, CV_COFF, CV_CROW, CV_CORNERS, CV_PLANE, CV_STAGE_C, CV_INTS, CV_INTS0, CV_PTS,
  CV_STAGE_P, CV_D0, CV_D1, CV_GG, CV_GD, CV_GOFF, CV_GLIST, CV_CONV, CV_CINFO, CV_KEEP, CV_NID,
  CV_SA2, CV_SB2, CV_SHARED2, CV_STAGE2, CV_XYZ2, CV_GRID2, CV_N
};

// bucket.hip scratch: per-bucket counts (+1: read in pairs), cursors and
// bases; small grids' per-bucket statistics rows; the LDS-record path's entry
// words; the member passes' workgroup parts; the octants' bases (two-level
// geometries)
enum { BK_CNT, BK_CUR, BK_BASE, BK_STAT, BK_EWORD, BK_PART, BK_OBASE, BK_N };

struct tnp_engine {
  int device = 0;
  OwnBox own{{1, 1, 1}, {0, 0, 0}};  // owned box of a shard (common.h); uncut axes: all
  // mark planes the complex lies within, per axis (the spatial buckets cover
  // only those cells); sp_hi[d] < sp_lo[d]: the whole axis
  int sp_lo[3] = {0, 0, 0}, sp_hi[3] = {-1, -1, -1};
  int curve = 0;          // 1: subpoly_(force=False) semantics
  int strict = 1;         // curve path: subpoly_(strict=...) -- 0 keeps every split (subpoly.py:198-202)
  int shards = 1;         // >1: one x-slab of a sharded complex
  int pend_tight = 0;
  tnp_collective_fn coll_fn = nullptr;  // a sharded step's in-step decisions (tnp_engine_set_collective)
  void* coll_ctx = nullptr;
  bool coll_err = false;  // this shard failed: the next collective says so (coll_fail)
  int gd_iters = 500;     // subpoly_debug.py:141
  int64_t max_pair_tests = 20000000000LL;
  bool kt_on = false;
  std::vector<KRec> kt;
  std::vector<std::string> kt_names;
  std::vector<double> kt_ms, kt_bytes;
  std::vector<int64_t> kt_n;
  NetDev net{};
  int K = 0;
  int kw = 1;  // sign-key words per vertex key (net_kw: 2 when K > 63)
  bool has_net = false;
  VSet cur, alt;
  Buf edges, edges_alt;
  // per-edge key bytes (step.hip k_prune_lb): dm = 1 + the highest plane on
  // which the endpoint keys differ, ef = the first plane >= mask_from that
  // splits the edge (EDGE_NOSPLIT: none); valid when masks_valid
  Buf edm, eef, edm_alt, eef_alt;
  Buf lzpart;  // the lazy prune's per-workgroup kept counts
  Buf kse_pz, kse_grid;  // split-eps faces: (pos, zero) / grid keys at subpoly's eps
  Buf xs;                // per-XCD shards of the connect phase (step.h XS_*)
  bool xs_clean = false;
  bool masks_valid = false;
  int mask_from = 0;       // plane the stored first split planes start at
  uint64_t act_bits = 0;   // OR of the edges' first split planes (bit p: plane p splits an edge)
  int64_t V = 0, E = 0;
  // E counts edge SLOTS: the pruning deletes lazily (EDGE_DEAD bytes, edges
  // keep their slots) and compacts only when most slots are dead or before
  // an export; E_live is the reference's edge count
  int64_t E_live = 0;
  int keep_all = 0;
  int valid_from = 0;  // pre planes [valid_from, K) are valid for every vertex
  int pend_keep = 0;   // the pending flat step's new vertices get planes [pend_keep, K) (new_keep_from)
  // Lazy compaction: during the hot loop vertex ids are SLOTS (V = slots in
  // use); pruned vertices stay in place, flagged dead in `used` (the live
  // flags).  Slot order == the reference's compacted id order (compaction
  // preserves ascending ids), so every id-ordered result is unchanged;
  // compact_now() renumbers once, before anything exports or reads ids.
  bool dirty = false;
  // a complex is loaded and consistent: a failed split / finish (an error
  // the reference raises mid-step, or a device failure) leaves the edges and
  // live flags half-updated, so the engine refuses to go on until a complex
  // is loaded again (tnp_engine_load / lattice / skeleton)
  bool valid = false;
  int64_t V_live = 0;
  Buf live;  // live-slot flags (uint8) of the lazily compacted vertex set
  // deferred live counts (tnp_engine_run_steps): a pruning step leaves
  // V_live (and, lazy prune, E_live) to the next split, whose hit workers read
  // every live flag anyway (HitArgs::hpart) and whose readback sums them
  // with the lazy prune's per-workgroup kept counts -- no count_live launch
  bool defer_counts = false;  // set by the run loop only
  bool cnt_pending = false;
  bool early_forward = true;          // TNP_EARLY_FWD=0: k_forward_new after S is read back (A/B)
  // the early k_forward_new's row bound (early_bound): the largest split
  // count this engine has seen, not the edge-slot count E -- E counts the
  // lazily deleted slots too (up to ~2x the live edges), and the vertex set
  // and the shared-plane words keep whatever capacity the bound asks for
  int64_t max_split_seen = 0;
  int64_t n_early_redo = 0;  // steps whose S exceeded the early bound (forward run again)
  bool early_bound_splits = true;  // TNP_EARLY_BOUND=0 at creation: the edge-slot bound E (round 5, A/B)
  // the connecting-edge sort: lo half + run pass for runs of <= sort_run keys
  // (sort.hip sort_keys_lex); 0: all 2 nb bits by onesweep.  TNP_SORT_RUN at creation
  int sort_run = 64;
  int64_t pend_lz_n = 0;              // lzpart entries holding E_live (0: E_live is known)
  tnp_step_stats* pend_st = nullptr;  // the step whose V_out / E_out wait for them
  Buf hpart;                          // the hit workers' live counts
  // step scratch
  Buf spcnt, spoff, part, ekey_a, ekey_b, eval_b, sort_scr2;
  // (pcell/ptoff: compacted pair cells and their first pair; ents: CellEnt
  // records in cell order; used/nid/flags: int32 scratch of compaction,
  // surface and skeleton)
  Buf blk, blkoff, sa, sb, stage, shared, members, pcn, pent, rstart, ent_v,
      ents, pcell, ptoff, bcell, ckeys_a, ckeys_b, sort_scr, flags, used, nid, ctr;
  uint64_t* ckeys = nullptr;  // sorted connecting edges of the current step
  int64_t* h_ctr = nullptr;  // host copy of ctr (the last readback)
  int64_t* h_map = nullptr;  // host-mapped mirror written by k_publish ([31]: sequence)
  int64_t* h_map_dev = nullptr;
  int64_t pub_seq = 0;
  // tnp_engine_run_steps: a step's last readback zeroes the counter words
  // (k_publish clear), and the next split skips its memset -- one host API
  // call less per step (hipMemsetAsync costs the host ~5-9 us, the
  // bunny-scale loop is launch-bound, profiles/r06_small_hip_trace.txt).
  // ctr_zero: the words are zero since the last publish; any other
  // publish, launch into the words or engine call in between clears it
  bool in_run = false;
  bool ctr_zero = false;
  // pending split
  int pend_idx = -1;
  int64_t pend_S = 0, pend_dup = 0;
  bool pend_hits = false;   // the pending split also found the plane's hit vertices
  int64_t pend_hoff = -1;   // ... at members[pend_hoff] (the split's E; -1: after the S new members)
  bool pend_fused = false;  // the pending split ran k_forward_new (flat path)
  // faces output
  Buf tri, faces;
  Buf tied_table;  // level-interleaved copy of the caller's table (NetDev::tied)
  int64_t n_tri = 0, n_faces = 0, dbg_F = 0, dbg_W = 0;
  // the final rows of extract_faces (faces_rows: F1-F4) are in the face
  // scratch for the loaded complex, net and eps; cleared by whatever changes
  // one of the three.  rows_F rows, the largest member count (all members /
  // those off the origin)
  bool rows_valid = false;
  int64_t rows_F = 0, rows_maxc = 0, rows_maxnz = 0;
  int64_t n_poly = 0, n_pidx = 0;  // the last tnp_engine_polygons (poly_valid: still in the scratch)
  bool poly_valid = false;
  // look-back states (a kernel may run two chains): [0] ticket counter,
  // [1..] tile status words; tickets issued so far; launch epoch
  Buf lb[2];
  uint64_t lb_tickets[2] = {0, 0};
  uint32_t lb_epoch[2] = {0, 0};
  int32_t lb_spin = -1;  // TNP_LB_SPIN: ticket-free look-back polls (0 forces the recompute path)
  Buf lbrc;              // look-back recompute counter (tnp_engine_debug_lb_recomputes)
  Buf sk_gload;   // skeleton_gmax: the tiles' max |grad sdf| words, then the [3][L] load counts
  Buf sk_gmax;    // skeleton_box: the caller's tile maxima on the device
  Buf fscr2[32];
  Buf sents;                // bucket-ordered packed entries before the in-bucket grouping
  Buf sents2;               // ... regrouped by octant (two-level bucket geometries, BK_OBASE: their bases)
  Buf bk[BK_N];             // bucket.hip scratch (BK_*)
  bool radix_cells = false; // TNP_RADIX_CELLS=1: the radix-sort bucketing path
  bool lds_records = true;  // TNP_LDS_RECORDS=0: the grouping's records go through memory
  bool bk_clean = false;    // bucket counters (BK_CNT, BK_CUR) are zero
  Buf cv[CV_N];
};

// the counter block is cleared as 32 words: a 248-byte memset takes two fill
// dispatches (aligned body + tail), 256 bytes one
constexpr size_t CTR_CLEAR_BYTES = 32 * sizeof(int64_t);
static_assert(CTR_N <= 32, "counter block");

// the helpers more than one piece calls (each documented at its definition),
// in a namespace: the shared object exports no unqualified name of theirs
namespace tnp_host {
// engine.cpp
extern thread_local std::string g_err;  // tnp_last_error()
size_t buf_grow_bytes(size_t have, size_t bytes);
int64_t connect_key_cap(size_t have_bytes, int64_t M, int xs_n);
int buf_ensure(Buf& b, size_t bytes, hipStream_t s, bool keep = false);
int post_ctr(tnp_engine* e, hipStream_t s, int64_t* seq_out, const int64_t* vpart = nullptr, int nv = 0,
             const int64_t* epart = nullptr, int ne = 0, bool clear = false);
int wait_ctr(tnp_engine* e, hipStream_t s, int64_t seq);
int read_ctr(tnp_engine* e, hipStream_t s, const int64_t* vpart = nullptr, int nv = 0,
             const int64_t* epart = nullptr, int ne = 0, bool clear = false);
void apply_counts(tnp_engine* e, int64_t V_live, int64_t E_live);
int resolve_counts(tnp_engine* e, hipStream_t s);
int ktimer_begin(tnp_engine* e, const char* name, double bytes, hipStream_t s);
double table_bytes(const NetDev& n);
void ktimer_set_bytes(tnp_engine* e, double bytes);
void ktimer_set_bytes(tnp_engine* e, const char* name, double bytes);
void ktimer_end(tnp_engine* e, int t, hipStream_t s);
int lb_begin(tnp_engine* e, int64_t tiles, hipStream_t s, TnpLB* out, int w = 0, bool ticketed = true);
int scan_counts(tnp_engine* e, const int32_t* in, int64_t* out, int64_t n, int slot, hipStream_t s);
int vset_ensure(tnp_engine* e, VSet& v, int64_t rows, int64_t keep_rows, hipStream_t s);
int set_alive(tnp_engine* e, int64_t from, int64_t n, hipStream_t s);
int reset_live(tnp_engine* e, hipStream_t s, bool edges_changed = true);
void span_all(tnp_engine* e);
void span_of(const tnp_engine* e, int lo[3], int hi[3]);
bool uses_buckets(const tnp_engine* e, BucketGeom* bg);
bool eps2(const tnp_engine* e);
int new_keep_from(const tnp_engine* e, int idx);
int compute_masks(tnp_engine* e, int from, int64_t* ctr, hipStream_t s);
int ensure_masks(tnp_engine* e, int idx, hipStream_t s);
int compact_now(tnp_engine* e, hipStream_t s);
int require_valid(const tnp_engine* e, const char* what);
NetDev to_dev(const tnp_net* n);
int check_net(const tnp_net* n);
// engine_curve.cpp
int coll(tnp_engine* e, int64_t* v, int n, int op);
int coll_fail(tnp_engine* e, int n, int op);
int fold32_sharded(const tnp_engine* e, int64_t rows, const char* what, int idx);
int curve_correct(tnp_engine* e, int idx, int64_t S, hipStream_t s);
int curve_filter(tnp_engine* e, int idx, int override_, hipStream_t s, int64_t* S_out);
}  // namespace tnp_host

#define TIMED(name, bytes, call)                                   \
  do {                                                             \
    int _t = ktimer_begin(e, name, (double)(bytes), s);            \
    if (call) return -1;                                           \
    ktimer_end(e, _t, s);                                          \
  } while (0)
