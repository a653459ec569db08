/*
 * tropical_hip_debug.h -- diagnostic entry points of libtropical_hip.so.
 *
 * Not part of the product surface (include/tropical_hip.h): self-checks and
 * intermediate dumps used by tests/ and tools/ only.  Same conventions as
 * tropical_hip.h (d_* device pointers, 0 / -1 returns, tnp_last_error()).
 */
#ifndef TROPICAL_HIP_DEBUG_H
#define TROPICAL_HIP_DEBUG_H

#include "tropical_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Self-check of the fp32 primitives the bitwise contract relies on:
 * out[8i..8i+7] = sqrt_rn(a), a/b (rn), fma(a,b,c), a*b, a+b, sqrtf(a),
 * a/b (default), tanhf(a). */
int tnp_debug_ops(const float* d_a, const float* d_b, const float* d_c, int64_t n,
                  float* d_out, void* stream);

/* Debug: padded angular scores (F x width fp32) of the last faces call. */
int tnp_engine_faces_debug(tnp_engine* eng, float* d_scores, int64_t cap, int64_t* F,
                           int64_t* width, void* stream);

/* Debug: the ticket-free look-back of the split, prune and count scans
 * (csrc/common.h lb_prefix_rc).  set_lb_spin: polls of an unpublished
 * predecessor tile before the waiting wave recomputes its aggregate (< 0: the
 * kernels' defaults, 0: recompute every unpublished predecessor -- the path
 * in-order dispatch makes rare).  lb_recomputes: recomputes since the last
 * reset (reset=1 zeroes the counter after reading it). */
int tnp_engine_debug_set_lb_spin(tnp_engine* eng, int spin);
int tnp_engine_debug_lb_recomputes(tnp_engine* eng, int64_t* n, int reset, void* stream);

/* Debug: the single-pass count scan (csrc/scan.hip k_scan_lb) on its own,
 * launched as the engine's steps launch it: through the engine's look-back
 * buffer (chain 0), its launch epoch and its lb_spin.  d_out[i] = sum of
 * d_in[0, i) (int32 counts, int64 offsets), *h_total (host) = the sum of all
 * n; synchronises the stream.  A tile's status word holds 40 value bits:
 * sums >= 2^40 are outside the scan's contract (counts of a complex never
 * come near it) and are not checked. */
int tnp_engine_debug_scan(tnp_engine* eng, const int32_t* d_in, int64_t n, int64_t* d_out,
                          int64_t* h_total, void* stream);

/* Debug: the launch epoch of look-back chain 0 / 1 (22 bits, advanced by
 * every single-pass launch; csrc/engine.cpp lb_begin clears the records when
 * it wraps).  *h_epoch (nullable): the epoch of the chain's last launch;
 * set >= 0 then overwrites it -- the host field only, no device work, so the
 * records in memory keep the epochs they were written with. */
int tnp_engine_debug_lb_epoch(tnp_engine* eng, int chain, int64_t set, int64_t* h_epoch);

/* Debug: the connecting-edge key sort (csrc/sort.hip sort_keys_lex) on n
 * unique keys lo << nb | hi (zero above bit 2 nb) with run threshold R, as
 * the connect phase calls it: private copies of the keys, a scratch of
 * exactly the size the sort asks for.  d_out: the n keys ascending; d_keys is
 * only read.  Synchronises the stream. */
int tnp_debug_sort_keys_lex(const uint64_t* d_keys, int64_t n, int nb, int R, uint64_t* d_out,
                            void* stream);

/* Debug: the batched fill (csrc/scan.hip launch_fill) on k byte ranges in ONE
 * call: range i is h_sizes[i] bytes at device pointer h_ptrs[i], set to the
 * low byte of h_bytes[i] (host arrays).  Null and empty ranges are skipped;
 * more non-empty ranges than one launch takes return -1. */
int tnp_debug_fill(void* const* h_ptrs, const uint64_t* h_sizes, const uint32_t* h_bytes, int k,
                   void* stream);

/* Debug: the grouping kernel's LDS-record path (csrc/bucket.hip
 * k_bucket_group; on by default, TNP_LDS_RECORDS=0 at engine creation turns
 * it off): on = 0 sends every bucket's records through memory, as before. */
int tnp_engine_debug_set_lds_records(tnp_engine* eng, int on);

/* Debug: the vertex set's row capacity (the cache, coordinates and keys are
 * sized by it) and how often the early k_forward_new's row bound (the
 * largest split count seen, csrc/engine.cpp early_bound) was below a step's
 * split count, so that the forward ran again once the count was known. */
int tnp_engine_debug_vertex_capacity(tnp_engine* eng, int64_t* rows, int64_t* early_redo);

/* Debug: the engine's capacity arithmetic, host only (csrc/engine.cpp
 * buf_grow_bytes, connect_key_cap).  grown_bytes: the size a buffer of
 * have_bytes grows to for a request of request_bytes; key_cap: the connect
 * phase's key capacity (keys, a multiple of xs_n) for a step of `members`
 * bucket members when the key buffer holds have_bytes.  A steady workload
 * must never ask for more than the buffer holds: key_cap * 8 <= have_bytes
 * whenever have_bytes already covers the floor. */
int tnp_debug_buf_growth(int64_t have_bytes, int64_t request_bytes, int64_t members, int xs_n,
                         int64_t* grown_bytes, int64_t* key_cap);

/* Debug: the curve branch's gradient-descent fallback (descend.h, the
 * engine's launch) on n arbitrary rows: row r descends along the edge
 * d_ends[r] (e0 xyz, e1 xyz) from the box parameters d_x[r] (in/out) on
 * plane pair (d_plane[r], idx) for exactly `iters` iterations (<= 512);
 * d_d0 / d_d1: the distances evaluated before the last update.  The batch
 * is the n rows (MKL row-count schedules).  per_thread: the one-thread-per-
 * row kernel.  Checked against the oracle's descend (oracle/curve.py). */
int tnp_debug_descend(const tnp_net* net, const float* d_ends, float* d_x, const int32_t* d_plane, int64_t n,
                      int idx, float eps, int iters, float* d_d0, float* d_d1, int per_thread, void* stream);

/* Debug: which coverage path tnp_render_raster takes (csrc/render.hip).  0 (default): by the
 * bounding box against TNP_RENDER_SMALL_MAX; 1: every triangle by one thread; 2: every triangle
 * by a workgroup.  The buffers must not depend on it.  Process-wide; returns the previous mode,
 * -1 for a mode outside 0 .. 2. */
int tnp_debug_render_path(int mode);

/* Debug: stage times of tnp_topology_build (csrc/topology.hip).  enable != 0: later builds on this
 * handle record an event between their stages.  ms != NULL: the milliseconds of the last timed
 * build's stages (at most n of them), in the order check_edges, edge_sort, label_polygons,
 * label_boundary, tables_alloc, component_counts, vertex_sort, polygon_order, geometry, loops.
 * Returns the number of stages (TNP_TOPOLOGY_STAGES), -1 on error. */
#define TNP_TOPOLOGY_STAGES 10
int tnp_debug_topology_stages(tnp_topology* t, int enable, double* ms, int n);

/* Debug: stage times of tnp_holes_build (csrc/holes.hip), as tnp_debug_topology_stages: in the
 * order check_edges, edge_sort, label_boundary, status, compact, rank, scatter.  A build that
 * finds no loop records none.  Returns the number of stages (TNP_HOLES_STAGES), -1 on error. */
#define TNP_HOLES_STAGES 7
int tnp_debug_holes_stages(tnp_holes* h, int enable, double* ms, int n);

/* Debug: stage times of tnp_weld_build (csrc/weld.hip), as tnp_debug_topology_stages: in the order
 * check_used, grid_keys, cell_sort, search, clusters, positions, rewrite.  A build with P = 0 records
 * none.  Returns the number of stages (TNP_WELD_STAGES), -1 on error. */
#define TNP_WELD_STAGES 7
int tnp_debug_weld_stages(tnp_weld* w, int enable, double* ms, int n);

/* Debug: stage times of tnp_simplify_build (csrc/simplify.hip), as tnp_debug_topology_stages: in the
 * order check_used, grid_keys, cell_sort, classes, positions, rewrite, duplicates.  A build with
 * P = 0 records none.  Returns the number of stages (TNP_SIMPLIFY_STAGES), -1 on error. */
#define TNP_SIMPLIFY_STAGES 7
int tnp_debug_simplify_stages(tnp_simplify* h, int enable, double* ms, int n);

#ifdef __cplusplus
}
#endif

#endif /* TROPICAL_HIP_DEBUG_H */
