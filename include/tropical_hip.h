/*
 * tropical_hip.h -- C ABI of the MI355X (gfx950) polyhedral-complex
 * extraction library (libtropical_hip.so).
 *
 * Every pointer named d_* is DEVICE memory on the engine's / caller's current
 * HIP device; `stream` is a hipStream_t passed as void* (0 = null stream).
 * No torch types cross this boundary.  All functions return 0 on success and
 * -1 on failure; tnp_last_error() then describes the failure (thread-local).
 *
 * The reference (seonghunn/tropical-nerf.pytorch) is pure Python/PyTorch and
 * has no FFI of its own; each entry point below names the reference
 * function (file:line under tropical/) whose semantics it implements.  The
 * Python host package (tropical-nerf.pytorch_amd/tropical) binds these with
 * ctypes behind the reference's own call surface.
 */
#ifndef TROPICAL_HIP_H
#define TROPICAL_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TNP_MAX_LEVELS 8
#define TNP_ABI_VERSION 1

/* Piecewise-trilinear SDF net: hash-grid encoding (tcnn Grid/Hash, 2
 * features/level, tropical.py:32-40) + ReLU MLP (model.py:38-50).
 * weights: fc.0.weight (H x 2L, row-major), fc.0.bias (H), fc.1.weight,
 * fc.1.bias, ..., fc.last.weight (2 x H), fc.last.bias (2), packed in that
 * order.  table: the flat `enc.module.params` (tcnn layout
 * params[(offset_l + index) * 2 + f]). */
typedef struct tnp_net {
  int32_t n_levels;   /* L  (2..8 are instantiated) */
  int32_t n_features; /* F  (must be 2) */
  int32_t num_layers; /* with num_hidden, one of the instantiated shapes */
  int32_t num_hidden; /* (layers, hidden): (2..4, 8) (2..4, 16) (2, 32) -- K <= 63 planes, every
                         operation; (5, 16) (3, 32) (4, 32) -- K = 65 / 97, two-word sign keys:
                         forward, region, sdf, skeleton and the flat single-device steps and
                         faces (no curve branch, sharding, training or autograd kernels) */
  int32_t n_marks;    /* len(TropicalHashGrid.marks) */
  float eps;          /* Net.eps (model.py:20) */
  float scales[TNP_MAX_LEVELS];    /* fp32 exp2(l*log2 b)*N_min - 1 */
  int32_t res[TNP_MAX_LEVELS];     /* ceil(scale)+1 */
  uint32_t sizes[TNP_MAX_LEVELS];  /* min(next_mult(res^3,8), 2^T) */
  uint32_t offsets[TNP_MAX_LEVELS];
  int32_t dense[TNP_MAX_LEVELS];   /* res^3 <= size */
  const float* d_table;
  const float* d_weights;
  const float* d_marks;
} tnp_net;

/* Per-step counters (the roofline model's inputs). */
typedef struct tnp_step_stats {
  int32_t idx;
  int64_t V_in, E_in, S, H, X, V_out, E_out;
  int64_t A;      /* augmented region rows the reference would build */
  int64_t P;      /* candidate in-region pairs the reference would build */
  int64_t pair_tests; /* member pairs this implementation tested */
  int32_t override_applied;
  uint64_t next_active; /* planes > idx a kept edge would split (pruning steps) */
  int64_t S_dup;        /* splits outside the owned slab (multi-GPU halo) */
  int64_t T;            /* (cell, member) entries of the pair test */
} tnp_step_stats;

const char* tnp_last_error(void);
int tnp_abi_version(void);
/* Hash of the sources the library was built from (csrc/build_id.sh); the
 * Python binding refuses a library whose id differs from its tree's. */
const char* tnp_build_id(void);
int tnp_device_count(int* n);

/* ---- stateless net ops -------------------------------------------------- */

/* Net.forward(x, gather=True)[1] concatenated (model.py:52-76): pre-
 * activations of every hidden neuron + (o1 - o0), written PLANE-MAJOR
 * d_pre[p * ld + i], p < K = (num_layers-1)*num_hidden + 1.  Bitwise equal
 * to the PyTorch-CPU reference (sequential-fma MLP, non-fused encoding). */
int tnp_forward(const tnp_net* net, const float* d_xyz, int64_t n,
                float* d_pre, int64_t ld, float* d_out2, void* stream);
/* d_out2 (nullable): the raw last-layer outputs [n][2] (Net.forward(x)
 * without gather).  d_pre may be null. */

/* TropicalHashGrid.forward(x) (tropical.py:46-47): x in [0,1]^3 (already
 * preprocessed), out [n][2L] fp32 (level-major, tcnn column order). */
int tnp_encode(const tnp_net* net, const float* d_x01, int64_t n, float* d_out,
               void* stream);

/* Net.forward(x, gather=True, group=8) (model.py:67-70): rows come in groups
 * of 8 box corners sharing one activation pattern. */
int tnp_forward_grouped(const tnp_net* net, const float* d_xyz, int64_t n,
                        float* d_pre, int64_t ld, float* d_out2, void* stream);

/* Net.region(v, output, eps) (model.py:90-103 + tropical.py:227-236):
 * d_m[n x (3+K)] int64 {grid mask 0/1, plane sign -1/0/1}, d_off[n x 3]
 * int64 offsets.  d_pre is plane-major with leading dimension ld. */
int tnp_region(const tnp_net* net, const float* d_xyz, const float* d_pre,
               int64_t ld, int64_t n, float eps, int64_t* d_m, int64_t* d_off,
               void* stream);

/* Net.sdf (model.py:84-88) and its input gradient (Net.normal,
 * model.py:105-123).  d_grad may be null. */
int tnp_sdf_grad(const tnp_net* net, const float* d_xyz, int64_t n,
                 float* d_sdf, float* d_grad, void* stream);

/* ---- stateful extraction engine ---------------------------------------- */

typedef struct tnp_engine tnp_engine;

int tnp_engine_create(tnp_engine** out, int device);
void tnp_engine_destroy(tnp_engine* eng);
int tnp_engine_set_net(tnp_engine* eng, const tnp_net* net);
/* Device memory the engine holds: *bytes = the sum of every scratch and
 * complex buffer (they grow geometrically and are reused across steps and
 * passes, so a repeated workload holds this constant after its first pass);
 * *buffers = buffers allocated; *key_bytes = the connect phase's key buffer
 * (the one round 4's growth bug inflated).  buffers / key_bytes may be null.
 * No reference counterpart (PyTorch's caching allocator there). */
int tnp_engine_scratch_bytes(tnp_engine* eng, int64_t* bytes, int64_t* buffers, int64_t* key_bytes);

/* Load a complex: vertices V x 3 fp32, edges E x 2 int64 (device).  d_pre:
 * optional cached outputs_ (V x K fp32, row-major as the reference keeps
 * them); null computes them (subpoly.py:92-93).  keep_all_planes=1 keeps
 * every cached column through compaction (needed to hand outputs_ back);
 * 0 keeps only the columns later steps read. */
int tnp_engine_load(tnp_engine* eng, const float* d_xyz, int64_t V,
                    const int64_t* d_edges, int64_t E, const float* d_pre,
                    int keep_all_planes, void* stream);

/* TropicalHashGrid.skeleton(net, unit) with PRUNING_MODE="distance"
 * (tropical.py:158-225) computed on the device and loaded as the complex;
 * falls back to get_hypercube(3, size) (subpoly.py:51-52, 731-750). */
int tnp_engine_skeleton(tnp_engine* eng, int unit, float size, void* stream,
                        int64_t* V, int64_t* E);
/* The same with the reference's pruning mode chosen (TropicalHashGrid.skeleton,
 * tropical/tropical.py:184-205: PRUNING_MODE is "distance" there; "sign" is
 * its dormant branch -> _skeleton, tropical.py:80-109, keeping an edge iff
 * the endpoints' eps-sign vectors over all planes differ). */
enum { TNP_SKELETON_DISTANCE = 0, TNP_SKELETON_SIGN = 1 };
int tnp_engine_skeleton_mode(tnp_engine* eng, int unit, float size, int mode, void* stream,
                             int64_t* n_vertices, int64_t* n_edges);
/* The distance-mode skeleton split over the ranks of a sharded extraction
 * (no reference counterpart: the reference runs one device).
 * skeleton_gmax: the tiles t of the reference's tile grid (tropical.py:
 * 176-181) with t % world == rank are evaluated whole; h_gmax[t] = the bits
 * of their max |grad sdf| (0 for the other tiles; the ranks' MAX is every
 * tile's), h_load[3][n_marks] (may be null) += per axis and mark plane the
 * points under the tile's edge threshold (the cuts' load balance; SUM over
 * the ranks).  *n_tiles = the tile count (<= cap).
 * skeleton_box: loads the part of the skeleton inside the mark box
 * [lo[d], hi[d]] -- exactly the whole skeleton with the vertices outside
 * the box and the edges leaving it dropped, order kept -- evaluating only
 * tile & box, with every tile's max |grad sdf| from h_gmax[n_tiles].  A box
 * the skeleton misses holds an empty complex (the whole skeleton's
 * emptiness, the hypercube fallback, is the caller's test). */
int tnp_engine_skeleton_gmax(tnp_engine* eng, int unit, int rank, int world, uint32_t* h_gmax,
                             int64_t* h_load, int cap, int* n_tiles, void* stream);
int tnp_engine_skeleton_box(tnp_engine* eng, int unit, const int32_t* lo, const int32_t* hi,
                            const uint32_t* h_gmax, int n_tiles, void* stream, int64_t* n_vertices,
                            int64_t* n_edges);

/* Load the full lattice over the marks restricted to the x-slab of mark
 * indices [x0, x1] (x0=0, x1=n_marks-1: the whole N^3 lattice) in the
 * layout of TropicalHashGrid._skeleton(..., pruning=False)
 * (tropical.py:103-109) with vertex ids (i-x0)*N^2 + j*N + k. */
int tnp_engine_lattice(tnp_engine* eng, int x0, int x1, int keep_all_planes,
                       void* stream, int64_t* V, int64_t* E);
/* The same lattice restricted to the box of mark indices [lo[d], hi[d]] per
 * axis (a block of a sharded lattice): vertex ids
 * (i-lo0)*ny*nz + (j-lo1)*nz + (k-lo2), edges in the same x / y / z order;
 * sets the span (tnp_engine_set_span) to the box. */
int tnp_engine_lattice_box(tnp_engine* eng, const int32_t* lo, const int32_t* hi, int keep_all_planes,
                           void* stream, int64_t* V, int64_t* E);

/* Bit p (p >= from) set iff some edge has endpoints with non-zero opposite
 * eps-signs on plane p, i.e. subpoly_ at idx=p would split (subpoly.py:104-110). */
int tnp_engine_active_planes(tnp_engine* eng, int from, uint64_t* mask,
                             void* stream);

/* subpoly_ phase 1 (subpoly.py:98-117, 180-189): sign test, order-preserving
 * split compaction, new vertices, their forward pass and the LOCAL
 * failover-override predicate.  Writes S (local split count) and fail
 * (0/1; -1 = left on the device -- single-device flat engines skip that
 * round trip; pass it on to tnp_engine_finish unchanged). */
int tnp_engine_split(tnp_engine* eng, int idx, void* stream, int64_t* S,
                     int32_t* fail);

/* subpoly_ phase 2 (subpoly.py:189-279): apply the override if `override`
 * (the GLOBAL predicate; -1: the device-resident local one), connecting edges, pruning (prune=1) and vertex
 * compaction.  Must follow tnp_engine_split on the same idx. */
int tnp_engine_finish(tnp_engine* eng, int idx, int prune, int override,
                      void* stream, tnp_step_stats* stats);

/* The whole hyperplane loop of subpoly.py:58-69 on one device: active
 * planes, then per active plane tnp_engine_split + tnp_engine_finish (prune
 * on every plane but the last), empty steps skipped (subpoly.py:110), the
 * next-active mask folded in after each pruning step -- the loop a host
 * driver would run, without a host round trip per step.  stats[0 ..
 * max_stats) receive the completed steps' stats, *n_steps their count.  Not
 * for a sharded engine (tnp_engine_set_shards > 1: its global decisions
 * fall between split and finish). */
int tnp_engine_run_steps(tnp_engine* eng, void* stream, tnp_step_stats* stats, int max_stats,
                         int* n_steps);

int tnp_engine_sizes(tnp_engine* eng, int64_t* V, int64_t* E);

/* Curve path: after tnp_engine_finish, the strict filter's keep flags
 * (int32 0/1) of the step's n candidate splits in edge order -- the mask
 * debug.strict_check returns (subpoly_debug.py:234-271) that the reference's
 * masked_scatter_ rewrites the caller's edges with (subpoly.py:209-212). */
int tnp_engine_split_keep(tnp_engine* eng, int32_t* d_keep, int64_t n, void* stream);

/* Copy the complex out: d_xyz V x 3, d_edges E x 2 int64, d_pre V x K
 * row-major (requires keep_all_planes, else may be null). */
int tnp_engine_export(tnp_engine* eng, float* d_xyz, int64_t* d_edges,
                      float* d_pre, void* stream);

/* extract_skeleton (subpoly.py:556-581) applied in place; writes the
 * surface sizes (0/0 when fewer than 3 surface vertices). */
int tnp_engine_surface(tnp_engine* eng, void* stream, int64_t* V, int64_t* E);

/* extract_faces (subpoly.py:584-728, geometry.py:483-556) on the current
 * (surface) complex: n_tri = rows of faces_with_indices, n_faces = rows of
 * the float faces (they differ only when a vertex sits exactly at the
 * origin, which the reference's norm>0 mask drops).  Read both with
 * tnp_engine_faces_export (d_tri n_tri x 3 int64, d_faces n_faces x 3 x 3;
 * device memory or pinned host memory -- the copies are asynchronous on
 * `stream`: synchronise it before reading host destinations). */
int tnp_engine_faces(tnp_engine* eng, void* stream, int64_t* n_tri, int64_t* n_faces);
int tnp_engine_faces_export(tnp_engine* eng, int64_t* d_tri, float* d_faces,
                            void* stream);

/* The surface as convex polygons: final row f of extract_faces (subpoly.py:620 order), its members in
 * the angular order of sort_polygon_vertices_batch, -1 pads dropped, ids de-duplicated keeping the first
 * (tensor_to_triangle_faces, subpoly.py:702-704), rows left with < 3 ids omitted. Fan-triangulating
 * polygon f as (p0, p[t+1], p[t+2]) and listing the triangles t-major is exactly tnp_engine_faces' tri.
 * The rows of a tnp_engine_faces call on the same complex, net and eps are reused (either order of
 * the two calls); a later tnp_engine_faces or another complex replaces the polygons held for export. */
int tnp_engine_polygons(tnp_engine* eng, void* stream, int64_t* n_poly, int64_t* n_idx);
/* offsets int64[n_poly+1], indices int64[n_idx] (surface vertex ids, as faces_with_indices),
 * normals float[n_poly*3] (the row's SDF gradient at its mean point, subpoly.py:635, not normalised);
 * any may be NULL; destinations on the device or in pinned host memory, as tnp_engine_faces_export. */
int tnp_engine_polygons_export(tnp_engine* eng, int64_t* d_offsets, int64_t* d_indices,
                               float* d_normals, void* stream);

/* Closedness, orientation and planarity of any polygon soup: polygon p is
 * d_indices[d_offsets[p] .. d_offsets[p+1]) over d_xyz (V x 3 fp32), all on the device.
 *  - The edges of a polygon are its consecutive pairs, cyclic (last, first included); the
 *    undirected key of an edge (a, b) is (min, max).  n_edges counts distinct undirected edges.
 *  - An edge used u times (over all polygons) is boundary (u = 1), manifold (u = 2) or
 *    non-manifold (u > 2).  e_misoriented counts the edges with u = 2 that both polygons
 *    traverse in the same direction (a consistently oriented surface has none).
 *  - n_vertices_used: distinct ids that occur; euler = n_vertices_used - n_edges + n_polygons.
 *  - Geometry in fp32, Newell about the mean c of the members: N = 1/2 sum_i (p_i - c) x (p_i+1 - c);
 *    a polygon's area is |N|, its planarity deviation dev = max_i |(p_i - c) . N| / |N| (0 when |N| = 0).
 *    area: the sum of the per-polygon areas in double, reduced in a fixed order (the same bits on
 *    every call with the same input); max_dev: the largest dev.
 * d_area / d_dev (P floats each, may be NULL) receive the per-polygon values.
 * Checked on the device before anything is read through an id, -1 with the first offender in
 * tnp_last_error(): offsets not starting at 0 or decreasing, a polygon with fewer than 3 ids
 * (the first such polygon); then an id outside [0, V), two equal consecutive ids, cyclic (the
 * first such index position).  V >= 2^31 is refused.  P = 0: all zero.  Synchronises `stream`. */
typedef struct tnp_polygon_stats {
  int64_t n_polygons, n_indices, max_degree, n_vertices_used;
  int64_t n_edges, e_boundary, e_manifold, e_nonmanifold, e_misoriented;
  int64_t euler;            /* n_vertices_used - n_edges + n_polygons */
  double area; float max_dev;
} tnp_polygon_stats;
int tnp_polygon_report(const float* d_xyz, int64_t V, const int64_t* d_offsets, const int64_t* d_indices,
                       int64_t P, tnp_polygon_stats* h_out, float* d_area, float* d_dev, void* stream);

/* Connected components and boundary loops of a polygon soup (csrc/topology.hip), the soup as
 * tnp_polygon_report takes it, with its checks, its first-offender rule and its message texts
 * (prefix "topology"); V and P must be below 2^31.  P = 0: 0 components, 0 loops.
 *
 * Components.  Two polygons are adjacent when they share an undirected edge (connect = 0) or a
 * vertex id (connect = 1); a component is a class of the transitive closure, so all users of a
 * non-manifold edge are one component, and two closed shells that touch at one vertex are two
 * components under connect = 0 and one under connect = 1.  Components are numbered by ascending
 * smallest polygon id: label[p] in [0, C) is a function of the input alone.  Every undirected edge
 * lies in exactly one component in both modes.  One tnp_component row per component:
 *  - first_polygon (its smallest polygon id), n_polygons, n_indices (the sum of its degrees);
 *  - n_vertices: the distinct ids its polygons use;
 *  - n_edges, e_boundary, e_manifold, e_nonmanifold, e_misoriented: tnp_polygon_report's classes
 *    over the component's edges (each column sums to the report's total);
 *  - euler = n_vertices - n_edges + n_polygons;
 *  - area: the sum in double of tnp_polygon_report's fp32 per-polygon areas (the same bits per polygon);
 *  - volume: with the fp32 coordinates converted to double, D = sum over the polygons and their fan
 *    triangles (p0, p[t+1], p[t+2]) of p0 . (p[t+1] x p[t+2]), each product and sum rounded once
 *    (p0x (p1y p2z - p1z p2y) + p0y (p1z p2x - p1x p2z) + p0z (p1x p2y - p1y p2x), left to right);
 *    volume = D / 6: the signed enclosed volume when the component is closed and consistently
 *    oriented (e_boundary = e_nonmanifold = e_misoriented = 0), outward winding positive;
 *  - lo, hi: the fp32 bounding box of the vertices its polygons use.
 *  A polygon's fan triangles are added left to right; the polygons' areas and determinant sums
 *  are reduced in a shape fixed by the input: the polygons in (label, polygon id) order,
 *  cut into pieces at the multiples of 256 of that order and at the component boundaries; a piece
 *  that is a whole 256-block is summed by a fixed tree, any other piece left to right; a component's
 *  pieces, in order, by 64 strided partial sums and a fixed tree.  The same bits on every call.
 *
 * Boundary loops.  The boundary graph has the vertex ids as nodes and the edges used exactly once
 * as edges; a loop is a connected component of it with at least one edge.  Loops are numbered by
 * ascending smallest vertex id.  One tnp_boundary_loop row per loop:
 *  - first_vertex (its smallest vertex id), n_edges, n_vertices;
 *  - simple: 1 iff every vertex of the loop has exactly two boundary edges;
 *  - component: the label of the polygon that owns the loop's smallest edge key (min << 32) | max;
 *  - length: each edge's length in double from the fp32 coordinates (differences, squares, their sum
 *    left to right, sqrt), summed over the loop's edges in ascending edge key in the shape above.
 *
 * build labels the soup, keeps the three tables in the handle (replacing those of an earlier build)
 * and returns the counts; export copies them to device memory (label int32 [P], C rows, L rows; any
 * may be NULL), asynchronously on `stream`.  build synchronises `stream`. */
typedef struct tnp_component {
  int64_t first_polygon, n_polygons, n_indices, n_vertices;
  int64_t n_edges, e_boundary, e_manifold, e_nonmanifold, e_misoriented;
  int64_t euler;
  double area, volume;
  float lo[3], hi[3];
} tnp_component;
typedef struct tnp_boundary_loop {
  int64_t first_vertex, n_edges, n_vertices;
  int64_t component;
  double length;
  int32_t simple, reserved; /* reserved: 0 */
} tnp_boundary_loop;
typedef struct tnp_topology tnp_topology;
int tnp_topology_create(tnp_topology** out, int device);
void tnp_topology_destroy(tnp_topology* t);
int tnp_topology_build(tnp_topology* t, const float* d_xyz, int64_t V, const int64_t* d_offsets,
                       const int64_t* d_indices, int64_t P, int connect, int64_t* n_components,
                       int64_t* n_loops, void* stream);
int tnp_topology_export(tnp_topology* t, int32_t* d_label, tnp_component* d_components,
                        tnp_boundary_loop* d_loops, void* stream);

/* The boundary loops of a polygon soup as ordered cycles, and the caps that close them
 * (csrc/holes.hip).  The result is again a polygon soup: the input polygons followed by the caps,
 * the input vertices followed by the new ones.
 *
 * Input.  The polygon soup of tnp_polygon_report / tnp_topology_build, with the same checks, the same
 * first-offender rule and the same message texts (prefix "holes"); V and P must be below 2^31.
 * P = 0: no loops.  No coordinates are read by build.
 *
 * Boundary edges, loops, loop numbers, simple: exactly tnp_topology_build's.  A loop's number is its
 * row number in the topology's loop table for the same soup.
 *
 * Direction.  A boundary edge is used once, by one polygon, which traverses it a -> b.  The cap
 * traverses it b -> a: succ[b] = a, which makes the edge manifold and not misoriented.
 *
 * Status of a loop (int32), the rules tested in this order:
 *  - TNP_HOLE_NONSIMPLE (1): simple = 0 (a pinch vertex: pairing the edges into cycles is a
 *    geometric choice);
 *  - TNP_HOLE_UNORIENTED (2): the loop is simple, but some vertex is the tail of two of its
 *    reversed edges (and another is then the head of two): the surface flips orientation along it;
 *  - TNP_HOLE_TOO_LONG (3): max_edges > 0 and n_edges > max_edges;
 *  - TNP_HOLE_CAPPED (0): every other loop.
 *  A simple loop has at least 3 edges: two boundary edges cannot share both ends.  Loops of status
 *  1, 2 and 3 are counted and left open.
 *
 * Cycle.  The k-th capped loop, in loop order, is cycle k: c_0 is the loop's first_vertex (its
 * smallest id), c_{i+1} = succ[c_i], the length m = n_edges.  Cycles are a function of the input alone.
 *
 * Caps, listed in cycle order.
 *  - mode 0 (polygon): cap k is the polygon (c_0 ... c_{m-1}).  No vertex is added.
 *  - mode 1 (star): a cycle with m = 3 is its own triangle.  A cycle with m >= 4 gets one new vertex
 *    V + s, s being the cycle's rank among the cycles with m >= 4, and the m triangles
 *    (c_i, c_{(i+1) mod m}, V + s), i = 0 ... m-1.  The new vertex is the mean of the cycle's fp32
 *    coordinates: summed in double, divided by m once, rounded to fp32.  The sum's shape is fixed by
 *    the input alone: the cycle positions in (cycle, i) order, cut into pieces at the multiples of
 *    256 of that order and at the cycle boundaries; a piece that is a whole 256-block is summed by a
 *    fixed tree, any other piece left to right; a cycle's pieces, in order, by 64 strided partial sums
 *    and a fixed tree (the topology's shape).  No float atomics: the same bits on every call.
 *
 * build runs the checks, finds the loops, their status and the ordered cycles and keeps them in the
 * handle (replacing those of an earlier build); it synchronises `stream`.  h_stats may be NULL.
 * export copies status int32 [n_loops], cycle_loop int64 [n_capped] (the loop number of cycle k),
 * cycle_offsets int64 [n_capped + 1] and cycle_vertices int64 [n_cycle_indices]; any may be NULL.
 * caps writes the caps of the build held.  mode 0: n_capped polygons (d_cap_offsets, n_capped + 1)
 * over n_cycle_indices ids; d_xyz and d_new_xyz are unused.  mode 1: n_triangles +
 * (n_cycle_indices - 3 n_triangles) triangles (d_cap_offsets one more, d_cap_indices three each) and
 * n_capped - n_triangles new vertices (d_new_xyz, fp32 x 3 each); d_xyz: the V x 3 input
 * coordinates.  mode 1 synchronises `stream`. */
#define TNP_HOLE_CAPPED 0
#define TNP_HOLE_NONSIMPLE 1
#define TNP_HOLE_UNORIENTED 2
#define TNP_HOLE_TOO_LONG 3
typedef struct tnp_hole_stats {
  int64_t n_loops, n_capped, n_nonsimple, n_unoriented, n_too_long;
  int64_t n_cycle_indices;   /* sum of the capped loops' n_edges */
  int64_t n_triangles;       /* capped loops with 3 edges */
  int64_t longest_capped;    /* edges; 0 when none */
} tnp_hole_stats;
typedef struct tnp_holes tnp_holes;
int tnp_holes_create(tnp_holes** out, int device);
void tnp_holes_destroy(tnp_holes* h);
int tnp_holes_build(tnp_holes* h, int64_t V, const int64_t* d_offsets, const int64_t* d_indices,
                    int64_t P, int64_t max_edges, tnp_hole_stats* h_stats, void* stream);
int tnp_holes_export(tnp_holes* h, int32_t* d_status, int64_t* d_cycle_loop,
                     int64_t* d_cycle_offsets, int64_t* d_cycle_vertices, void* stream);
int tnp_holes_caps(tnp_holes* h, int mode, const float* d_xyz, int64_t* d_cap_offsets,
                   int64_t* d_cap_indices, float* d_new_xyz, void* stream);

/* Near-coincident vertices of a polygon soup welded, and the soup rewritten over the clusters'
 * representatives (csrc/weld.hip): the first stage of the repair chain, in front of keeping components
 * and capping holes.  Everything below is a function of the input alone: two calls give the same bits.
 *
 * Input.  The polygon soup of tnp_polygon_report, with the same checks, the same first-offender rule
 * and the same message texts (prefix "weld"); V and P must be below 2^31.  tol must be finite and >= 0,
 * mode 0 or 1 (-1 otherwise).  A used vertex with a coordinate that is not finite is refused (-1), the
 * message naming the smallest such id; an unused vertex may hold anything.  P = 0: all-zero stats, no
 * polygon, the identity map and the input's coordinate bits.
 *
 * Used vertices.  A vertex is used when its id occurs in d_indices.  Only used vertices take part: an
 * unused vertex maps to itself, keeps its coordinate bits and never bridges two used ones.
 *
 * Close pairs.  With the fp32 coordinates converted to double, dx = xi - xj (dy, dz likewise) and
 * d2 = dx dx + dy dy + dz dz, left to right, every difference, product and sum rounded exactly once
 * (no fused multiply-add), used vertices i and j are close iff d2 <= (double)tol (double)tol.
 * tol = 0 therefore welds bitwise-coincident positions, +0 being equal to -0.
 *
 * Clusters and the map.  A cluster is a class of the transitive closure of "close" (single linkage);
 * its representative is its smallest id, and map[v] is the representative of v's class.
 *
 * Positions.  mode 0 (first): every member takes its representative's fp32 coordinates (their bits).
 *  mode 1 (mean): every member of a class of m >= 2 takes the mean of the class's fp32 coordinates:
 *  summed in double over the members in ascending id, divided by m once, rounded to fp32 once; a class
 *  of one keeps its bits.  The sum's shape is the topology's: the used vertices in (representative, id)
 *  order, cut into pieces at the multiples of 256 of that order and at the class boundaries; a piece
 *  that is a whole 256-block is summed by a fixed tree, any other piece left to right; a class's pieces,
 *  in order, by 64 strided partial sums and a fixed tree.  No float atomics.
 *
 * Welded polygons.  Every id is replaced by map[id].  Position i of a polygon is kept iff its mapped id
 * differs from the mapped id of its cyclic predecessor (the last position is the first's).  A polygon
 * with fewer than 3 kept positions is dropped.  The survivors keep their order, their kept positions
 * theirs; source[k] is the input polygon of output polygon k.  A surviving polygon in which some id
 * still occurs twice (never consecutively) is pinched: it is kept and counted, and the soup checks
 * accept it.  Duplicate polygons are not removed.
 *
 * tnp_weld_stats: n_used; n_pairs, the close pairs i < j; n_clusters, the classes of >= 2 members;
 * n_merged = n_used - the number of classes; max_cluster, the largest class (1 when nothing welds);
 * n_polygons and n_indices of the output; n_dropped_polygons; n_pinched; max_shift, the largest
 * distance from a used vertex to its output position: sqrt(d2) by the rule above in double, rounded to
 * fp32, reduced by an integer maximum over the bit patterns.
 *
 * build runs the checks and keeps the result in the handle (replacing that of an earlier build); it
 * synchronises `stream`.  h_stats may be NULL.  export copies map int64 [V], the positions fp32 [V x 3],
 * offsets int64 [n_polygons + 1], indices int64 [n_indices] and source int64 [n_polygons]; any may be
 * NULL.
 *
 * Cost.  The pairs are proposed by a uniform grid of cell size h = max(tol (1 + 2^-10), largest extent
 * of the used vertices' box / 2^21) and decided by the predicate alone: a vertex meets the population of
 * its own and the 26 neighbouring cells, so a tolerance near the whole extent makes the search
 * O(n_used^2) -- correct, and slow.  The pinch test costs the sum of the squared output degrees. */
typedef struct tnp_weld_stats {
  int64_t n_used, n_pairs, n_clusters, n_merged, max_cluster;
  int64_t n_polygons, n_indices, n_dropped_polygons, n_pinched;
  float max_shift;
} tnp_weld_stats;
typedef struct tnp_weld tnp_weld;
int tnp_weld_create(tnp_weld** out, int device);
void tnp_weld_destroy(tnp_weld* w);
int tnp_weld_build(tnp_weld* w, const float* d_xyz, int64_t V, const int64_t* d_offsets,
                   const int64_t* d_indices, int64_t P, float tol, int mode, tnp_weld_stats* h_stats,
                   void* stream);
int tnp_weld_export(tnp_weld* w, int64_t* d_map, float* d_xyz_out, int64_t* d_offsets,
                    int64_t* d_indices, int64_t* d_source, void* stream);

/* The polygon surface simplified by vertex clustering (csrc/simplify.hip): the used vertices of a
 * polygon soup that share a cell of a uniform grid become one vertex, the soup is rewritten over the
 * cells' representatives and the duplicate polygons that makes are removed.  It sits in the repair
 * chain behind tnp_weld_* and in front of keeping components and capping holes, and is the budget
 * control of the surface: `cell` is the answer's resolution.  Everything below is a function of the
 * input alone: two calls give the same bits.
 *
 * Input.  The polygon soup of tnp_polygon_report, with the same checks, the same first-offender rule
 * and the same message texts (prefix "simplify"); V and P must be below 2^31.  cell must be finite and
 * > 0, mode 0 or 1 (-1 otherwise).  A used vertex with a coordinate that is not finite is refused (-1),
 * the message naming the smallest such id; an unused vertex may hold anything.  P = 0: all-zero stats,
 * no polygon, the identity map and the input's coordinate bits.
 *
 * Used vertices.  As tnp_weld_*: a vertex is used when its id occurs in d_indices.  Only used vertices
 * take part: an unused vertex maps to itself and keeps its coordinate bits.
 *
 * The grid.  lo is the per-axis minimum of the used vertices' fp32 coordinates, as double.  A vertex's
 * cell coordinate on an axis is floor(((double)x - lo) / (double)cell): one rounded difference, one
 * rounded quotient, no fused multiply-add.  An axis that needs more than 2^21 cells (the largest cell
 * coordinate on it + 1) is refused (-1), the message naming the axis and the count: nothing is clamped,
 * because here the cell is the answer.
 *
 * Classes and the map.  A class is the set of used vertices of one cell; its representative is its
 * smallest id, and map[v] is the representative of v's class.
 *
 * Positions.  mode 0 (mean): every member of a class of m >= 2 takes the mean of the class's fp32
 *  coordinates by exactly tnp_weld_*'s mode-1 rule: the used vertices in (representative, id) order, cut
 *  into pieces at the multiples of 256 of that order and at the class boundaries, the double sums in
 *  that fixed shape, one division by m, one rounding to fp32; a class of one keeps its bits.
 *  mode 1 (nearest): every member takes the coordinate bits of the member whose d2 to that fp32 mean is
 *  smallest, d2 being tnp_weld_*'s predicate arithmetic in double; ties go to the smallest id.  The
 *  output positions are then a subset of the input's.  No float atomics: the minimum is taken by integer
 *  atomics over the bit pattern of d2, then over the ids that reach it.
 *
 * Rewritten polygons.  tnp_weld_*'s rule, unchanged: every id is replaced by map[id]; a position is
 * kept iff its mapped id differs from that of its cyclic predecessor; a polygon with fewer than 3 kept
 * positions is dropped (n_dropped_polygons); a survivor in which an id still occurs twice is pinched.
 *
 * Duplicates.  A survivor's canonical form is the lexicographically smallest rotation of its id
 * sequence (pinched polygons included).  A survivor whose canonical form equals that of an earlier
 * survivor is a duplicate: it is removed and counted in n_duplicate_polygons.  A survivor that is not
 * a duplicate and whose reversed sequence has the canonical form of an earlier survivor is folded: it is
 * kept and counted in n_folded.  The comparison is exact, id by id; a 64-bit hash of the canonical form
 * only buckets the polygons, and no result depends on it.  The polygons that remain keep their order
 * and their ids as rewritten (not rotated); source[k] is the input polygon of output polygon k.
 *
 * tnp_simplify_stats: n_used; n_cells, the occupied cells = the classes; max_cell, the largest class;
 * n_polygons and n_indices of the output; n_dropped_polygons; n_duplicate_polygons; n_folded;
 * n_pinched, the pinched polygons of the output; max_shift as tnp_weld_*'s -- at most sqrt(3) cell
 * plus rounding, every member and the mean lying in one cell.
 *
 * build runs the checks and keeps the result in the handle (replacing that of an earlier build); it
 * synchronises `stream`.  h_stats may be NULL.  export copies map int64 [V], the positions fp32 [V x 3],
 * offsets int64 [n_polygons + 1], indices int64 [n_indices] and source int64 [n_polygons]; any may be
 * NULL.
 *
 * Cost.  One sort of the used vertices by cell key, one by (representative, id) when a class has two
 * members, one of the survivors by hash.  The canonical form costs a polygon its degree times the
 * occurrences of its smallest id; the duplicate search costs the sum over the runs of equal hash of the
 * squared run length times the degree -- a soup of n copies of one polygon is O(n^2), correct and slow.
 * The pinch test costs the sum of the squared degrees after the rewrite. */
typedef struct tnp_simplify_stats {
  int64_t n_used, n_cells, max_cell;
  int64_t n_polygons, n_indices, n_dropped_polygons, n_duplicate_polygons, n_folded, n_pinched;
  float max_shift;
} tnp_simplify_stats;
typedef struct tnp_simplify tnp_simplify;
int tnp_simplify_create(tnp_simplify** out, int device);
void tnp_simplify_destroy(tnp_simplify* h);
int tnp_simplify_build(tnp_simplify* h, const float* d_xyz, int64_t V, const int64_t* d_offsets,
                       const int64_t* d_indices, int64_t P, float cell, int mode,
                       tnp_simplify_stats* h_stats, void* stream);
int tnp_simplify_export(tnp_simplify* h, int64_t* d_map, float* d_xyz_out, int64_t* d_offsets,
                        int64_t* d_indices, int64_t* d_source, void* stream);

/* 1: subpoly_(..., force=False) -- the curve-approximation branch
 * (subpoly.py:120-177, 201-207; geometry.py:24-138, 259-299;
 * subpoly_debug.py:121-165, 234-271): new vertices of non-axis-aligned split
 * edges move to the intersection of the two trilinear level sets (largest
 * real root in [0,1] of the xz-plane quartic, gradient-descent fallback) and
 * the strict filter drops splits that miss their planes.  0: flat (default).
 * On x-slab shards the branch takes its whole-complex decisions through
 * the collective of tnp_engine_set_collective. */
int tnp_engine_set_curve(tnp_engine* eng, int on);

/* Collective for the decisions a sharded engine takes inside a step (the
 * curve branch: the curve rows' and descent rows' global counts, which pick
 * MKL's row-count schedules, the descent's stop iteration -- an AND over
 * the shards' per-iteration convergence words, subpoly_debug.py:141 -- and
 * the strict filter's "some kept c row misses its plane" flag,
 * subpoly_debug.py:253-257).  fn reduces n int64 words in place over the
 * shards (op: TNP_COLL_SUM, _MAX, _AND, _OR bitwise) and returns 0; the
 * engine calls it only with tnp_engine_set_shards(n > 1), every shard the
 * same calls in the same order.  fn == NULL: none (the branch then refuses
 * n > 1 shards).  Binds to the host language's all-reduce (the Python
 * driver: torch.distributed, tropical/_engine.py run_steps).  Every call
 * carries one word more than the decision it takes: the shard's failure
 * flag, so a shard that fails between two collectives still joins the next
 * one and every shard returns -1 from that same call (none waits on a
 * collective its peer never reaches). */
enum { TNP_COLL_SUM = 0, TNP_COLL_MAX = 1, TNP_COLL_AND = 2, TNP_COLL_OR = 3 };
typedef int (*tnp_collective_fn)(int64_t* vec, int n, int op, void* ctx);
int tnp_engine_set_collective(tnp_engine* eng, tnp_collective_fn fn, void* ctx);

/* Curve path: subpoly_(..., strict=...) (subpoly.py:198-203).  1 (default):
 * debug.strict_check drops splits that miss their planes
 * (subpoly_debug.py:234-271); 0: every split stays (the reference then only
 * prints a diagnostic). */
int tnp_engine_set_strict(tnp_engine* eng, int on);

/* Multi-GPU x-slabs, each extracted with a halo of cells on either side
 * (tropical/distributed.py; the halo width is the caller's, checked by
 * halo_check): this shard OWNS the mark planes
 * (lo, hi] (lo == 0: [0, hi]) and the cells between them; new vertices
 * outside (halo work, also computed by the neighbour that owns them) are
 * counted in tnp_step_stats.S_dup so the global split count counts each
 * split once.  lo > hi (default) = everything owned.  Flat path only. */
int tnp_engine_set_owned(tnp_engine* eng, int lo, int hi);
/* The same for a block of the mark grid (shards cut along several axes):
 * along axis d the shard owns the planes (lo[d], hi[d]] (plane 0 by the
 * shard with lo[d] == 0) and the cells between them; lo[d] > hi[d]: the
 * axis is not cut.  A vertex is owned iff it is owned along every cut axis. */
int tnp_engine_set_owned_box(tnp_engine* eng, const int32_t* lo, const int32_t* hi);

/* subpoly(net, d, size, eps) / subpoly_(..., eps, ...) with eps != Net.eps
 * (subpoly.py:24, 90): the following steps take the sign test, split point,
 * hit vertices and failover predicate at `eps` (subpoly.py:98-117, 233;
 * subpoly_debug.py:43), extract_skeleton and extract_faces too
 * (subpoly.py:556-606), while the region keys of the pair tests and the
 * pruning stay at Net.eps (Net.region without eps, subpoly.py:118, 184,
 * 256).  In this mode every cached plane is kept (first split planes come
 * from the plane values) and the pruning deletes edges lazily.  tnp_engine_set_net
 * resets it to Net.eps. */
int tnp_engine_set_eps(tnp_engine* eng, float eps);

/* The loaded complex lies between the x mark planes x0 and x1 (an x-slab
 * with its halo): the step's spatial buckets then cover only those cells.
 * tnp_engine_lattice sets it, tnp_engine_load / _skeleton reset it to the
 * whole grid (x1 < x0).  A vertex outside fails the step with an error.
 * Performance only: the results do not depend on it.  No reference
 * counterpart (multi-GPU sharding). */
int tnp_engine_set_xspan(tnp_engine* eng, int x0, int x1);
/* Per axis: the complex lies between the mark planes lo[d] and hi[d]
 * (hi[d] < lo[d]: anywhere along d) -- a block with its halo; x-slabs are
 * tnp_engine_set_xspan. */
int tnp_engine_set_span(tnp_engine* eng, const int32_t* lo, const int32_t* hi);

/* world > 1: this engine holds one x-slab of a complex sharded over `world`
 * devices.  A step the other shards split may leave this one without any
 * connecting pair; the reference's empty-torch.cat error (subpoly.py:505-513)
 * then only applies to the whole complex, not to a shard. */
int tnp_engine_set_shards(tnp_engine* eng, int world);

/* HIP-event timing of every engine kernel launch (on=1 clears and starts;
 * on=0 stops, synchronizes and aggregates per kernel name); read the
 * aggregates with tnp_engine_kernel_stat (ms, launches, modelled
 * algorithmic bytes). */
int tnp_engine_kernel_timer(tnp_engine* eng, int on, void* stream, int32_t* n_kernels);
int tnp_engine_kernel_stat(tnp_engine* eng, int i, char* name, int cap, double* ms,
                           int64_t* launches, double* bytes);

/* ---- single-node rank agreements (bench.py / tropical/distributed.py) ----
 * The per-step global decisions of the sharded loop (subpoly.py:110 "does
 * anything split", subpoly_debug.py:43-49 the failover override, and the OR
 * of the ranks' next-active plane masks) between the processes of ONE node
 * through a POSIX shared-memory segment: every rank writes <= 16 int64 words,
 * arrives on an atomic counter and spins until all have (no library
 * collective, no device copies).  Rank 0 creates the segment (create=1)
 * before the others open it; it can be unlinked once all have.  allreduce
 * op: TNP_SHM_MAX, TNP_SHM_OR (bitwise, 64-bit masks), TNP_SHM_SUM or
 * TNP_SHM_AND (bitwise). */
typedef struct tnp_shm tnp_shm;
enum { TNP_SHM_MAX = 0, TNP_SHM_OR = 1, TNP_SHM_SUM = 2, TNP_SHM_AND = 3 };
int tnp_shm_open(const char* name, int rank, int world, int create, tnp_shm** out);
int tnp_shm_unlink(const char* name);
void tnp_shm_close(tnp_shm* shm);
int tnp_shm_allreduce(tnp_shm* shm, const int64_t* in, int n, int op, int64_t* out);

/* ---- SDF training (train.py:169-224, dataset.py:80-96; csrc/train.hip) --
 * Gradient of one batch's loss (train.py:181-201) for the n points d_x
 * (n x 3 in [-1, 1]^3) with target distances d_gt (n):
 *   L = mean |clamp(sdf(x)) - clamp(gt)| + eik_w (||J||_F - 1)^2 / eik_batch,
 * clamp to [-clamp_t, clamp_t], sdf = tanh(o1 - o0) (model.py:84-87),
 * J = d sdf / d x (n x 3) -- the L1 and eikonal terms (eik_batch: the
 * reference's BATCH_SIZE constant, train.py:197, which equals n except for a
 * partial last batch; <= 0 takes n); the weight-norm term
 * (train.py:200-201) involves only the fc weights and is the caller's.  The
 * eikonal term's parameter gradient (the reference's double backward) is
 * written out in closed form.  ACCUMULATES into d_grad_table (the table's
 * own layout, params[(offset_l + idx) * 2 + f]) and d_grad_weights (the
 * packed weight layout of tnp_net); d_stats (2 doubles, device, zeroed by
 * the call) receives sum |clamp(sdf) - clamp(gt)| and sum ||J_i||^2.  Float
 * atomics: the summation order is not fixed.  Every instantiated net shape. */
int tnp_sdf_train_grad(const tnp_net* net, const float* d_x, const float* d_gt, int64_t n, float clamp_t,
                       float eik_w, int64_t eik_batch, float* d_grad_table, float* d_grad_weights,
                       double* d_stats, void* stream);

/* Autograd through Net.sdf (model.py:84-88): the vector-Jacobian product
 * sum_i d_gout[i] * d sdf(x_i) / d theta, ACCUMULATED into d_grad_table (the
 * table's own layout) and d_grad_weights (the packed weight layout) -- the
 * backward of a caller's net.sdf(x) w.r.t. the parameters (the input
 * gradient is tnp_sdf_grad's).  Float atomics; every instantiated net shape. */
int tnp_sdf_vjp(const tnp_net* net, const float* d_x, const float* d_gout, int64_t n, float* d_grad_table,
                float* d_grad_weights, void* stream);

/* Autograd through Net.normal(create_graph=True) (model.py:105-123: J =
 * d sdf / d x with a graph): the VJP sum_i d_gJ[i] . d J_i / d theta,
 * ACCUMULATED into d_grad_table / d_grad_weights, and (d_grad_x != null)
 * d_gJ[i] . d J_i / d x_i -- the Hessian of sdf along d_gJ[i] -- ACCUMULATED
 * into d_grad_x (n x 3).  Replaces the reference's double backward through
 * tcnn (train.py:196).  Float atomics. */
int tnp_normal_vjp(const tnp_net* net, const float* d_x, const float* d_gJ, int64_t n, float* d_grad_table,
                   float* d_grad_weights, float* d_grad_x, void* stream);

/* Autograd through Net.forward(x, gather=True) (model.py:52-76): upstream
 * gradients of the gathered planes (d_gpre, plane-major [K][ld] as
 * tnp_forward writes them: every hidden pre-activation, then o1 - o0) and
 * of the output (d_gout, n x 2); either may be null.  ACCUMULATES into
 * d_grad_table, d_grad_weights and (when given) d_grad_x (n x 3). */
int tnp_forward_vjp(const tnp_net* net, const float* d_x, int64_t n, const float* d_gpre, int64_t ld,
                    const float* d_gout, float* d_grad_table, float* d_grad_weights, float* d_grad_x, void* stream);

/* Signed distance of n points d_p (n x 3) to a closed triangle mesh (d_V
 * nV x 3 fp32, d_F nF x 3 int32, indices in [0, nV)): replaces
 * cubvh.cuBVH(V, F).signed_distance (dataset.py:77, 92).  Exact distance to
 * the closest triangle; the sign from the generalized winding number,
 * positive inside (dataset.py:96).  d_work: 2 n floats of scratch. */
int tnp_mesh_signed_distance(const float* d_V, int64_t nV, const int32_t* d_F, int64_t nF, const float* d_p,
                             int64_t n, float* d_work, float* d_dist, void* stream);

/* ---- `-e` evaluation stack (train.py:275-354; csrc/evaluate.hip) ------- */

/* Marching cubes over vol[n0][n1][n2] (x slowest), inside = value < iso,
 * case table int8 [256][16] (tropical/utils/mc_table.py).  Replaces
 * mcubes.marching_cubes (train.py:284).  Phase 1: d_eoff [3*n0*n1*n2 + 1]
 * int64 -> vertex id of every crossed lattice edge (point-major, axis
 * minor), d_coff [(n0-1)(n1-1)(n2-1) + 1] int64 -> first triangle of every
 * cube; returns the vertex and triangle counts.  Phase 2: vertices fp64
 * [n_verts][3] in index space (interpolated in double, as PyMCubes),
 * triangles int64 [n_tris][3]. */
int tnp_mc_count(const float* d_vol, int n0, int n1, int n2, float iso, const int8_t* d_table,
                 int64_t* d_eoff, int64_t* d_coff, int64_t* n_verts, int64_t* n_tris,
                 void* stream);
int tnp_mc_emit(const float* d_vol, int n0, int n1, int n2, float iso, const int8_t* d_table,
                const int64_t* d_eoff, const int64_t* d_coff, double* d_verts, int64_t* d_tris,
                void* stream);

/* Nearest-hit ray casting against a triangle mesh (replaces
 * cubvh.cuBVH(vertices, faces).ray_trace, chamfer_distance.py:184-212):
 * uniform-grid acceleration over the caller's bounding box; the mesh
 * buffers must outlive the caster.  cast: t (fp32, +inf on a miss) and face
 * id (-1 on a miss) per ray; rays are origins/directions fp32 [n][3]. */
typedef struct tnp_raycaster tnp_raycaster;
int tnp_raycaster_create(tnp_raycaster** out, int device);
void tnp_raycaster_destroy(tnp_raycaster* rc);
int tnp_raycaster_build(tnp_raycaster* rc, const float* d_V, int64_t nV, const int32_t* d_F,
                        int64_t nF, const float* bbox_lo, const float* bbox_hi, void* stream);
int tnp_raycaster_cast(tnp_raycaster* rc, const float* d_o, const float* d_d, int64_t nR,
                       float* d_t, int32_t* d_face, void* stream);

/* Exact nearest-neighbour L2 distance of every point of a [na][3] to the set
 * b [nb][3] (replaces sklearn NearestNeighbors in chamfer_distance.py:39-48). */
int tnp_nn_min_dist(const float* d_a, int64_t na, const float* d_b, int64_t nb, float* d_out,
                    void* stream);

/* ---- marching tetrahedra (tropical/utils/mtet.py; csrc/mtet.hip) -------- */

/* marching_tetrahedras(vertices fp32 [n_points][3], tets int64 [n_tets][4]
 * (16-byte aligned), sdf fp32 [n_points]) in three calls; the caller
 * allocates the outputs from the counts in between.  n_points < 2^31.
 * Inside is sdf > 0; a tet whose det[(b-a), (c-a), (d-a)] (double) is
 * negative has its first two ids swapped IN d_tets.
 *   classify: d_case uint8 [n_tets], d_tile int64 [3 * (tiles + 1) + 2] with
 *     tiles = ceil(n_tets / 256) (scanned per-tile counts, kept for the next
 *     two calls); returns the number of crossed-edge keys and of 1- and
 *     2-triangle tets.  Returns 1 when an id lies outside [0, n_points): such
 *     a tet is never gathered from.
 *   edges: d_keys uint64 [2 * n_keys]; leaves the unique crossed edges
 *     lo << nb | hi (nb = bits of n_points) sorted in d_keys[0, n_verts).
 *   emit: verts fp32 [n_verts][3], interp int64 [n_verts][2] (the edge ends,
 *     lo < hi, 16-byte aligned), faces int64 [n_one + 2 n_two][3] and tet_idx
 *     int64 [n_one + 2 n_two]: the 1-triangle tets in tet order, then the
 *     2-triangle tets in tet order.  Vertex i is the i-th edge in the
 *     lexicographic order of (lo, hi). */
int tnp_mt_classify(const float* d_vertices, const float* d_sdf, int64_t n_points, int64_t* d_tets,
                    int64_t n_tets, uint8_t* d_case, int64_t* d_tile, int64_t* n_keys,
                    int64_t* n_one, int64_t* n_two, void* stream);
int tnp_mt_edges(const int64_t* d_tets, int64_t n_tets, int64_t n_points, const uint8_t* d_case,
                 int64_t* d_tile, int64_t n_keys, uint64_t* d_keys, int64_t* n_verts, void* stream);
int tnp_mt_emit(const float* d_vertices, const float* d_sdf, int64_t n_points, const int64_t* d_tets,
                int64_t n_tets, const uint8_t* d_case, const int64_t* d_tile, const uint64_t* d_keys,
                int64_t n_verts, int64_t n_one, float* d_verts, int64_t* d_interp, int64_t* d_faces,
                int64_t* d_tet_idx, void* stream);

/* ---- rasteriser (tropical/utils/render.py; csrc/render.hip) --------------
 * Replaces the matplotlib plot_trisurf figures of tropical/stanford/visualize.py:13-67 (a CPU
 * painter's algorithm) by an exact integer z-buffer rasteriser that also draws polygon boundaries.
 *
 * Input: the polygon soup of tnp_polygon_report -- d_xyz (V x 3 fp32), d_offsets (int64, P + 1),
 * d_indices (int64); a triangle mesh is offsets 0, 3, 6, ...  Polygon p is drawn as its fan
 * (p0, p[t+1], p[t+2]), t = 0 .. deg - 3; fan triangles are numbered polygon-major (triangle number
 * T = sum of (deg - 2) over the polygons before p, plus t).  Checked on the device before anything is
 * read through an id, with tnp_polygon_report's checks and its first-offender rule; V and the
 * triangle count must be below 2^31.  P = 0 is valid: an all-background image.
 *
 * Projection (one thread per vertex, fp32, every operation rounded to nearest in the stated order):
 *   d = p - center;  c_r = (right0 d0 + right1 d1) + right2 d2, likewise c_u (up), c_t (toward).
 *   s = 1 (persp_dist D = 0, orthographic) or D / (D - c_t)  (D > 0, perspective).
 *   sx = round((W / 2 + (scale s) c_r) 16),  sy = round((H / 2 - (scale s) c_u) 16)
 *     in 1/16-pixel units, row 0 at the top (round: to nearest, ties to even).
 *   sz = floor(((1 - q) / 2) 2^20) clamped to [0, 2^20 - 1]; a smaller sz is nearer the viewer.
 *     Orthographic: q = c_t / h (h = depth_half).  Perspective: q is s mapped affinely so that
 *     c_t = -h, +h give -1, +1, evaluated as q = (c_t D - h h) / (h (D - c_t)); s is linear in
 *     screen space, so plain interpolation of sz over a triangle is exact.
 *   A vertex is FLAGGED when |sx| or |sy| exceeds 2^18 (or is not a number), q lies outside
 *   [-1, 1], or, under perspective, c_t >= D.  Every polygon that uses a flagged vertex is dropped
 *   and counted; there is no clipping stage.  d_screen (V x 3 int32, may be NULL) receives
 *   (sx, sy, sz), and (0, 0, -1) for a flagged vertex.
 *
 * Coverage and depth are integer: the result depends neither on launch order nor on rounding.
 *   e(a, b, p) = (b.x - a.x)(p.y - a.y) - (b.y - a.y)(p.x - a.x) in int64.
 *   A2 = e(v0, v1, v2); A2 < 0: v1 and v2 are swapped; A2 = 0: the triangle draws nothing.
 *   Pixel (i, j) (column i, row j) has centre p = (16 i + 8, 16 j + 8).
 *   w0 = e(v1, v2, p), w1 = e(v2, v0, p), w2 = e(v0, v1, p).  The pixel is covered iff for every k
 *   w_k > 0, or w_k = 0 and the edge a -> b of w_k, d = b - a, owns its points: d.y > 0, or
 *   d.y = 0 and d.x < 0.  (Two triangles sharing an edge never both cover, or both miss, a centre
 *   on it.)  Depth z = (w0 z0 + w1 z1 + w2 z2) // A2 (every product stays below 2^60).
 *   Visibility: one 64-bit atomic minimum of (z << 32) | T per covered pixel, background all ones:
 *   the nearest wins, ties go to the lowest triangle number; no back-face culling.
 *   Two coverage paths with identical results: a triangle whose bounding box of pixel centres,
 *   clamped to the image, is at most TNP_RENDER_SMALL_MAX pixels wide and high is drawn by one
 *   thread; the others are compacted into a list (scan.hip) and drawn a workgroup per triangle,
 *   16 x 16-pixel tiles of the clamped box, a tile skipped when an edge excludes all of it.
 *
 * Resolve (one thread per pixel): d_prim (int32 H x W) the winning polygon id, -1 background;
 *   d_tri (int32 H x W, may be NULL) the winning triangle number T, -1 background; d_edge (uint8
 *   H x W, may be NULL) 1 iff the pixel centre lies within edge_half_width (1/16 px, 0 .. 256) of a
 *   polygon-boundary edge a -> b of the winning triangle: |e(a, b, p)| <= edge_half_width
 *   isqrt(|b - a|^2), isqrt the exact integer square root.  The boundary edges of fan triangle t
 *   are (p[t+1], p[t+2]) always, (p0, p1) when t = 0 and (p[deg-1], p0) when t = deg - 3; fan
 *   diagonals are never edges.  Background pixels have edge 0.
 * h_stats (host): polygons drawn / dropped (a flagged vertex) / degenerate (not dropped, every fan
 *   triangle has A2 = 0), fan triangles, those sent down the workgroup path, pixels covered.
 * Synchronises `stream`. */
#define TNP_RENDER_SMALL_MAX 8
typedef struct tnp_render_view {
  float right[3], up[3], toward[3]; /* rotation rows; toward points at the viewer */
  float center[3];
  float scale;        /* pixels per world unit */
  float persp_dist;   /* D; 0: orthographic */
  float depth_half;   /* h > 0 */
  int32_t width, height; /* the raster, 1 .. 8192 each */
} tnp_render_view;
typedef struct tnp_render_stats {
  int64_t n_polygons, n_drawn, n_dropped, n_degenerate;
  int64_t n_triangles, n_large, pixels_covered;
} tnp_render_stats;
int tnp_render_raster(const float* d_xyz, int64_t V, const int64_t* d_offsets, const int64_t* d_indices,
                      int64_t P, const tnp_render_view* view, int32_t edge_half_width, int32_t* d_screen,
                      int32_t* d_prim, int32_t* d_tri, uint8_t* d_edge, tnp_render_stats* h_stats,
                      void* stream);

/* Shade: d_prim / d_edge (nullable) of a width x height raster -> RGBA8 (height / ss) x (width / ss),
 * ss in {1, 2, 4} dividing both.  Per raster pixel: background (id outside [0, P)) is (0, 0, 0, 0);
 * an edge pixel takes edge_rgba (4 bytes, host); else (lut[k], 255) with d_lut 256 x 3 uint8 and
 * k = clamp(floor((v - vmin) / (vmax - vmin) 255 + 0.5), 0, 255) in fp32, each operation rounded to
 * nearest in that order, v = d_value[id] (P floats; not a number: k = 0); vmax > vmin.  Each
 * ss x ss block is then averaged per channel as (sum + n / 2) // n, n = ss ss, in integers. */
int tnp_render_shade(const int32_t* d_prim, const uint8_t* d_edge, int32_t width, int32_t height,
                     const float* d_value, int64_t P, float vmin, float vmax, const uint8_t* d_lut,
                     const uint8_t* edge_rgba, int32_t ss, uint8_t* d_rgba, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TROPICAL_HIP_H */
