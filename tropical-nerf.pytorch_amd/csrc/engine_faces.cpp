// Host side of extract_faces and the polygon export (kernels in faces.hip).
#include "engine.h"
#include "faces.h"

using namespace tnp_host;

// ---------------------------------------------------------------------------
// extract_faces (subpoly.py:584-728) on the current complex
// ---------------------------------------------------------------------------
enum { FS_TABLE, FS_CNT, FS_KC, FS_KF, FS_MEMOFF, FS_RID, FS_MEM, FS_CUR, FS_ROFF, FS_RCNT,
       FS_BCNT, FS_BOFF, FS_BCUR, FS_ROWS, FS_KEEP, FS_KOFF, FS_FROW, FS_MEAN, FS_NRM, FS_SDF,
       FS_KEY, FS_ORDV, FS_CALL, FS_CNZ, FS_HIST, FS_BASE, FS_POFF, FS_PIDX, FS_N };

// F1-F4: the final rows of extract_faces on the current complex.  Leaves, for
// rows_F rows, the row list (FS_FROW), every row's members in angular order
// (FS_ORDV at FS_ROFF of its row), their count (FS_CALL; FS_CNZ: those off
// the origin) and the normal that ordered them (FS_NRM) in the face scratch,
// and sets rows_valid: tnp_engine_faces (F5) and tnp_engine_polygons (F6)
// both emit from them.
static int faces_rows(tnp_engine* e, hipStream_t s) {
  e->rows_valid = e->poly_valid = false;
  e->rows_F = e->rows_maxc = e->rows_maxnz = 0;
  if (compact_now(e, s)) return -1;
  static_assert(FS_N <= 32, "face scratch slots");
  Buf* fs = e->fscr2;
  const int64_t V = e->V;
  const int K = e->K;
  if (V == 0) { e->rows_valid = true; return 0; }
  if (e->net.n_marks + 2 >= 1024) {
    tnp_set_error("faces: region keys hold n_marks + 2 < 1024 cells per axis");
    return -1;
  }
  int64_t* ctr = P<int64_t>(e->ctr);
  const uint64_t* pos = VP(e->cur, e->kw);
  const uint64_t* zero = VZ(e->cur, e->kw);
  const uint64_t* grid = P<uint64_t>(e->cur.grid);
  const float* xyz = P<float>(e->cur.xyz);
  if (eps2(e)) {
    // extract_faces takes the regions at subpoly's eps (net.region(vertices,
    // outputs, eps), subpoly.py:606): keys of every plane from the cache
    if (e->valid_from != 0) { tnp_set_error("split-eps faces: cached planes were dropped"); return -1; }
    // kse_pz: the keys at subpoly's eps, (pos, zero) interleaved as pz; kse_grid: grid words
    if (buf_ensure(e->kse_pz, V * sizeof(uint64_t) * 2 * e->kw, s)) return -1;
    if (buf_ensure(e->kse_grid, V * sizeof(uint64_t), s)) return -1;
    NetDev ns = e->net;
    ns.eps = ns.eps_s;
    if (launch_keys(ns, xyz, P<float>(e->cur.pre), e->cur.cap, V, K, P<uint64_t>(e->kse_pz),
                    P<uint64_t>(e->kse_pz) + e->kw, P<uint64_t>(e->kse_grid), s, P<uint64_t>(e->kse_pz)))
      return -1;
    pos = P<uint64_t>(e->kse_pz);
    zero = P<uint64_t>(e->kse_pz) + e->kw;
    grid = P<uint64_t>(e->kse_grid);
  }
  TNP_CHECK(hipMemsetAsync(ctr, 0, CTR_CLEAR_BYTES, s));
  // F1: augmented-row count and region hash table
  TIMED("faces_count", 24.0 * V,
        launch_face_count(V, grid, pos, zero, K, ctr + CTR_AUX - 1, s));
  if (read_ctr(e, s)) return -1;
  const int64_t A = e->h_ctr[CTR_AUX - 1];
  if (e->h_ctr[CTR_AUX] > 30) { tnp_set_error("faces: a vertex lies on %lld planes", (long long)e->h_ctr[CTR_AUX]); return -1; }
  int64_t cap = 1024;
  while (cap < 2 * A) cap <<= 1;
  // region table: cap sign words + cap cell words (faces.hip probe_insert);
  // two-word keys: cap cell words + 2 cap sign words + cap ready words
  if (buf_ensure(fs[FS_TABLE], cap * 16 * e->kw, s) || buf_ensure(fs[FS_CNT], cap * 4, s) ||
      buf_ensure(fs[FS_KC], cap * 4, s) || buf_ensure(fs[FS_KF], cap * 4, s) ||
      buf_ensure(fs[FS_MEMOFF], cap * 8, s) || buf_ensure(fs[FS_RID], cap * 8, s) ||
      buf_ensure(fs[FS_CUR], cap * 4, s))
    return -1;
  if (e->kw == 1) {  // EMPTY signs, NO_CELL, counts, cursors: one dispatch
    const FillOp f[4] = {{fs[FS_TABLE].p, (uint64_t)cap * 8, 0xFF},
                         {static_cast<char*>(fs[FS_TABLE].p) + cap * 8, (uint64_t)cap * 8, 0},
                         {fs[FS_CNT].p, (uint64_t)cap * 4, 0},
                         {fs[FS_CUR].p, (uint64_t)cap * 4, 0}};
    if (launch_fill(f, 4, s)) return -1;
  } else {  // NO_CELL claim words and not-ready words (the sign words are written before use)
    const FillOp f[4] = {{fs[FS_TABLE].p, (uint64_t)cap * 8, 0},
                         {static_cast<char*>(fs[FS_TABLE].p) + cap * 24, (uint64_t)cap * 8, 0},
                         {fs[FS_CNT].p, (uint64_t)cap * 4, 0},
                         {fs[FS_CUR].p, (uint64_t)cap * 4, 0}};
    if (launch_fill(f, 4, s)) return -1;
  }
  TIMED("faces_insert", 24.0 * V + 16.0 * cap,
        launch_face_insert(V, grid, pos, zero, K, P<uint64_t>(fs[FS_TABLE]), (uint64_t)cap - 1,
                         P<int32_t>(fs[FS_CNT]), s));
  TIMED("faces_keep_counts", 12.0 * cap,
        launch_keep_counts(P<int32_t>(fs[FS_CNT]), cap, P<int32_t>(fs[FS_KC]), P<int32_t>(fs[FS_KF]), s));
  // padded width of r_idx_as_tensor = the largest region over ALL regions
  {
    const FillOp f{ctr + CTR_COMPAT, sizeof(int64_t), 0};
    if (launch_fill(&f, 1, s)) return -1;
  }
  TIMED("faces_width", 4.0 * cap,
        launch_max_i32(P<int32_t>(fs[FS_CNT]), cap, ctr + CTR_COMPAT, s));
  if (scan_counts(e, P<int32_t>(fs[FS_KC]), P<int64_t>(fs[FS_MEMOFF]), cap, CTR_T, s)) return -1;
  if (scan_counts(e, P<int32_t>(fs[FS_KF]), P<int64_t>(fs[FS_RID]), cap, CTR_X, s)) return -1;
  if (read_ctr(e, s)) return -1;
  const int64_t Mtot = e->h_ctr[CTR_T], R = e->h_ctr[CTR_X];
  const int width = (int)e->h_ctr[CTR_COMPAT];
  if (width > (1 << 16)) {
    tnp_set_error("faces: a region with %d vertices (degenerate complex)", width);
    return -1;
  }
  if (R == 0) { e->rows_valid = true; return 0; }
  // F2: member lists (k, v)-sorted
  if (buf_ensure(fs[FS_MEM], Mtot * 8, s) || buf_ensure(fs[FS_ROFF], R * 8, s) ||
      buf_ensure(fs[FS_RCNT], R * 4, s))
    return -1;
  TIMED("faces_scatter", 24.0 * V + 8.0 * Mtot,
        launch_face_scatter(V, grid, pos, zero, K, P<uint64_t>(fs[FS_TABLE]), (uint64_t)cap - 1,
                          P<int32_t>(fs[FS_CNT]), P<int64_t>(fs[FS_MEMOFF]), P<int32_t>(fs[FS_CUR]),
                          P<uint64_t>(fs[FS_MEM]), s));
  TIMED("faces_regions", 16.0 * cap + 12.0 * R,
        launch_region_finalize(cap, P<int32_t>(fs[FS_KF]), P<int64_t>(fs[FS_RID]), P<int32_t>(fs[FS_CNT]),
                             P<int64_t>(fs[FS_MEMOFF]), P<uint64_t>(fs[FS_MEM]), P<int64_t>(fs[FS_ROFF]),
                             P<int32_t>(fs[FS_RCNT]), s));
  // F3: lexicographic row order + unique
  if (buf_ensure(fs[FS_BCNT], V * 4, s) || buf_ensure(fs[FS_BOFF], V * 8, s) ||
      buf_ensure(fs[FS_BCUR], V * 4, s) || buf_ensure(fs[FS_ROWS], R * 4, s) ||
      buf_ensure(fs[FS_KEEP], R * 4, s) || buf_ensure(fs[FS_KOFF], R * 8, s))
    return -1;
  {
    const FillOp f[2] = {{fs[FS_BCNT].p, (uint64_t)V * 4, 0}, {fs[FS_BCUR].p, (uint64_t)V * 4, 0}};
    if (launch_fill(f, 2, s)) return -1;
  }
  const uint64_t* mem = P<uint64_t>(fs[FS_MEM]);
  const int64_t* roff = P<int64_t>(fs[FS_ROFF]);
  const int32_t* rcnt = P<int32_t>(fs[FS_RCNT]);
  TIMED("faces_row_count", 8.0 * Mtot + 12.0 * R,
        launch_row_buckets(R, V, mem, roff, rcnt, P<int32_t>(fs[FS_BCNT]), nullptr, nullptr, nullptr, nullptr, 0, s));
  if (scan_counts(e, P<int32_t>(fs[FS_BCNT]), P<int64_t>(fs[FS_BOFF]), V, CTR_AUX, s)) return -1;
  TIMED("faces_row_place", 8.0 * Mtot + 16.0 * R,
        launch_row_buckets(R, V, mem, roff, rcnt, nullptr, P<int64_t>(fs[FS_BOFF]), P<int32_t>(fs[FS_BCUR]),
                         P<int32_t>(fs[FS_ROWS]), nullptr, 1, s));
  TIMED("faces_row_unique", 8.0 * Mtot + 16.0 * R,
        launch_row_buckets(R, V, mem, roff, rcnt, P<int32_t>(fs[FS_BCNT]), P<int64_t>(fs[FS_BOFF]), nullptr,
                         P<int32_t>(fs[FS_ROWS]), P<int32_t>(fs[FS_KEEP]), 2, s));
  if (scan_counts(e, P<int32_t>(fs[FS_KEEP]), P<int64_t>(fs[FS_KOFF]), R, CTR_E, s)) return -1;
  if (read_ctr(e, s)) return -1;
  const int64_t F = e->h_ctr[CTR_E];
  if (buf_ensure(fs[FS_FROW], F * 4, s) || buf_ensure(fs[FS_MEAN], F * 12, s) ||
      buf_ensure(fs[FS_NRM], F * 12, s) || buf_ensure(fs[FS_SDF], F * 4, s) ||
      buf_ensure(fs[FS_KEY], row_order_scratch(F, width), s) || buf_ensure(fs[FS_ORDV], Mtot * 4, s) ||
      buf_ensure(fs[FS_CALL], F * 4, s) || buf_ensure(fs[FS_CNZ], F * 4, s))
    return -1;
  TIMED("faces_compact_rows", 16.0 * R,
        launch_compact_rows(R, P<int32_t>(fs[FS_KEEP]), P<int64_t>(fs[FS_KOFF]), P<int32_t>(fs[FS_ROWS]),
                          P<int32_t>(fs[FS_FROW]), s));
  const int32_t* frow = P<int32_t>(fs[FS_FROW]);
  e->dbg_F = F;
  e->dbg_W = width;
  // F4: normals at the row means, angular order
  TIMED("faces_row_mean", 20.0 * Mtot + 12.0 * F,
        launch_row_mean(F, frow, mem, roff, rcnt, width, xyz, P<float>(fs[FS_MEAN]), s));
  TIMED("faces_normals", 28.0 * F,
        launch_sdf_grad(e->net, P<float>(fs[FS_MEAN]), F, P<float>(fs[FS_SDF]), P<float>(fs[FS_NRM]), s));
  TIMED("faces_row_order", 20.0 * Mtot + 12.0 * F,
        launch_row_order(F, frow, mem, roff, rcnt, width, xyz, P<float>(fs[FS_NRM]), F == 3 ? 1 : 0,
                       fs[FS_KEY].p, P<int32_t>(fs[FS_ORDV]), P<int32_t>(fs[FS_CALL]),
                       P<int32_t>(fs[FS_CNZ]), s));
  {
    const FillOp f{ctr + CTR_TRI, 2 * sizeof(int64_t), 0};
    if (launch_fill(&f, 1, s)) return -1;
  }
  TIMED("faces_fan_width", 8.0 * F,
        launch_max_i32(P<int32_t>(fs[FS_CALL]), F, ctr + CTR_TRI, s, P<int32_t>(fs[FS_CNZ]), ctr + CTR_FACES));
  if (read_ctr(e, s)) return -1;
  e->rows_F = F;
  e->rows_maxc = e->h_ctr[CTR_TRI];
  e->rows_maxnz = e->h_ctr[CTR_FACES];
  e->rows_valid = true;
  return 0;
}

extern "C" int tnp_engine_faces(tnp_engine* e, void* stream, int64_t* n_tri, int64_t* n_faces) {
  hipStream_t s = (hipStream_t)stream;
  TNP_CHECK(hipSetDevice(e->device));
  e->n_tri = e->n_faces = 0;
  *n_tri = *n_faces = 0;
  if (require_valid(e, "faces")) return -1;
  if (faces_rows(e, s)) return -1;
  Buf* fs = e->fscr2;
  const int64_t F = e->rows_F;
  if (F == 0) return 0;
  const int32_t* frow = P<int32_t>(fs[FS_FROW]);
  const int64_t* roff = P<int64_t>(fs[FS_ROFF]);
  const int32_t* rcnt = P<int32_t>(fs[FS_RCNT]);
  const float* xyz = P<float>(e->cur.xyz);
  // F5: fan triangles, fan-position-major
  const int64_t nb = fan_blocks(F);
  for (int floats = 0; floats < 2; ++floats) {
    const int32_t* cnt = P<int32_t>(fs[floats ? FS_CNZ : FS_CALL]);
    int T = (int)(floats ? e->rows_maxnz : e->rows_maxc) - 2;
    if (T <= 0) continue;
    if (buf_ensure(fs[FS_HIST], (int64_t)T * nb * 4, s) || buf_ensure(fs[FS_BASE], (int64_t)T * nb * 8, s))
      return -1;
    TIMED("faces_fan_hist", 4.0 * F,
        launch_fan_hist(F, cnt, T, P<int32_t>(fs[FS_HIST]), s));
    if (scan_counts(e, P<int32_t>(fs[FS_HIST]), P<int64_t>(fs[FS_BASE]), (int64_t)T * nb, CTR_AUX, s)) return -1;
    if (read_ctr(e, s)) return -1;
    int64_t n = e->h_ctr[CTR_AUX];
    if (floats) {
      if (buf_ensure(e->faces, std::max<int64_t>(n, 1) * 9 * sizeof(float), s)) return -1;
      e->n_faces = n;
    } else {
      if (buf_ensure(e->tri, std::max<int64_t>(n, 1) * 3 * sizeof(int64_t), s)) return -1;
      e->n_tri = n;
    }
    TIMED("faces_fan_emit", (floats ? 36.0 : 24.0) * n + 8.0 * F,
        launch_fan_emit(F, frow, P<int32_t>(fs[FS_ORDV]), roff, rcnt, cnt, T, P<int64_t>(fs[FS_BASE]), floats,
                        xyz, P<int64_t>(e->tri), P<float>(e->faces), s));
  }
  TNP_CHECK(hipStreamSynchronize(s));
  *n_tri = e->n_tri;
  *n_faces = e->n_faces;
  return 0;
}

extern "C" int tnp_engine_faces_export(tnp_engine* e, int64_t* d_tri, float* d_faces, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  TNP_CHECK(hipSetDevice(e->device));
  if (d_tri && e->n_tri > 0)
    TNP_CHECK(hipMemcpyAsync(d_tri, e->tri.p, e->n_tri * 3 * sizeof(int64_t), hipMemcpyDefault, s));
  if (d_faces && e->n_faces > 0)  // (device or pinned host destinations: one DMA each)
    TNP_CHECK(hipMemcpyAsync(d_faces, e->faces.p, e->n_faces * 9 * sizeof(float), hipMemcpyDefault, s));
  return 0;
}

// The final rows as polygons (F6).  Every final row is a polygon: a row has
// >= 3 members (k_keep_counts drops smaller regions before any row exists)
// and a region's members are distinct vertices, so the de-duplication and the
// < 3 filter of tensor_to_triangle_faces never remove anything -- polygon f is
// row f, and FS_NRM (one normal per row) is already the [P, 3] normal array.
extern "C" int tnp_engine_polygons(tnp_engine* e, void* stream, int64_t* n_poly, int64_t* n_idx) {
  hipStream_t s = (hipStream_t)stream;
  TNP_CHECK(hipSetDevice(e->device));
  e->n_poly = e->n_pidx = 0;
  e->poly_valid = false;
  *n_poly = *n_idx = 0;
  if (require_valid(e, "polygons")) return -1;
  if (!e->rows_valid && faces_rows(e, s)) return -1;
  Buf* fs = e->fscr2;
  const int64_t F = e->rows_F;
  if (buf_ensure(fs[FS_POFF], (F + 1) * sizeof(int64_t), s)) return -1;
  if (F == 0) {  // offsets [0]
    TNP_CHECK(hipMemsetAsync(fs[FS_POFF].p, 0, sizeof(int64_t), s));
    TNP_CHECK(hipStreamSynchronize(s));
    e->poly_valid = true;
    return 0;
  }
  if (scan_counts(e, P<int32_t>(fs[FS_CALL]), P<int64_t>(fs[FS_POFF]), F, CTR_AUX, s)) return -1;
  if (read_ctr(e, s)) return -1;
  const int64_t n = e->h_ctr[CTR_AUX];
  if (buf_ensure(fs[FS_PIDX], std::max<int64_t>(n, 1) * sizeof(int64_t), s)) return -1;
  // 4 n member ids in, 8 n indices + 8 F offsets out; the search's offset and
  // row-start reads hit the cache (8 F + 12 F bytes from memory once)
  TIMED("faces_poly_emit", 12.0 * n + 28.0 * F,
        launch_poly_emit(n, F, P<int64_t>(fs[FS_POFF]), P<int32_t>(fs[FS_FROW]), P<int64_t>(fs[FS_ROFF]),
                         P<int32_t>(fs[FS_ORDV]), P<int64_t>(fs[FS_PIDX]), s));
  TNP_CHECK(hipStreamSynchronize(s));
  e->n_poly = *n_poly = F;
  e->n_pidx = *n_idx = n;
  e->poly_valid = true;
  return 0;
}

extern "C" int tnp_engine_polygons_export(tnp_engine* e, int64_t* d_offsets, int64_t* d_indices, float* d_normals,
                                          void* stream) {
  hipStream_t s = (hipStream_t)stream;
  TNP_CHECK(hipSetDevice(e->device));
  Buf* fs = e->fscr2;
  if (!e->poly_valid) {
    tnp_set_error("polygons_export: no polygons in the engine (call tnp_engine_polygons; a later "
                  "tnp_engine_faces or another complex replaces them)");
    return -1;
  }
  if (d_offsets)
    TNP_CHECK(hipMemcpyAsync(d_offsets, fs[FS_POFF].p, (e->n_poly + 1) * sizeof(int64_t), hipMemcpyDefault, s));
  if (d_indices && e->n_pidx > 0)
    TNP_CHECK(hipMemcpyAsync(d_indices, fs[FS_PIDX].p, e->n_pidx * sizeof(int64_t), hipMemcpyDefault, s));
  if (d_normals && e->n_poly > 0)
    TNP_CHECK(hipMemcpyAsync(d_normals, fs[FS_NRM].p, e->n_poly * 3 * sizeof(float), hipMemcpyDefault, s));
  return 0;
}

// debugging aid: the padded angular scores of the last tnp_engine_faces call
// (F x width fp32, final-row order); returns F and width
extern "C" int tnp_engine_faces_debug(tnp_engine* e, float* d_scores, int64_t cap, int64_t* F, int64_t* width,
                                      void* stream) {
  hipStream_t s = (hipStream_t)stream;
  *F = e->dbg_F;
  *width = e->dbg_W;
  int64_t n = e->dbg_F * e->dbg_W;
  if (d_scores && n > 0 && n <= cap)
    TNP_CHECK(hipMemcpyAsync(d_scores, e->fscr2[FS_KEY].p, n * sizeof(float), hipMemcpyDeviceToDevice, s));
  return 0;
}
