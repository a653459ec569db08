// The complexes the engine builds itself: the lattice over the marks (its two
// kernels are here) and the skeleton (kernels in skeleton.hip).
#include "engine.h"
#include "skeleton.h"

using namespace tnp_host;

// ---------------------------------------------------------------------------
// full lattice over the marks, box [lo, hi] of mark indices per axis
// (tropical.py:103-109 layout: x-edges, then y, then z, each (hi, lo),
// meshgrid-ij order; the whole grid is the reference's lattice, an x-slab or
// a block of a sharded one keeps the same order within the box)
// ---------------------------------------------------------------------------
namespace {
__global__ void k_lattice_vertices(const float* __restrict__ marks, int x0, int y0, int z0, int nx, int ny,
                                   int nz, float* __restrict__ xyz) {
  int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t nv = (int64_t)nx * ny * nz;
  if (v >= nv) return;
  int k = (int)(v % nz) + z0, j = (int)((v / nz) % ny) + y0, i = (int)(v / ((int64_t)ny * nz)) + x0;
  // preprocess_inverse: x * 2 - 1 (model.py:81-82)
  xyz[3 * v + 0] = __fsub_rn(__fmul_rn(marks[i], 2.0f), 1.0f);
  xyz[3 * v + 1] = __fsub_rn(__fmul_rn(marks[j], 2.0f), 1.0f);
  xyz[3 * v + 2] = __fsub_rn(__fmul_rn(marks[k], 2.0f), 1.0f);
}
__global__ void k_lattice_edges(int nx, int ny, int nz, int32_t* __restrict__ edges) {
  const int64_t NN = (int64_t)ny * nz;
  const int64_t ex = (int64_t)(nx - 1) * NN;
  const int64_t ey = (int64_t)nx * (ny - 1) * nz;
  const int64_t ez = (int64_t)nx * ny * (nz - 1);
  int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t lo, hi;
  if (e < ex) {
    lo = e;
    hi = e + NN;
  } else if (e < ex + ey) {
    int64_t r = e - ex;  // shape (nx, ny-1, nz)
    int64_t k = r % nz, j = (r / nz) % (ny - 1), i = r / ((int64_t)(ny - 1) * nz);
    lo = i * NN + j * nz + k;
    hi = lo + nz;
  } else if (e < ex + ey + ez) {
    int64_t r = e - ex - ey;  // shape (nx, ny, nz-1)
    int64_t k = r % (nz - 1), j = (r / (nz - 1)) % ny, i = r / ((int64_t)ny * (nz - 1));
    lo = i * NN + j * nz + k;
    hi = lo + 1;
  } else {
    return;
  }
  edges[2 * e] = (int32_t)hi;
  edges[2 * e + 1] = (int32_t)lo;
}
}  // namespace

extern "C" int tnp_engine_lattice_box(tnp_engine* e, const int32_t* lo3, const int32_t* hi3, int keep_all,
                                      void* stream, int64_t* V_out, int64_t* E_out) {
  hipStream_t s = (hipStream_t)stream;
  e->rows_valid = false;
  if (!e->has_net) { tnp_set_error("engine has no net"); return -1; }
  TNP_CHECK(hipSetDevice(e->device));
  const int N = e->net.n_marks;
  int n[3];
  for (int d = 0; d < 3; ++d) {
    if (lo3[d] < 0 || hi3[d] >= N || hi3[d] < lo3[d]) {
      tnp_set_error("bad lattice box: axis %d marks [%d, %d] of %d", d, lo3[d], hi3[d], N);
      return -1;
    }
    n[d] = hi3[d] - lo3[d] + 1;
    e->sp_lo[d] = lo3[d];
    e->sp_hi[d] = hi3[d];
  }
  const int64_t V = (int64_t)n[0] * n[1] * n[2];
  const int64_t E = (int64_t)(n[0] - 1) * n[1] * n[2] + (int64_t)n[0] * (n[1] - 1) * n[2] +
                    (int64_t)n[0] * n[1] * (n[2] - 1);
  if (V >= (1LL << 31) || E >= (1LL << 31)) { tnp_set_error("lattice too large for int32 ids"); return -1; }
  if (buf_ensure(e->ctr, CTR_CLEAR_BYTES, s)) return -1;
  if (vset_ensure(e, e->cur, V, 0, s)) return -1;
  if (buf_ensure(e->edges, std::max<int64_t>(E, 1) * 2 * sizeof(int32_t), s)) return -1;
  hipLaunchKernelGGL(k_lattice_vertices, dim3(tnp_grid(V)), dim3(TNP_BLOCK), 0, s, e->net.marks, lo3[0], lo3[1],
                     lo3[2], n[0], n[1], n[2], P<float>(e->cur.xyz));
  hipLaunchKernelGGL(k_lattice_edges, dim3(tnp_grid(E)), dim3(TNP_BLOCK), 0, s, n[0], n[1], n[2],
                     P<int32_t>(e->edges));
  TNP_CHECK(hipGetLastError());
  // the lattice's full forward (12 B coordinates in; K planes, 40 B of keys out)
  TIMED("forward", (12.0 + 4.0 * e->K + 40.0) * V + table_bytes(e->net),
        launch_forward(e->net, P<float>(e->cur.xyz), V, P<float>(e->cur.pre), e->cur.cap, 1, s, nullptr,
                       VP(e->cur, e->kw), VZ(e->cur, e->kw), P<uint64_t>(e->cur.grid),
                       P<uint64_t>(e->cur.pz)));
  e->V = V;
  e->E = E;
  e->E_live = E;
  e->keep_all = keep_all;
  e->valid_from = 0;
  e->pend_idx = -1;
  *V_out = V;
  *E_out = E;
  return reset_live(e, s);
}

extern "C" int tnp_engine_lattice(tnp_engine* e, int x0, int x1, int keep_all, void* stream,
                                  int64_t* V_out, int64_t* E_out) {
  if (!e->has_net) { tnp_set_error("engine has no net"); return -1; }
  const int N = e->net.n_marks;
  if (x0 < 0 || x1 >= N || x1 < x0) { tnp_set_error("bad slab [%d, %d] of %d marks", x0, x1, N); return -1; }
  const int32_t lo[3] = {x0, 0, 0}, hi[3] = {x1, N - 1, N - 1};
  return tnp_engine_lattice_box(e, lo, hi, keep_all, stream, V_out, E_out);
}

// ---------------------------------------------------------------------------
// skeleton (tropical.py:158-225) + hypercube fallback (subpoly.py:51-52)
// ---------------------------------------------------------------------------
static int load_hypercube(tnp_engine* e, float size, hipStream_t s) {
  float x[2] = {-size, size};
  std::vector<float> v;
  for (int i = 0; i < 2; ++i)
    for (int j = 0; j < 2; ++j)
      for (int k = 0; k < 2; ++k) {
        v.push_back(x[i]);
        v.push_back(x[j]);
        v.push_back(x[k]);
      }
  std::vector<int32_t> ed;
  for (int i = 0; i < 8; ++i)
    for (int j = i + 1; j < 8; ++j) {
      int neg = 0;
      for (int d = 0; d < 3; ++d) neg += (v[3 * i + d] * v[3 * j + d] < 0.f);
      if (neg == 1) {
        ed.push_back(i);
        ed.push_back(j);
      }
    }
  if (vset_ensure(e, e->cur, 8, 0, s)) return -1;
  if (buf_ensure(e->edges, ed.size() * sizeof(int32_t), s)) return -1;
  TNP_CHECK(hipMemcpyAsync(e->cur.xyz.p, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice, s));
  TNP_CHECK(hipMemcpyAsync(e->edges.p, ed.data(), ed.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
  TNP_CHECK(hipStreamSynchronize(s));  // host vectors go out of scope
  e->V = 8;
  e->E = (int64_t)ed.size() / 2;
  e->E_live = (int64_t)ed.size() / 2;
  return 0;
}

extern "C" int tnp_engine_skeleton(tnp_engine* e, int unit, float size, void* stream, int64_t* V_out,
                                   int64_t* E_out) {
  return tnp_engine_skeleton_mode(e, unit, size, TNP_SKELETON_DISTANCE, stream, V_out, E_out);
}

// torch.diff(marks).max().item() (the skeleton's edge-length bound)
static int marks_dmax(tnp_engine* e, hipStream_t s, float* dmax) {
  const int L = e->net.n_marks;
  std::vector<float> mk(L);
  TNP_CHECK(hipMemcpyAsync(mk.data(), e->net.marks, L * sizeof(float), hipMemcpyDeviceToHost, s));
  TNP_CHECK(hipStreamSynchronize(s));
  float d = -INFINITY;
  for (int i = 0; i + 1 < L; ++i) d = std::max(d, mk[i + 1] - mk[i]);
  *dmax = d;
  return 0;
}

// the reference's skeleton tiles (tropical.py:176-181): starts range(0, L,
// unit - 1) per axis, unit marks each (1-mark overlap), x-major order
struct SkelTile {
  int o[3], n[3];
};
static std::vector<SkelTile> skeleton_tiles(int L, int unit) {
  std::vector<SkelTile> t;
  for (int i0 = 0; i0 < L; i0 += unit - 1)
    for (int j0 = 0; j0 < L; j0 += unit - 1)
      for (int k0 = 0; k0 < L; k0 += unit - 1)
        t.push_back(SkelTile{{i0, j0, k0},
                             {std::min(L, i0 + unit) - i0, std::min(L, j0 + unit) - j0, std::min(L, k0 + unit) - k0}});
  return t;
}

// TropicalHashGrid.skeleton on the device.  box_lo / box_hi (distance mode
// only): the part of the skeleton inside the mark box [lo, hi] -- every tile
// meeting the box evaluated on tile & box only, with its max |grad sdf| from
// tile_gmax (device, one word per tile: the whole tile's, tnp_engine_
// skeleton_gmax); the edges (both endpoints in the box) come out in the
// whole skeleton's order, so the result is box_restrict of the whole one.
static int skeleton_build(tnp_engine* e, int unit, float size, int mode, const int32_t* box_lo,
                          const int32_t* box_hi, const unsigned int* tile_gmax, hipStream_t s, int64_t* V_out,
                          int64_t* E_out) {
  e->rows_valid = false;
  if (!e->has_net) { tnp_set_error("engine has no net"); return -1; }
  if (unit < 2) { tnp_set_error("unit must be >= 2"); return -1; }
  TNP_CHECK(hipSetDevice(e->device));
  span_all(e);  // the whole grid
  const int L = e->net.n_marks;
  if ((int64_t)L * L * L >= (1LL << 31)) { tnp_set_error("too many marks for int32 ids"); return -1; }
  float dmax;
  if (marks_dmax(e, s, &dmax)) return -1;
  if (buf_ensure(e->ctr, CTR_CLEAR_BYTES, s)) return -1;
  const int64_t LLL = (int64_t)L * L * L;
  if (buf_ensure(e->used, LLL * sizeof(int32_t), s)) return -1;
  if (buf_ensure(e->nid, LLL * sizeof(int64_t), s)) return -1;
  const FillOp fu{e->used.p, (uint64_t)LLL * sizeof(int32_t), 0};
  if (launch_fill(&fu, 1, s)) return -1;
  if (mode != TNP_SKELETON_DISTANCE && mode != TNP_SKELETON_SIGN) {
    tnp_set_error("skeleton mode %d (0: distance, 1: sign)", mode);
    return -1;
  }
  const bool sign = mode == TNP_SKELETON_SIGN;
  const bool box = box_lo != nullptr;
  if (box && (sign || !tile_gmax)) {
    tnp_set_error("skeleton box: distance mode with the tiles' max |grad sdf| only");
    return -1;
  }
  int64_t tile_pts = (int64_t)std::min(unit, L) * std::min(unit, L) * std::min(unit, L);
  if (buf_ensure(e->stage, tile_pts * sizeof(float) * (sign ? e->K : 1), s)) return -1;
  // sign mode: the tile's points, their forward and packed keys (grid words;
  // pz: (pos, zero) interleaved, 2 kw words a point) in the curve path's
  // scratch slots
  Buf* sk = e->cv;
  if (sign) {
    if (buf_ensure(sk[CV_CORNERS], tile_pts * 3 * sizeof(float), s)) return -1;
    if (buf_ensure(sk[CV_GG], tile_pts * sizeof(uint64_t), s)) return -1;
    if (buf_ensure(sk[CV_STAGE_C], tile_pts * 2 * e->kw * sizeof(uint64_t), s)) return -1;
  }
  if (buf_ensure(e->shared, 16, s)) return -1;
  unsigned int* gmax = P<unsigned int>(e->shared);
  const std::vector<SkelTile> tiles = skeleton_tiles(L, unit);
  int64_t total = 0;
  for (size_t t = 0; t < tiles.size(); ++t) {
    int o[3], n[3];
    bool empty = false;
    for (int d = 0; d < 3; ++d) {
      o[d] = tiles[t].o[d];
      n[d] = tiles[t].n[d];
      if (box) {  // tile & box
        const int a = std::max(o[d], box_lo[d]), b = std::min(o[d] + n[d] - 1, box_hi[d]);
        empty |= b < a;
        o[d] = a;
        n[d] = b - a + 1;
      }
    }
    if (empty) continue;
    const int i0 = o[0], j0 = o[1], k0 = o[2], n0 = n[0], n1 = n[1], n2 = n[2];
    const uint64_t* keys = nullptr;
    const unsigned int* gm = box ? tile_gmax + t : gmax;
    if (sign) {
      // Net.region on the tile's vertices (tropical.py:199-201): the
      // forward of every point with its eps-sign keys
      const int64_t np_ = (int64_t)n0 * n1 * n2;
      if (launch_skel_points(i0, j0, k0, n0, n1, n2, e->net.marks, P<float>(sk[CV_CORNERS]), s)) return -1;
      if (launch_forward(e->net, P<float>(sk[CV_CORNERS]), np_, P<float>(e->stage), np_, 1, s, nullptr,
                         P<uint64_t>(sk[CV_STAGE_C]), P<uint64_t>(sk[CV_STAGE_C]) + e->kw,
                         P<uint64_t>(sk[CV_GG]), P<uint64_t>(sk[CV_STAGE_C])))
        return -1;
      keys = P<uint64_t>(sk[CV_STAGE_C]);
    } else {
      // (box: the sub-tile's |sdf|; its own gradient maximum is not used)
      TNP_CHECK(hipMemsetAsync(gmax, 0, sizeof(unsigned int), s));
      if (launch_skel_eval(e->net, i0, j0, k0, n0, n1, n2, P<float>(e->stage), gmax, s)) return -1;
    }
    int64_t N = skel_candidates(n0, n1, n2);
    int64_t nt = skel_tiles(N);
    if (nt == 0) continue;
    if (buf_ensure(e->blk, (nt + 1) * sizeof(int32_t), s)) return -1;
    if (buf_ensure(e->blkoff, (nt + 1) * sizeof(int64_t), s)) return -1;
    if (launch_skel_edges(false, i0, j0, k0, n0, n1, n2, L, P<float>(e->stage), keys, dmax, gm,
                          P<int32_t>(e->blk), nullptr, 0, nullptr, nullptr, s, e->kw))
      return -1;
    if (scan_counts(e, P<int32_t>(e->blk), P<int64_t>(e->blkoff), nt, CTR_AUX, s)) return -1;
    if (read_ctr(e, s)) return -1;
    int64_t cnt = e->h_ctr[CTR_AUX];
    if (cnt > 0) {
      if (buf_ensure(e->edges_alt, (total + cnt) * 2 * sizeof(int32_t), s, true)) return -1;
      if (launch_skel_edges(true, i0, j0, k0, n0, n1, n2, L, P<float>(e->stage), keys, dmax, gm,
                            nullptr, P<int64_t>(e->blkoff), total, P<int32_t>(e->edges_alt),
                            P<int32_t>(e->used), s, e->kw))
        return -1;
    }
    total += cnt;
  }
  e->pend_idx = -1;
  e->valid_from = 0;
  if (total == 0 && !box) {
    if (load_hypercube(e, size, s)) return -1;
  } else {
    // (box: a box without skeleton edges holds an empty complex -- the whole
    // skeleton's emptiness, the hypercube fallback, is the caller's check)
    if (scan_counts(e, P<int32_t>(e->used), P<int64_t>(e->nid), LLL, CTR_V, s)) return -1;
    if (read_ctr(e, s)) return -1;
    int64_t V = e->h_ctr[CTR_V];
    if (vset_ensure(e, e->cur, std::max<int64_t>(V, 1), 0, s)) return -1;
    if (launch_skel_vertices(P<int32_t>(e->used), P<int64_t>(e->nid), LLL, L, e->net.marks,
                             P<float>(e->cur.xyz), s))
      return -1;
    if (launch_remap_i32(P<int32_t>(e->edges_alt), 2 * total, P<int64_t>(e->nid), s)) return -1;
    if (total > 0) std::swap(e->edges, e->edges_alt);
    e->V = V;
    e->E = total;
    e->E_live = total;
  }
  if (launch_forward(e->net, P<float>(e->cur.xyz), e->V, P<float>(e->cur.pre), e->cur.cap, 1, s, nullptr,
                     VP(e->cur, e->kw), VZ(e->cur, e->kw), P<uint64_t>(e->cur.grid),
                     P<uint64_t>(e->cur.pz)))
    return -1;
  e->keep_all = 0;
  *V_out = e->V;
  *E_out = e->E;
  return reset_live(e, s);
}

extern "C" int tnp_engine_skeleton_mode(tnp_engine* e, int unit, float size, int mode, void* stream,
                                        int64_t* V_out, int64_t* E_out) {
  return skeleton_build(e, unit, size, mode, nullptr, nullptr, nullptr, (hipStream_t)stream, V_out, E_out);
}

extern "C" int tnp_engine_skeleton_gmax(tnp_engine* e, int unit, int rank, int world, uint32_t* h_gmax,
                                        int64_t* h_load, int cap, int* n_tiles, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  e->rows_valid = false;
  if (!e->has_net) { tnp_set_error("engine has no net"); return -1; }
  if (unit < 2 || world < 1 || rank < 0 || rank >= world) {
    tnp_set_error("skeleton_gmax: unit %d, rank %d of %d", unit, rank, world);
    return -1;
  }
  TNP_CHECK(hipSetDevice(e->device));
  const int L = e->net.n_marks;
  const std::vector<SkelTile> tiles = skeleton_tiles(L, unit);
  *n_tiles = (int)tiles.size();
  if ((int)tiles.size() > cap) {
    tnp_set_error("skeleton_gmax: %d tiles, room for %d", (int)tiles.size(), cap);
    return -1;
  }
  float dmax;
  if (marks_dmax(e, s, &dmax)) return -1;
  const int64_t T = (int64_t)tiles.size();
  int64_t tile_pts = (int64_t)std::min(unit, L) * std::min(unit, L) * std::min(unit, L);
  if (buf_ensure(e->stage, tile_pts * sizeof(float), s)) return -1;
  // [T] gmax words, then [3][L] int64 load counts
  const size_t gbytes = (size_t)((T + 1) / 2 * 2) * sizeof(uint32_t);
  if (buf_ensure(e->sk_gload, gbytes + 3 * (size_t)L * sizeof(int64_t), s)) return -1;
  unsigned int* gm = P<unsigned int>(e->sk_gload);
  int64_t* load = reinterpret_cast<int64_t*>(static_cast<char*>(e->sk_gload.p) + gbytes);
  TNP_CHECK(hipMemsetAsync(e->sk_gload.p, 0, gbytes + 3 * (size_t)L * sizeof(int64_t), s));
  for (int64_t t = rank; t < T; t += world) {
    const SkelTile& q = tiles[t];
    if (launch_skel_eval(e->net, q.o[0], q.o[1], q.o[2], q.n[0], q.n[1], q.n[2], P<float>(e->stage), gm + t, s))
      return -1;
    if (launch_skel_load(q.o[0], q.o[1], q.o[2], q.n[0], q.n[1], q.n[2], L, P<float>(e->stage), dmax, gm + t,
                         load, s))
      return -1;
  }
  TNP_CHECK(hipMemcpyAsync(h_gmax, gm, T * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  if (h_load) TNP_CHECK(hipMemcpyAsync(h_load, load, 3 * (size_t)L * sizeof(int64_t), hipMemcpyDeviceToHost, s));
  TNP_CHECK(hipStreamSynchronize(s));
  return 0;
}

extern "C" int tnp_engine_skeleton_box(tnp_engine* e, int unit, const int32_t* lo, const int32_t* hi,
                                       const uint32_t* h_gmax, int n_tiles, void* stream, int64_t* V_out,
                                       int64_t* E_out) {
  hipStream_t s = (hipStream_t)stream;
  if (!e->has_net) { tnp_set_error("engine has no net"); return -1; }
  TNP_CHECK(hipSetDevice(e->device));
  const int L = e->net.n_marks;
  if ((int)skeleton_tiles(L, unit).size() != n_tiles) {
    tnp_set_error("skeleton_box: %d tile maxima for %d tiles", n_tiles, (int)skeleton_tiles(L, unit).size());
    return -1;
  }
  for (int d = 0; d < 3; ++d)
    if (lo[d] < 0 || hi[d] >= L || lo[d] > hi[d]) {
      tnp_set_error("skeleton_box: axis %d box [%d, %d] outside the %d marks", d, lo[d], hi[d], L);
      return -1;
    }
  if (buf_ensure(e->sk_gmax, (size_t)std::max(n_tiles, 1) * sizeof(uint32_t), s)) return -1;
  TNP_CHECK(hipMemcpyAsync(e->sk_gmax.p, h_gmax, n_tiles * sizeof(uint32_t), hipMemcpyHostToDevice, s));
  return skeleton_build(e, unit, 0.f, TNP_SKELETON_DISTANCE, lo, hi, P<unsigned int>(e->sk_gmax), s, V_out, E_out);
}
