"""The rasteriser's contract (include/tropical_hip.h, "rasteriser") restated in
numpy int64 / float64, and the hand-made scenes the render tests draw.

    project64      the projection formulas in float64
    fan            fan triangles of a polygon soup, polygon-major
    raster_oracle  coverage, depth, tie-break, resolve and boundary-edge mask
    shade_oracle   look-up-table index, edge colour, background
    box_filter     the integer ss x ss average
    scenes()       name -> Scene (pixel-space polygons under the pixel camera)
"""
import os
import re
from dataclasses import dataclass, field

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tropical_hip.h")
BG = np.uint64(0xFFFFFFFFFFFFFFFF)
GUARD = 1 << 18
ZMAX = (1 << 20) - 1


def small_max() -> int:
    """TNP_RENDER_SMALL_MAX as the header states it."""
    return int(re.search(r"#define\s+TNP_RENDER_SMALL_MAX\s+(\d+)", open(HEADER).read()).group(1))


# ---- projection ----------------------------------------------------------------
def project64(xyz, right, up, toward, center, scale, D, h, W, H):
    """(sx, sy, sz) as float64 before the integer conversion's clamp, and the
    flag, from the header's formulas evaluated in float64."""
    d = np.asarray(xyz, np.float64) - np.asarray(center, np.float64)
    cr, cu, ct = d @ np.asarray(right, np.float64), d @ np.asarray(up, np.float64), d @ np.asarray(toward, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        if D > 0:
            s = D / (D - ct)
            q = (ct * D - h * h) / (h * (D - ct))
        else:
            s, q = np.ones_like(ct), ct / h
        sx = np.rint((W / 2 + scale * s * cr) * 16)
        sy = np.rint((H / 2 - scale * s * cu) * 16)
        sz = np.clip(np.floor((1 - q) / 2 * 2 ** 20), 0, ZMAX)
    flag = ~((np.abs(sx) <= GUARD) & (np.abs(sy) <= GUARD) & (q >= -1) & (q <= 1))
    if D > 0:
        flag |= ct >= D
    return sx, sy, sz, flag, q


# ---- the fan ---------------------------------------------------------------------
def fan(off, idx):
    """ids [nT, 3], polygon [nT], fan position t [nT], degree [nT]; polygon-major."""
    off, idx = np.asarray(off, np.int64), np.asarray(idx, np.int64)
    deg = np.diff(off)
    nt = deg - 2
    pid = np.repeat(np.arange(len(deg)), nt)
    t = np.arange(int(nt.sum())) - np.repeat(np.cumsum(nt) - nt, nt)
    first = off[:-1][pid]
    return np.stack([idx[first], idx[first + t + 1], idx[first + t + 2]], 1).reshape(-1, 3), pid, t, deg[pid]


def _e(a, b, px, py):
    return (b[0] - a[0]) * (py - a[1]) - (b[1] - a[1]) * (px - a[0])


def _owns(a, b):
    dx, dy = int(b[0] - a[0]), int(b[1] - a[1])
    return dy > 0 or (dy == 0 and dx < 0)


def isqrt(n):
    """exact floor(sqrt(n)) of an int64 array (n < 2^52)."""
    n = np.asarray(n, np.int64)
    r = np.floor(np.sqrt(n.astype(np.float64))).astype(np.int64)
    r = np.where(r * r > n, r - 1, r)
    return np.where((r + 1) * (r + 1) <= n, r + 1, r)


def raster_oracle(screen, off, idx, W, H, hw):
    """screen: int [V, 3] (sx, sy, sz; sz < 0: flagged).  Returns prim, tri
    (int32 [H, W]), edge (uint8 [H, W]) and the stats dict."""
    scr = np.asarray(screen, np.int64)
    off, idx = np.asarray(off, np.int64), np.asarray(idx, np.int64)
    P = len(off) - 1
    vis = np.full((H, W), BG, dtype=np.uint64)
    st = dict(n_polygons=P, n_drawn=0, n_dropped=0, n_degenerate=0, n_triangles=0, n_large=0, pixels_covered=0)
    prim, tri = np.full((H, W), -1, np.int32), np.full((H, W), -1, np.int32)
    edge = np.zeros((H, W), np.uint8)
    if P == 0:
        return prim, tri, edge, st
    ids, pid, tpos, tdeg = fan(off, idx)
    st["n_triangles"] = len(ids)
    S = small_max()
    dropped = np.array([(scr[idx[off[p]:off[p + 1]], 2] < 0).any() for p in range(P)])
    has_area = np.zeros(P, bool)
    for T, (a, b, c) in enumerate(ids):
        p = pid[T]
        if dropped[p]:
            continue
        v0, v1, v2 = scr[a], scr[b], scr[c]
        A2 = int(_e(v0, v1, v2[0], v2[1]))
        if A2 < 0:
            v1, v2, A2 = v2, v1, -A2
        if A2 == 0:
            continue
        has_area[p] = True
        xs, ys = (int(v0[0]), int(v1[0]), int(v2[0])), (int(v0[1]), int(v1[1]), int(v2[1]))
        i0, i1 = max(-((8 - min(xs)) // 16), 0), min((max(xs) - 8) // 16, W - 1)  # ceil, floor
        j0, j1 = max(-((8 - min(ys)) // 16), 0), min((max(ys) - 8) // 16, H - 1)
        if i1 < i0 or j1 < j0:
            continue
        if not (i1 - i0 < S and j1 - j0 < S):
            st["n_large"] += 1
        px, py = np.meshgrid(16 * np.arange(i0, i1 + 1, dtype=np.int64) + 8, 16 * np.arange(j0, j1 + 1, dtype=np.int64) + 8)
        cov = np.ones(px.shape, bool)
        w = []
        for a_, b_ in ((v1, v2), (v2, v0), (v0, v1)):
            wk = _e(a_, b_, px, py)
            cov &= (wk > 0) | ((wk == 0) & _owns(a_, b_))
            w.append(wk)
        z = (w[0] * v0[2] + w[1] * v1[2] + w[2] * v2[2]) // A2
        key = (z.astype(np.uint64) << np.uint64(32)) | np.uint64(T)
        sub = vis[j0:j1 + 1, i0:i1 + 1]
        sub[cov] = np.minimum(sub[cov], key[cov])
    st["n_dropped"] = int(dropped.sum())
    st["n_degenerate"] = int((~dropped & ~has_area).sum())
    st["n_drawn"] = P - st["n_dropped"] - st["n_degenerate"]
    hit = vis != BG
    st["pixels_covered"] = int(hit.sum())
    jj, ii = np.nonzero(hit)
    T = (vis[hit] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    tri[hit], prim[hit] = T, pid[T]
    # the boundary edges of fan triangle t: (b, c) always, (a, b) at t = 0, (c, a) at t = deg - 3
    px, py = 16 * ii + 8, 16 * jj + 8
    a, b, c = (scr[ids[T, k]] for k in range(3))

    def near(u, v):
        w = np.abs((v[:, 0] - u[:, 0]) * (py - u[:, 1]) - (v[:, 1] - u[:, 1]) * (px - u[:, 0]))
        return w <= hw * isqrt((v[:, 0] - u[:, 0]) ** 2 + (v[:, 1] - u[:, 1]) ** 2)

    edge[hit] = near(b, c) | ((tpos[T] == 0) & near(a, b)) | ((tpos[T] == tdeg[T] - 3) & near(c, a))
    return prim, tri, edge, st


# ---- shading -----------------------------------------------------------------------
def lut_index64(value, vmin, vmax):
    v = np.asarray(value, np.float64)
    return np.clip(np.floor((v - vmin) / (vmax - vmin) * 255 + 0.5), 0, 255).astype(np.int64)


def shade_oracle(prim, edge, index, lut, edge_rgba):
    """uint8 [H, W, 4] at ss = 1 from per-polygon LUT indices."""
    out = np.zeros(prim.shape + (4,), np.uint8)
    hit = prim >= 0
    out[hit, :3] = np.asarray(lut, np.uint8)[np.asarray(index)[prim[hit]]]
    out[hit, 3] = 255
    if edge is not None:
        out[hit & (edge != 0)] = np.asarray(edge_rgba, np.uint8)
    return out


def box_filter(rgba, ss):
    H, W, _ = rgba.shape
    s = rgba.astype(np.int64).reshape(H // ss, ss, W // ss, ss, 4).sum((1, 3))
    n = ss * ss
    return ((s + n // 2) // n).astype(np.uint8)


# ---- scenes ----------------------------------------------------------------------------
# The pixel camera: right = +x, up = +y, toward = +z, centre 0, scale 1, h = 1,
# orthographic.  A point at pixel coordinates (X, Y) (Y down) and depth value q
# is the world point (X - W/2, H/2 - Y, q); multiples of 1/16 are exact in fp32.
@dataclass
class Scene:
    W: int
    H: int
    polys: list                     # [[(X, Y, q), ...], ...] one list per polygon
    hw: int = 8
    note: str = ""
    xyz: np.ndarray = field(init=False)
    off: np.ndarray = field(init=False)
    idx: np.ndarray = field(init=False)

    def __post_init__(self):
        pts = [p for poly in self.polys for p in poly]
        a = np.array(pts, np.float64).reshape(-1, 3)
        self.xyz = np.stack([a[:, 0] - self.W / 2, self.H / 2 - a[:, 1], a[:, 2]], 1).astype(np.float32)
        deg = [len(p) for p in self.polys]
        self.off = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
        self.idx = np.arange(len(pts), dtype=np.int64)


PIXEL_CAMERA = dict(right=(1, 0, 0), up=(0, 1, 0), toward=(0, 0, 1), center=(0, 0, 0), scale=1.0, persp_dist=0.0,
                    depth_half=1.0)


def _flat(pts, q):
    return [(x, y, q) for x, y in pts]


def scenes():
    S = small_max()
    rng = np.random.default_rng(11)
    out = {}
    # two quads whose corners and diagonals run through pixel centres: one split on each diagonal
    qa = [(1.5, 0.5), (4.5, 0.5), (4.5, 3.5), (1.5, 3.5)]
    qb = [(8.5, 0.5), (11.5, 0.5), (11.5, 3.5), (8.5, 3.5)]
    out["quad_diagonals_17x5"] = Scene(17, 5, [
        _flat([qa[0], qa[1], qa[2]], 0.0), _flat([qa[0], qa[2], qa[3]], 0.0),
        _flat([qb[0], qb[1], qb[3]], 0.25), _flat([qb[1], qb[2], qb[3]], 0.25)])
    out["interpenetrating_64"] = Scene(64, 64, [
        [(4.2, 6.1, -0.8), (60.3, 10.7, 0.7), (20.9, 58.4, 0.1)],
        [(58.6, 5.3, -0.6), (8.8, 30.2, 0.9), (50.1, 61.9, -0.2)]])
    t = [(10.3, 8.2, 0.3), (50.6, 20.4, -0.4), (22.7, 55.9, 0.6)]
    out["coplanar_duplicates_64"] = Scene(64, 64, [[t[1], t[2], t[0]], [t[0], t[1], t[2]], [t[2], t[1], t[0]]])
    # one triangle over the whole image, behind 4,000 sub-pixel triangles: both paths in one frame
    polys = [[(-10.0, -10.0, -0.5), (200.0, -10.0, -0.5), (-10.0, 200.0, -0.25)]]
    c = rng.uniform(-1, 65, (4000, 1, 2))
    d = rng.uniform(-0.9, 0.9, (4000, 3, 2))
    q = rng.uniform(-0.9, 0.9, (4000, 3))
    polys += [[(c[k, 0, 0] + d[k, v, 0], c[k, 0, 1] + d[k, v, 1], q[k, v]) for v in range(3)] for k in range(4000)]
    out["full_over_4000_64"] = Scene(64, 64, polys)
    # boxes of S and S + 1 pixel centres, in either direction
    def corner(x, y, nx, ny, q):
        return [(x + 0.2, y + 0.2, q), (x + nx - 0.4, y + 0.2, q), (x + 0.2, y + ny - 0.4, q)]
    out["threshold_130x67"] = Scene(130, 67, [corner(3, 3, S, S, 0.1), corner(20, 3, S + 1, S, 0.2),
                                             corner(40, 3, S, S + 1, 0.3), corner(60, 3, S + 1, S + 1, 0.4),
                                             # overlapping pair, one on each path, interleaved in depth
                                             [(80.1, 30.3, -0.5), (80.1 + S - 0.4, 30.3, 0.5), (80.1, 30.3 + S - 0.4, 0.0)],
                                             [(78.3, 28.2, 0.5), (78.3 + S + 3, 28.2, -0.5), (78.3, 28.2 + S + 3, 0.0)]])
    out["off_image_130x67"] = Scene(130, 67, [
        [(-20.5, 10.2, 0.0), (15.3, -8.1, 0.2), (12.8, 30.6, -0.2)],         # across the left and top borders
        [(120.4, 50.3, 0.1), (160.2, 60.9, 0.1), (125.7, 90.2, 0.1)],        # across the right and bottom borders
        [(140.5, 10.0, 0.0), (170.5, 12.0, 0.0), (150.0, 40.0, 0.0)],        # wholly to the right
        [(10.0, -30.0, 0.0), (40.0, -5.0, 0.0), (20.0, -1.0, 0.0)],          # wholly above
        [(-400.0, -300.0, -0.9), (900.0, -100.0, -0.9), (100.0, 700.0, -0.9)],  # everything, far behind
        [(127.2, 1.1, 0.5), (133.0, 1.3, 0.5), (128.1, 6.2, 0.5)]])          # small, across the right border
    out["slivers_64"] = Scene(64, 64, [
        [(1.6, 3.6, 0.0), (30.4, 3.7, 0.0), (15.0, 3.9, 0.0)],       # between two rows of centres
        [(7.6, 2.0, 0.0), (7.9, 60.0, 0.0), (7.7, 30.0, 0.0)],       # between two columns
        [(40.6, 40.6, 0.0), (41.4, 40.7, 0.0), (41.0, 41.4, 0.0)],  # inside one pixel, off its centre
        [(5.0, 5.0, 0.0), (10.0, 10.0, 0.0), (20.0, 20.0, 0.0)],      # zero area
        [(50.0, 50.0, 0.1), (50.0, 50.0, 0.2), (50.0, 50.0, 0.3)]])   # a point
    ang = 2 * np.pi * np.arange(7) / 7 + 0.1
    hept = [(30.0 + 24.0 * np.cos(a), 31.0 + 24.0 * np.sin(a), 0.2 * np.cos(a)) for a in ang]
    tri3 = [(50.2, 48.3, 0.8), (62.7, 50.1, 0.8), (55.5, 62.4, 0.8)]
    out["heptagon_hw8_64"] = Scene(64, 64, [hept, tri3], hw=8)
    out["heptagon_hw40_64"] = Scene(64, 64, [hept, tri3], hw=40)
    out["pixel_1x1"] = Scene(1, 1, [[(-3.0, -3.0, 0.0), (5.0, -3.0, 0.0), (-3.0, 5.0, 0.5)],
                                    [(0.6, 0.6, -0.5), (0.9, 0.6, -0.5), (0.6, 0.9, -0.5)]])
    # a vertex exactly on a pixel centre, and a fan around that centre
    f = [(10.5, 10.5), (14.0, 8.0), (15.0, 12.0), (11.0, 15.0), (6.0, 13.0), (7.0, 7.0)]
    out["vertex_on_centre_17x5"] = Scene(17, 5, [_flat([(2.5, 2.5), (6.5, 1.5), (4.5, 4.5)], 0.0),
                                                  _flat([(10.5, 2.5), (14.5, 0.5), (15.5, 3.5)], 0.0)])
    out["fan_about_centre_64"] = Scene(64, 64, [_flat([f[0], f[k], f[k % 5 + 1]], 0.0) for k in range(1, 6)])
    out["empty_64"] = Scene(64, 64, [])
    return out
