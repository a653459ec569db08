"""Shared by the weld tests: a numpy restatement of tnp_weld_* written from
include/tropical_hip.h alone (a grid search of its own, checked against the
plain all-pairs search by test_weld_host), and the synthetic soups.  Maps,
polygons and counts are integers; a mode-0 position is its representative's
bits, a mode-1 mean is math.fsum of the fp32 coordinates / m."""
from __future__ import annotations

import math

import numpy as np

from topology_cases import _classes, soup

STAT_KEYS = ["n_used", "n_pairs", "n_clusters", "n_merged", "max_cluster", "n_polygons", "n_indices",
             "n_dropped_polygons", "n_pinched", "max_shift"]
MODES = {"first": 0, "mean": 1}


def tol2_of(tol) -> float:
    t = float(np.float32(tol))
    return t * t


def _d2(a, b):
    """The header's squared distance of float64 rows: every operation rounded once, left to right."""
    d = a - b
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def used_ids(V, indices) -> np.ndarray:
    return np.unique(np.asarray(indices, np.int64))


def close_pairs_brute(verts, indices, tol) -> np.ndarray:
    """The close pairs (i < j) [K, 2] by all pairs: one row of distances per used vertex, no grid."""
    v = np.asarray(verts, np.float32).reshape(-1, 3).astype(np.float64)
    u = used_ids(len(v), indices)
    t2, out = tol2_of(tol), []
    for k in range(len(u)):
        later = u[k + 1:]
        hit = later[_d2(v[later], v[u[k]]) <= t2]
        out.append(np.stack([np.full(len(hit), u[k]), hit], 1))
    return np.concatenate(out) if out else np.zeros((0, 2), np.int64)


def close_pairs(verts, indices, tol) -> np.ndarray:
    """The same pairs by a uniform grid of cells no smaller than tol: candidates
    from a vertex's own and the 26 neighbouring cells, decided by the predicate."""
    v = np.asarray(verts, np.float32).reshape(-1, 3).astype(np.float64)
    u = used_ids(len(v), indices)
    if len(u) == 0:
        return np.zeros((0, 2), np.int64)
    x = v[u]
    lo = x.min(0)
    ext = float((x.max(0) - lo).max())
    h = max(float(np.float32(tol)) * 1.01, ext / 2.0 ** 19)
    h = h if h > 0 else 1.0
    c = np.floor((x - lo) / h).astype(np.int64) + 1  # (1 ..: a neighbour's coordinate stays >= 0)
    M = int(c.max()) + 2
    key = (c[:, 0] * M + c[:, 1]) * M + c[:, 2]
    order = np.argsort(key, kind="stable")
    sk, t2, out = key[order], tol2_of(tol), []
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                want = key + (dx * M + dy) * M + dz
                a, b = np.searchsorted(sk, want, "left"), np.searchsorted(sk, want, "right")
                n = b - a
                i = np.repeat(np.arange(len(u)), n)
                j = order[np.repeat(a, n) + (np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n))]
                m = u[i] < u[j]
                i, j = i[m], j[m]
                hit = _d2(x[i], x[j]) <= t2
                out.append(np.stack([u[i[hit]], u[j[hit]]], 1))
    p = np.concatenate(out)
    return p[np.lexsort((p[:, 1], p[:, 0]))]


def max_shift_of(verts, positions, indices) -> np.float32:
    """max over the used vertices of fp32(sqrt(d2(input, output)))."""
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    u = used_ids(len(v), indices)
    if len(u) == 0:
        return np.float32(0)
    d = np.sqrt(_d2(v[u].astype(np.float64), np.asarray(positions, np.float32).reshape(-1, 3)[u].astype(np.float64)))
    return d.astype(np.float32).max()


def weld_ref(verts, offsets, indices, tol, position="first", pairs=None):
    """dict(map, positions fp32 [V, 3], offsets, indices, source (int64), stats, clusters: the
    member ids of every class of >= 2); pairs: the close pairs when already known."""
    v32 = np.asarray(verts, np.float32).reshape(-1, 3)
    off, idx = np.asarray(offsets, np.int64), np.asarray(indices, np.int64)
    V, P = len(v32), len(off) - 1
    if P == 0:
        st = dict.fromkeys(STAT_KEYS, 0)
        st["max_shift"] = 0.0
        z = np.zeros(0, np.int64)
        return dict(map=np.arange(V, dtype=np.int64), positions=v32.copy(), offsets=np.zeros(1, np.int64), indices=z,
                    source=z, stats=st, clusters=[])
    idx = idx[:off[-1]]
    u = used_ids(V, idx)
    if pairs is None:
        pairs = close_pairs(v32, idx, tol)
    root, roots = _classes(V, pairs)
    size = np.bincount(root[u], minlength=V)
    pos = v32[root].copy()
    clusters = [u[root[u] == r] for r in np.nonzero(size >= 2)[0]]
    if position == "mean":
        pos = v32.copy()
        for mem in clusters:
            p = v32[mem].astype(np.float64)
            pos[mem] = [np.float32(math.fsum(p[:, q]) / len(mem)) for q in range(3)]
    elif position != "first":
        raise ValueError(position)
    # ---- the polygons over the representatives ----
    m = root[idx]
    prev = np.arange(len(idx)) - 1
    prev[off[:-1]] = off[1:] - 1
    keep = m != m[prev]
    deg = np.add.reduceat(keep.astype(np.int64), off[:-1])
    alive = deg >= 3
    take = keep & np.repeat(alive, np.diff(off))
    new_idx, new_deg = m[take], deg[alive]
    new_off = np.concatenate([[0], np.cumsum(new_deg)]).astype(np.int64)
    pinched = sum(len(set(new_idx[a:b].tolist())) < b - a for a, b in zip(new_off[:-1], new_off[1:]))
    st = dict(n_used=len(u), n_pairs=len(pairs), n_clusters=len(clusters), n_merged=len(u) - len(np.unique(root[u])),
              max_cluster=int(size.max()), n_polygons=int(alive.sum()), n_indices=int(new_deg.sum()),
              n_dropped_polygons=int((~alive).sum()), n_pinched=int(pinched),
              max_shift=float(max_shift_of(v32, pos, idx)))
    return dict(map=root, positions=pos, offsets=new_off, indices=new_idx, source=np.nonzero(alive)[0].astype(np.int64),
                stats=st, clusters=clusters)


# ---- the synthetic soups: name -> (vertices fp32, offsets, indices, tol) --------------------------
def triples(n, skip=()):
    """Triangles (k, k + 1, k + 2), k = 0, 3, ... (wrapping) over the ids [0, n) but `skip`: every id is used."""
    ids = np.array([i for i in range(n) if i not in set(skip)], np.int64)
    return soup([ids[(k + np.arange(3)) % len(ids)] for k in range(0, len(ids), 3)])


def lattice():
    """3 x 3 x 3 points 0.5 apart about the origin: neighbours at exactly 0.5."""
    g = np.array([[x, y, z] for x in (-0.5, 0, 0.5) for y in (-0.5, 0, 0.5) for z in (-0.5, 0, 0.5)], np.float32)
    return (g, *triples(27))


BORDER_TOL = np.float32(0.01)
DIRECTIONS = [(x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1) if (x, y, z) != (0, 0, 0)]


def cell_borders(factor):
    """Pairs factor * tol apart across the faces, edges and corners of the
    library's grid (the box is [-1, 1]^3, so h = tol (1 + 2^-10) from -1), one
    pair per direction, 12 cells apart; two pairs at the box's own corners (they
    span it) and two inside its faces x = -1 and y = 1.  ids: pair k is (2k, 2k + 1)."""
    tol = float(BORDER_TOL)
    h = tol * (1.0 + 2.0 ** -10)
    pts = []
    for n, d in enumerate(DIRECTIONS):
        d = np.array(d, np.float64)
        cell = np.array([15 + 12 * (n % 5), 20 + 12 * (n // 5), 30 + 6 * n], np.float64)  # spread over both signs
        c = -1.0 + (cell + np.where(d != 0, 0.0, 0.5)) * h  # on the border along d, mid-cell elsewhere
        step = 0.5 * factor * tol * d / np.linalg.norm(d)
        pts += [c - step, c + step]
    s = factor * tol / math.sqrt(3.0)
    pts += [np.array([-1.0, -1.0, -1.0]), np.array([-1.0 + s, -1.0 + s, -1.0 + s])]
    pts += [np.array([1.0, 1.0, 1.0]), np.array([1.0 - s, 1.0 - s, 1.0 - s])]
    y0 = -1.0 + 30 * h  # a cell border
    pts += [np.array([-1.0, y0 - 0.5 * factor * tol, 0.3]), np.array([-1.0, y0 + 0.5 * factor * tol, 0.3])]
    pts += [np.array([y0 - 0.5 * factor * tol, 1.0, -0.3]), np.array([y0 + 0.5 * factor * tol, 1.0, -0.3])]
    v = np.array(pts, np.float32)
    return (v, *triples(len(v)))


CHAIN_TOL = np.float32(0.01)


def chain(n, seed):
    """n points 0.9 tol apart along a slanted line, ids permuted."""
    t = np.arange(n, dtype=np.float64)[:, None] * 0.9 * float(CHAIN_TOL)
    line = np.array([-3.0, 1.0, 0.5]) + t * (np.array([2.0, -1.0, 2.0]) / 3.0)
    perm = np.random.default_rng(seed).permutation(n)
    v = np.empty((n, 3), np.float32)
    v[perm] = line
    return (v, *triples(n))


BALL_TOL = np.float32(0.02)


def ball():
    """300 points in a cube of diagonal < tol: all close, all in one cell."""
    rng = np.random.default_rng(5)
    v = (np.array([0.3, -0.7, 1.1]) + (rng.random((300, 3)) - 0.5) * float(BALL_TOL) * 0.57).astype(np.float32)
    return (v, *triples(300))


BRIDGE_TOL = np.float32(0.1)


def bridge(unused_nan=False, used_nan=False):
    """0 and 2 are 1.2 tol apart and used; 1 lies between them (0.6 tol from
    each) and is unused, as is 5."""
    t = float(BRIDGE_TOL)
    v = np.array([[0, 0, 0], [0.6 * t, 0, 0], [1.2 * t, 0, 0], [0, 1, 0], [1, 1, 0], [0.5, 0.5, 0.5], [1, 0, 1]],
                 np.float32)
    if unused_nan:
        v[5] = [np.nan, np.inf, 0]
    if used_nan:
        v[4, 1] = np.nan
        v[6, 2] = np.inf
    return (v, *soup([[0, 2, 3], [3, 4, 6, 0]]))


CUBE_Q = [[0, 1, 3, 2], [4, 6, 7, 5], [0, 4, 5, 1], [2, 3, 7, 6], [0, 2, 6, 4], [1, 5, 7, 3]]  # outward, id = 4x + 2y + z


def split_cube():
    """The unit cube as six quads over 24 vertices of their own; some zeros are -0.0."""
    corner = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float32)
    v = corner[np.array(CUBE_Q).reshape(-1)].copy()
    neg = np.random.default_rng(9).random(v.shape) < 0.5
    v[neg & (v == 0)] = -0.0
    assert np.signbit(v).any() and (v == 0).sum() > np.signbit(v).sum()
    return (v, *soup([list(range(4 * q, 4 * q + 4)) for q in range(6)]))


REWRITE_TOL = np.float32(1e-3)


def rewrite():
    """Every way a polygon changes.  A site is a point 1 apart from the others;
    a vertex sits at its site or 0.4 tol beside it (a twin).  In polygon order:
    a 5-gon that collapses to 3; a quad that collapses to 2 (dropped); a quad
    whose run of equal ids wraps past its end; a triangle on one site (dropped);
    a pinched quad; an untouched triangle; a 513-gon whose odd vertices are the
    twins of their predecessors; a triangle that collapses to 2 (dropped); an
    untouched quad."""
    t = float(REWRITE_TOL)
    verts, polys = [], []

    def add(sites):  # [(site number, twin?)] -> one polygon over new vertices
        ids = []
        for s, twin in sites:
            ids.append(len(verts))
            verts.append([float(s % 40), float(s // 40), 0.25 * (s % 3) + (0.4 * t if twin else 0.0)])
        polys.append(ids)

    add([(0, 0), (0, 1), (1, 0), (1, 1), (2, 0)])
    add([(3, 0), (3, 1), (4, 0), (4, 1)])
    add([(5, 1), (6, 0), (7, 0), (5, 0)])
    add([(8, 0), (8, 1), (8, 0)])
    add([(9, 0), (10, 0), (9, 1), (11, 0)])
    add([(12, 0), (13, 0), (14, 0)])
    add([(100 + k // 2, k % 2) for k in range(512)] + [(400, 0)])
    add([(15, 0), (16, 0), (16, 1)])
    add([(17, 0), (18, 0), (19, 0), (20, 0)])
    return (np.array(verts, np.float32), *soup(polys))


def identical(n=40):
    return (np.tile(np.float32([0.25, -3.0, 7.5]), (n, 1)), *triples(n))


FAR_TOL = np.float32(1e-6)


def far_box():
    """2000 points in [1000, 1003]^3, where an fp32 step is 6e-5 > tol and the
    grid's cell is the box / 2^21: 300 exact copies weld, 100 neighbours one step away do not."""
    rng = np.random.default_rng(11)
    v = (1000.0 + 3.0 * rng.random((1600, 3))).astype(np.float32)
    v[0], v[1] = 1000.0, 1003.0
    copies = v[rng.choice(1600, 300, replace=False)]
    near = v[rng.choice(1600, 100, replace=False)].copy()
    near[:, 0] = np.nextafter(near[:, 0], np.float32(0))
    v = np.concatenate([v, copies, near])
    perm = rng.permutation(len(v))
    return (v[perm], *triples(len(v)))


RANDOM_TOL = np.float32(0.0128)


def random_cube():
    v = np.random.default_rng(13).random((8192, 3)).astype(np.float32)
    return (v, *triples(8192))


_soups = {}


def soups():
    """name -> (vertices, offsets, indices, tol): every synthetic case with the tolerance it is welded at."""
    if not _soups:
        half = np.float32(0.5)
        _soups.update({
            "lattice_at_tol": (*lattice(), half),
            "lattice_below_tol": (*lattice(), np.nextafter(half, np.float32(0))),
            "borders_0.9": (*cell_borders(0.9), BORDER_TOL),
            "borders_1.1": (*cell_borders(1.1), BORDER_TOL),
            "chain_1000": (*chain(1000, 1), CHAIN_TOL),
            "chain_257": (*chain(257, 2), CHAIN_TOL),
            "ball_300": (*ball(), BALL_TOL),
            "bridge": (*bridge(), BRIDGE_TOL),
            "bridge_unused_nan": (*bridge(unused_nan=True), BRIDGE_TOL),
            "split_cube": (*split_cube(), np.float32(0)),
            "rewrite": (*rewrite(), REWRITE_TOL),
            "identical": (*identical(), np.float32(0)),
            "identical_tol": (*identical(), np.float32(0.5)),
            "far_box": (*far_box(), FAR_TOL),
            "random_8192": (*random_cube(), RANDOM_TOL),
            "no_polygons": (np.arange(15, dtype=np.float32).reshape(5, 3), np.zeros(1, np.int64), np.zeros(0, np.int64),
                            np.float32(1.0)),
            "nothing": (np.zeros((0, 3), np.float32), np.zeros(1, np.int64), np.zeros(0, np.int64), np.float32(1.0)),
        })
    return _soups


_refs = {}


def reference(name, position="first", data=None, tol=None):
    """weld_ref of a named soup (or of `data` = (verts, offsets, indices) at `tol` under that name),
    computed once; the close pairs are shared between the two modes."""
    v, off, idx, t = soups()[name] if data is None else (*data, tol)
    key = (name, float(np.float32(t)))
    if (key, "pairs") not in _refs:
        _refs[key, "pairs"] = close_pairs(v, idx[:off[-1]], t)
    if (key, position) not in _refs:
        _refs[key, position] = weld_ref(v, off, idx, t, position, _refs[key, "pairs"])
    return _refs[key, position]


def welded_soup(ref):
    """(vertices, offsets, indices) of a reference's output, for polygon_stats."""
    return ref["positions"], ref["offsets"], ref["indices"]
