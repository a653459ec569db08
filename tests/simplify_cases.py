"""Shared by the simplify tests: a numpy restatement of tnp_simplify_* written
from include/tropical_hip.h alone, and the synthetic soups.  Cells come from a
plain np.floor in float64, the class means from the header's fixed-shape double
sum restated step by step (`fixed_shape_sums`; weld_cases states weld's mean as
math.fsum, which the fixed shape equals whenever no partial sum rounds -- the
host test checks both), canonical forms are Python tuples and duplicates are
found by dict lookup."""
from __future__ import annotations

import math

import numpy as np

from topology_cases import soup
from weld_cases import _d2, bridge, max_shift_of, rewrite, triples, used_ids

STAT_KEYS = ["n_used", "n_cells", "max_cell", "n_polygons", "n_indices", "n_dropped_polygons", "n_duplicate_polygons",
             "n_folded", "n_pinched", "max_shift"]
MODES = {"mean": 0, "nearest": 1}
MAX_CELLS = 1 << 21
BLOCK = 256


def cells_of(verts, indices, cell) -> tuple:
    """(used ids, their integer cell coordinates [U, 3]) by np.floor in float64; ValueError as the
    library refuses: a used vertex that is not finite, an axis of more than 2^21 cells."""
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    u = used_ids(len(v), indices)
    x = v[u].astype(np.float64)
    bad = ~np.isfinite(x).all(1)
    if bad.any():
        raise ValueError(f"simplify: vertex {u[bad][0]} has a coordinate that is not finite")
    h = float(np.float32(cell))
    c = np.floor((x - x.min(0)) / h)
    for q in range(3):
        if c[:, q].max() + 1 > MAX_CELLS:
            raise ValueError(f"simplify: axis {'xyz'[q]} needs {c[:, q].max() + 1:.0f} cells")
    return u, c.astype(np.int64)


def _tree64(x):
    """Lane 0 of the xor tree over 64 lanes (offsets 32, 16, ..., 1); x [64, 3]."""
    for o in (32, 16, 8, 4, 2, 1):
        x = x[:o] + x[o:2 * o]
    return x[0]


def fixed_shape_sums(vals, starts) -> np.ndarray:
    """The header's sum of every class: vals float64 [U, 3] in (representative, id) order, class c at
    [starts[c], starts[c + 1]).  Pieces are cut at the multiples of 256 and at the class boundaries; a
    piece that is a whole 256-block by the fixed tree (per 64, then the four left to right), any other
    left to right; the pieces by 64 strided partial sums from 0.0 and the tree."""
    out = np.zeros((len(starts) - 1, 3))
    for c in range(len(starts) - 1):
        s, e = int(starts[c]), int(starts[c + 1])
        cuts = [s] + list(range((s // BLOCK + 1) * BLOCK, e, BLOCK)) + [e]
        lanes = np.zeros((64, 3))
        for r, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
            if a % BLOCK == 0 and b - a == BLOCK:
                w = [_tree64(vals[a + 64 * k:a + 64 * k + 64]) for k in range(4)]
                piece = ((w[0] + w[1]) + w[2]) + w[3]
            else:
                piece = vals[a].copy()
                for t in range(a + 1, b):
                    piece = piece + vals[t]
            lanes[r % 64] = lanes[r % 64] + piece
        out[c] = _tree64(lanes)
    return out


def canonical(ids) -> tuple:
    """The lexicographically smallest rotation of an id sequence."""
    ids = tuple(int(i) for i in ids)
    lo = min(ids)
    return min(ids[r:] + ids[:r] for r in range(len(ids)) if ids[r] == lo)


def simplify_ref(verts, offsets, indices, cell, position="mean"):
    """dict(map, positions fp32 [V, 3], offsets, indices, source (int64), stats, classes: the member
    ids of every class of >= 2, cells: the used ids and their cell coordinates)."""
    if position not in MODES:
        raise ValueError(position)
    v32 = np.asarray(verts, np.float32).reshape(-1, 3)
    off, idx = np.asarray(offsets, np.int64), np.asarray(indices, np.int64)
    V, P = len(v32), len(off) - 1
    if P == 0:
        st = dict.fromkeys(STAT_KEYS, 0)
        z = np.zeros(0, np.int64)
        return dict(map=np.arange(V, dtype=np.int64), positions=v32.copy(), offsets=np.zeros(1, np.int64), indices=z,
                    source=z, stats=st, classes=[], cells=(z, np.zeros((0, 3), np.int64)))
    idx = idx[:off[-1]]
    u, c = cells_of(v32, idx, cell)
    # ---- the classes: one per occupied cell, the smallest id its representative ----
    first = {}
    root = np.arange(V, dtype=np.int64)
    for i, key in zip(u.tolist(), map(tuple, c.tolist())):  # (u ascends: the first id met is the smallest)
        root[i] = first.setdefault(key, i)
    size = np.bincount(root[u], minlength=V)
    # ---- the means, in (representative, id) order ----
    order = u[np.lexsort((u, root[u]))]
    reps, starts = np.unique(root[order], return_index=True)
    starts = np.append(starts, len(order))
    sums = fixed_shape_sums(v32[order].astype(np.float64), starts)
    pos = v32.copy()
    classes = []
    for k, r in enumerate(reps):
        mem = order[starts[k]:starts[k + 1]]
        if len(mem) < 2:
            continue
        classes.append(mem)
        mean = (sums[k] / float(len(mem))).astype(np.float32)
        if position == "mean":
            pos[mem] = mean
        else:
            d2 = _d2(v32[mem].astype(np.float64), mean.astype(np.float64))
            pos[mem] = v32[mem[int(np.argmin(d2))]]  # (mem ascends, argmin takes the first: the smallest id)
    # ---- weld's rewrite ----
    m = root[idx]
    prev = np.arange(len(idx)) - 1
    prev[off[:-1]] = off[1:] - 1
    keep = m != m[prev]
    deg = np.add.reduceat(keep.astype(np.int64), off[:-1])
    alive = deg >= 3
    take = keep & np.repeat(alive, np.diff(off))
    mid_idx, mid_off = m[take], np.concatenate([[0], np.cumsum(deg[alive])])
    mid_src = np.nonzero(alive)[0]
    # ---- the duplicates ----
    seen, polys, src, folded, pinched, dup = {}, [], [], 0, 0, 0
    for p, a, b in zip(mid_src, mid_off[:-1], mid_off[1:]):
        ids = mid_idx[a:b].tolist()
        form = canonical(ids)
        if form in seen:
            dup += 1
            continue
        folded += canonical(ids[::-1]) in seen
        seen[form] = p
        pinched += len(set(ids)) < len(ids)
        polys.append(ids)
        src.append(p)
    new_off = np.concatenate([[0], np.cumsum([len(q) for q in polys])]).astype(np.int64)
    new_idx = np.array([i for q in polys for i in q], np.int64)
    st = dict(n_used=len(u), n_cells=len(reps), max_cell=int(size.max()), n_polygons=len(polys), n_indices=len(new_idx),
              n_dropped_polygons=int((~alive).sum()), n_duplicate_polygons=dup, n_folded=int(folded),
              n_pinched=int(pinched), max_shift=float(max_shift_of(v32, pos, idx)))
    return dict(map=root, positions=pos, offsets=new_off, indices=new_idx, source=np.array(src, np.int64), stats=st,
                classes=classes, cells=(u, c))


# ---- the synthetic soups: name -> (vertices fp32, offsets, indices, cell) ------------------------
BORDER_CELL = np.float32(0.3)


def borders():
    """Vertices at lo + k cell (as fp32 holds it) and one fp32 step below, k = 1 .. 3 on each axis,
    the box from 1000 (so the difference rounds) and a cell that is no power of two; vertex 0 is lo."""
    h = float(BORDER_CELL)
    pts = [[1000.0, 1000.0, 1000.0]]
    for q in range(3):
        for k in (1, 2, 3):
            at = np.float32(1000.0 + k * h)
            for x in (at, np.nextafter(at, np.float32(0))):
                p = [1000.125, 1000.125, 1000.125]
                p[q] = x
                pts.append(p)
    v = np.array(pts, np.float32)
    return (v, *triples(len(v)))


def grid_limit(axis, over):
    """One triangle spanning exactly 2^21 cells of size 1 on `axis` (one more when over)."""
    v = np.array([[0, 0, 0], [0.5, 0.25, 0.75], [5, 7.5, 2.25]], np.float32)
    v[1, axis] = MAX_CELLS - 1 + (1 if over else 0)
    return (v, *soup([[0, 1, 2]]))


def int_cube(n=4):
    """The cube [0, n]^3 with each face an n x n grid of unit quads over shared integer vertices, outward."""
    ids, verts, polys = {}, [], []

    def vid(p):
        if p not in ids:
            ids[p] = len(verts)
            verts.append(p)
        return ids[p]

    for axis in range(3):
        a, b = (axis + 1) % 3, (axis + 2) % 3
        for side in (0, n):
            for i in range(n):
                for j in range(n):
                    quad = []
                    for di, dj in ((0, 0), (1, 0), (1, 1), (0, 1)):
                        p = [0, 0, 0]
                        p[axis], p[a], p[b] = side, i + di, j + dj
                        quad.append(vid(tuple(p)))
                    polys.append(quad if side else quad[::-1])
    return (np.array(verts, np.float32), *soup(polys))


HEAVY_CELL = np.float32(0.25)


def heavy():
    """A 513-gon over three cells -- 300 vertices in the first, 200 in the second, 13 in the third --
    and 57 triangles, each over a vertex of its own in the second cell (257 members then) and the
    513-gon's vertices 500 and 0: the classes cross the 256-piece boundaries of the sum, the 513-gon
    becomes the triangle [0, 300, 500] and every other triangle its rotation [300, 500, 0]."""
    rng = np.random.default_rng(21)
    p = (rng.random((570, 3)) * 0.2).astype(np.float32)
    p[0] = 0.0
    p[300:500, 0] += 0.5
    p[500:513, 0] += 1.0
    p[513:, 0] += 0.5
    return (p, *soup([list(range(513))] + [[513 + i, 500, 0] for i in range(57)]))


def ties():
    """Cell 1.  Class A (ids 0 .. 3): x = 0, 0.125, 0.03125, 0.09375, mean 0.0625 -- ids 2 and 3 are
    equally near, 2 wins.  Class B (4 .. 7) one cell on: the same with the near pair first (4, 5).
    Class C (8, 9): two members, equally far from their mean unless rounding breaks it."""
    v = np.zeros((10, 3), np.float32)
    v[0:4, 0] = [0, 0.125, 0.03125, 0.09375]
    v[4:8, 0] = [1.09375, 1.03125, 1.0, 1.125]
    v[8:10] = [[2.1, 0.3, 0.7], [2.7, 0.9, 0.1]]
    return (v, *soup([[0, 4, 8], [1, 5, 9], [2, 6, 8], [3, 7, 9]]))


def by_sites(polys):
    """A soup over fresh vertices: a polygon is [(site, twin)], site s lies in cell (s, 0, 0) of the
    unit grid from 0.25, a twin 0.1 beside it."""
    verts, out = [[0.25, 0.25, 0.25]], []  # (vertex 0, at site 0: the box's corner)
    for sites in polys:
        ids = []
        for s, twin in sites:
            ids.append(len(verts))
            verts.append([s + 0.25 + (0.1 if twin else 0.0), 0.25, 0.25])
        out.append(ids)
    return (np.array(verts, np.float32), *soup(out))


A, B, C, D = (0, 0), (1, 0), (2, 0), (3, 0)
A2, C2 = (0, 1), (2, 1)
DUPLICATES = {  # name: (polygons by sites, (n_polygons, n_dropped, n_duplicate, n_folded, n_pinched))
    "dup_rotated": ([[A, A2, B, C], [B, C, C2, A]], (1, 0, 1, 0, 0)),
    "dup_reversed": ([[A, A2, B, C], [C, C2, B, A]], (2, 0, 0, 1, 0)),
    "dup_three_and_reversed": ([[A, B, C], [B, C, A, A2], [C, B, A], [C, A, B]], (2, 0, 2, 1, 0)),
    "dup_pinched": ([[A, B, A2, C], [A, C, A2, B]], (1, 0, 1, 0, 1)),
    "dup_same_set": ([[A, B, C, D], [A, C, B, D]], (2, 0, 0, 0, 0)),
}


def same_triangle(n=1000):
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    return (v, *soup([[0, 1, 2]] * n))


def distinct_triangles(n=4096):
    """n different vertex triples of a 4 x 4 x 4 lattice, each in a random order, shuffled."""
    rng = np.random.default_rng(23)
    v = np.array([[x, y, z] for x in range(4) for y in range(4) for z in range(4)], np.float32)
    seen = set()
    while len(seen) < n:
        seen.add(tuple(sorted(rng.choice(64, 3, replace=False).tolist())))
    tris = [list(rng.permutation(t)) for t in sorted(seen)]
    return (v, *soup([tris[i] for i in rng.permutation(n)]))


REWRITE_CELL = np.float32(0.2)  # a twin (0.4e-3 beside its site) shares its site's cell, two sites (1 apart) never

_soups = {}


def soups():
    """name -> (vertices, offsets, indices, cell)."""
    if not _soups:
        _soups.update({
            "borders": (*borders(), BORDER_CELL),
            "grid_limit_x": (*grid_limit(0, False), np.float32(1)),
            "grid_limit_z": (*grid_limit(2, False), np.float32(1)),
            "one_cell": (*int_cube(4), np.float32(8)),
            "heavy": (*heavy(), HEAVY_CELL),
            "ties": (*ties(), np.float32(1)),
            **{name: (*by_sites(polys), np.float32(1)) for name, (polys, _) in DUPLICATES.items()},
            "same_1000": (*same_triangle(), np.float32(0.5)),
            "distinct_4096": (*distinct_triangles(), np.float32(0.5)),
            "rewrite": (*rewrite(), REWRITE_CELL),
            "bridge_unused_nan": (*bridge(unused_nan=True), np.float32(0.05)),
            "cube_8_cells": (*int_cube(4), np.float32(2.5)),
            "cube_cell_2": (*int_cube(4), np.float32(2)),
            "no_polygons": (np.arange(15, dtype=np.float32).reshape(5, 3), np.zeros(1, np.int64), np.zeros(0, np.int64),
                            np.float32(1.0)),
            "nothing": (np.zeros((0, 3), np.float32), np.zeros(1, np.int64), np.zeros(0, np.int64), np.float32(1.0)),
        })
    return _soups


_refs = {}


def reference(name, position="mean", data=None, cell=None):
    """simplify_ref of a named soup (or of `data` = (verts, offsets, indices) at `cell` under that name), computed once."""
    v, off, idx, h = soups()[name] if data is None else (*data, cell)
    key = (name, float(np.float32(h)), position)
    if key not in _refs:
        _refs[key] = simplify_ref(v, off, idx, h, position)
    return _refs[key]


def simplified_soup(ref):
    """(vertices, offsets, indices) of a reference's output, for polygon_stats."""
    return ref["positions"], ref["offsets"], ref["indices"]


def fsum_mean(v32, mem):
    """weld_cases' statement of a class mean: math.fsum of the fp32 coordinates / m."""
    p = np.asarray(v32, np.float32)[mem].astype(np.float64)
    return np.array([np.float32(math.fsum(p[:, q]) / len(mem)) for q in range(3)], np.float32)
