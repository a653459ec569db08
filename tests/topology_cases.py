"""Shared by the topology tests: a numpy restatement of tnp_topology_*
(include/tropical_hip.h states the definitions) and the synthetic soups.
The inputs are small, so the union-find is a plain Python loop; the geometry
is float64 from the fp32 coordinates, sums by math.fsum."""
from __future__ import annotations

import math

import numpy as np

COMP_INT = ["first_polygon", "n_polygons", "n_indices", "n_vertices", "n_edges", "e_boundary", "e_manifold",
            "e_nonmanifold", "e_misoriented", "euler"]
LOOP_INT = ["first_vertex", "n_edges", "n_vertices", "component", "simple"]
EDGE_COLS = ["n_edges", "e_boundary", "e_manifold", "e_nonmanifold", "e_misoriented"]


def _classes(n, pairs):
    """Canonical labels of the classes of [0, n) under the unions `pairs`
    (numbered by ascending smallest member), and every member's root."""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in pairs:
        a, b = find(int(a)), find(int(b))
        if a != b:
            parent[max(a, b)] = min(a, b)
    root = np.array([find(x) for x in range(n)], dtype=np.int64)
    return root, np.unique(root)


def topology_ref(verts, offsets, indices, connect="edge"):
    """dict(labels, components, loops, det_abs, n_tri): the tables as dicts of
    columns; det_abs[c] = sum over the component's fan triangles of the sum
    of the absolute values of the determinant's six products, n_tri[c] their
    number (the volume's error bound)."""
    v32 = np.asarray(verts, np.float32).reshape(-1, 3)
    v = v32.astype(np.float64)
    off, idx = np.asarray(offsets, np.int64), np.asarray(indices, np.int64)
    P, V = len(off) - 1, len(v)
    comp_cols = COMP_INT + ["area", "volume"]
    if P == 0:
        comps = {k: np.zeros(0, np.int64 if k in COMP_INT else np.float64) for k in comp_cols}
        comps["lo"] = comps["hi"] = np.zeros((0, 3), np.float32)
        loops = {k: np.zeros(0, np.int64) for k in LOOP_INT}
        loops["length"] = np.zeros(0)
        return dict(labels=np.zeros(0, np.int32), components=comps, loops=loops, det_abs=np.zeros(0),
                    n_tri=np.zeros(0, np.int64))
    deg = np.diff(off)
    n = len(idx)
    pid = np.repeat(np.arange(P), deg)
    nxt = np.arange(n) + 1
    nxt[off[1:] - 1] = off[:-1]
    a, b = idx, idx[nxt]
    und, first, inv, cnt = np.unique(np.minimum(a, b) * (1 << 32) + np.maximum(a, b), return_index=True,
                                     return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    by = inv if connect == "edge" else idx  # uses grouped by undirected edge, or by vertex
    order = np.argsort(by, kind="stable")
    same = by[order][1:] == by[order][:-1]
    root, roots = _classes(P, zip(pid[order][1:][same], pid[order][:-1][same]))
    labels = np.searchsorted(roots, root)
    C = len(roots)
    # ---- components ----
    c = {"first_polygon": roots, "n_polygons": np.bincount(labels, minlength=C),
         "n_indices": np.bincount(labels, weights=deg, minlength=C).astype(np.int64)}
    lv = np.unique(labels[pid] * (1 << 32) + idx)
    c["n_vertices"] = np.bincount(lv >> 32, minlength=C)
    ec = labels[pid[first]]  # every use of an edge lies in one component
    down = np.bincount(inv, weights=(a > b), minlength=len(und))
    for k, m in zip(EDGE_COLS, [cnt > 0, cnt == 1, cnt == 2, cnt > 2, (cnt == 2) & (down != 1)]):
        c[k] = np.bincount(ec[m], minlength=C)
    c["euler"] = c["n_vertices"] - c["n_edges"] + c["n_polygons"]
    p = v[idx]
    cen = np.add.reduceat(p, off[:-1], axis=0) / deg[:, None]
    u = p - cen[pid]
    N = 0.5 * np.add.reduceat(np.cross(u, u[nxt]), off[:-1], axis=0)
    area = np.sqrt((N * N).sum(1))
    nt = deg - 2
    t0 = np.repeat(off[:-1], nt)
    tt = np.arange(int(nt.sum())) - np.repeat(np.cumsum(nt) - nt, nt)
    p0, p1, p2 = v[idx[t0]], v[idx[t0 + tt + 1]], v[idx[t0 + tt + 2]]
    prods = np.stack([p0[:, 0] * p1[:, 1] * p2[:, 2], p0[:, 0] * p1[:, 2] * p2[:, 1],
                      p0[:, 1] * p1[:, 2] * p2[:, 0], p0[:, 1] * p1[:, 0] * p2[:, 2],
                      p0[:, 2] * p1[:, 0] * p2[:, 1], p0[:, 2] * p1[:, 1] * p2[:, 0]], 1)
    det = (p0[:, 0] * (p1[:, 1] * p2[:, 2] - p1[:, 2] * p2[:, 1]) + p0[:, 1] * (p1[:, 2] * p2[:, 0] - p1[:, 0] * p2[:, 2])
           + p0[:, 2] * (p1[:, 0] * p2[:, 1] - p1[:, 1] * p2[:, 0]))
    tl = labels[np.repeat(np.arange(P), nt)]
    c["area"] = np.array([math.fsum(area[labels == k]) for k in range(C)])
    c["volume"] = np.array([math.fsum(det[tl == k]) / 6.0 for k in range(C)])
    det_abs = np.array([math.fsum(np.abs(prods[tl == k]).sum(1)) for k in range(C)])
    lo, hi = np.full((C, 3), np.inf, np.float32), np.full((C, 3), -np.inf, np.float32)
    np.minimum.at(lo, labels[pid], v32[idx])
    np.maximum.at(hi, labels[pid], v32[idx])
    c["lo"], c["hi"] = lo, hi
    # ---- boundary loops ----
    bk = und[cnt == 1]  # ascending edge keys
    ba, bb = bk >> 32, bk & 0xFFFFFFFF
    vroot, _ = _classes(V, zip(ba, bb))
    bdeg = np.bincount(np.concatenate([ba, bb]), minlength=V)
    lroots = np.unique(vroot[bdeg > 0])
    L = len(lroots)
    el = np.searchsorted(lroots, vroot[ba])
    vl = np.searchsorted(lroots, vroot[bdeg > 0])
    d = v[bb] - v[ba]
    elen = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    owner = labels[pid[first[cnt == 1]]]
    lp = {"first_vertex": lroots, "n_edges": np.bincount(el, minlength=L), "n_vertices": np.bincount(vl, minlength=L),
          "simple": (np.bincount(vl, weights=(bdeg[bdeg > 0] != 2), minlength=L) == 0).astype(np.int64),
          "component": np.array([owner[np.nonzero(el == k)[0][0]] for k in range(L)], dtype=np.int64),
          "length": np.array([math.fsum(elen[el == k]) for k in range(L)])}
    return dict(labels=labels.astype(np.int32), components=c, loops=lp, det_abs=det_abs,
                n_tri=np.bincount(tl, minlength=C))


# ---- synthetic soups: name -> (vertices fp32, offsets, indices) ---------------------------------
def soup(polys):
    d = [len(p) for p in polys]
    return (np.concatenate([[0], np.cumsum(d)]).astype(np.int64),
            np.concatenate(polys).astype(np.int64) if polys else np.zeros(0, np.int64))


CUBE_V = np.array([[x, y, z] for x in (0, 2) for y in (0, 2) for z in (0, 2)], dtype=np.float32)  # id = 4x + 2y + z
CUBE_Q = [[0, 1, 3, 2], [4, 6, 7, 5], [0, 4, 5, 1], [2, 3, 7, 6], [0, 2, 6, 4], [1, 5, 7, 3]]  # outward


def _ring(n, m, closed):
    """n quads around (cyclic) x m along (cyclic when closed, else m + 1 rows)."""
    rows = m if closed else m + 1
    q = [[i * rows + j, ((i + 1) % n) * rows + j, ((i + 1) % n) * rows + (j + 1) % rows, i * rows + (j + 1) % rows]
         for i in range(n) for j in range(m)]
    i, j = np.meshgrid(np.arange(n), np.arange(rows), indexing="ij")
    th = 2 * np.pi * i / n
    if closed:
        ph = 2 * np.pi * j / rows
        r = 1.0 + 0.4 * np.cos(ph)
        v = np.stack([r * np.cos(th), r * np.sin(th), 0.4 * np.sin(ph)], -1)
    else:
        v = np.stack([np.cos(th), np.sin(th), 0.25 * j], -1)
    return v.reshape(-1, 3).astype(np.float32), q


def _strip(n, seed, permute_vertices):
    """n quads over 2 x (n + 1) vertices, the polygon order (and the vertex ids) shuffled."""
    rng = np.random.default_rng(seed)
    k = np.arange(n)
    q = np.stack([k, k + 1, n + 1 + k + 1, n + 1 + k], 1)[rng.permutation(n)]
    x = np.arange(n + 1) * 0.01
    v = np.concatenate([np.stack([x, 0 * x, 0.1 * np.sin(x)], 1), np.stack([x, 0 * x + 0.02, 0.1 * np.sin(x)], 1)])
    if permute_vertices:
        perm = rng.permutation(2 * (n + 1))  # old id -> new id
        q = perm[q]
        w = np.empty_like(v)
        w[perm] = v
        v = w
    return v.astype(np.float32), [list(r) for r in q]


def make_soups():
    rng = np.random.default_rng(11)
    s = {}
    v, q = _ring(8, 8, True)
    s["torus"] = (v, *soup(q))
    v, q = _ring(8, 7, False)
    s["cylinder"] = (v, *soup(q))
    tet = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    tv = np.concatenate([-tet[[1, 2, 3]] * 0.7, tet])  # ids 0..2, then 3 (the shared origin), 4, 5, 6
    s["two_tets"] = (tv, *soup([[3, 1, 0], [3, 0, 2], [3, 2, 1], [0, 1, 2],       # the mirror image: wound inward
                                [3, 5, 4], [3, 4, 6], [3, 6, 5], [4, 5, 6]]))
    s["cube"] = (CUBE_V, *soup(CUBE_Q))
    s["cube_reversed"] = (CUBE_V, *soup([p[::-1] for p in CUBE_Q]))
    N = 8
    mv = np.array([[np.cos(2 * np.pi * k / N) * (1 + 0.3 * (2 * r - 1) * np.cos(np.pi * k / N)),
                    np.sin(2 * np.pi * k / N) * (1 + 0.3 * (2 * r - 1) * np.cos(np.pi * k / N)),
                    0.3 * (2 * r - 1) * np.sin(np.pi * k / N)] for r in (0, 1) for k in range(N)], np.float32)
    mq = [[k, k + 1, N + k + 1, N + k] for k in range(N - 1)] + [[N - 1, N, 0, 2 * N - 1]]  # the twist
    s["moebius"] = (mv, *soup(mq))
    fv = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [-1, 0, 0.5], [-1, -1, 0.5], [0, -1, 0.5]], np.float32)
    s["two_fans"] = (fv, *soup([[0, 1, 2], [0, 2, 3], [0, 4, 5], [0, 5, 6]]))
    s["one"] = (rng.uniform(-1, 1, (3, 3)).astype(np.float32), *soup([[0, 1, 2]]))
    s["empty"] = (rng.uniform(-1, 1, (5, 3)).astype(np.float32), *soup([]))
    s["isolated_1000"] = (rng.uniform(-1, 1, (3000, 3)).astype(np.float32),
                          *soup([[3 * t, 3 * t + 1, 3 * t + 2] for t in range(1000)]))
    v, q = _strip(4096, 21, False)
    s["strip_4096"] = (v, *soup(q))
    v, q = _strip(4096, 22, True)
    s["strip_4096_vperm"] = (v, *soup(q))
    a = 2 * np.pi * np.arange(1000) / 1000
    bv = np.concatenate([[[0, 0, 0], [0, 0, 1]], np.stack([np.cos(a), np.sin(a), 0.5 + 0 * a], 1)]).astype(np.float32)
    s["book_1000"] = (bv, *soup([[0, 1, 2 + k] for k in range(1000)]))
    return s


_soups, _refs = {}, {}


def soups():
    if not _soups:
        _soups.update(make_soups())
    return _soups


def reference(name, connect, data=None):
    """topology_ref of a named soup (or of `data` under that name), computed once."""
    key = (name, connect)
    if key not in _refs:
        _refs[key] = topology_ref(*(soups()[name] if data is None else data), connect=connect)
    return _refs[key]
