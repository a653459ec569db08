"""Shared by the hole-filling tests: a numpy / Python restatement of
tnp_holes_* (include/tropical_hip.h states the definitions) on top of
topology_cases, and three more synthetic soups.  Status, cycles and caps are
integers; a star cap's centre is math.fsum of the fp32 coordinates / m."""
from __future__ import annotations

import math

import numpy as np

from topology_cases import _classes, _ring, soup, soups as topo_soups

CAPPED, NONSIMPLE, UNORIENTED, TOO_LONG = 0, 1, 2, 3
STAT_KEYS = ["n_loops", "n_capped", "n_nonsimple", "n_unoriented", "n_too_long", "n_cycle_indices", "n_triangles",
             "longest_capped"]


def holes_ref(V, offsets, indices, max_edges=0):
    """dict(status int32 [L], cycle_loop, offsets, vertices (int64), stats,
    first_vertex / n_edges / simple per loop)."""
    off, idx = np.asarray(offsets, np.int64), np.asarray(indices, np.int64)
    P = len(off) - 1
    first = np.zeros(0, np.int64)
    n_edges, simple, status, cycles = first, first, np.zeros(0, np.int32), []
    if P > 0:
        nxt = np.arange(len(idx)) + 1
        nxt[off[1:] - 1] = off[:-1]
        a, b = idx, idx[nxt]  # the polygons traverse a -> b
        und, inv, cnt = np.unique(np.minimum(a, b) * (1 << 32) + np.maximum(a, b), return_inverse=True,
                                  return_counts=True)
        lone = cnt[inv.reshape(-1)] == 1
        ba, bb = a[lone], b[lone]
        vroot, _ = _classes(V, zip(ba, bb))
        bdeg = np.bincount(np.concatenate([ba, bb]), minlength=V)
        first = np.unique(vroot[bdeg > 0])  # loop l: its smallest vertex
        L = len(first)
        el = np.searchsorted(first, vroot[ba])
        n_edges = np.bincount(el, minlength=L)
        on = np.nonzero(bdeg > 0)[0]
        vl = np.searchsorted(first, vroot[on])
        simple = (np.bincount(vl, weights=(bdeg[on] != 2), minlength=L) == 0).astype(np.int64)
        outd = np.bincount(bb, minlength=V)  # the cap traverses b -> a: b is the tail
        flipped = np.bincount(vl, weights=(outd[on] != 1), minlength=L) > 0
        status = np.where(simple == 0, NONSIMPLE,
                          np.where(flipped, UNORIENTED,
                                   np.where((max_edges > 0) & (n_edges > max_edges), TOO_LONG, CAPPED))).astype(np.int32)
        succ = {}
        for x, y, l in zip(ba.tolist(), bb.tolist(), el.tolist()):
            if status[l] == CAPPED:
                assert y not in succ
                succ[y] = x
        for l in np.nonzero(status == CAPPED)[0]:
            c = [int(first[l])]
            for _ in range(int(n_edges[l]) - 1):
                c.append(succ[c[-1]])
            assert succ[c[-1]] == c[0] and len(set(c)) == len(c) >= 3
            cycles.append(c)
    lens = np.array([len(c) for c in cycles], np.int64)
    stats = dict(n_loops=len(status), n_capped=len(cycles), n_nonsimple=int((status == NONSIMPLE).sum()),
                 n_unoriented=int((status == UNORIENTED).sum()), n_too_long=int((status == TOO_LONG).sum()),
                 n_cycle_indices=int(lens.sum()), n_triangles=int((lens == 3).sum()),
                 longest_capped=int(lens.max()) if len(lens) else 0)
    return dict(status=status, cycle_loop=np.nonzero(status == CAPPED)[0].astype(np.int64),
                offsets=np.concatenate([[0], np.cumsum(lens)]).astype(np.int64),
                vertices=np.array([v for c in cycles for v in c], np.int64), stats=stats,
                first_vertex=first, n_edges=n_edges, simple=simple)


def caps_ref(ref, mode, V, verts=None):
    """(cap offsets, cap indices, new vertices fp32 [S, 3]) of holes_ref's cycles."""
    off, cv = ref["offsets"], ref["vertices"]
    if mode == "polygon":
        return off.copy(), cv.copy(), np.zeros((0, 3), np.float32)
    v32 = np.asarray(verts, np.float32).reshape(-1, 3)
    tris, new = [], []
    for k in range(len(off) - 1):
        c = cv[off[k]:off[k + 1]]
        m = len(c)
        if m == 3:
            tris.append(c)
            continue
        s = V + len(new)
        tris += [[c[i], c[(i + 1) % m], s] for i in range(m)]
        p = v32[c].astype(np.float64)
        new.append([np.float32(math.fsum(p[:, q]) / m) for q in range(3)])
    T = len(tris)
    return (3 * np.arange(T + 1, dtype=np.int64), np.array(tris, np.int64).reshape(-1),
            np.array(new, np.float32).reshape(-1, 3))


def filled_soup(verts, offsets, indices, cap_off, cap_idx, new=None):
    """The input polygons followed by the caps, the input vertices followed by the new ones."""
    off, idx = np.asarray(offsets, np.int64), np.asarray(indices, np.int64)
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    if new is not None and len(new):
        v = np.concatenate([v, np.asarray(new, np.float32).reshape(-1, 3)])
    return v, np.concatenate([off, off[-1] + np.asarray(cap_off, np.int64)[1:]]), np.concatenate([idx, cap_idx])


# ---- the extra soups ------------------------------------------------------------------------------
NGON_SIZES = [3, 4, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 8193]


def _ngons():
    """One m-gon per size, all vertex ids shuffled across the soup: each
    boundary is one cycle of m edges (the lengths sit at wave, block and
    doubling-round edges)."""
    rng = np.random.default_rng(31)
    polys, vs, base = [], [], 0
    for t, m in enumerate(NGON_SIZES):
        a = 2 * np.pi * np.arange(m) / m
        vs.append(np.stack([3.0 * t + np.cos(a), np.sin(a), 0.1 * np.cos(3 * a)], 1))
        polys.append(np.arange(base, base + m))
        base += m
    v = np.concatenate(vs)
    perm = rng.permutation(base)  # old id -> new id
    w = np.empty_like(v)
    w[perm] = v
    return w.astype(np.float32), [perm[p] for p in polys]


GRID_N = 24
GRID_SINGLE = [(2, 2), (2, 9), (5, 5), (9, 2), (9, 14), (12, 20), (20, 3)]  # isolated quads: 4-edge holes
GRID_BLOCK = [(i, j) for i in (15, 16) for j in (8, 9, 10)]                 # 2 x 3: a 10-edge hole
GRID_DIAG = [(19, 18), (20, 19)]                                            # pinched at their shared corner


def _punched_grid():
    rng = np.random.default_rng(32)
    n = GRID_N
    gone = set(GRID_SINGLE + GRID_BLOCK + GRID_DIAG)
    vid = lambda i, j: i * (n + 1) + j  # noqa: E731
    q = [[vid(i, j), vid(i + 1, j), vid(i + 1, j + 1), vid(i, j + 1)] for i in range(n) for j in range(n)
         if (i, j) not in gone]
    i, j = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    v = np.stack([i * 0.1, j * 0.1, 0.05 * np.sin(0.3 * i) * np.cos(0.2 * j)], -1).reshape(-1, 3)
    perm = rng.permutation(len(v))
    w = np.empty_like(v)
    w[perm] = v
    return w.astype(np.float32), [perm[p] for p in np.array(q)]


def _flipped_cylinder():
    """The cylinder with one quad on the j = 0 rim reversed: that end flips
    orientation along its loop, the other end can be capped."""
    v, q = _ring(8, 7, False)
    q = [list(p) for p in q]
    q[0] = q[0][::-1]  # (i, j) = (0, 0)
    return v, q


_extra = {}


def soups():
    """topology_cases' soups and the three of this file."""
    if not _extra:
        for name, make in (("ngons", _ngons), ("punched_grid", _punched_grid), ("flipped_cylinder", _flipped_cylinder)):
            v, q = make()
            _extra[name] = (v, *soup(q))
    return {**topo_soups(), **_extra}


_refs = {}


def reference(name, max_edges=0, data=None):
    """holes_ref of a named soup (or of `data` = (verts, offsets, indices) under that name), computed once."""
    key = (name, max_edges)
    if key not in _refs:
        v, off, idx = soups()[name] if data is None else data
        _refs[key] = holes_ref(len(v), off, idx, max_edges)
    return _refs[key]
