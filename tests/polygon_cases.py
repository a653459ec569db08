"""Shared by the polygon tests: the fixture reader, the fan, and the numpy
restatement of tnp_polygon_report (include/tropical_hip.h states the
definitions; tests/golden/make_polygon_golden.py keeps its own copy, whose
results the fixture records)."""
from __future__ import annotations

import os

import numpy as np

from golden_io import GOLDEN

FULL = ["small_sphere", "small_torus", "h8l3_sphere", "small_sphere_curve"]  # stored in full
FLAT = ["small_sphere", "small_torus", "h8l3_sphere"]  # force=True fits: every polygon winds about its normal
ALL = FULL + ["h32l3_rand"]  # K = 65, stored as SHA + counts + stats
_cache = {}


def fixture(case: str) -> dict:
    """offsets / indices (int64) / normals of a case stored in full, its
    ``sha`` over (offsets, indices) as int64 and its recorded ``stats``."""
    if not _cache:
        with np.load(os.path.join(GOLDEN, "polygons.npz"), allow_pickle=False) as z:
            _cache.update({k: z[k] for k in z.files})
    z = _cache
    names = [str(k) for k in z["int_stats"]]
    d = {"sha": str(z[f"{case}:sha"]),
         "stats": dict(zip(names, (int(v) for v in z[f"{case}:stats_int"])))}
    d["stats"]["area"], d["stats"]["max_dev"] = (float(v) for v in z[f"{case}:stats_float"])
    if f"{case}:offsets" in z:
        d["offsets"] = z[f"{case}:offsets"].astype(np.int64)
        d["indices"] = z[f"{case}:indices"].astype(np.int64)
        d["normals"] = z[f"{case}:normals"]
    return d


def fan_t_major(offsets, indices) -> np.ndarray:
    """Triangles (p0, p[t+1], p[t+2]) of every polygon, fan position t major."""
    offsets, indices = np.asarray(offsets, np.int64), np.asarray(indices, np.int64)
    deg = np.diff(offsets)
    out = [np.zeros((0, 3), np.int64)]
    for t in range(int(deg.max()) - 2 if len(deg) else 0):
        s = offsets[:-1][deg >= t + 3]
        out.append(np.stack([indices[s], indices[s + t + 1], indices[s + t + 2]], 1))
    return np.concatenate(out)


def polygon_stats(verts, offsets, indices, dtype=np.float64):
    """(stats, per-polygon area, per-polygon dev) by the header's definitions;
    the geometry in ``dtype`` (sums over a polygon's members in their order)."""
    offsets, indices = np.asarray(offsets, np.int64), np.asarray(indices, np.int64)
    P, deg = len(offsets) - 1, np.diff(offsets)
    pid = np.repeat(np.arange(P), deg)
    nxt = np.arange(len(indices)) + 1
    nxt[offsets[1:] - 1] = offsets[:-1]
    a, b = indices, indices[nxt]  # the polygon's consecutive pairs, cyclic
    und, inv, cnt = np.unique(np.minimum(a, b) * (1 << 32) + np.maximum(a, b), return_inverse=True,
                              return_counts=True)
    down = np.bincount(inv.reshape(-1), weights=(a > b), minlength=len(und))  # uses that run max -> min
    st = dict(n_polygons=P, n_indices=len(indices), max_degree=int(deg.max()),
              n_vertices_used=len(np.unique(indices)), n_edges=len(und), e_boundary=int((cnt == 1).sum()),
              e_manifold=int((cnt == 2).sum()), e_nonmanifold=int((cnt > 2).sum()),
              e_misoriented=int(((cnt == 2) & (down != 1)).sum()))
    st["euler"] = st["n_vertices_used"] - st["n_edges"] + st["n_polygons"]
    p = np.asarray(verts, dtype)[indices]
    c = np.add.reduceat(p, offsets[:-1], axis=0) / deg[:, None].astype(dtype)
    u = p - c[pid]
    N = dtype(0.5) * np.add.reduceat(np.cross(u, u[nxt]), offsets[:-1], axis=0)
    area = np.sqrt((N * N).sum(1))
    d = np.maximum.reduceat(np.abs((u * N[pid]).sum(1)), offsets[:-1])
    dev = np.where(area > 0, d / np.where(area > 0, area, 1), 0).astype(dtype)
    st["area"], st["max_dev"] = float(area.astype(np.float64).sum()), float(dev.max())
    return st, area, dev
