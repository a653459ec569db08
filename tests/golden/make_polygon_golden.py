"""Generate tests/golden/polygons.npz: the polygons behind the committed
goldens' triangles, captured from the REFERENCE on CPU (build container only,
as make_golden.py).

    python tests/golden/make_polygon_golden.py [case ...]

extract_faces (subpoly.py:584-652) orders every final region row by angle
(``v_indices.gather(1, indices)``) and hands the rows to
``tensor_to_triangle_faces``, which fans them.  Both calls are wrapped here:
the rows are cloned before the fan mutates them, and the ``jacobians`` that
ordered them are recorded.  A row becomes a polygon by the rule of
tnp_engine_polygons (include/tropical_hip.h): -1 pads dropped, ids
de-duplicated keeping the first, rows left with < 3 ids omitted.  The t-major
fan of the polygons must reproduce the case's stored ``sha_tri``.

Per case the file holds offsets / indices (int32) and normals (fp32) -- cases
above FULL_MAX_TRI triangles only their SHA-256 and counts -- and the
statistics of tnp_polygon_report computed by the plain numpy restatement
below (recorded results: the tests read them).
"""
from __future__ import annotations

import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from golden_io import golden_eps, load, sha  # noqa: E402
from make_golden import FULL_MAX_TRI, _surface_check  # noqa: E402

CASES = ["small_sphere", "small_torus", "h8l3_sphere", "small_sphere_curve", "h32l3_rand"]
INT_STATS = ["n_polygons", "n_indices", "max_degree", "n_vertices_used", "n_edges", "e_boundary",
             "e_manifold", "e_nonmanifold", "e_misoriented", "euler"]


def rows_to_polygons(rows: np.ndarray, jac: np.ndarray):
    """(offsets, indices, normals) of the padded, ordered rows."""
    polys, keep = [], []
    for f, row in enumerate(rows):
        arr = row[row != -1]
        _, first = np.unique(arr, return_index=True)
        ids = arr[np.sort(first)]
        if len(ids) >= 3:
            polys.append(ids)
            keep.append(f)
    deg = np.array([len(p) for p in polys], dtype=np.int64)
    offsets = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    indices = np.concatenate(polys).astype(np.int64) if polys else np.zeros(0, np.int64)
    return offsets, indices, jac[keep].astype(np.float32)


def fan_t_major(offsets, indices):
    """Triangles (p0, p[t+1], p[t+2]) of every polygon, listed t-major."""
    deg = np.diff(offsets)
    out = []
    for t in range(int(deg.max()) - 2 if len(deg) else 0):
        s = offsets[:-1][deg >= t + 3]
        out.append(np.stack([indices[s], indices[s + t + 1], indices[s + t + 2]], 1))
    return np.concatenate(out).astype(np.int64) if out else np.zeros((0, 3), np.int64)


def polygon_stats(verts, offsets, indices, dtype=np.float64):
    """The numpy restatement of tnp_polygon_report (the header's definitions)."""
    offsets, indices = np.asarray(offsets, np.int64), np.asarray(indices, np.int64)
    P, deg = len(offsets) - 1, np.diff(offsets)
    pid = np.repeat(np.arange(P), deg)
    nxt = np.arange(len(indices)) + 1
    nxt[offsets[1:] - 1] = offsets[:-1]
    a, b = indices, indices[nxt]
    und, inv, cnt = np.unique(np.minimum(a, b) * (1 << 32) + np.maximum(a, b), return_inverse=True,
                              return_counts=True)
    fwd = np.bincount(inv.reshape(-1), weights=(a > b), minlength=len(und))
    st = dict(n_polygons=P, n_indices=len(indices), max_degree=int(deg.max()),
              n_vertices_used=len(np.unique(indices)), n_edges=len(und), e_boundary=int((cnt == 1).sum()),
              e_manifold=int((cnt == 2).sum()), e_nonmanifold=int((cnt > 2).sum()),
              e_misoriented=int(((cnt == 2) & (fwd != 1)).sum()))
    st["euler"] = st["n_vertices_used"] - st["n_edges"] + st["n_polygons"]
    p = np.asarray(verts, dtype)[indices]
    c = np.add.reduceat(p, offsets[:-1], axis=0) / deg[:, None].astype(dtype)
    u = p - c[pid]
    N = dtype(0.5) * np.add.reduceat(np.cross(u, u[nxt]), offsets[:-1], axis=0)
    area = np.sqrt((N * N).sum(1))
    d = np.maximum.reduceat(np.abs((u * N[pid]).sum(1)), offsets[:-1])
    dev = np.where(area > 0, d / np.where(area > 0, area, 1), 0)
    st["area"], st["max_dev"] = float(area.astype(np.float64).sum()), float(dev.max())
    return st, area, dev


def run_case(name, out):
    sp, model = __import__("ref_loader").import_reference()
    d = load(name)
    net = model.Net(**d["cfg"])
    net.load_state_dict({k: torch.from_numpy(v) for k, v in d["params"].items()})
    force = str(d["kind"]) != "curve"
    if not force:
        sp.check_new_vertices_on_surface = _surface_check
    rec = {}
    orig_fan, orig_sort = sp.tensor_to_triangle_faces, sp.gm.sort_polygon_vertices_batch

    def fan(tensor, *a, **k):
        rec["rows"] = tensor.clone().numpy()
        return orig_fan(tensor, *a, **k)

    def sort(points, jacobians, *a, **k):
        rec["jac"] = jacobians.detach().numpy().copy()
        return orig_sort(points, jacobians, *a, **k)

    sp.tensor_to_triangle_faces, sp.gm.sort_polygon_vertices_batch = fan, sort
    t0 = time.time()
    try:
        _, Vs, fwi = sp.subpoly(net, 3, 1.2, golden_eps(d), force=force)
    finally:
        sp.tensor_to_triangle_faces, sp.gm.sort_polygon_vertices_batch = orig_fan, orig_sort
    assert rec["rows"].shape[0] == rec["jac"].shape[0]
    off, idx, nrm = rows_to_polygons(rec["rows"], rec["jac"])
    tri = fan_t_major(off, idx)
    assert np.array_equal(tri, np.asarray(fwi, dtype=np.int64))
    assert sha(tri) == str(d["sha_tri"]), name
    Vs = Vs.detach().numpy()
    assert sha(Vs) == str(d["sha_surf"]), name
    st, _, _ = polygon_stats(Vs, off, idx)
    out[f"{name}:sha"] = np.array(sha(off, idx))
    out[f"{name}:stats_int"] = np.array([st[k] for k in INT_STATS], dtype=np.int64)
    out[f"{name}:stats_float"] = np.array([st["area"], st["max_dev"]], dtype=np.float64)
    out[f"{name}:sha_normals"] = np.array(sha(nrm))
    out[f"{name}:nrm_absmax"] = np.float32(np.abs(nrm).max())
    if tri.shape[0] <= FULL_MAX_TRI:
        out[f"{name}:offsets"], out[f"{name}:indices"] = off.astype(np.int32), idx.astype(np.int32)
        out[f"{name}:normals"] = nrm
    print(f"{name}: {st} ({time.time() - t0:.0f}s)", flush=True)


if __name__ == "__main__":
    path = os.path.join(HERE, "polygons.npz")
    out = {"int_stats": np.array(INT_STATS)}
    names = sys.argv[1:] or CASES
    if sys.argv[1:] and os.path.exists(path):  # regenerate only the named cases
        with np.load(path, allow_pickle=False) as z:
            out.update({k: z[k] for k in z.files})
    for nm in names:
        run_case(nm, out)
    out["cases"] = np.array(sorted({k.split(":")[0] for k in out if ":" in k}))
    np.savez_compressed(path, **out)
    print(f"-> {path} {os.path.getsize(path) / 1e3:.0f} kB")
