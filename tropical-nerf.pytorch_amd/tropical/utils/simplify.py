"""The polygon surface simplified by vertex clustering on the GPU
(csrc/simplify.hip; the definitions are in include/tropical_hip.h): the used
vertices that share a cell of a uniform grid become one, the polygons are
rewritten over them and the duplicates that makes are removed.  In the repair
chain it sits behind `weld` and in front of `keep_components` and `fill_holes`.

    res = cluster_vertices(pm.vertices, pm.offsets, pm.indices, cell=0.05)  # position="mean" | "nearest"
    res.map, res.positions, res.offsets, res.indices, res.source, res.stats
    coarse, stats = simplify(pm, cell=0.05)                                 # a PolygonMesh again
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from .mesh import PolygonMesh
from .soup import Handle, current_device, soup_on_device, stage_ms

POSITIONS = {"mean": 0, "nearest": 1}
STAGES = ("check_used", "grid_keys", "cell_sort", "classes", "positions", "rewrite", "duplicates")


class SimplifyResult:
    """``map`` (numpy int64 [V], every vertex's representative), ``positions``
    (float32 [V, 3]), the simplified soup ``offsets`` / ``indices`` (int64, over
    the input's vertex ids) and ``source`` (int64, the input polygon of every
    output polygon), ``stats`` (dict, tnp_simplify_stats); ``stage_ms`` when the
    build was timed."""

    def __init__(self, map, positions, offsets, indices, source, stats, stage_ms=None):
        self.map, self.positions, self.offsets, self.indices, self.source = map, positions, offsets, indices, source
        self.stats, self.stage_ms = stats, stage_ms

    def __len__(self):
        return len(self.source)


def check_cell(cell) -> float:
    """`cell` as a float; ValueError unless it is a finite number > 0 that stays so in fp32."""
    ok = isinstance(cell, (int, float, np.floating, np.integer)) and not isinstance(cell, bool)
    if ok and math.isfinite(cell):
        with np.errstate(over="ignore"):
            c32 = float(np.float32(cell))
        ok = math.isfinite(c32) and c32 > 0
    else:
        ok = False
    if not ok:
        raise ValueError(f"cell = {cell!r} (finite, > 0)")
    return float(cell)


def simplify_handle():
    """A tnp_simplify handle on the current device for repeated builds
    (``cluster_vertices(..., handle=h)``); ``h.close()`` frees it."""
    return _simplify_handle(current_device())


def _simplify_handle(dev):
    return Handle(dev, "tnp_simplify_create", "tnp_simplify_destroy")


def cluster_vertices(vertices, offsets, indices, cell: float, position: str = "mean", timed: bool = False,
                     handle: "Handle | None" = None) -> SimplifyResult:
    """Cluster the used vertices of a polygon soup by the cells of a grid of
    size `cell` from the used vertices' lower corner, rewrite the polygons over
    the cells' smallest ids and remove the duplicate polygons
    (tnp_simplify_build / tnp_simplify_export).  position: "mean" (the class's
    mean) or "nearest" (the member nearest to that mean, so the output vertices
    are a subset of the input's).  numpy arrays or tensors, as polygon_report
    takes them; host inputs are moved to the current device.  A bad `cell` or
    `position` raises ValueError before any GPU call; malformed input, a used
    vertex that is not finite and a grid of more than 2^21 cells on an axis
    raise RuntimeError naming the offender.  timed: record the build's stage
    times (``stage_ms``, a dict).  handle: a `simplify_handle()` to build on
    (else one is made and closed)."""
    if position not in POSITIONS:
        raise ValueError(f"position = {position!r} (mean, nearest)")
    cell = check_cell(cell)
    import torch

    from .. import _hip
    dev = current_device()
    v, off, idx, P = soup_on_device(vertices, offsets, indices, dev)
    V = v.shape[0]
    own = handle is None
    hd = _simplify_handle(dev) if own else handle
    try:
        lib, stream = _hip.lib(), C.c_void_p(_hip.stream_ptr(dev))
        if timed:
            lib.tnp_debug_simplify_stages(hd.h, 1, None, 0)
        st = _hip.TnpSimplifyStats()
        _hip.check(lib.tnp_simplify_build(hd.h, _hip.ptr(v), V, _hip.ptr(off), _hip.ptr(idx), P, cell,
                                          POSITIONS[position], C.byref(st), stream), "tnp_simplify_build")
        stats = st.as_dict()
        vmap = torch.empty(V, dtype=torch.int64, device=dev)
        pos = torch.empty((V, 3), dtype=torch.float32, device=dev)
        ooff = torch.empty(stats["n_polygons"] + 1, dtype=torch.int64, device=dev)
        oidx = torch.empty(stats["n_indices"], dtype=torch.int64, device=dev)
        src = torch.empty(stats["n_polygons"], dtype=torch.int64, device=dev)
        _hip.check(lib.tnp_simplify_export(hd.h, _hip.ptr(vmap), _hip.ptr(pos), _hip.ptr(ooff), _hip.ptr(oidx),
                                           _hip.ptr(src), stream), "tnp_simplify_export")
        times = stage_ms(lib.tnp_debug_simplify_stages, hd, STAGES) if timed else None
        out = [t.cpu().numpy() for t in (vmap, pos, ooff, oidx, src)]
    finally:
        if own:
            hd.close()
    return SimplifyResult(*out, stats, times)


def simplify(pmesh: PolygonMesh, cell: float, position: str = "mean", compact: bool = True):
    """Simplify a PolygonMesh: ``(simplified, stats)``.  The polygons that
    remain keep their order and their normals; compact drops the vertices no
    polygon uses any more and keeps the rest in order (as `weld` does), else
    the vertex array keeps its length and the merged vertices stay behind
    unused."""
    if position not in POSITIONS:
        raise ValueError(f"position = {position!r} (mean, nearest)")
    cell = check_cell(cell)
    res = cluster_vertices(pmesh.vertices, pmesh.offsets, pmesh.indices, cell, position)
    verts, idx = res.positions.astype(pmesh.vertices.dtype), res.indices
    if compact:
        used = np.zeros(len(verts), dtype=bool)
        used[idx] = True
        remap = np.cumsum(used) - 1
        verts, idx = verts[used], remap[idx]
    normals = None if pmesh.normals is None else pmesh.normals[res.source]
    return PolygonMesh(verts, res.offsets, idx, normals), res.stats


def cluster_triangles(vertices: np.ndarray, faces: np.ndarray, cell: float):
    """A triangle mesh (float [V, 3], int [F, 3]) clustered as a soup with
    offsets 0, 3, 6, ..., position "nearest", duplicates removed:
    ``(vertices, faces, stats)``, compacted, in the input's dtypes."""
    cell = check_cell(cell)
    faces = np.asarray(faces)
    off = 3 * np.arange(len(faces) + 1, dtype=np.int64)
    res = cluster_vertices(np.asarray(vertices, np.float32), off, faces.reshape(-1).astype(np.int64), cell, "nearest")
    assert np.array_equal(res.offsets, 3 * np.arange(len(res.source) + 1))  # (a triangle never pinches)
    used = np.zeros(len(res.positions), dtype=bool)
    used[res.indices] = True
    remap = np.cumsum(used) - 1
    return (res.positions[used].astype(np.asarray(vertices).dtype), remap[res.indices].reshape(-1, 3).astype(faces.dtype),
            res.stats)
