"""Near-coincident vertices of a polygon soup welded on the GPU (csrc/weld.hip;
the definitions are in include/tropical_hip.h): the first stage of the repair
chain, in front of `keep_components` and `fill_holes`.

    res = weld_vertices(pm.vertices, pm.offsets, pm.indices, tol=1e-3)      # position="first" | "mean"
    res.map, res.positions, res.offsets, res.indices, res.source, res.stats
    welded, stats = weld(pm, tol=1e-3)                                      # a PolygonMesh again
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from .mesh import PolygonMesh
from .soup import Handle, current_device, soup_on_device, stage_ms

POSITIONS = {"first": 0, "mean": 1}
STAGES = ("check_used", "grid_keys", "cell_sort", "search", "clusters", "positions", "rewrite")


class WeldResult:
    """``map`` (numpy int64 [V], every vertex's representative), ``positions``
    (float32 [V, 3]), the welded soup ``offsets`` / ``indices`` (int64, over the
    input's vertex ids) and ``source`` (int64, the input polygon of every output
    polygon), ``stats`` (dict, tnp_weld_stats); ``stage_ms`` when the build was timed."""

    def __init__(self, map, positions, offsets, indices, source, stats, stage_ms=None):
        self.map, self.positions, self.offsets, self.indices, self.source = map, positions, offsets, indices, source
        self.stats, self.stage_ms = stats, stage_ms

    def __len__(self):
        return len(self.source)


def weld_handle():
    """A tnp_weld handle on the current device for repeated builds
    (``weld_vertices(..., handle=h)``); ``h.close()`` frees it."""
    return _weld_handle(current_device())


def _weld_handle(dev):
    return Handle(dev, "tnp_weld_create", "tnp_weld_destroy")


def weld_vertices(vertices, offsets, indices, tol: float, position: str = "first", timed: bool = False,
                  handle: "Handle | None" = None) -> WeldResult:
    """Weld the used vertices of a polygon soup that lie within `tol` of each
    other, by single linkage, and rewrite the polygons over the clusters'
    smallest ids (tnp_weld_build / tnp_weld_export).  position: "first" (the
    representative's coordinates) or "mean" (the cluster's mean).  numpy arrays
    or tensors, as polygon_report takes them; host inputs are moved to the
    current device.  Malformed input, a tolerance that is negative or not finite
    and a used vertex that is not finite raise RuntimeError naming the first
    offender.  timed: record the build's stage times (``stage_ms``, a dict).
    handle: a `weld_handle()` to build on (else one is made and closed)."""
    import torch

    from .. import _hip
    if position not in POSITIONS:
        raise ValueError(f"position = {position!r} (first, mean)")
    dev = current_device()
    v, off, idx, P = soup_on_device(vertices, offsets, indices, dev)
    V = v.shape[0]
    own = handle is None
    hd = _weld_handle(dev) if own else handle
    try:
        lib, stream = _hip.lib(), C.c_void_p(_hip.stream_ptr(dev))
        if timed:
            lib.tnp_debug_weld_stages(hd.h, 1, None, 0)
        st = _hip.TnpWeldStats()
        _hip.check(lib.tnp_weld_build(hd.h, _hip.ptr(v), V, _hip.ptr(off), _hip.ptr(idx), P, float(tol),
                                      POSITIONS[position], C.byref(st), stream), "tnp_weld_build")
        stats = st.as_dict()
        vmap = torch.empty(V, dtype=torch.int64, device=dev)
        pos = torch.empty((V, 3), dtype=torch.float32, device=dev)
        ooff = torch.empty(stats["n_polygons"] + 1, dtype=torch.int64, device=dev)
        oidx = torch.empty(stats["n_indices"], dtype=torch.int64, device=dev)
        src = torch.empty(stats["n_polygons"], dtype=torch.int64, device=dev)
        _hip.check(lib.tnp_weld_export(hd.h, _hip.ptr(vmap), _hip.ptr(pos), _hip.ptr(ooff), _hip.ptr(oidx),
                                       _hip.ptr(src), stream), "tnp_weld_export")
        times = stage_ms(lib.tnp_debug_weld_stages, hd, STAGES) if timed else None
        out = [t.cpu().numpy() for t in (vmap, pos, ooff, oidx, src)]
    finally:
        if own:
            hd.close()
    return WeldResult(*out, stats, times)


def weld(pmesh: PolygonMesh, tol: float, position: str = "first", compact: bool = True):
    """Weld a PolygonMesh: ``(welded, stats)``.  The polygons that survive keep
    their order and their normals; compact drops the vertices no polygon uses
    any more and keeps the rest in order (as `keep_components` does), else the
    vertex array keeps its length and the merged vertices stay behind unused."""
    if not (isinstance(tol, (int, float, np.floating, np.integer)) and math.isfinite(tol) and tol >= 0):
        raise ValueError(f"tol = {tol!r} (finite, >= 0)")
    res = weld_vertices(pmesh.vertices, pmesh.offsets, pmesh.indices, tol, position)
    verts, idx = res.positions.astype(pmesh.vertices.dtype), res.indices
    if compact:
        used = np.zeros(len(verts), dtype=bool)
        used[idx] = True
        remap = np.cumsum(used) - 1
        verts, idx = verts[used], remap[idx]
    normals = None if pmesh.normals is None else pmesh.normals[res.source]
    return PolygonMesh(verts, res.offsets, idx, normals), res.stats
