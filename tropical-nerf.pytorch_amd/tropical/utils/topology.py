"""Connected components and boundary loops of a polygon complex on the GPU
(csrc/topology.hip; the definitions are in include/tropical_hip.h), and the
plumbing around them: keep some components, pick the largest.

    topo = polygon_topology(pm.vertices, pm.offsets, pm.indices)      # connect="edge" | "vertex"
    topo.n_components, topo.n_loops
    topo.labels                       # int32 [P] on the device
    topo.components["area"]           # numpy structured arrays, one row per component / loop
    main = keep_components(pm, topo.labels, largest_components(topo.components, 1))
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .mesh import PolygonMesh

# the rows of tnp_component / tnp_boundary_loop
COMPONENT_DTYPE = np.dtype([(k, "<i8") for k in ("first_polygon", "n_polygons", "n_indices", "n_vertices", "n_edges",
                                                  "e_boundary", "e_manifold", "e_nonmanifold", "e_misoriented",
                                                  "euler")]
                           + [("area", "<f8"), ("volume", "<f8"), ("lo", "<f4", (3,)), ("hi", "<f4", (3,))])
LOOP_DTYPE = np.dtype([(k, "<i8") for k in ("first_vertex", "n_edges", "n_vertices", "component")]
                      + [("length", "<f8"), ("simple", "<i4"), ("reserved", "<i4")])
assert COMPONENT_DTYPE.itemsize == 120 and LOOP_DTYPE.itemsize == 48
CONNECT = {"edge": 0, "vertex": 1}
STAGES = ("check_edges", "edge_sort", "label_polygons", "label_boundary", "tables_alloc", "component_counts",
          "vertex_sort", "polygon_order", "geometry", "loops")


class PolygonTopology:
    """``labels`` (device int32 [P], the component of every polygon),
    ``components`` / ``loops`` (numpy structured arrays, COMPONENT_DTYPE /
    LOOP_DTYPE), ``n_components``, ``n_loops``, ``connect``; ``stage_ms``
    when the build was timed."""

    def __init__(self, labels, components, loops, connect, stage_ms=None):
        self.labels, self.components, self.loops, self.connect = labels, components, loops, connect
        self.stage_ms = stage_ms

    @property
    def n_components(self) -> int:
        return len(self.components)

    @property
    def n_loops(self) -> int:
        return len(self.loops)


class _Handle:
    def __init__(self, dev):
        from .. import _hip
        self._hip, self.h = _hip, C.c_void_p()
        _hip.check(_hip.lib().tnp_topology_create(C.byref(self.h), dev.index), "tnp_topology_create")

    def close(self):
        if self.h:
            self._hip.lib().tnp_topology_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def polygon_topology(vertices, offsets, indices, connect: str = "edge", timed: bool = False,
                     handle: "_Handle | None" = None) -> PolygonTopology:
    """Label the components of a polygon soup and trace its boundary loops
    (tnp_topology_build / tnp_topology_export).  connect: "edge" (polygons
    sharing an undirected edge) or "vertex" (sharing a vertex id).  numpy
    arrays or tensors, as polygon_report takes them; host inputs are moved to
    the current device.  Malformed input raises RuntimeError naming the first
    offender.  timed: record the build's stage times (``stage_ms``, a dict).
    handle: a `topology_handle()` to build on (else one is made and closed)."""
    import torch

    from .. import _hip
    if connect not in CONNECT:
        raise ValueError(f"connect = {connect!r} (edge, vertex)")
    dev = torch.device("cuda", torch.cuda.current_device())

    def t(x, dtype):
        x = x.detach() if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
        return x.to(dev, dtype).contiguous()

    v, off, idx = t(vertices, torch.float32).reshape(-1, 3), t(offsets, torch.int64), t(indices, torch.int64)
    P = off.numel() - 1
    if P < 0:
        raise ValueError("offsets holds P + 1 entries")
    if P > 0 and idx.numel() < int(off[-1]):  # (the library reads indices[:offsets[-1]])
        raise ValueError(f"offsets end at {int(off[-1])}, only {idx.numel()} indices given")
    own = handle is None
    hd = _Handle(dev) if own else handle
    try:
        lib, stream = _hip.lib(), C.c_void_p(_hip.stream_ptr(dev))
        if timed:
            lib.tnp_debug_topology_stages(hd.h, 1, None, 0)
        nc, nl = C.c_int64(), C.c_int64()
        _hip.check(lib.tnp_topology_build(hd.h, _hip.ptr(v), v.shape[0], _hip.ptr(off), _hip.ptr(idx), P,
                                          CONNECT[connect], C.byref(nc), C.byref(nl), stream), "tnp_topology_build")
        labels = torch.empty(P, dtype=torch.int32, device=dev)
        comps = torch.empty(nc.value * COMPONENT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        loops = torch.empty(nl.value * LOOP_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        _hip.check(lib.tnp_topology_export(hd.h, _hip.ptr(labels), _hip.ptr(comps), _hip.ptr(loops), stream),
                   "tnp_topology_export")
        stage_ms = None
        if timed:
            ms = (C.c_double * len(STAGES))()
            lib.tnp_debug_topology_stages(hd.h, 0, ms, len(STAGES))
            stage_ms = dict(zip(STAGES, (float(x) for x in ms)))
        comps_h = comps.cpu().numpy().view(COMPONENT_DTYPE).copy()
        loops_h = loops.cpu().numpy().view(LOOP_DTYPE).copy()
    finally:
        if own:
            hd.close()
    return PolygonTopology(labels, comps_h, loops_h, connect, stage_ms)


def topology_handle():
    """A tnp_topology handle on the current device for repeated builds
    (``polygon_topology(..., handle=h)``); ``h.close()`` frees it."""
    import torch
    return _Handle(torch.device("cuda", torch.cuda.current_device()))


def largest_components(components, n: int, by: str = "area") -> np.ndarray:
    """The ids of the n largest components by column `by` (``area``,
    ``n_polygons``, ...; |volume| for ``volume``), largest first; ties go to
    the lower id."""
    key = np.asarray(components[by])
    if by == "volume":
        key = np.abs(key)
    order = np.argsort(-key.astype(np.float64), kind="stable")  # stable: equal keys keep ascending ids
    return order[:max(int(n), 0)].astype(np.int64)


def keep_components(pmesh: PolygonMesh, labels, ids) -> PolygonMesh:
    """The polygons of the listed components, in their order; vertices no kept
    polygon uses are dropped, the rest keep their order; normals are carried
    along.  labels: [P] (numpy or tensor)."""
    lab = labels.detach().cpu().numpy() if hasattr(labels, "detach") else np.asarray(labels)
    lab = lab.reshape(-1)
    if len(lab) != len(pmesh):
        raise ValueError(f"{len(lab)} labels for {len(pmesh)} polygons")
    keep = np.isin(lab, np.asarray(ids, dtype=np.int64).reshape(-1))
    deg = pmesh.degrees()
    idx = pmesh.indices[np.repeat(keep, deg)]
    used = np.zeros(len(pmesh.vertices), dtype=bool)
    used[idx] = True
    remap = np.cumsum(used) - 1
    offsets = np.concatenate([[0], np.cumsum(deg[keep])]).astype(np.int64)
    return PolygonMesh(pmesh.vertices[used], offsets, remap[idx],
                       None if pmesh.normals is None else pmesh.normals[keep])
