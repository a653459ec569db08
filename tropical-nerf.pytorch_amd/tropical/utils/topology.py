"""Connected components and boundary loops of a polygon complex on the GPU
(csrc/topology.hip; the definitions are in include/tropical_hip.h), and the
plumbing around them: keep some components, pick the largest.

    topo = polygon_topology(pm.vertices, pm.offsets, pm.indices)      # connect="edge" | "vertex"
    topo.n_components, topo.n_loops
    topo.labels                       # int32 [P] on the device
    topo.components["area"]           # numpy structured arrays, one row per component / loop
    main = keep_components(pm, topo.labels, largest_components(topo.components, 1))

and the repair of the simple holes (csrc/holes.hip):

    cyc = boundary_cycles(pm.vertices, pm.offsets, pm.indices)        # ordered loops, status per loop
    filled, stats = fill_holes(main, max_edges=6)                     # mode="polygon" | "star"
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .mesh import PolygonMesh
from .soup import Handle, current_device, soup_on_device, stage_ms, to_device

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
HOLE_STATUS = {"capped": 0, "nonsimple": 1, "unoriented": 2, "too_long": 3}
HOLE_STAGES = ("check_edges", "edge_sort", "label_boundary", "status", "compact", "rank", "scatter")
CAP_MODES = {"polygon": 0, "star": 1}


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


def polygon_topology(vertices, offsets, indices, connect: str = "edge", timed: bool = False,
                     handle: "Handle | None" = None) -> PolygonTopology:
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
    dev = current_device()
    v, off, idx, P = soup_on_device(vertices, offsets, indices, dev)
    own = handle is None
    hd = _topology_handle(dev) if own else handle
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
        times = stage_ms(lib.tnp_debug_topology_stages, hd, STAGES) if timed else None
        comps_h = comps.cpu().numpy().view(COMPONENT_DTYPE).copy()
        loops_h = loops.cpu().numpy().view(LOOP_DTYPE).copy()
    finally:
        if own:
            hd.close()
    return PolygonTopology(labels, comps_h, loops_h, connect, times)


def topology_handle():
    """A tnp_topology handle on the current device for repeated builds
    (``polygon_topology(..., handle=h)``); ``h.close()`` frees it."""
    return _topology_handle(current_device())


def _topology_handle(dev):
    return Handle(dev, "tnp_topology_create", "tnp_topology_destroy")


def _holes_handle(dev):
    return Handle(dev, "tnp_holes_create", "tnp_holes_destroy")


class BoundaryCycles:
    """The boundary loops of a soup as ordered cycles (tnp_holes_*): ``status``
    (numpy int32 [L], HOLE_STATUS by loop number), ``cycle_loop`` (int64 [K],
    the loop number of cycle k), ``offsets`` (int64 [K + 1]), ``vertices``
    (int64: cycle k is ``vertices[offsets[k]:offsets[k + 1]]``, from the loop's
    smallest id on, against the direction of the polygons along it), ``stats``
    (dict, tnp_hole_stats); ``stage_ms`` when the build was timed."""

    def __init__(self, status, cycle_loop, offsets, vertices, stats, stage_ms=None):
        self.status, self.cycle_loop, self.offsets, self.vertices = status, cycle_loop, offsets, vertices
        self.stats, self.stage_ms = stats, stage_ms

    def __len__(self):
        return len(self.cycle_loop)


def holes_handle():
    """A tnp_holes handle on the current device for repeated builds
    (``boundary_cycles(..., handle=h)``); ``h.close()`` frees it."""
    return _holes_handle(current_device())


def _build_cycles(hd, dev, V, offsets, indices, max_edges, timed=False):
    """tnp_holes_build + tnp_holes_export -> BoundaryCycles."""
    import torch

    from .. import _hip
    lib, stream = _hip.lib(), C.c_void_p(_hip.stream_ptr(dev))
    _, off, idx, P = soup_on_device(None, offsets, indices, dev)
    if timed:
        lib.tnp_debug_holes_stages(hd.h, 1, None, 0)
    st = _hip.TnpHoleStats()
    _hip.check(lib.tnp_holes_build(hd.h, V, _hip.ptr(off), _hip.ptr(idx), P, int(max_edges), C.byref(st), stream),
               "tnp_holes_build")
    stats = st.as_dict()
    status = torch.empty(stats["n_loops"], dtype=torch.int32, device=dev)
    loop = torch.empty(stats["n_capped"], dtype=torch.int64, device=dev)
    coff = torch.empty(stats["n_capped"] + 1, dtype=torch.int64, device=dev)
    cv = torch.empty(stats["n_cycle_indices"], dtype=torch.int64, device=dev)
    _hip.check(lib.tnp_holes_export(hd.h, _hip.ptr(status), _hip.ptr(loop), _hip.ptr(coff), _hip.ptr(cv), stream),
               "tnp_holes_export")
    times = stage_ms(lib.tnp_debug_holes_stages, hd, HOLE_STAGES) if timed else None
    return BoundaryCycles(status.cpu().numpy(), loop.cpu().numpy(), coff.cpu().numpy(), cv.cpu().numpy(), stats, times)


def _caps(hd, dev, mode, stats, xyz):
    """tnp_holes_caps of the build held -> (offsets, indices, new vertices fp32 [S, 3]) as numpy."""
    import torch

    from .. import _hip
    K, M, nt = stats["n_capped"], stats["n_cycle_indices"], stats["n_triangles"]
    n_cap, n_idx, n_new = (K, M, 0) if mode == "polygon" else (nt + M - 3 * nt, 3 * (nt + M - 3 * nt), K - nt)
    coff = torch.empty(n_cap + 1, dtype=torch.int64, device=dev)
    cidx = torch.empty(n_idx, dtype=torch.int64, device=dev)
    new = torch.empty((n_new, 3), dtype=torch.float32, device=dev)
    _hip.check(_hip.lib().tnp_holes_caps(hd.h, CAP_MODES[mode], _hip.ptr(xyz), _hip.ptr(coff), _hip.ptr(cidx),
                                         _hip.ptr(new), C.c_void_p(_hip.stream_ptr(dev))), "tnp_holes_caps")
    return coff.cpu().numpy(), cidx.cpu().numpy(), new.cpu().numpy()


def boundary_cycles(vertices, offsets, indices, max_edges: int = 0, handle: "Handle | None" = None,
                    timed: bool = False) -> BoundaryCycles:
    """The soup's boundary loops, classified and put into cyclic order
    (tnp_holes_build / tnp_holes_export; include/tropical_hip.h has the
    definitions).  A loop's number is its row in ``polygon_topology(...).loops``.
    vertices: the coordinates or just their number V (none are read).
    max_edges > 0 leaves longer loops open.  Malformed input raises
    RuntimeError naming the first offender.  handle: a `holes_handle()` to
    build on (else one is made and closed); its caps are `cycle_caps`'."""
    dev = current_device()
    V = int(vertices) if np.isscalar(vertices) else int(np.prod(tuple(vertices.shape))) // 3
    own = handle is None
    hd = _holes_handle(dev) if own else handle
    try:
        return _build_cycles(hd, dev, V, offsets, indices, max_edges, timed)
    finally:
        if own:
            hd.close()


def cycle_caps(handle: Handle, cycles: BoundaryCycles, mode: str = "polygon", vertices=None):
    """The caps of the build `handle` holds (tnp_holes_caps) as numpy
    ``(offsets, indices, new_vertices)``; mode "star" reads `vertices` (the
    soup's V x 3 coordinates) and returns the fp32 centres it adds."""
    import torch
    if mode not in CAP_MODES:
        raise ValueError(f"mode = {mode!r} (polygon, star)")
    dev = current_device()
    xyz = None
    if mode == "star":
        if vertices is None:
            raise ValueError("mode = 'star' needs the vertices")
        xyz = to_device(vertices, dev, torch.float32).reshape(-1, 3)
    return _caps(handle, dev, mode, cycles.stats, xyz)


def newell_normals(vertices, offsets, indices) -> np.ndarray:
    """Unit Newell normals of polygons (float32 [P, 3]; zero where the polygon
    has no area), in float64 from the coordinates given."""
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    off, idx = np.asarray(offsets, np.int64), np.asarray(indices, np.int64)
    if len(off) <= 1:
        return np.zeros((0, 3), np.float32)
    nxt = np.arange(len(idx)) + 1
    nxt[off[1:] - 1] = off[:-1]
    N = np.add.reduceat(np.cross(v[idx], v[idx[nxt]]), off[:-1], axis=0)
    ln = np.sqrt((N * N).sum(1, keepdims=True))
    return (N / np.where(ln > 0, ln, 1.0)).astype(np.float32)


def append_caps(pmesh: PolygonMesh, cap_offsets, cap_indices, new_vertices=None) -> PolygonMesh:
    """The filled soup: pmesh's polygons followed by the caps, its vertices
    followed by the new ones; with normals, each cap row gets its Newell normal."""
    cap_offsets, cap_indices = np.asarray(cap_offsets, np.int64), np.asarray(cap_indices, np.int64)
    verts = pmesh.vertices
    if new_vertices is not None and len(new_vertices):
        verts = np.concatenate([verts, np.asarray(new_vertices, np.float64).reshape(-1, 3)])
    offsets = np.concatenate([pmesh.offsets, pmesh.offsets[-1] + cap_offsets[1:]])
    indices = np.concatenate([pmesh.indices, cap_indices])
    normals = None
    if pmesh.normals is not None:
        normals = np.concatenate([pmesh.normals, newell_normals(verts, cap_offsets, cap_indices)])
    return PolygonMesh(verts, offsets, indices, normals)


def fill_holes(pmesh: PolygonMesh, max_edges: int = 0, mode: str = "polygon"):
    """Close the simple, consistently oriented boundary loops of a PolygonMesh
    (those of at most max_edges edges when max_edges > 0): ``(filled, stats)``.
    mode "polygon": one polygon per loop, no new vertex; "star": a triangle
    fan about the loop's mean vertex (a 3-loop is its own triangle).  The
    filled mesh lists pmesh's polygons and vertices first; non-simple and
    unoriented loops are counted in ``stats`` and left open."""
    import torch
    if mode not in CAP_MODES:
        raise ValueError(f"mode = {mode!r} (polygon, star)")
    dev = current_device()
    xyz = to_device(pmesh.vertices, dev, torch.float32).reshape(-1, 3) if mode == "star" else None
    hd = _holes_handle(dev)
    try:
        cyc = _build_cycles(hd, dev, len(pmesh.vertices), pmesh.offsets, pmesh.indices, max_edges)
        coff, cidx, new = _caps(hd, dev, mode, cyc.stats, xyz)
    finally:
        hd.close()
    return append_caps(pmesh, coff, cidx, new), cyc.stats


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
