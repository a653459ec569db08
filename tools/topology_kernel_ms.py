"""Stage times of one tnp_topology_build on the synth64h surface (the 64^3
hashed lattice after all 33 steps, as tools/polygons_kernel_ms.py), next to
tnp_polygon_report on the same input -- the report is the yardstick: the
topology does the report's sort plus two labellings and two small sorts.
    python tools/topology_kernel_ms.py
One JSON line: the build's stage times (events between the stages, one
build; the stages are listed in include/tropical_hip_debug.h), wall times
(median of 5, stream-synchronised) of polygon_topology in both modes and of
polygon_report, and their ratio."""
import json

from soup_surface import synth64h_surface, wall  # (first: it sets the import path)
from tropical.utils.mesh import polygon_report  # noqa: E402
from tropical.utils.topology import polygon_topology, topology_handle  # noqa: E402

_, verts, off, idx = synth64h_surface()
h = topology_handle()
polygon_topology(verts, off, idx, handle=h)  # (warm: the allocator's pools, the sorts' first launch)
polygon_report(verts, off, idx)
topo = polygon_topology(verts, off, idx, handle=h, timed=True)
t_edge = wall(lambda: polygon_topology(verts, off, idx, handle=h))
t_vert = wall(lambda: polygon_topology(verts, off, idx, connect="vertex", handle=h))
t_rep = wall(lambda: polygon_report(verts, off, idx))
h.close()
big = topo.components[int(topo.components["area"].argmax())]
out = {"config": "synth64h surface", "V": int(verts.shape[0]), "n_poly": int(off.numel() - 1),
       "n_idx": int(idx.numel()), "n_components": topo.n_components, "n_loops": topo.n_loops,
       "largest_component_polygons": int(big["n_polygons"]),
       "stage_ms": {k: round(v, 4) for k, v in topo.stage_ms.items()},
       "stage_ms_total": round(sum(topo.stage_ms.values()), 4),
       "topology_edge_wall_ms": t_edge, "topology_vertex_wall_ms": t_vert, "polygon_report_wall_ms": t_rep,
       "ratio_to_report": round(t_edge / t_rep, 2)}
print(json.dumps(out), flush=True)
