"""Stage times of one tnp_holes_build on the synth64h surface (the 64^3
hashed lattice after all 33 steps, as tools/topology_kernel_ms.py), both cap
modes, and tnp_topology_build on the same input in the same run -- the
topology is the yardstick: the holes share its front half (checks, edge keys,
sort, boundary union) and add the status pass and the list ranking.
    python tools/holes_kernel_ms.py
One JSON line: the build's stage times (events between the stages, one build;
the stages are listed in include/tropical_hip_debug.h), wall times (median of
5, stream-synchronised) of the build + export, of each cap mode, of
polygon_topology, and the ratio of the build to the topology."""
import json

from soup_surface import synth64h_surface, wall  # (first: it sets the import path)
from tropical.utils.topology import (boundary_cycles, cycle_caps, holes_handle, polygon_topology,  # noqa: E402
                                     topology_handle)

_, verts, off, idx = synth64h_surface()
V = int(verts.shape[0])
th, hh = topology_handle(), holes_handle()
topo = polygon_topology(verts, off, idx, handle=th)  # (warm: the allocator's pools, the sorts' first launch)
boundary_cycles(V, off, idx, handle=hh)
stage_ms = boundary_cycles(V, off, idx, handle=hh, timed=True).stage_ms
t_build = wall(lambda: boundary_cycles(V, off, idx, handle=hh))
t_build6 = wall(lambda: boundary_cycles(V, off, idx, max_edges=6, handle=hh))
cyc = boundary_cycles(V, off, idx, handle=hh)  # (the caps below are those of max_edges = 0)
t_poly = wall(lambda: cycle_caps(hh, cyc, "polygon"))
t_star = wall(lambda: cycle_caps(hh, cyc, "star", verts))
t_topo = wall(lambda: polygon_topology(verts, off, idx, handle=th))
th.close()
hh.close()
rounds = max(cyc.stats["longest_capped"] - 1, 0).bit_length()
out = {"config": "synth64h surface", "V": V, "n_poly": int(off.numel() - 1), "n_idx": int(idx.numel()),
       "n_loops_topology": topo.n_loops, "stats": cyc.stats, "doubling_rounds": rounds,
       "stage_ms": {k: round(v, 4) for k, v in stage_ms.items()},
       "stage_ms_total": round(sum(stage_ms.values()), 4),
       "holes_build_wall_ms": t_build, "holes_build_max6_wall_ms": t_build6, "caps_polygon_wall_ms": t_poly,
       "caps_star_wall_ms": t_star, "topology_edge_wall_ms": t_topo,
       "ratio_to_topology": round(t_build / t_topo, 2)}
print(json.dumps(out), flush=True)
