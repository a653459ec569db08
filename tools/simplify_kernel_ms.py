"""Stage times of tnp_simplify_build on the synth64h surface (the 64^3 hashed
lattice after all 33 steps, as tools/weld_kernel_ms.py), both position modes at
cell = 1, 2 and 4 x the surface's median edge length (the edges of its
polygons, measured here), and tnp_weld_build and tnp_topology_build on the same
input in the same run for scale.
    python tools/simplify_kernel_ms.py
One JSON line: per cell and mode the stats, the stage times (events between the
stages, one build; the stages are listed in include/tropical_hip_debug.h) and
the wall time (median of 5, stream-synchronised) of the build + export; the
wall times of weld_vertices (first, tol = 0.05 x the median edge) and of
polygon_topology."""
import json

import numpy as np

from soup_surface import synth64h_surface, wall  # (first: it sets the import path)
from tropical.utils.simplify import cluster_vertices, simplify_handle  # noqa: E402
from tropical.utils.topology import polygon_topology, topology_handle  # noqa: E402
from tropical.utils.weld import weld_handle, weld_vertices  # noqa: E402

FACTORS = (1, 2, 4)

_, verts, off, idx = synth64h_surface()
v, o, i = verts.cpu().numpy(), off.cpu().numpy(), idx.cpu().numpy()
nxt = np.arange(len(i)) + 1
nxt[o[1:] - 1] = o[:-1]
edge = np.sqrt(((v[i].astype(np.float64) - v[i[nxt]].astype(np.float64)) ** 2).sum(1))
median_edge = float(np.median(edge))
th, wh, sh = topology_handle(), weld_handle(), simplify_handle()
polygon_topology(verts, off, idx, handle=th)  # (warm: the allocator's pools, the sorts' first launch)
out = {"config": "synth64h surface", "V": int(verts.shape[0]), "n_poly": int(off.numel() - 1),
       "n_idx": int(idx.numel()), "median_edge": median_edge, "runs": []}
for f in FACTORS:
    cell = float(np.float32(f * median_edge))
    for position in ("mean", "nearest"):
        cluster_vertices(verts, off, idx, cell, position, handle=sh)
        res = cluster_vertices(verts, off, idx, cell, position, handle=sh, timed=True)
        out["runs"].append({
            "cell_factor": f, "cell": cell, "position": position, "stats": res.stats,
            "stage_ms": {k: round(t, 4) for k, t in res.stage_ms.items()},
            "stage_ms_total": round(sum(res.stage_ms.values()), 4),
            "wall_ms": wall(lambda: cluster_vertices(verts, off, idx, cell, position, handle=sh))})
tol = float(np.float32(0.05 * median_edge))
weld_vertices(verts, off, idx, tol, "first", handle=wh)
out["weld_first_wall_ms"] = wall(lambda: weld_vertices(verts, off, idx, tol, "first", handle=wh))
out["topology_edge_wall_ms"] = wall(lambda: polygon_topology(verts, off, idx, handle=th))
for h in (th, wh, sh):
    h.close()
print(json.dumps(out), flush=True)
