"""Stage times of one tnp_weld_build on the synth64h surface (the 64^3 hashed
lattice after all 33 steps, as tools/topology_kernel_ms.py), both position
modes at one tolerance, and tnp_topology_build on the same input in the same
run -- the topology is the yardstick: it is what runs next on the welded soup.
    python tools/weld_kernel_ms.py
The tolerance is TOL_FRACTION of the surface's median edge length (the edges
of its polygons, measured here).  One JSON line: the stage times of each mode
(events between the stages, one build; the stages are listed in
include/tropical_hip_debug.h), wall times (median of 5, stream-synchronised)
of the build + export per mode, at tol = 0 and of polygon_topology, and the
ratio of the mode-0 build to the topology."""
import json

import numpy as np

from soup_surface import synth64h_surface, wall  # (first: it sets the import path)
from tropical.utils.topology import polygon_topology, topology_handle  # noqa: E402
from tropical.utils.weld import weld_handle, weld_vertices  # noqa: E402

TOL_FRACTION = 0.05

_, verts, off, idx = synth64h_surface()
v, o, i = verts.cpu().numpy(), off.cpu().numpy(), idx.cpu().numpy()
nxt = np.arange(len(i)) + 1
nxt[o[1:] - 1] = o[:-1]
edge = np.sqrt(((v[i].astype(np.float64) - v[i[nxt]].astype(np.float64)) ** 2).sum(1))
median_edge = float(np.median(edge))
tol = float(np.float32(TOL_FRACTION * median_edge))
th, wh = topology_handle(), weld_handle()
polygon_topology(verts, off, idx, handle=th)  # (warm: the allocator's pools, the sorts' first launch)
out = {"config": "synth64h surface", "V": int(verts.shape[0]), "n_poly": int(off.numel() - 1),
       "n_idx": int(idx.numel()), "median_edge": median_edge, "tol_fraction": TOL_FRACTION, "tol": tol}
for position in ("first", "mean"):
    weld_vertices(verts, off, idx, tol, position, handle=wh)
    res = weld_vertices(verts, off, idx, tol, position, handle=wh, timed=True)
    out[f"stats_{position}"] = res.stats
    out[f"stage_ms_{position}"] = {k: round(t, 4) for k, t in res.stage_ms.items()}
    out[f"stage_ms_{position}_total"] = round(sum(res.stage_ms.values()), 4)
    out[f"weld_{position}_wall_ms"] = wall(lambda: weld_vertices(verts, off, idx, tol, position, handle=wh))
out["weld_tol0_wall_ms"] = wall(lambda: weld_vertices(verts, off, idx, 0.0, "first", handle=wh))
out["topology_edge_wall_ms"] = wall(lambda: polygon_topology(verts, off, idx, handle=th))
out["ratio_to_topology"] = round(out["weld_first_wall_ms"] / out["topology_edge_wall_ms"], 2)
th.close()
wh.close()
print(json.dumps(out), flush=True)
