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
import os
import statistics
import sys
import time

sys.path[:0] = [os.getcwd(), os.path.join(os.getcwd(), "tropical-nerf.pytorch_amd"),
                os.path.join(os.getcwd(), "tests")]
import torch  # noqa: E402

from golden_io import load  # noqa: E402
from helpers import product_net  # noqa: E402
from tropical._engine import engine_for  # noqa: E402
from tropical.utils.mesh import polygon_report  # noqa: E402
from tropical.utils.topology import polygon_topology, topology_handle  # noqa: E402

dev = torch.device("cuda", 0)
net = product_net(load("synth64h"), dev)
eng = engine_for(net)
eng.lattice()
eng.run_steps([])
eng.surface()
verts, _, _ = eng.export(edges=False)
eng.faces()
off, idx, nrm = eng.polygons()


def wall(fn, reps=5):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize(dev)
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize(dev)
        ts.append((time.perf_counter() - t) * 1e3)
    return round(statistics.median(ts), 4)


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
