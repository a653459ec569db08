"""Kernel times of faces + polygons + the polygon report on the synth64h
complex (the 64^3 hashed lattice after all 33 steps, as bench.finish_check):
    python tools/polygons_kernel_ms.py
One JSON line: the engine's kernel timer over faces() then polygons() (the
faces_* entries; faces_poly_emit is F6, faces_fan_emit F5 for both outputs),
and wall times (median of 5, stream-synchronised) of polygons() alone on
cached rows and of polygon_report() on the result."""
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

dev = torch.device("cuda", 0)
net = product_net(load("synth64h"), dev)
eng = engine_for(net)
eng.lattice()
eng.run_steps([])
eng.surface()
verts, _, _ = eng.export(edges=False)
eng.faces()
eng.polygons()  # (grows the buffers)
eng.kernel_timer(True)
tri, _ = eng.faces()
off, idx, nrm = eng.polygons()
kt = eng.kernel_timer(False)


def wall(fn, reps=5):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize(dev)
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize(dev)
        ts.append((time.perf_counter() - t) * 1e3)
    return round(statistics.median(ts), 4)


rep = polygon_report(verts, off, idx)
out = {"config": "synth64h surface", "V": int(verts.shape[0]), "n_tri": int(tri.shape[0]),
       "n_poly": int(off.numel() - 1), "n_idx": int(idx.numel()),
       "faces_kernels": {k: {"ms": round(v["ms"], 4), "GBps": round(v["bytes"] / max(v["ms"], 1e-9) / 1e6, 1),
                             "launches": v["launches"]}
                         for k, v in sorted(kt.items(), key=lambda kv: -kv[1]["ms"]) if k.startswith("faces") or k == "scan"},
       "polygons_cached_rows_wall_ms": wall(lambda: eng.polygons()),
       "polygon_report_wall_ms": wall(lambda: polygon_report(verts, off, idx)),
       "polygon_report_per_polygon_wall_ms": wall(lambda: polygon_report(verts, off, idx, per_polygon=True)),
       "report": rep}
print(json.dumps(out), flush=True)
