"""Kernel times of faces + polygons + the polygon report on the synth64h
complex (the 64^3 hashed lattice after all 33 steps, as bench.finish_check):
    python tools/polygons_kernel_ms.py
One JSON line: the engine's kernel timer over faces() then polygons() (the
faces_* entries; faces_poly_emit is F6, faces_fan_emit F5 for both outputs),
and wall times (median of 5, stream-synchronised) of polygons() alone on
cached rows and of polygon_report() on the result."""
import json

from soup_surface import synth64h_surface, wall  # (first: it sets the import path)
from tropical.utils.mesh import polygon_report  # noqa: E402

eng, verts, _, _ = synth64h_surface()  # (grows the buffers)
eng.kernel_timer(True)
tri, _ = eng.faces()
off, idx, nrm = eng.polygons()
kt = eng.kernel_timer(False)
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
