"""Render times on the synth64h surface (the 64^3 hashed lattice after all 33
steps, as tools/polygons_kernel_ms.py builds it: 1.84 M fan triangles) at
2048 x 2048 with ssaa = 2 (a 4096 x 4096 raster), and on the small_sphere
surface at 1024 x 1024:
    python tools/render_kernel_ms.py [--png DIR]
One JSON line per surface: wall times (median of 5, stream-synchronised) of
tnp_render_raster (validation, projection, both coverage paths, resolve, with
its scratch allocation and readbacks) and of tnp_render_shade, the raster's
stats, and the rates triangles/s and covered raster pixels/s of the raster
call (profiles/render_kernel_ms.log).  The wall times hold the scratch
allocation, three readbacks and the launches; the kernels' own times are the
k_rv_* / k_soup_offsets / k_scan_lb / k_fill rows of a rocprofv3 kernel trace
of this tool,
    rocprofv3 --kernel-trace --stats -d DIR -o run --output-format csv -- python tools/render_kernel_ms.py
recorded as profiles/render_kernel_stats.csv (both surfaces, 6 raster and 6
shade calls each).  --png DIR also writes the two figures."""
import json
import os
import sys

from soup_surface import dev, synth64h_surface, wall  # (first: it sets the import path)
import torch  # noqa: E402

from helpers import product_net  # noqa: E402
from golden_io import load  # noqa: E402
from tropical.utils.image import write_png  # noqa: E402
from tropical.utils.render import Camera, newell_normals, rasterize, render, shade  # noqa: E402
from tropical.utils.colormap import lut  # noqa: E402

png_dir = sys.argv[sys.argv.index("--png") + 1] if "--png" in sys.argv else None


def measure(name, verts, off, idx, size, ssaa):
    W, H = size[0] * ssaa, size[1] * ssaa
    cam = Camera.from_angles(15, 120).fit(verts, size[0], size[1])
    soup = (verts.to(dev, torch.float32).contiguous(), off.to(dev), idx.to(dev), None)
    hw = 8 * ssaa
    buf = rasterize(soup, cam, (W, H), scale_by=ssaa, edge_half_width=hw)  # (and the first call's allocations)
    value = newell_normals(soup[0], soup[1], soup[2])[:, 2]
    table = torch.from_numpy(lut("plasma")).to(dev)
    raster_ms = wall(lambda: rasterize(soup, cam, (W, H), scale_by=ssaa, edge_half_width=hw))
    shade_ms = wall(lambda: shade(buf["prim"], buf["edge"], value, -1.0, 1.0, table, ss=ssaa))
    st = buf["stats"]
    out = {"config": name, "image": list(size), "ssaa": ssaa, "raster": [W, H], "V": int(verts.shape[0]),
           "stats": st, "raster_wall_ms": raster_ms, "shade_wall_ms": shade_ms,
           "triangles_per_s": round(st["n_triangles"] / (raster_ms * 1e-3)),
           "covered_pixels_per_s": round(st["pixels_covered"] / (raster_ms * 1e-3))}
    print(json.dumps(out), flush=True)
    if png_dir:
        write_png(os.path.join(png_dir, f"{name}.png"),
                  render(soup[:3], cam, size=size, ssaa=ssaa, value=value))


_, verts, off, idx = synth64h_surface()
measure("synth64h", verts, off, idx, (2048, 2048), 2)

import tropical.subpoly as sp  # noqa: E402

net = product_net(load("small_sphere"), dev)
_, verts, _, pm = sp.subpoly(net, 3, 1.2, force=True, polygons=True)
measure("small_sphere", verts, torch.from_numpy(pm.offsets), torch.from_numpy(pm.indices), (1024, 1024), 1)
