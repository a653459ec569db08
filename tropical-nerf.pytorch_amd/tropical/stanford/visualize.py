"""python -m tropical.stanford.visualize -- the reference's figures
(tropical/stanford/visualize.py) on the MI355X path: every mesh a `train`
run (`--polygons` for the polygon file) and an `evaluate` run left under
{out}/{d}/ is drawn shaded by a component of its face normals (plasma) on a
transparent background and written as a PNG under {png_dir}/{d}/:

    our_poly_mesh_{m}_{s}.ply  (preferred; polygon boundaries drawn over it)
    our_mesh_{m}_{s}.ply       (when there is no polygon file)      -> {m}_ours.png
    mc{i:03d}_mesh_{m}_{s}.ply, mtet{i:03d}_mesh_{m}_{s}.ply        -> {m}_mc{i:03d}.png, {m}_mtet{i:03d}.png

Flags: -d dataset, -s seed, -m model size, --out DIR (the mesh directory), as
`evaluate` has them; --size W H, --ssaa 1|2|4, --no-edges, --view ELEV AZIM
(instead of the dataset's), --persp, --png-dir DIR (default `outputs`);
--color component writes one more image of the polygon file,
{m}_poly_components.png: the same raster, every polygon coloured by its
edge-connected component's rank by area (tropical.utils.topology) through a
qualitative table that repeats above 255.

The reference draws with matplotlib's plot_trisurf and crops the figure; here
csrc/render.hip rasterises the mesh and the camera is fitted to the box around
all the meshes of the run, so its figures share a view.  Colours map the normal
component over the fixed range [-1, 1] (the reference normalises min..max per
figure).  Nothing runs at import: `parse_args(argv)` and `main(argv)`.
"""
from __future__ import annotations

import argparse
import glob
import os
import re
import sys

import numpy as np
import torch

# per dataset: view_init(elev, azim, roll, vertical_axis), whether the
# reference plots (x, z, y) instead of (x, y, z), its projection and the
# normal component it colours by -- the numbers of the reference's
# visualize_mesh (visualize.py:19-64), restated
VIEWS = {
    "dragon": (15, -10, 10, "y", False, "persp", "z"),
    "armadillo": (15, -60, 0, "z", True, "ortho", "-z"),
    "happy": (10, 120, 0, "z", True, "ortho", "z"),
    "drill": (10, 120, 0, "z", True, "ortho", "z"),
    "lucy": (5, 110, 0, "z", False, "ortho", "y"),
    "bunny": (15, 120, 0, "z", True, "ortho", "z"),
}


def parse_args(argv=None):
    p = argparse.ArgumentParser(prog="python -m tropical.stanford.visualize",
                                description="Render the extracted and the marching meshes to PNG")
    p.add_argument("-d", "--dataset", default="dragon", choices=sorted(VIEWS), help="Stanford 3D scanning model name")
    p.add_argument("-s", "--seed", default=45, type=int, help="Seed")
    p.add_argument("-m", "--model_size", default="small", choices=["small", "medium", "large"], help="Model size")
    p.add_argument("--out", default="meshes", help="mesh directory (input)")
    p.add_argument("--png-dir", default="outputs", help="image directory (output)")
    p.add_argument("--size", nargs=2, type=int, default=[1000, 800], metavar=("W", "H"), help="image size in pixels")
    p.add_argument("--ssaa", type=int, default=2, choices=[1, 2, 4], help="supersampling factor")
    p.add_argument("--no-edges", action="store_true", help="do not draw the polygon boundaries")
    p.add_argument("--view", nargs=2, type=float, default=None, metavar=("ELEV", "AZIM"),
                   help="view angles in degrees instead of the dataset's")
    p.add_argument("--persp", action="store_true", help="perspective projection")
    p.add_argument("--color", default="normal", choices=["normal", "component"],
                   help="component: one more image of the polygon file, coloured by connected component")
    return p.parse_args(argv)


def find_meshes(mesh_dir: str, tag: str):
    """[(ply path, png stem suffix, is_polygon_file)] of what exists: ours first, then mc / mtet by resolution."""
    found = []
    poly, tri = (os.path.join(mesh_dir, f"{n}_{tag}.ply") for n in ("our_poly_mesh", "our_mesh"))
    if os.path.isfile(poly):
        found.append((poly, "ours", True))
    elif os.path.isfile(tri):
        found.append((tri, "ours", False))
    rest = []
    for path in glob.glob(os.path.join(glob.escape(mesh_dir), f"*_mesh_{tag}.ply")):
        g = re.fullmatch(rf"(mc|mtet)(\d{{3,}})_mesh_{re.escape(tag)}\.ply", os.path.basename(path))
        if g:
            rest.append((g.group(1), int(g.group(2)), path))
    found += [(path, f"{method}{i:03d}", False) for method, i, path in sorted(rest)]
    return found


def plotted_axis(axis: str, swap_yz: bool, newell: bool) -> str:
    """The component of the PLOTTED mesh's normal that equals component `axis`
    ("x", "y", "z", "-" negates) of the mesh's own normal.  Swapping y and z is
    a reflection: it exchanges the two components, and it reverses the Newell
    normal (which follows the winding) but not a stored normal vector."""
    name, neg = axis.lstrip("-"), axis.startswith("-")
    if swap_yz:
        name = {"x": "x", "y": "z", "z": "y"}[name]
        neg ^= newell
    return ("-" if neg else "") + name


def output_name(png_dir: str, dataset: str, model_size: str, suffix: str) -> str:
    return os.path.join(png_dir, dataset, f"{model_size}_{suffix}.png")


def component_lut() -> np.ndarray:
    """A qualitative [256, 3] uint8 table: hues stepped by the golden angle,
    three lightness / saturation bands, so neighbouring ranks differ."""
    import colorsys
    k = np.arange(256)
    rgb = [colorsys.hls_to_rgb((0.61803398875 * i) % 1.0, (0.45, 0.6, 0.72)[i % 3], (0.85, 0.65, 0.75)[(i // 3) % 3])
           for i in k]
    return np.round(np.array(rgb) * 255).astype(np.uint8)


def component_values(pm) -> torch.Tensor:
    """Per polygon: its component's rank by area (largest 0), modulo 256, as float."""
    from tropical.utils.topology import largest_components, polygon_topology
    topo = polygon_topology(pm.vertices, pm.offsets, pm.indices, connect="edge")
    order = largest_components(topo.components, topo.n_components, by="area")
    rank = np.empty(topo.n_components, dtype=np.int64)
    rank[order] = np.arange(topo.n_components)
    rank_t = torch.from_numpy(rank % 256).to(topo.labels.device)
    return rank_t[topo.labels.long()].float()


def main(argv=None):
    args = parse_args(argv)
    print(args)
    mesh_dir = os.path.join(args.out, args.dataset)
    tag = f"{args.model_size}_{args.seed}"
    meshes = find_meshes(mesh_dir, tag)
    if not meshes:
        print(f"Mesh path is not found: {os.path.join(mesh_dir, f'our_mesh_{tag}.ply')}")
        return 0
    if not torch.cuda.is_available():
        raise SystemExit("tropical.stanford.visualize needs a ROCm GPU (no CPU fallback)")
    from tropical.utils.image import write_png
    from tropical.utils.mesh import PolygonMesh, load_ply, load_polygon_ply
    from tropical.utils.render import Camera, render, shade
    elev, azim, roll, vertical, swap_yz, proj, axis = VIEWS[args.dataset]
    if args.view is not None:
        elev, azim, roll = args.view[0], args.view[1], 0
    cam = Camera.from_angles(elev, azim, roll, vertical, "persp" if args.persp else proj)
    W, H = args.size
    loaded = []
    for path, suffix, is_poly in meshes:
        if is_poly:
            pm = load_polygon_ply(path)
        else:
            m = load_ply(path, process=False)
            pm = PolygonMesh(m.vertices, np.arange(0, 3 * len(m.faces) + 1, 3), m.faces.reshape(-1))
        if swap_yz:  # the reference plots (x, z, y)
            pm = PolygonMesh(pm.vertices[:, [0, 2, 1]], pm.offsets, pm.indices,
                             None if pm.normals is None else pm.normals[:, [0, 2, 1]])
        loaded.append((path, suffix, pm))
    # one camera for the run, fitted to the box around all the meshes: the figures are comparable and no
    # mesh reaches outside the image or the depth range
    boxes = np.array([f(pm.vertices, axis=0) for _, _, pm in loaded if len(pm.vertices) for f in (np.min, np.max)])
    cam.fit(boxes if len(boxes) else np.zeros((1, 3)), W, H)
    for path, suffix, pm in loaded:
        rgba, buf = render(pm, cam, size=(W, H), ssaa=args.ssaa, edges=suffix == "ours" and not args.no_edges,
                           axis=plotted_axis(axis, swap_yz, pm.normals is None), return_buffers=True)
        out = output_name(args.png_dir, args.dataset, args.model_size, suffix)
        write_png(out, rgba)
        print(f"{path} -> {out} ({len(pm)} faces)")
        if buf["stats"]["n_dropped"]:
            print(f"warning: {buf['stats']['n_dropped']} faces of {path} lie outside the view and were not drawn")
        if args.color == "component" and suffix == "ours" and os.path.basename(path).startswith("our_poly_mesh"):
            rgba = shade(buf["prim"], None if args.no_edges else buf["edge"], component_values(pm), 0.0, 255.0,
                         component_lut(), ss=args.ssaa)
            out = output_name(args.png_dir, args.dataset, args.model_size, "poly_components")
            write_png(out, rgba)
            print(f"{path} -> {out} (components)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
