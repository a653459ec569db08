"""python -m tropical.stanford.train -- the reference's entry point
(tropical/stanford/train.py) on the MI355X path.

Same flags (train.py:39-51, including the inverted `-c` and `-f`): -d
dataset, -s seed, -c disables the checkpoint cache, -m model size, -e runs
the evaluation, -f turns the flat assumption OFF (curve approximation on).
Same flow for a cached model: load the state_dict, extract the mesh with
tropical.subpoly.subpoly (prints " take T"), scale by 1/R, write
meshes/{d}/our_mesh_{m}_{seed}.ply, and with -e mesh the SDF by marching
cubes at the reference's resolutions (pseudo ground truth at 512), sample
both surfaces with 100k rays from the origin and print the
"#samples, #vertices, CD, AD, time" table (train.py:275-354).  Every step
runs on the GPU: subpoly on the HIP engine, the SDF grid through the fused
net kernel, marching cubes, ray casting and nearest neighbours in
csrc/evaluate.hip.

Without a cached model (or with -c) the net is trained first, as the
reference's loop (train.py:153-231): StanfordDataset samples (dataset.py,
signed distances by the HIP mesh kernel), batches of 1000, Adam + cosine
schedule, one closed-form gradient call per batch (csrc/train.hip), the
reference's progress lines, one subpoly per 10 batches once past 5 * EPOCH
of them, the state_dict saved to the cache path.  The Stanford scans are not
part of this repository: pass --mesh PATH (any closed PLY mesh) when the
dataset's own file is absent.  Extra flags: --weights PATH loads a
state_dict from PATH instead of the cache location; --epochs overrides
EPOCH (train.py:67); --layers / --hidden pick another net shape than the
reference's 3 x 16 (any shape the library has kernels for, `supported_shapes`;
model and mesh file names then carry a `_l{layers}h{hidden}` suffix);
--polygons also writes meshes/{d}/our_poly_mesh_{m}_{seed}.ply, the same
surface as the convex polygons the triangles are fans of, and prints
"Ours (polygons): P faces, mean degree D, edges E (boundary B, non-manifold
N, misoriented M), euler X, max planarity dev Y" (tnp_polygon_report);
--components (implies --polygons) then prints "Ours (components): C pieces
(edge-connected), L boundary loops (S simple), longest loop N edges / length
X", one line for each of the ten largest components by area (polygons, area,
share of the total, boundary edges, Euler number, and the enclosed volume of a
closed, consistently oriented one) and a count of the rest (tnp_topology_*);
--keep-largest N (implies --components) also writes
our_poly_mesh_{m}_{seed}_largest{N}.ply, the N largest components by area;
--fill-holes N (N >= 3, implies --components) caps every simple, consistently
oriented boundary loop of at most N edges of that file (of the polygon file
without --keep-largest) with one polygon, writes the result next to it as
..._filled.ply and prints "Ours (holes): L loops, K capped (<= N edges), S
non-simple, U unoriented, T longer; boundary edges B0 -> B1, closed components
C0 -> C1" (tnp_holes_*);
--weld TOL (TOL > 0, implies --components) first welds the polygon surface's
vertices that lie within TOL of each other (single linkage, the cluster's
smallest id stays), writes our_poly_mesh_{m}_{seed}_welded.ply and prints
"Ours (weld): tol T, M of U vertices merged into C clusters (largest K, moved
<= S), D polygons dropped, boundary edges B0 -> B1, non-manifold N0 -> N1,
Euler E0 -> E1" (tnp_weld_*); --components, --keep-largest and --fill-holes
then act on the welded surface, their files named ..._welded_largest{N}.ply
and so on;
--simplify CELL (CELL > 0, implies --components; behind --weld, in front of
--keep-largest and --fill-holes) clusters the polygon surface's vertices by the
cells of a grid of size CELL (--simplify-position mean | nearest: the cell's
mean, or its vertex nearest to the mean), removes the duplicate polygons that
makes, writes ..._simplified.ply (..._welded_simplified.ply behind --weld) and
prints "Ours (simplify): cell C (mean), U vertices -> K cells (largest M),
polygons P0 -> P1 (D dropped, X duplicate, F folded, Q pinched), moved <= S,
boundary edges B0 -> B1, non-manifold N0 -> N1, misoriented M0 -> M1, Euler
E0 -> E1" (tnp_simplify_*);
--mesh-cell CELL (with --mesh) clusters the normalised training mesh the same
way (nearest, duplicates removed) before the signed-distance kernel and the
sampling see it, and prints the triangle count before and after.
"""
from __future__ import annotations

import argparse
import os
import random
import re
import sys
import time

import numpy as np
import torch

import tropical.subpoly as sp
from tropical._buildid import CSRC
from tropical.stanford.model import Net
from tropical.utils.chamfer_distance import chamfer_distance, sample_surface_from_rays
from tropical.utils.marching_cubes import marching_cubes_torch
from tropical.utils.mesh import Mesh, PolygonMesh, polygon_report

DIM = 3
CANVAS_SIZE = 1.2
R = 0.8  # StanfordDataset.R (dataset.py:27): the scans are scaled into [-R, R]
MC_SIZES = [512, 16, 24, 32, 40, 48, 56, 64, 128, 192, 224, 256]


def supported_shapes():
    """The (layers, hidden) shapes the library has kernels for, read from the
    one list it is compiled from (csrc/net_device.h TNP_NET_SHAPES and
    TNP_WIDE_SHAPES, the full build's definitions); None when the sources are
    not next to the package -- the library itself then refuses an
    uninstantiated shape at its first call."""
    try:
        with open(os.path.join(CSRC, "net_device.h")) as fh:
            src = fh.read()
    except OSError:
        return None
    shapes = []
    for macro in ("TNP_NET_SHAPES", "TNP_WIDE_SHAPES"):
        bodies = re.findall(rf"^#define {macro}\(X\)(.*)$", src, flags=re.M)
        if not bodies:
            return None
        body = max(bodies, key=len)  # (the experiment build's list is a subset)
        shapes += [(int(nl), int(h)) for h, nl in re.findall(r"X\((\d+),\s*(\d+)\)", body)]
    return sorted(shapes)


def check_shape(num_layers: int, num_hidden: int):
    """ValueError for a net shape without kernels, naming the supported ones."""
    shapes = supported_shapes()
    if shapes is not None and (num_layers, num_hidden) not in shapes:
        names = ", ".join(f"{nl} x {h}" for nl, h in shapes)
        raise ValueError(f"no kernels for a net of {num_layers} layers x {num_hidden} hidden units; "
                         f"supported (layers x hidden): {names}")


def shape_suffix(num_layers: int = 3, num_hidden: int = 16) -> str:
    """File-name suffix of a net shape: empty for the reference's 3 x 16."""
    return "" if (num_layers, num_hidden) == (3, 16) else f"_l{num_layers}h{num_hidden}"


def _cell(text: str) -> float:
    """argparse type of --simplify / --mesh-cell: a finite float > 0, as fp32 too (argparse names the flag)."""
    from tropical.utils.simplify import check_cell
    try:
        return check_cell(float(text))
    except ValueError:
        raise argparse.ArgumentTypeError(f"a finite CELL > 0, not {text!r}")


def parse_args(argv=None):
    p = argparse.ArgumentParser(prog="python -m tropical.stanford.train",
                                description="Polyhedral complex derivation from piecewise trilinear networks")
    p.add_argument("-d", "--dataset", default="dragon",
                   choices=["bunny", "dragon", "happy", "armadillo", "drill", "lucy", "bunny_npy"],
                   help="Stanford 3D scanning model name")
    p.add_argument("-s", "--seed", default=45, type=int, help="Seed")
    p.add_argument("-c", "--cache", default=True, action="store_false", help="Cache the trained SDF?")
    p.add_argument("-m", "--model_size", default="small", choices=["small", "medium", "large"],
                   help="Model size")
    p.add_argument("-e", "--eval", default=False, action="store_true", help="Run evaluation?")
    p.add_argument("-f", "--force", default=True, action="store_false",
                   help="Force flat assumption to skip curve approximation.")
    p.add_argument("--weights", default=None, help="state_dict to load instead of the cache path")
    p.add_argument("--mesh", default=None, help="training mesh (PLY) instead of the dataset's scan file")
    p.add_argument("--epochs", default=None, type=int, help="training epochs (default: the reference's EPOCH)")
    p.add_argument("--out", default="meshes", help="mesh output directory")
    p.add_argument("--polygons", default=False, action="store_true",
                   help="also write the surface as convex polygons (our_poly_mesh_*.ply) and report its edges")
    p.add_argument("--components", default=False, action="store_true",
                   help="report the polygon surface's connected components and boundary loops (implies --polygons)")
    p.add_argument("--keep-largest", default=0, type=int, metavar="N",
                   help="also write the N largest components by area as our_poly_mesh_*_largestN.ply "
                        "(implies --components)")
    p.add_argument("--fill-holes", default=0, type=int, metavar="N",
                   help="also cap the simple boundary loops of at most N >= 3 edges of the last mesh written and "
                        "write it as *_filled.ply (implies --components)")
    p.add_argument("--weld", default=0.0, type=float, metavar="TOL",
                   help="first weld the polygon surface's vertices within TOL > 0 of each other, write it as "
                        "*_welded.ply and run --components / --keep-largest / --fill-holes on it (implies --components)")
    p.add_argument("--simplify", default=None, type=_cell, metavar="CELL",
                   help="cluster the polygon surface's vertices by the cells of a grid of size CELL > 0 (behind --weld), "
                        "remove the duplicate polygons, write it as *_simplified.ply and run --components / "
                        "--keep-largest / --fill-holes on it (implies --components)")
    p.add_argument("--simplify-position", default="mean", choices=["mean", "nearest"],
                   help="--simplify: a cell's vertex is the mean of its vertices, or the one nearest to that mean")
    p.add_argument("--mesh-cell", default=None, type=_cell, metavar="CELL",
                   help="cluster the (normalised) --mesh by cells of size CELL > 0 before training on it")
    p.add_argument("--layers", default=3, type=int, help="linear layers of the net (the reference: 3)")
    p.add_argument("--hidden", default=16, type=int, help="hidden units per layer (the reference: 16)")
    args = p.parse_args(argv)
    if args.keep_largest < 0:
        p.error("--keep-largest: N >= 0")
    if args.fill_holes < 0 or args.fill_holes in (1, 2):
        p.error("--fill-holes: N >= 3 (a loop has at least 3 edges), or 0 for none")
    if args.weld != 0.0 and not (args.weld > 0 and args.weld < float("inf")):
        p.error("--weld: a finite TOL > 0 (0 for none)")
    if args.mesh_cell is not None and args.mesh is None:
        p.error("--mesh-cell: needs --mesh")
    args.components = (args.components or args.keep_largest > 0 or args.fill_holes > 0 or args.weld > 0
                       or args.simplify is not None)
    args.polygons = args.polygons or args.components
    try:
        check_shape(args.layers, args.hidden)
    except ValueError as e:
        p.error(str(e))
    return args


def net_config(model_size: str, dataset: str, num_layers: int = 3, num_hidden: int = 16) -> dict:
    """train.py:70-82 (T defaults to 19 where the reference leaves it unset);
    the reference's nets are 3 x 16."""
    check_shape(num_layers, num_hidden)
    r_min, r_max = {"small": (2, 32), "medium": (4, 64), "large": (8, 128)}[model_size]
    T = 21 if (model_size == "large" and "bunny" in dataset.lower()) else 19
    return dict(num_layers=num_layers, num_hidden=num_hidden, levels=4, r_min=r_min, r_max=r_max, T=T)


def model_path(dataset: str, model_size: str, seed: int, num_layers: int = 3, num_hidden: int = 16) -> str:
    """The cache path: the reference's name for its 3 x 16 nets, a shape
    suffix for any other (a cached 3 x 16 state_dict never meets a wider net)."""
    return os.path.join(os.path.dirname(__file__), f"models/{dataset}/{dataset}_sdf_{model_size}_{seed}"
                                                   f"{shape_suffix(num_layers, num_hidden)}.pth")


@torch.no_grad()
def run_marching_cubes(net, n: int) -> Mesh:
    """train.py:275-293: SDF on an n^3 grid over [-C, C]^3, MC of -sdf at 0."""
    s = torch.linspace(-CANVAS_SIZE, CANVAS_SIZE, n)
    gx, gy, gz = torch.meshgrid(s, s, s, indexing="ij")
    pts = torch.stack([gx, gy, gz], dim=-1).reshape(-1, 3).to(net.device())
    sdfs = net.sdf(pts)[:, 0].reshape(n, n, n)
    v, t = marching_cubes_torch(-sdfs, 0.0)
    v = v / (n - 1.0) * 2 * CANVAS_SIZE - CANVAS_SIZE
    v = v / R
    return Mesh(v.cpu().numpy(), t.cpu().numpy())  # float64, as the reference's trimesh


def get_rays(n: int = 100000):
    """train.py:296-304 (CPU RNG, as the reference)."""
    theta = torch.rand(n) * 2 * torch.pi
    phi = torch.rand(n) * 2 * torch.pi
    x = torch.cos(theta) * torch.sin(phi)
    y = torch.sin(theta) * torch.sin(phi)
    z = torch.cos(phi)
    d = torch.stack([x, y, z], 1)
    return torch.zeros_like(d), d


def angular_distance(x, y):
    deg = np.degrees(np.arccos(np.clip(np.sum(x * y, axis=-1), -1, 1)))
    return np.mean(deg), np.std(deg)


def evaluate(net, our_mesh: Mesh, our_t: float, out_dir: str, tag: str, sizes=None):
    sizes = MC_SIZES if sizes is None else sizes
    rays_o, rays_d = get_rays()
    our_samples, our_normals, our_mask = sample_surface_from_rays(rays_o, rays_d, our_mesh,
                                                                  return_normal=True)
    print("Marching Cubes Results:")
    print("#samples, #vertices, CD, AD, time")
    gt = None
    rows = []
    for i in sizes:
        t = time.time()
        mc_mesh = run_marching_cubes(net, i)
        torch.cuda.synchronize()
        t = time.time() - t
        mc_samples, mc_normals, mc_mask = sample_surface_from_rays(rays_o, rays_d, mc_mesh,
                                                                   return_normal=True)
        if len(mc_samples) == 0:
            print(f"{i:4d}, {0:5d}, {0:0.6f}, {0:4.1f}, {t:.2f}")
            continue
        if gt is None:  # the first (512) is the pseudo ground truth
            gt = (mc_samples, mc_normals, mc_mask)
            our_cd = chamfer_distance(our_samples, gt[0])
            common = our_mask & gt[2]
            our_ad, _ = angular_distance(our_normals[common], gt[1][common])
            print(f"{'Ours'}, {our_mesh.vertices.shape[0]:5d}, {our_cd:0.6f}, {our_ad:4.1f}, {our_t:.2f}")
            rows.append(("ours", our_mesh.vertices.shape[0], our_cd, our_ad, our_t))
        mc_cd = chamfer_distance(mc_samples, gt[0])
        common = mc_mask & gt[2]
        mc_ad, _ = angular_distance(mc_normals[common], gt[1][common])
        print(f"{i:4d}, {mc_mesh.vertices.shape[0]:5d}, {mc_cd:0.6f}, {mc_ad:4.1f}, {t:.2f}")
        rows.append((i, mc_mesh.vertices.shape[0], mc_cd, mc_ad, t))
        mc_mesh.export(os.path.join(out_dir, f"mc{i:03d}_mesh_{tag}.ply"))
    print()
    return rows


BATCH_SIZE = 1000  # train.py:66


def draw_canvas(net, force: bool, polygons: bool = False):
    """train.py:117-129 without the matplotlib canvas: subpoly, timed.  The
    fifth value is the surface as a PolygonMesh (--polygons), else None."""
    t = time.time()
    out = sp.subpoly(net, DIM, CANVAS_SIZE, force=force, polygons=polygons)
    torch.cuda.synchronize()
    our_t = time.time() - t
    print(f" take {our_t:.2f}")
    return out[0], out[1], out[2], our_t, (out[3] if polygons else None)


def export_polygons(pmesh: PolygonMesh, verts, path: str):
    """--polygons: the surface's convex polygons as a PLY over our_mesh's
    (scaled) vertices `verts`, and one line on whether they close up."""
    pm = PolygonMesh(verts, pmesh.offsets, pmesh.indices, pmesh.normals)
    pm.export(path)
    r = polygon_report(pm.vertices, pm.offsets, pm.indices)
    mean = r["n_indices"] / max(r["n_polygons"], 1)
    print(f"Ours (polygons): {r['n_polygons']} faces, mean degree {mean:.2f}, edges {r['n_edges']} "
          f"(boundary {r['e_boundary']}, non-manifold {r['e_nonmanifold']}, misoriented {r['e_misoriented']}), "
          f"euler {r['euler']}, max planarity dev {r['max_dev']:.3g}")


def export_welded(pmesh: PolygonMesh, verts, path: str, tol: float):
    """--weld TOL: the polygon surface (over our_mesh's scaled vertices
    `verts`) with the vertices within `tol` of each other welded, written next
    to `path`, the polygon file (..._welded.ply), and one line on what that
    closed.  Returns (welded mesh, its file's path): what --components,
    --keep-largest and --fill-holes then work on."""
    from tropical.utils.weld import weld
    pm = PolygonMesh(verts, pmesh.offsets, pmesh.indices, pmesh.normals)
    welded, st = weld(pm, tol, position="first")
    out = f"{os.path.splitext(path)[0]}_welded.ply"
    welded.export(out)
    r0 = polygon_report(pm.vertices, pm.offsets, pm.indices)
    r1 = polygon_report(welded.vertices, welded.offsets, welded.indices)
    print(f"Ours (weld): tol {tol:g}, {st['n_merged']} of {st['n_used']} vertices merged into {st['n_clusters']} "
          f"clusters (largest {st['max_cluster']}, moved <= {st['max_shift']:.3g}), "
          f"{st['n_dropped_polygons']} polygons dropped, boundary edges {r0['e_boundary']} -> {r1['e_boundary']}, "
          f"non-manifold {r0['e_nonmanifold']} -> {r1['e_nonmanifold']}, Euler {r0['euler']} -> {r1['euler']}")
    return welded, out


def export_simplified(pmesh: PolygonMesh, verts, path: str, cell: float, position: str = "mean"):
    """--simplify CELL: the polygon surface (over the vertices `verts`)
    clustered by cells of size `cell`, written next to `path` (..._simplified.ply),
    and one line on what that did.  Returns (simplified mesh, its file's path):
    what --components, --keep-largest and --fill-holes then work on."""
    from tropical.utils.simplify import simplify
    pm = PolygonMesh(verts, pmesh.offsets, pmesh.indices, pmesh.normals)
    out_pm, st = simplify(pm, cell, position=position)
    out = f"{os.path.splitext(path)[0]}_simplified.ply"
    out_pm.export(out)
    r0 = polygon_report(pm.vertices, pm.offsets, pm.indices)
    r1 = polygon_report(out_pm.vertices, out_pm.offsets, out_pm.indices)
    print(f"Ours (simplify): cell {cell:g} ({position}), {st['n_used']} vertices -> {st['n_cells']} cells "
          f"(largest {st['max_cell']}), polygons {r0['n_polygons']} -> {st['n_polygons']} "
          f"({st['n_dropped_polygons']} dropped, {st['n_duplicate_polygons']} duplicate, {st['n_folded']} folded, "
          f"{st['n_pinched']} pinched), moved <= {st['max_shift']:.3g}, "
          f"boundary edges {r0['e_boundary']} -> {r1['e_boundary']}, "
          f"non-manifold {r0['e_nonmanifold']} -> {r1['e_nonmanifold']}, "
          f"misoriented {r0['e_misoriented']} -> {r1['e_misoriented']}, Euler {r0['euler']} -> {r1['euler']}")
    return out_pm, out


def export_components(pmesh: PolygonMesh, verts, path: str, keep_largest: int = 0):
    """--components: which pieces the polygon surface (over our_mesh's scaled
    vertices `verts`) falls into and where its holes are; --keep-largest N
    writes the N largest pieces by area next to `path`, the polygon file
    (..._largestN.ply).  Returns the topology."""
    from tropical.utils.topology import keep_components, largest_components, polygon_topology
    pm = PolygonMesh(verts, pmesh.offsets, pmesh.indices, pmesh.normals)
    topo = polygon_topology(pm.vertices, pm.offsets, pm.indices, connect="edge")
    comps, loops = topo.components, topo.loops
    longest = int(np.argmax(loops["n_edges"])) if len(loops) else -1  # (argmax: the lowest id among equals)
    n_long, len_long = (int(loops["n_edges"][longest]), float(loops["length"][longest])) if len(loops) else (0, 0.0)
    print(f"Ours (components): {len(comps)} pieces (edge-connected), {len(loops)} boundary loops "
          f"({int(loops['simple'].sum())} simple), longest loop {n_long} edges / length {len_long:.6g}")
    total = float(comps["area"].sum())
    for c in largest_components(comps, 10, by="area"):
        r = comps[c]
        line = (f"  component {c}: {r['n_polygons']} polygons, area {r['area']:.6g} "
                f"({100 * r['area'] / total if total > 0 else 0:.1f}%), boundary edges {r['e_boundary']}, "
                f"euler {r['euler']}")
        if r["e_boundary"] == 0 and r["e_nonmanifold"] == 0 and r["e_misoriented"] == 0:
            line += f", volume {r['volume']:.6g}"
        print(line)
    if len(comps) > 10:
        print(f"  and {len(comps) - 10} smaller components")
    if keep_largest > 0:
        kept = keep_components(pm, topo.labels, largest_components(comps, keep_largest, by="area"))
        kept.export(f"{os.path.splitext(path)[0]}_largest{keep_largest}.ply")
    return topo


def _closed_components(comps) -> int:
    return int(((comps["e_boundary"] == 0) & (comps["e_nonmanifold"] == 0) & (comps["e_misoriented"] == 0)).sum())


def export_filled(pmesh: PolygonMesh, verts, path: str, max_edges: int, topo=None, keep_largest: int = 0):
    """--fill-holes N: cap the simple boundary loops of at most N edges of the
    mesh the run ends with -- the N largest pieces of --keep-largest (`topo`:
    export_components' return), else the whole polygon surface -- with one
    polygon each, write it next to that mesh's file (..._filled.ply) and print
    what was closed.  Returns (filled mesh, stats)."""
    from tropical.utils.topology import fill_holes, keep_components, largest_components, polygon_topology
    pm = PolygonMesh(verts, pmesh.offsets, pmesh.indices, pmesh.normals)
    base = os.path.splitext(path)[0]
    if keep_largest > 0:
        if topo is None:
            topo = polygon_topology(pm.vertices, pm.offsets, pm.indices, connect="edge")
        pm = keep_components(pm, topo.labels, largest_components(topo.components, keep_largest, by="area"))
        base = f"{base}_largest{keep_largest}"
        topo = None
    if topo is None:
        topo = polygon_topology(pm.vertices, pm.offsets, pm.indices, connect="edge")
    filled, st = fill_holes(pm, max_edges=max_edges, mode="polygon")
    filled.export(f"{base}_filled.ply")
    b0 = polygon_report(pm.vertices, pm.offsets, pm.indices)["e_boundary"]
    b1 = polygon_report(filled.vertices, filled.offsets, filled.indices)["e_boundary"]
    c0 = _closed_components(topo.components)
    c1 = _closed_components(polygon_topology(filled.vertices, filled.offsets, filled.indices, connect="edge").components)
    print(f"Ours (holes): {st['n_loops']} loops, {st['n_capped']} capped (<= {max_edges} edges), "
          f"{st['n_nonsimple']} non-simple, {st['n_unoriented']} unoriented, {st['n_too_long']} longer; "
          f"boundary edges {b0} -> {b1}, closed components {c0} -> {c1}")
    return filled, st


def train_sdf(net, args, path: str):
    """The training loop of train.py:153-231 (no checkpoint, or -c)."""
    from tropical.stanford.dataset import StanfordDataset
    from tropical.stanford.sdf_train import SDFTrainer
    epochs = args.epochs or (6 if "drill" == args.dataset else 10)  # train.py:67
    print(f"warning: cannot find a pretrained model for seed ({args.seed})! This training code is not "
          f"guarantee the convergence of training nor a reliable SDF.", flush=True)
    training_data = StanfordDataset(args.dataset, mesh=args.mesh, mesh_cell=args.mesh_cell)
    loader = torch.utils.data.DataLoader(training_data, batch_size=BATCH_SIZE, shuffle=True)
    trainer = SDFTrainer(net, lr=1e-3, T_max=epochs * len(training_data) / BATCH_SIZE, batch_size=BATCH_SIZE)
    result = None
    for epoch in range(epochs):
        running_loss = torch.zeros((), device=net.device())
        training_data.resample()  # train.py:170 (also before the first epoch)
        for i, (inputs, labels) in enumerate(loader):
            loss, l1 = trainer.step(inputs.cuda(), labels.cuda())
            running_loss += loss
            if i % 10 == 9:
                print(f"[{epoch + 1}, {i + 1:5d}] lr: {trainer.sched.get_last_lr()[0]:.4f}, "
                      f"loss: {running_loss.item() / 10:.5f}", f"l1: {l1.item() / 10:.5f}", end="")
                running_loss.zero_()
                it = len(training_data) * epoch // BATCH_SIZE // 10 + (i + 1) // 10
                if 5 * epochs > it:
                    print(" mesh calculation skipped.")
                    continue
                result = draw_canvas(net, args.force, args.polygons)
    print("Finished training.", flush=True)
    if args.cache:
        os.makedirs(os.path.dirname(path), exist_ok=True)
        torch.save(net.state_dict(), path)
    return result


def main(argv=None):
    args = parse_args(argv)
    print(args)
    seed = args.seed
    torch.manual_seed(seed)
    random.seed(seed)
    np.random.seed(seed)
    if not torch.cuda.is_available():
        raise SystemExit("tropical.stanford.train needs a ROCm GPU (no CPU fallback)")
    net = Net(**net_config(args.model_size, args.dataset, args.layers, args.hidden)).cuda()
    path = args.weights or model_path(args.dataset, args.model_size, seed, args.layers, args.hidden)
    if (args.cache or args.weights) and os.path.isfile(path):
        sd = torch.load(path, map_location=net.device(), weights_only=True)
        net.load_state_dict(sd)
        print(f"The pretrained model loaded from {path}")
        polygons, vertices, faces_with_indices, our_t, pmesh = draw_canvas(net, args.force, args.polygons)
    else:
        if args.weights:
            raise SystemExit(f"--weights: no file at {path}")
        result = train_sdf(net, args, path)
        if result is None:
            result = draw_canvas(net, args.force, args.polygons)
        polygons, vertices, faces_with_indices, our_t, pmesh = result

    verts = vertices.cpu().numpy() / R
    our_mesh = Mesh(verts, np.asarray(faces_with_indices, dtype=np.int64))
    print(f"Ours: {our_mesh.vertices.shape}/{our_mesh.faces.shape}")
    out_dir = os.path.join(args.out, args.dataset)
    tag = f"{args.model_size}_{seed}{shape_suffix(args.layers, args.hidden)}"
    our_mesh.export(os.path.join(out_dir, f"our_mesh_{tag}.ply"))
    if args.polygons:
        export_polygons(pmesh, verts, os.path.join(out_dir, f"our_poly_mesh_{tag}.ply"))
    if args.components:
        poly_path = os.path.join(out_dir, f"our_poly_mesh_{tag}.ply")
        poly_verts = verts
        if args.weld:
            pmesh, poly_path = export_welded(pmesh, verts, poly_path, args.weld)
            poly_verts = pmesh.vertices
        if args.simplify is not None:
            pmesh, poly_path = export_simplified(pmesh, poly_verts, poly_path, args.simplify, args.simplify_position)
            poly_verts = pmesh.vertices
        topo = export_components(pmesh, poly_verts, poly_path, args.keep_largest)
        if args.fill_holes:
            export_filled(pmesh, poly_verts, poly_path, args.fill_holes, topo, args.keep_largest)
    if not args.eval:
        return 0
    evaluate(net, our_mesh, our_t, out_dir, tag)
    return 0


if __name__ == "__main__":
    sys.exit(main())
