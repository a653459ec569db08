"""python -m tropical.stanford.evaluate -- the reference's post-hoc
comparison (tropical/stanford/evaluate.py) on the MI355X path.

Same flags: -d dataset, -s seed, -m model size, -t mc | mtet.  It loads the
checkpoint and the mesh a `train` run left (meshes/{d}/our_mesh_{m}_{s}.ply),
prints the number of mesh vertices near the grid marks, then meshes the SDF
at every resolution of RESOLS by marching cubes or marching tetrahedra,
samples each surface with 100k rays from the origin and prints the
"#samples, #vertices, CD, AD, time" table against the marching-cubes mesh at
GT_RES (the pseudo ground truth, always marching cubes).  The `Ours` row has
time -1.00: the extraction is not run here.  Every mesh is written as
{method}{i:03d}_mesh_{m}_{s}.ply.  Extra flags, as `train` has them:
--weights PATH (a state_dict instead of the cache location) and --out DIR
(the mesh directory, default `meshes`).

The net is `train`'s for the size (`train.net_config`: 3 x 16, 4 levels,
r_min / r_max by size, and the hash size `train` gives it), so the checkpoint
`train` saved always loads.

Unlike the reference nothing runs at import: `parse_args(argv)` and
`main(argv)`.  Every step is on the GPU: the SDF grid through the fused net
kernel, marching cubes / ray casting / nearest neighbours in
csrc/evaluate.hip, marching tetrahedra in csrc/mtet.hip.
"""
from __future__ import annotations

import argparse
import os
import random
import sys
import time

import numpy as np
import torch

from tropical.stanford.model import Net
from tropical.stanford.train import (CANVAS_SIZE, R, angular_distance, get_rays, model_path, net_config,
                                     run_marching_cubes)
from tropical.utils.chamfer_distance import chamfer_distance, sample_surface_from_rays
from tropical.utils.mesh import Mesh, load_ply
from tropical.utils.mtet import marching_tetrahedras

OUR_T = -1  # the extraction is not timed here
# resolution of the marching-cubes pseudo ground truth, by model size
GT_RES = {"small": 256, "medium": 512, "large": 512}
_MC = [16, 24, 32, 40, 48, 56, 64, 128, 192, 224]
_MT = [16, 32, 48, 64, 96]
# resolutions per (method, model size), the pseudo ground truth first
RESOLS = {
    ("mc", "small"): [256] + _MC, ("mc", "medium"): [512] + _MC, ("mc", "large"): [512] + _MC,
    ("mtet", "small"): [256] + _MT, ("mtet", "medium"): [512] + _MT,
    ("mtet", "large"): [512] + _MT + [128, 192],
}
METHOD_NAMES = {"mc": "Cubes", "mtet": "Tetrahedra"}


def parse_args(argv=None):
    p = argparse.ArgumentParser(prog="python -m tropical.stanford.evaluate",
                                description="Polyhedral complex derivation from piecewise trilinear networks")
    p.add_argument("-d", "--dataset", default="dragon",
                   choices=["bunny", "dragon", "happy", "armadillo", "drill", "lucy"],
                   help="Stanford 3D scanning model name")
    p.add_argument("-s", "--seed", default=45, type=int, help="Seed")
    p.add_argument("-m", "--model_size", default="small", choices=["small", "medium", "large"],
                   help="Model size")
    p.add_argument("-t", "--method", default="mc", choices=["mc", "mtet"], help="Mesh extraction method")
    p.add_argument("--weights", default=None, help="state_dict to load instead of the cache path")
    p.add_argument("--out", default="meshes", help="mesh directory (input and outputs)")
    return p.parse_args(argv)


def count_vertices_near_values(vertices, values, threshold=1e-4, chunk=1 << 16):
    """Vertices with at least one coordinate within `threshold` of a value."""
    vertices, values = np.asarray(vertices), np.asarray(values)
    count = 0
    for i in range(0, len(vertices), chunk):
        near = np.abs(vertices[i:i + chunk, :, None] - values) < threshold
        count += int(np.sum(np.any(near, axis=(-1, -2))))
    return count


# corners of a cube as offsets (dx, dy, dz) and its six tets over them (the
# reference's list; its comment says five).  The split is not conforming
# across cubes, as the reference's is not: its meshes are not watertight.
_CORNERS = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)]
_CUBE_TETS = [[0, 1, 2, 6], [1, 2, 4, 6], [0, 1, 3, 6], [1, 3, 5, 6], [4, 5, 6, 7], [1, 4, 5, 6]]


def generate_tetrahedra_indices(n: int, device=None) -> torch.Tensor:
    """int64 [6 (n-1)^3, 4]: six tets per cube of the n^3 grid (point id
    x n^2 + y n + z), cubes in x, y, z order (z fastest)."""
    c = torch.arange(n - 1, dtype=torch.int64, device=device)
    x, y, z = torch.meshgrid(c, c, c, indexing="ij")
    v0 = ((x * n + y) * n + z).reshape(-1)
    off = torch.tensor([(dx * n + dy) * n + dz for dx, dy, dz in _CORNERS], dtype=torch.int64, device=device)
    local = off[torch.tensor(_CUBE_TETS, dtype=torch.int64, device=device)]  # [6, 4]
    return (v0[:, None, None] + local[None]).reshape(-1, 4)


@torch.no_grad()
def run_marching_tetrahedras(net, n: int) -> Mesh:
    """SDF on the n^3 grid over [-C, C]^3, marching tetrahedra over the
    six-tet split of its cubes, vertices scaled by 1 / R."""
    s = torch.linspace(-CANVAS_SIZE, CANVAS_SIZE, n)
    gx, gy, gz = torch.meshgrid(s, s, s, indexing="ij")
    pts = torch.stack([gx, gy, gz], dim=-1).reshape(-1, 3).to(net.device())
    sdfs = net.sdf(pts)[:, 0].reshape(-1)
    tets = generate_tetrahedra_indices(n, device=pts.device)
    v, t = marching_tetrahedras(pts, tets, sdfs, False)
    v = v.cpu().numpy()
    v /= R  # in fp32, as the reference
    return Mesh(v, t.cpu().numpy())


def evaluate(net, our_mesh: Mesh, method: str, model_size: str, out_dir: str, tag: str):
    gt_res = GT_RES[model_size]
    rays_o, rays_d = get_rays()
    our_samples, our_normals, our_mask = sample_surface_from_rays(rays_o, rays_d, our_mesh,
                                                                  return_normal=True)
    print(f"Marching {METHOD_NAMES[method]} Results:")
    print("#samples, #vertices, CD, AD, time")
    gt = None
    rows = []
    for i in RESOLS[(method, model_size)]:
        t = time.time()
        if "mc" == method or gt_res == i:
            mc_mesh = run_marching_cubes(net, i)
        else:
            mc_mesh = run_marching_tetrahedras(net, i)
        torch.cuda.synchronize()
        t = time.time() - t
        mc_samples, mc_normals, mc_mask = sample_surface_from_rays(rays_o, rays_d, mc_mesh,
                                                                   return_normal=True)
        if len(mc_samples) == 0:
            print(f"{i:4d}, {0:5d}, {0:0.6f}, {0:4.1f}, {t:.2f}")
            continue
        if gt_res == i and gt is None:
            gt = (mc_samples, mc_normals, mc_mask)
            our_cd = chamfer_distance(our_samples, gt[0])
            common = our_mask & gt[2]
            our_ad, _ = angular_distance(our_normals[common], gt[1][common])
            print(f"{'Ours'}, {our_mesh.vertices.shape[0]:5d}, {our_cd:0.6f}, {our_ad:4.1f}, {OUR_T:.2f}")
            rows.append(("ours", our_mesh.vertices.shape[0], our_cd, our_ad, OUR_T))
        if gt is None:
            raise RuntimeError(f"no pseudo ground truth: the first resolution must be GT_RES ({gt_res}) "
                               "and its mesh must be hit by the rays")
        mc_cd = chamfer_distance(mc_samples, gt[0])
        common = mc_mask & gt[2]
        mc_ad, _ = angular_distance(mc_normals[common], gt[1][common])
        print(f"{i:4d}, {mc_mesh.vertices.shape[0]:5d}, {mc_cd:0.6f}, {mc_ad:4.1f}, {t:.2f}")
        rows.append((i, mc_mesh.vertices.shape[0], mc_cd, mc_ad, t))
        mc_mesh.export(os.path.join(out_dir, f"{method}{i:03d}_mesh_{tag}.ply"))
    return rows


def main(argv=None):
    args = parse_args(argv)
    print(args)
    seed = args.seed
    torch.manual_seed(seed)
    random.seed(seed)
    np.random.seed(seed)
    path = args.weights or model_path(args.dataset, args.model_size, seed)
    out_dir = os.path.join(args.out, args.dataset)
    tag = f"{args.model_size}_{seed}"
    mesh_path = os.path.join(out_dir, f"our_mesh_{tag}.ply")
    if not os.path.isfile(path):
        print(f"Model path is not found: {path}")
        return 0
    if not os.path.isfile(mesh_path):
        print(f"Mesh path is not found: {mesh_path}")
        return 0
    if not torch.cuda.is_available():
        raise SystemExit("tropical.stanford.evaluate needs a ROCm GPU (no CPU fallback)")
    net = Net(**net_config(args.model_size, args.dataset)).cuda()
    net.load_state_dict(torch.load(path, map_location=net.device(), weights_only=True))
    print(f"The pretrained model is loaded from {path}")
    our_mesh = load_ply(mesh_path)
    print(f"The mesh is loaded from {mesh_path}")
    print(f"Ours: {our_mesh.vertices.shape}/{our_mesh.faces.shape}")
    count = count_vertices_near_values(our_mesh.vertices, net.enc.marks.cpu().numpy())
    print(f"Number of vertices near the grid marks: {count} ({count / max(len(our_mesh.vertices), 1):.4f})")
    evaluate(net, our_mesh, args.method, args.model_size, out_dir, tag)
    return 0


if __name__ == "__main__":
    sys.exit(main())
