"""Generate tests/golden/mtet_cases.npz by running the REFERENCE's marching
tetrahedra (tropical/utils/mtet.py) and its tet-grid loop
(tropical/stanford/evaluate.py generate_tetrahedra_indices) on the CPU.

Run in the build container only (the reference never travels to the GPU box):

    python tests/golden/make_mtet_golden.py

The reference's mtet.py cannot run as committed: `= sdf` and `[interp_v]`
stand on two lines (179-180).  The statement is joined in memory; nothing of
the reference's text is written anywhere.  evaluate.py works at import, so
only the source of its generate_tetrahedra_indices is extracted and executed.

Per case the file holds the inputs and the joined reference's outputs
(arrays for the small cases, SHA-256 for sphere40), the tet list for n = 4,
its hash for n = 12 and 40, and the 16 x 6 triangle table with the triangle
counts.  No `kind` key: golden_io.cases() lists subpoly cases by it.

Conditions asserted on every case's inputs, so that the bitwise test does not
hinge on an ill-conditioned sign or quotient: the reference's flips (fp32 LU
determinant) equal the sign of the double triple product, and every crossed
edge has |s_lo - s_hi| >= 1e-3.  Seeds are searched until both hold.
"""
from __future__ import annotations

import os
import re
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from golden_io import sha  # noqa: E402

REF_ROOT = os.environ.get("TROPICAL_REFERENCE", "/root/reference")
OUT = os.path.join(HERE, "mtet_cases.npz")
CANVAS, RADIUS = 1.2, 0.8


def load_reference():
    """(namespace of the joined mtet.py, generate_tetrahedra_indices)."""
    sys.dont_write_bytecode = True
    with open(os.path.join(REF_ROOT, "tropical", "utils", "mtet.py")) as fh:
        src = fh.read()
    src, n = re.subn(r"= sdf[ \t]*\n[ \t]*\[interp_v\]", "= sdf[interp_v]", src)
    assert n == 1, "the split statement of mtet.py was not found"
    ns = {"__name__": "ref_mtet"}
    exec(compile(src, "ref_mtet", "exec"), ns)
    with open(os.path.join(REF_ROOT, "tropical", "stanford", "evaluate.py")) as fh:
        ev = fh.read()
    m = re.search(r"^def generate_tetrahedra_indices\(.*?(?=^\S)", ev, flags=re.S | re.M)
    assert m, "generate_tetrahedra_indices not found in evaluate.py"
    gns = {"torch": torch}
    exec(compile(m.group(0), "ref_evaluate_tets", "exec"), gns)
    return ns, gns["generate_tetrahedra_indices"]


def grid_points(n: int) -> np.ndarray:
    """fp32 [n^3, 3], x slowest, over [-CANVAS, CANVAS]^3 (float64 linspace,
    rounded once: the same on every machine)."""
    s = np.linspace(-CANVAS, CANVAS, n)
    g = np.stack(np.meshgrid(s, s, s, indexing="ij"), -1).reshape(-1, 3)
    return g.astype(np.float32)


def sphere_sdf(p: np.ndarray) -> np.ndarray:
    q = p.astype(np.float64)
    return (np.sqrt((q * q).sum(-1)) - RADIUS).astype(np.float32)


def triple_sign(v: np.ndarray, tets: np.ndarray) -> np.ndarray:
    p = v.astype(np.float64)[tets]
    e = p[:, 1:] - p[:, :1]
    det = np.einsum("ti,ti->t", e[:, 0], np.cross(e[:, 1], e[:, 2]))
    return det < 0


def run_case(ns, v: np.ndarray, tets: np.ndarray, sdf: np.ndarray):
    """The joined reference on (v, tets, sdf); None when a condition on the
    inputs fails."""
    tv, ts = torch.from_numpy(v), torch.from_numpy(sdf)
    tt = torch.from_numpy(tets.copy())
    flips = ns["_orientation_test"](tv, tt).numpy()
    if not np.array_equal(flips, triple_sign(v, tets)):
        return None
    verts, faces, tet_idx = ns["marching_tetrahedras"](tv, tt, ts, True)
    after = tt.numpy()
    want = tets.copy()
    want[flips, 0], want[flips, 1] = tets[flips, 1], tets[flips, 0]
    assert np.array_equal(after, want)
    # the crossed edges, as the product numbers them
    occ = sdf > 0
    ei = np.array([[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]])
    valid = (occ[after].sum(-1) > 0) & (occ[after].sum(-1) < 4)
    e = np.sort(after[valid][:, ei].reshape(-1, 2), -1)
    e = np.unique(e, axis=0)
    e = e[occ[e].sum(-1) == 1]
    assert len(e) == len(verts)
    if len(e) and np.abs(sdf[e[:, 0]].astype(np.float64) - sdf[e[:, 1]]).min() < 1e-3:
        return None
    # the documented op order, one rounded fp32 op each, is the reference's bit for bit
    sa, sb = sdf[e[:, 0]], sdf[e[:, 1]]
    n = -sb
    d = sa + n
    w0, w1 = n / d, sa / d
    mine = v[e[:, 0]] * w0[:, None] + v[e[:, 1]] * w1[:, None]
    assert np.array_equal(mine.astype(np.float32).view(np.uint32), verts.numpy().view(np.uint32))
    return dict(verts=verts.numpy(), faces=faces.numpy(), tet_idx=tet_idx.numpy(), flips=flips,
                interp_v=e.astype(np.int64))


def noise_inputs(seed: int):
    g = torch.Generator().manual_seed(seed)
    sdf = torch.randn(1000, generator=g)
    sdf[torch.randperm(1000, generator=g)[:40]] = 0.0
    return grid_points(10), sdf.numpy()


def soup_inputs(seed: int):
    g = torch.Generator().manual_seed(seed)
    v = torch.rand(300, 3, generator=g) * 2 - 1
    tets = torch.stack([torch.randperm(300, generator=g)[:4] for _ in range(3000)])
    sdf = torch.randn(300, generator=g)
    return v.numpy(), tets.numpy().astype(np.int64), sdf.numpy()


def main():
    ns, ref_tets = load_reference()
    out = {}
    table = ns["triangle_table"].numpy().astype(np.int8)
    out["triangle_table"] = table
    out["num_triangles"] = ns["num_triangles_table"].numpy().astype(np.int8)
    grids = {n: ref_tets(n).numpy().astype(np.int64) for n in (4, 6, 10, 12, 40)}
    out["tets_n4"] = grids[4].astype(np.int32)
    out["tets_n12_sha"] = np.array(sha(grids[12]))
    out["tets_n40_sha"] = np.array(sha(grids[40]))

    def store(name, v, tets, sdf, r, full=True):
        print(f"{name}: {len(tets)} tets ({int(r['flips'].sum())} flip) -> {len(r['verts'])} vertices, "
              f"{len(r['faces'])} faces")
        out[f"{name}:counts"] = np.array([len(tets), len(r["verts"]), len(r["faces"])], dtype=np.int64)
        if full:
            out[f"{name}:vertices"] = v
            out[f"{name}:sdf"] = sdf
            out[f"{name}:tets"] = tets.astype(np.int32)
            out[f"{name}:flips"] = np.packbits(r["flips"])
            out[f"{name}:verts"] = r["verts"]
            out[f"{name}:faces"] = r["faces"].astype(np.int32)
            out[f"{name}:tet_idx"] = r["tet_idx"].astype(np.int32)
            out[f"{name}:interp_v"] = r["interp_v"].astype(np.int32)
        else:  # the inputs are the recipe's; everything by hash
            after = tets.copy()
            f = r["flips"]
            after[f, 0], after[f, 1] = tets[f, 1], tets[f, 0]
            out[f"{name}:in_sha"] = np.array(sha(v, sdf, tets))
            out[f"{name}:verts_sha"] = np.array(sha(r["verts"]))
            out[f"{name}:faces_sha"] = np.array(sha(r["faces"].astype(np.int64)))
            out[f"{name}:tet_idx_sha"] = np.array(sha(r["tet_idx"].astype(np.int64)))
            out[f"{name}:tets_after_sha"] = np.array(sha(after))

    for name, n, full in (("sphere12", 12, True), ("sphere40", 40, False)):
        v = grid_points(n)
        sdf = sphere_sdf(v)
        r = run_case(ns, v, grids[n], sdf)
        assert r is not None, name
        store(name, v, grids[n], sdf, r, full)

    v = grid_points(6)
    sdf = np.ones(len(v), dtype=np.float32)
    r = run_case(ns, v, grids[6], sdf)
    assert r is not None and len(r["verts"]) == 0 and len(r["faces"]) == 0
    store("allpos", v, grids[6], sdf, r)

    for seed in range(100):
        v, sdf = noise_inputs(seed)
        r = run_case(ns, v, grids[10], sdf)
        if r is not None:
            break
    assert r is not None
    print(f"noise10: seed {seed}")
    occ = sdf > 0
    cases = set(((occ[r_] * [1, 2, 4, 8]).sum()) for r_ in grids[10])
    assert cases == set(range(16)), sorted(cases)
    store("noise10", v, grids[10], sdf, r)

    for seed in range(100):
        v, tets, sdf = soup_inputs(seed)
        r = run_case(ns, v, tets, sdf)
        if r is not None:
            break
    assert r is not None
    print(f"soup: seed {seed}")
    store("soup", v, tets, sdf, r)

    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {os.path.getsize(OUT) / 1024:.0f} KB")


if __name__ == "__main__":
    main()
