"""GPU marching tetrahedra (tropical/utils/mtet.py of the reference, derived
from kaolin's `marching_tetrahedra` with an orientation test added).

`marching_tetrahedras(vertices, tets, sdf, return_tet_idx=False)` on the HIP
kernels of csrc/mtet.hip.  The reference's file cannot run as committed: its
lines 179-180 split `sdf[interp_v]` into `= sdf` and a dangling
`[interp_v]`; what is reproduced here is the function with that statement
joined.  Contract, all of it independent of any atomic arrival order:

* a tet whose det[(b - a), (c - a), (d - a)] is negative gets its first two
  ids swapped IN THE CALLER'S `tets` (the reference mutates its argument);
  the sign is taken in double (the reference: an fp32 LU, so a
  near-degenerate tet may differ);
* inside is `sdf > 0`; the case is sum(occ[i] << i) over the flipped order;
* one vertex per crossed edge (lo, hi), numbered by the lexicographic rank
  of (lo, hi) -- the reference's `torch.unique(dim=0)` order -- at
  p_lo * (-s_hi / (s_lo - s_hi)) + p_hi * (s_lo / (s_lo - s_hi)), every op
  rounded to fp32 on its own;
* faces: the triangles of the 1-triangle tets in tet order, then those of the
  2-triangle tets in tet order; `tet_idx` likewise;
* an id outside [0, N) raises IndexError (no gather is made from it; tets
  ahead of the offending one may already have been flipped).

With `requires_grad` on `vertices` or `sdf` the vertices are recomputed from
the kernel's edge list with torch ops in the same op order, so the values
are the kernel's bit for bit and autograd is torch's own.  ROCm tensors
only: there is no CPU fallback."""
from __future__ import annotations

import ctypes as C

import torch

from .. import _hip

TILE = 256  # tets per tile of the kernels' scanned counts (csrc/common.h TNP_BLOCK)


def _extract(vertices: torch.Tensor, tets: torch.Tensor, sdf: torch.Tensor):
    """-> (verts fp32 [V, 3], interp_v int64 [V, 2], faces int64 [F, 3],
    tet_idx int64 [F]); flips `tets` in place."""
    dev = vertices.device
    N, T = vertices.shape[0], tets.shape[0]
    L = _hip.lib()
    s = C.c_void_p(_hip.stream_ptr(dev))
    tiles = (T + TILE - 1) // TILE
    case = torch.empty(max(T, 1), dtype=torch.uint8, device=dev)
    tile = torch.empty(3 * (tiles + 1) + 2, dtype=torch.int64, device=dev)
    nk, n1, n2 = C.c_int64(), C.c_int64(), C.c_int64()
    rc = L.tnp_mt_classify(_hip.ptr(vertices), _hip.ptr(sdf), N, _hip.ptr(tets), T, _hip.ptr(case),
                           _hip.ptr(tile), C.byref(nk), C.byref(n1), C.byref(n2), s)
    if rc == 1:
        raise IndexError(L.tnp_last_error().decode(errors="replace"))
    _hip.check(rc, "tnp_mt_classify")
    keys = torch.empty(max(2 * nk.value, 1), dtype=torch.int64, device=dev)
    nv = C.c_int64()
    _hip.check(L.tnp_mt_edges(_hip.ptr(tets), T, N, _hip.ptr(case), _hip.ptr(tile), nk.value,
                              _hip.ptr(keys), C.byref(nv), s), "tnp_mt_edges")
    V, F = nv.value, n1.value + 2 * n2.value
    verts = torch.empty(V, 3, dtype=torch.float32, device=dev)
    interp = torch.empty(V, 2, dtype=torch.int64, device=dev)
    faces = torch.empty(F, 3, dtype=torch.int64, device=dev)
    tet_idx = torch.empty(F, dtype=torch.int64, device=dev)
    _hip.check(L.tnp_mt_emit(_hip.ptr(vertices), _hip.ptr(sdf), N, _hip.ptr(tets), T, _hip.ptr(case),
                             _hip.ptr(tile), _hip.ptr(keys), V, n1.value, _hip.ptr(verts),
                             _hip.ptr(interp), _hip.ptr(faces), _hip.ptr(tet_idx), s), "tnp_mt_emit")
    return verts, interp, faces, tet_idx


def marching_tetrahedras(vertices: torch.Tensor, tets: torch.Tensor, sdf: torch.Tensor,
                         return_tet_idx: bool = False):
    """vertices fp32 [N, 3], tets int64 [T, 4], sdf fp32 [N] on a ROCm device
    -> (verts [V, 3], faces int64 [F, 3][, tet_idx int64 [F]]) on that
    device; empty results have shapes (0, 3), (0, 3) and (0,)."""
    for t, what in ((vertices, "vertices"), (tets, "tets"), (sdf, "sdf")):
        _hip.require_cuda(t, f"marching_tetrahedras({what})")
    if vertices.dim() != 2 or vertices.shape[1] != 3:
        raise ValueError(f"marching_tetrahedras: vertices must be [N, 3], got {tuple(vertices.shape)}")
    if tets.dim() != 2 or tets.shape[1] != 4 or tets.dtype != torch.int64:
        raise ValueError(f"marching_tetrahedras: tets must be int64 [T, 4], got {tets.dtype} "
                         f"{tuple(tets.shape)}")
    if sdf.dim() != 1 or sdf.shape[0] != vertices.shape[0]:
        raise ValueError(f"marching_tetrahedras: sdf must be [N] = [{vertices.shape[0]}], "
                         f"got {tuple(sdf.shape)}")
    if vertices.shape[0] >= 2 ** 31:
        raise ValueError("marching_tetrahedras: needs fewer than 2^31 vertices")
    v = vertices.detach().to(torch.float32).contiguous()
    sd = sdf.detach().to(torch.float32).contiguous()
    # the kernels flip the caller's buffer; a view they cannot address
    # directly is flipped in a copy and written back
    direct = tets.is_contiguous() and tets.data_ptr() % 16 == 0
    tt = tets if direct else tets.clone(memory_format=torch.contiguous_format)
    try:
        verts, interp, faces, tet_idx = _extract(v, tt, sd)
    finally:
        if not direct:
            with torch.no_grad():
                tets.copy_(tt)
    if torch.is_grad_enabled() and (vertices.requires_grad or sdf.requires_grad):
        # the kernel's formula in torch ops, op for op (index, negate, add,
        # divide, multiply, add): the same values, with torch's autograd
        a, b = interp[:, 0], interp[:, 1]
        pa, pb = vertices[a], vertices[b]
        sa, sb = sdf[a], sdf[b]
        n = -sb
        den = sa + n
        w0, w1 = n / den, sa / den
        verts = pa * w0[:, None] + pb * w1[:, None]
    if return_tet_idx:
        return verts, faces, tet_idx
    return verts, faces
