"""Render a triangle mesh or a polygon complex on the GPU (csrc/render.hip,
contract in include/tropical_hip.h): the figures of the reference's
tropical/stanford/visualize.py -- faces coloured by a component of their
normal, polyhedral edges drawn over them -- without matplotlib's painter.

    cam = Camera.from_angles(15, 120).fit(mesh.vertices, 1024, 1024)
    rgba = render(mesh, cam, size=(1024, 1024), ssaa=2)      # uint8 [H, W, 4], on the device
    write_png("figure.png", rgba)                            # tropical.utils.image
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from .. import _hip
from .colormap import lut as _lut
from .mesh import Mesh, PolygonMesh
from .soup import current_device, soup_on_device, to_device

_AXES = {"x": 0, "y": 1, "z": 2}
EDGE_RGBA = (0, 0, 0, 255)


class Camera:
    """Rotation rows right / up / toward (toward the viewer), a centre, a scale
    in pixels per world unit, the perspective distance (0: orthographic) and
    the half depth range: the fields of tnp_render_view."""

    def __init__(self, right, up, toward, center=(0.0, 0.0, 0.0), scale=1.0, persp_dist=0.0, depth_half=1.0,
                 persp=False):
        self.right, self.up, self.toward = (np.asarray(v, dtype=np.float64).reshape(3) for v in (right, up, toward))
        self.center = np.asarray(center, dtype=np.float64).reshape(3)
        self.scale, self.persp_dist, self.depth_half = float(scale), float(persp_dist), float(depth_half)
        self.persp = bool(persp) or self.persp_dist > 0

    @classmethod
    def from_angles(cls, elev, azim, roll=0.0, vertical_axis="z", proj="ortho"):
        """matplotlib's view_init(elev, azim, roll, vertical_axis) in degrees:
        the viewer sits at elevation `elev` above the plane normal to the
        vertical axis and at azimuth `azim` about that axis; `roll` turns the
        camera about its line of sight.  proj: "ortho" or "persp"."""
        if proj not in ("ortho", "persp"):
            raise ValueError(f"proj = {proj!r} (ortho, persp)")
        k = _AXES[vertical_axis] if isinstance(vertical_axis, str) else int(vertical_axis)
        e, a, r = (math.radians(float(v)) for v in (elev, azim, roll))
        # in the frame whose third axis is the vertical one; np.roll turns it
        # (cyclically, so handedness is kept) into world axes
        toward = np.roll([math.cos(e) * math.cos(a), math.cos(e) * math.sin(a), math.sin(e)], k - 2)
        # vertical x toward, normalised; matplotlib flips the vertical axis past
        # the pole (|elev| > 90), so the formula holds for every elevation
        right = np.roll([-math.sin(a), math.cos(a), 0.0], k - 2)
        up = np.cross(toward, right)
        if r != 0.0:  # a positive roll of the camera turns the world the other way
            c, s = math.cos(-r), math.sin(-r)
            right, up = c * right + s * np.cross(toward, right), c * up + s * np.cross(toward, up)
        return cls(right, up, toward, persp=proj == "persp")

    def rotation(self) -> np.ndarray:
        return np.stack([self.right, self.up, self.toward])

    def fit(self, vertices, width, height, margin=0.05):
        """Centre, scale and depth range from the vertices' bounding box so that
        every vertex lands inside the width x height image with `margin` (a
        fraction of the image) free on every side and inside the depth range:
        nothing is dropped.  Under perspective the viewer stands ten
        half-depths from the centre (matplotlib's focal default, dist 10 on a
        unit box).  Returns self."""
        v = vertices.detach().cpu().numpy() if isinstance(vertices, torch.Tensor) else np.asarray(vertices)
        v = v.reshape(-1, 3).astype(np.float64)
        lo, hi = (v.min(0), v.max(0)) if len(v) else (np.zeros(3), np.zeros(3))
        self.center = 0.5 * (lo + hi)
        corners = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
        c = (corners - self.center) @ self.rotation().T
        ext = np.maximum(np.abs(c).max(0), 1e-6)
        self.depth_half = 1.05 * ext[2]
        s = 1.0
        if self.persp:
            self.persp_dist = 10.0 * self.depth_half
            s = self.persp_dist / (self.persp_dist - ext[2])  # the largest magnification inside the box
        use = 1.0 - 2.0 * margin
        self.scale = min(0.5 * use * width / (s * ext[0]), 0.5 * use * height / (s * ext[1]))
        return self

    def view(self, width: int, height: int, scale_by: int = 1) -> _hip.TnpRenderView:
        """The C struct for a raster of width x height pixels (scale_by: the
        supersampling factor the scale is multiplied by)."""
        vw = _hip.TnpRenderView()
        for name in ("right", "up", "toward", "center"):
            getattr(vw, name)[:] = [float(x) for x in getattr(self, name)]
        vw.scale, vw.persp_dist, vw.depth_half = self.scale * scale_by, self.persp_dist, self.depth_half
        vw.width, vw.height = int(width), int(height)
        return vw


def _soup(mesh, dev):
    """(vertices fp32 [V, 3], offsets int64 [P + 1], indices int64, normals or None) on the device."""
    normals = None
    if isinstance(mesh, PolygonMesh):
        v, off, idx, normals = mesh.vertices, mesh.offsets, mesh.indices, mesh.normals
    elif isinstance(mesh, Mesh):
        v, off, idx = mesh.vertices, None, mesh.faces
    elif isinstance(mesh, (tuple, list)) and len(mesh) == 2:
        v, off, idx = mesh[0], None, mesh[1]
    elif isinstance(mesh, (tuple, list)) and len(mesh) in (3, 4):
        v, off, idx = mesh[:3]
        normals = mesh[3] if len(mesh) == 4 else None
    else:
        raise TypeError("render: a Mesh, a PolygonMesh, (vertices, faces) or (vertices, offsets, indices[, normals])")
    if off is None:
        idx = to_device(idx, dev, torch.int64)
        off = torch.arange(0, idx.numel() + 1, 3, device=dev)
    v, off, idx, _ = soup_on_device(v, off, idx, dev, "render: ")
    return v, off, idx, (None if normals is None else to_device(normals, dev, torch.float32).reshape(-1, 3))


def newell_normals(v: torch.Tensor, off: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """Unit Newell normal of every polygon ([P, 3]; zero for a polygon without
    area), with torch gathers: only for a soup the library has checked
    (rasterize() raises before this may follow a bad offset or id)."""
    P = off.numel() - 1
    n = int(off[-1]) if P > 0 else 0
    deg = off[1:] - off[:-1]
    pid = torch.repeat_interleave(torch.arange(P, device=v.device), deg)
    nxt = torch.arange(1, n + 1, device=v.device)
    nxt[off[1:] - 1] = off[:-1]
    p = v[idx[:n]]
    N = torch.zeros(P, 3, device=v.device, dtype=v.dtype).index_add_(0, pid, torch.linalg.cross(p, p[nxt]))
    return N / N.norm(dim=1, keepdim=True).clamp_min(1e-30)


def rasterize(mesh, camera: Camera, size, scale_by: int = 1, edge_half_width: int = 8, screen: bool = False):
    """tnp_render_raster on a width x height raster: a dict with the device
    tensors ``prim`` (int32 [H, W] polygon id, -1 background), ``tri`` (the
    winning fan triangle), ``edge`` (uint8 mask), optionally ``screen``
    ([V, 3] int32), and ``stats``."""
    dev = current_device()
    v, off, idx, _ = _soup(mesh, dev)  # (tensors already in place pass through unchanged)
    W, H = int(size[0]), int(size[1])
    ok = 1 <= W <= 8192 and 1 <= H <= 8192  # (the library refuses; nothing is allocated for a bad size)
    prim = torch.empty((H, W) if ok else (1, 1), dtype=torch.int32, device=dev)
    tri, edge = torch.empty_like(prim), torch.empty(prim.shape, dtype=torch.uint8, device=dev)
    scr = torch.empty((v.shape[0], 3), dtype=torch.int32, device=dev) if screen else None
    st = _hip.TnpRenderStats()
    vw = camera.view(W, H, scale_by)
    _hip.check(_hip.lib().tnp_render_raster(_hip.ptr(v), v.shape[0], _hip.ptr(off), _hip.ptr(idx), off.numel() - 1,
                                            C.byref(vw), int(edge_half_width), _hip.ptr(scr), _hip.ptr(prim),
                                            _hip.ptr(tri), _hip.ptr(edge), C.byref(st),
                                            C.c_void_p(_hip.stream_ptr(dev))), "tnp_render_raster")
    out = {"prim": prim, "tri": tri, "edge": edge, "stats": st.as_dict()}
    if screen:
        out["screen"] = scr
    return out


def shade(prim, edge, value, vmin, vmax, lut, edge_rgba=EDGE_RGBA, ss: int = 1) -> torch.Tensor:
    """tnp_render_shade: uint8 [H / ss, W / ss, 4] from an id raster, an edge
    mask (or None), per-polygon values and a [256, 3] uint8 table."""
    dev = prim.device
    H, W = prim.shape
    value = value.to(dev, torch.float32).contiguous()
    lut = torch.as_tensor(lut, dtype=torch.uint8).to(dev).contiguous()
    if lut.shape != (256, 3):
        raise ValueError(f"shade: the look-up table is [256, 3] uint8, got {tuple(lut.shape)}")
    ok = ss in (1, 2, 4) and H % ss == 0 and W % ss == 0
    out = torch.empty((H // ss, W // ss, 4) if ok else (1, 1, 4), dtype=torch.uint8, device=dev)
    rgba = (C.c_uint8 * 4)(*[int(x) for x in edge_rgba])
    _hip.check(_hip.lib().tnp_render_shade(_hip.ptr(prim), _hip.ptr(edge), W, H, _hip.ptr(value), value.numel(),
                                           float(vmin), float(vmax), _hip.ptr(lut), rgba, int(ss), _hip.ptr(out),
                                           C.c_void_p(_hip.stream_ptr(dev))), "tnp_render_shade")
    return out


def render(mesh, camera: Camera, size=(1024, 1024), ssaa: int = 1, edges: bool = True, edge_width: float = 1.0,
           value=None, vmin=-1.0, vmax=1.0, cmap="plasma", return_buffers: bool = False, axis="z"):
    """The figure as a uint8 [H, W, 4] tensor on the device (transparent
    background).  mesh: a Mesh, a PolygonMesh, or device tensors (vertices,
    faces) / (vertices, offsets, indices[, normals]).  size = (W, H); the
    raster is ssaa (1, 2, 4) times that in each direction and box-filtered.
    edges: draw polygon boundaries `edge_width` output pixels wide.
    value: one scalar per polygon; the default is the component along `axis`
    ("x", "y", "z", with a leading "-" negated) of the unit normal --
    PolygonMesh.normals where present, else the Newell normal -- mapped over
    the fixed range [vmin, vmax] = [-1, 1], so two figures are comparable;
    vmin="auto" maps min..max as the reference's Normalize() does.
    cmap: "plasma", "gray" or a [256, 3] uint8 table.
    return_buffers: also return rasterize()'s dict (at the raster's size)."""
    dev = current_device()
    if ssaa not in (1, 2, 4):
        raise ValueError(f"ssaa = {ssaa} (1, 2, 4)")
    v, off, idx, normals = _soup(mesh, dev)
    P = off.numel() - 1
    W, H = int(size[0]), int(size[1])
    hw = max(0, min(256, int(round(8 * edge_width * ssaa)))) if edges else 0
    # first: the library checks the offsets and ids on the device and raises for
    # malformed input, so the torch gathers below only ever see a checked soup
    buf = rasterize((v, off, idx, None), camera, (W * ssaa, H * ssaa), scale_by=ssaa, edge_half_width=hw)
    if value is None:
        neg = isinstance(axis, str) and axis.startswith("-")
        k = _AXES[axis.lstrip("-")] if isinstance(axis, str) else int(axis)
        n = newell_normals(v, off, idx) if normals is None else \
            normals / normals.norm(dim=1, keepdim=True).clamp_min(1e-30)
        value = -n[:, k] if neg else n[:, k]
    else:
        value = torch.as_tensor(value, dtype=torch.float32).to(dev).reshape(-1)
    if value.numel() != P:
        raise ValueError(f"render: {value.numel()} values for {P} polygons")
    if isinstance(vmin, str):
        if vmin != "auto":
            raise ValueError(f"vmin = {vmin!r} (a number or 'auto')")
        fin = value[torch.isfinite(value)]
        vmin, vmax = (float(fin.min()), float(fin.max())) if fin.numel() else (0.0, 1.0)
        if not vmax > vmin:
            vmax = vmin + 1.0
    table = _lut(cmap) if isinstance(cmap, str) else cmap
    rgba = shade(buf["prim"], buf["edge"] if edges else None, value, vmin, vmax, table, ss=ssaa)
    return (rgba, buf) if return_buffers else rgba
