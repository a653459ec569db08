"""GPU: the rasteriser (tnp_render_raster / tnp_render_shade, csrc/render.hip)
against the numpy restatement of its contract in render_cases: projection
within one unit of float64, coverage / depth / tie-break / edge mask exact,
both coverage paths identical, shading and the box filter, refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

from golden_io import load
from helpers import product_net
from render_cases import (GUARD, PIXEL_CAMERA, box_filter, fan, lut_index64, project64, raster_oracle, scenes,
                          shade_oracle)

pytestmark = pytest.mark.gpu
SCENES = scenes()
GREY = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, 1)
EDGE = (200, 30, 40, 255)
STAT_KEYS = ["n_polygons", "n_drawn", "n_dropped", "n_degenerate", "n_triangles", "n_large", "pixels_covered"]


def pixel_camera():
    from tropical.utils.render import Camera
    return Camera(**PIXEL_CAMERA)


def draw(xyz, off, idx, cam, W, H, hw, mode=0):
    """rasterize() under coverage-path mode `mode`; everything as numpy."""
    from tropical import _hip
    from tropical.utils.render import rasterize
    assert _hip.lib().tnp_debug_render_path(mode) >= 0
    try:
        r = rasterize((xyz, off, idx), cam, (W, H), edge_half_width=hw, screen=True)
    finally:
        _hip.lib().tnp_debug_render_path(0)
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in r.items()}


def check_exact(r, off, idx, W, H, hw, label):
    """The buffers against the oracle fed with the GPU's own screen coordinates."""
    prim, tri, edge, st = raster_oracle(r["screen"], off, idx, W, H, hw)
    bad = (r["prim"] != prim).sum(), (r["tri"] != tri).sum(), (r["edge"] != edge).sum()
    print(f"{label}: {W}x{H}, {st['n_triangles']} triangles ({st['n_large']} large), {st['pixels_covered']} px covered, "
          f"{int(edge.sum())} edge px; mismatches prim/tri/edge {bad}")
    assert r["prim"].shape == (H, W) and r["prim"].dtype == np.int32 and r["edge"].dtype == np.uint8
    assert bad == (0, 0, 0)
    assert {k: r["stats"][k] for k in STAT_KEYS} == st
    return prim, tri, edge, st


# ---- 1. projection ---------------------------------------------------------------------
@pytest.mark.parametrize("proj", ["ortho", "persp"])
def test_projection_matches_float64(cuda, proj):
    from tropical.utils.render import Camera
    rng = np.random.default_rng(21)
    W, H = 130, 67
    inside = rng.uniform(-1, 1, (3000, 3)).astype(np.float32) * np.float32(0.8)
    cam = Camera.from_angles(25, -40, 12, "y", proj).fit(np.array([[-1, -1, -1], [1, 1, 1]]) * 0.8, W, H)
    vw = cam.view(W, H)
    R = [np.array(list(getattr(vw, k)), np.float64) for k in ("right", "up", "toward", "center")]  # the fp32 fields
    h, D, sc = float(vw.depth_half), float(vw.persp_dist), float(vw.scale)
    # outside: far along `right` (past the guard band), beyond either depth end, and behind the viewer
    far = np.array(list(vw.right)) * (1.5 * GUARD / 16 / sc) + [0.01, 0.02, 0.03]
    deep, near = -np.array(list(vw.toward)) * 1.5 * h, np.array(list(vw.toward)) * 1.3 * h
    out = [far, -far, deep, near, np.array(list(vw.up)) * (-2.0 * GUARD / 16 / sc)]
    if proj == "persp":
        out.append(np.array(list(vw.toward)) * 1.5 * D)
    xyz = np.concatenate([inside, np.array(out, np.float32)])
    nin = len(inside)
    # triangles over the inside vertices, then one through each outside vertex
    tris = [list(rng.choice(nin, 3, replace=False)) for _ in range(300)]
    tris += [[nin + k, k, k + 1] for k in range(len(out))]
    off, idx = np.arange(0, 3 * len(tris) + 1, 3), np.array(tris).reshape(-1)
    r = draw(xyz, off, idx, cam, W, H, 8)
    sx, sy, sz, flag, q = project64(xyz.astype(np.float64), *R, sc, D, h, W, H)
    assert not flag[:nin].any() and flag[nin:].all()
    assert np.abs(np.abs(q[:nin]) - 1).min() > 1e-3      # (no inside vertex near a depth end: the flags are clear-cut)
    got = r["screen"].astype(np.int64)
    err = [np.abs(got[:nin, k] - w[:nin]).max() for k, w in enumerate((sx, sy, sz))]
    print(f"{proj}: max |d_screen - float64| in sx, sy, sz = {err} units (bound 1)")
    assert max(err) <= 1
    assert (got[nin:] == [0, 0, -1]).all()        # flagged rows
    assert sz[:nin].min() > 0 and sz[:nin].max() < (1 << 20) - 1 and got[:nin, 2].std() > 1000
    # their polygons are dropped and counted, and none of their pixels appear
    prim, _, _, st = check_exact(r, off, idx, W, H, 8, f"projection {proj}")
    assert st["n_dropped"] == len(out) and r["stats"]["n_dropped"] == len(out)
    assert not np.isin(r["prim"], np.arange(300, 300 + len(out))).any() and (r["prim"] >= 0).sum() > 1000


# ---- 2. raster, exact --------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SCENES))
def test_raster_is_the_oracle_on_both_paths(cuda, name):
    sc = SCENES[name]
    r = draw(sc.xyz, sc.off, sc.idx, pixel_camera(), sc.W, sc.H, sc.hw)
    prim, tri, edge, st = check_exact(r, sc.off, sc.idx, sc.W, sc.H, sc.hw, name)
    # every triangle by one thread, then every triangle by a workgroup: the same buffers
    for mode in (1, 2):
        m = draw(sc.xyz, sc.off, sc.idx, pixel_camera(), sc.W, sc.H, sc.hw, mode)
        for k in ("screen", "prim", "tri", "edge"):
            assert np.array_equal(m[k], r[k]), (name, mode, k)
        assert m["stats"]["pixels_covered"] == st["pixels_covered"]
        assert m["stats"]["n_large"] == (0 if mode == 1 else _n_drawable(r["screen"], sc) if st["n_triangles"] else 0)


def _n_drawable(screen, sc):
    """Triangles with area, not dropped, whose clamped box holds a pixel centre."""
    ids, _, _, _ = fan(sc.off, sc.idx)
    v = screen.astype(np.int64)[ids]                                  # [nT, 3, 3]
    area = (v[:, 1, 0] - v[:, 0, 0]) * (v[:, 2, 1] - v[:, 0, 1]) - (v[:, 1, 1] - v[:, 0, 1]) * (v[:, 2, 0] - v[:, 0, 0])
    i0, i1 = np.maximum(-((8 - v[:, :, 0].min(1)) // 16), 0), np.minimum((v[:, :, 0].max(1) - 8) // 16, sc.W - 1)
    j0, j1 = np.maximum(-((8 - v[:, :, 1].min(1)) // 16), 0), np.minimum((v[:, :, 1].max(1) - 8) // 16, sc.H - 1)
    return int(((v[:, :, 2] >= 0).all(1) & (area != 0) & (i1 >= i0) & (j1 >= j0)).sum())


def test_scenes_run_what_they_are_for(cuda):
    """The scenes' own claims, from the GPU's buffers: both paths in one frame,
    the threshold crossed, the ties, the empty image."""
    r = draw(*(getattr(SCENES["full_over_4000_64"], k) for k in ("xyz", "off", "idx")), pixel_camera(), 64, 64, 8)
    assert r["stats"]["n_large"] == 1 and r["stats"]["n_triangles"] == 4001 and r["stats"]["pixels_covered"] == 64 * 64
    assert (r["prim"] == 0).sum() > 500 and (r["prim"] > 0).sum() > 500
    sc = SCENES["threshold_130x67"]
    r = draw(sc.xyz, sc.off, sc.idx, pixel_camera(), sc.W, sc.H, sc.hw)
    # boxes of (S, S), (S + 1, S), (S, S + 1), (S + 1, S + 1) centres (S = TNP_RENDER_SMALL_MAX), then an overlapping small / large pair
    assert r["stats"]["n_large"] == 4 and all((r["prim"] == p).any() for p in range(6))
    r = draw(*(getattr(SCENES["coplanar_duplicates_64"], k) for k in ("xyz", "off", "idx")), pixel_camera(), 64, 64, 8)
    assert set(np.unique(r["prim"])) == {-1, 0}
    e = SCENES["empty_64"]
    r = draw(e.xyz.reshape(0, 3), e.off, e.idx, pixel_camera(), 64, 64, 8)
    assert (r["prim"] == -1).all() and (r["tri"] == -1).all() and (r["edge"] == 0).all()
    assert all(r["stats"][k] == 0 for k in STAT_KEYS)
    s = SCENES["slivers_64"]
    r = draw(s.xyz, s.off, s.idx, pixel_camera(), 64, 64, 8)
    assert (r["prim"] == -1).all() and (r["stats"]["n_drawn"], r["stats"]["n_degenerate"]) == (3, 2)
    one = SCENES["pixel_1x1"]
    r = draw(one.xyz, one.off, one.idx, pixel_camera(), 1, 1, 8)
    assert r["prim"].tolist() == [[0]]


# ---- 3. the extracted surface ---------------------------------------------------------------
def test_extracted_surface_renders_exactly(cuda):
    import tropical.subpoly as sp
    from tropical.utils.render import Camera
    net = product_net(load("small_sphere"), cuda)
    _, verts, _, pm = sp.subpoly(net, 3, 1.2, force=True, polygons=True)
    print()
    W = H = 128
    cam = Camera.from_angles(15, 120).fit(pm.vertices, W, H)
    xyz = pm.vertices.astype(np.float32)
    r = draw(xyz, pm.offsets, pm.indices, cam, W, H, 8)
    prim, tri, edge, st = check_exact(r, pm.offsets, pm.indices, W, H, 8, "small_sphere polygons")
    assert st["n_dropped"] == 0 and st["pixels_covered"] > 2000
    assert r["prim"].max() < len(pm) and r["prim"].min() == -1 and r["tri"].max() < st["n_triangles"]
    # the fan triangles as a triangle mesh: the same image, ids mapped back to polygons
    ids, pid, _, _ = fan(pm.offsets, pm.indices)
    assert np.array_equal(ids, pm.triangles())
    t = draw(xyz, np.arange(0, 3 * len(ids) + 1, 3), ids.reshape(-1), cam, W, H, 8)
    check_exact(t, np.arange(0, 3 * len(ids) + 1, 3), ids.reshape(-1), W, H, 8, "small_sphere triangles")
    assert np.array_equal(t["prim"], r["tri"]) and np.array_equal(t["tri"], r["tri"])
    assert np.array_equal(np.where(t["prim"] >= 0, pid[t["prim"]], -1), r["prim"])
    # fan diagonals are edges of the triangle mesh only
    assert (r["edge"] <= t["edge"]).all() and 0 < r["edge"].sum() < t["edge"].sum()
    # and the whole figure through render(): the default value is the normals' z
    from tropical.utils.render import render
    rgba, buf = render(pm, cam, size=(W, H), return_buffers=True)
    assert rgba.shape == (H, W, 4) and rgba.dtype == torch.uint8 and rgba.is_cuda
    assert np.array_equal(buf["prim"].cpu().numpy(), r["prim"])
    a = rgba.cpu().numpy()
    assert ((a[..., 3] == 255) == (r["prim"] >= 0)).all() and (a[r["prim"] < 0] == 0).all()
    assert (a[r["edge"] == 1] == [0, 0, 0, 255]).all()


# ---- 4. shade ------------------------------------------------------------------------------------
def test_shade_index_edges_background_and_box_filter(cuda):
    from tropical.utils.render import shade
    sc = SCENES["full_over_4000_64"]
    r = draw(sc.xyz, sc.off, sc.idx, pixel_camera(), 64, 64, 6)
    P = len(sc.off) - 1
    rng = np.random.default_rng(8)
    value = rng.uniform(-1.3, 1.3, P).astype(np.float32)
    value[:5] = [-1.0, 1.0, 0.0, -2.0, 7.5]
    prim, edge = (torch.from_numpy(r[k]).to(cuda) for k in ("prim", "edge"))
    img = {ss: shade(prim, edge, torch.from_numpy(value), -1.0, 1.0, GREY, EDGE, ss).cpu().numpy() for ss in (1, 2, 4)}
    a = img[1]
    assert a.shape == (64, 64, 4) and img[2].shape == (32, 32, 4) and img[4].shape == (16, 16, 4)
    bg, ed = r["prim"] < 0, (r["prim"] >= 0) & (r["edge"] == 1)
    face = (r["prim"] >= 0) & ~ed
    assert ed.sum() > 100 and face.sum() > 1000
    assert (a[ed] == EDGE).all()                                   # edge pixels: exact
    want = lut_index64(value.astype(np.float64), -1.0, 1.0)[r["prim"][face]]
    got = a[face]
    assert (got[:, 0] == got[:, 1]).all() and (got[:, 0] == got[:, 2]).all() and (got[:, 3] == 255).all()
    err = np.abs(got[:, 0].astype(np.int64) - want)
    print(f"LUT index: max |gpu - float64| = {err.max()} (bound 1), {int((err > 0).sum())} of {err.size} differ")
    assert err.max() <= 1
    # a background: the 1 x 1 scene's neighbour image with nothing in it
    e = SCENES["empty_64"]
    rb = draw(e.xyz.reshape(0, 3), e.off, e.idx, pixel_camera(), 64, 64, 6)
    none = shade(torch.from_numpy(rb["prim"]).to(cuda), None, torch.zeros(0), -1.0, 1.0, GREY, EDGE, 1).cpu().numpy()
    assert (none == 0).all() and (a[bg] == 0).all()
    # the supersampled outputs are the integer box filter of the ss = 1 image, exactly
    for ss in (2, 4):
        assert np.array_equal(img[ss], box_filter(a, ss)), ss
    # and with the oracle's indices replaced by the GPU's the whole image is the oracle's
    index = lut_index64(value.astype(np.float64), -1.0, 1.0)
    ref = shade_oracle(r["prim"], r["edge"], index, GREY, EDGE)
    assert np.abs(a.astype(np.int64) - ref).max() <= 1 and np.array_equal(a[..., 3], ref[..., 3])
    for bad, msg in [(dict(ss=3), "ss = 3"), (dict(vmax=-1.0), "vmax must be larger")]:
        kw = dict(vmin=-1.0, vmax=1.0, ss=1)
        kw.update(bad)
        with pytest.raises(RuntimeError, match=msg):
            shade(prim, edge, torch.from_numpy(value), kw["vmin"], kw["vmax"], GREY, EDGE, kw["ss"])


# ---- 5. determinism ---------------------------------------------------------------------------------
def test_two_runs_are_byte_identical(cuda):
    from tropical.utils.mesh import PolygonMesh
    from tropical.utils.render import render
    sc = SCENES["full_over_4000_64"]
    pm = PolygonMesh(sc.xyz, sc.off, sc.idx)
    runs = [render(pm, pixel_camera(), size=(32, 32), ssaa=2, edge_width=0.5, return_buffers=True) for _ in range(2)]
    (a, ba), (b, bb) = runs
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    for k in ("prim", "tri", "edge"):
        assert ba[k].cpu().numpy().tobytes() == bb[k].cpu().numpy().tobytes()
    assert ba["stats"] == bb["stats"] and ba["prim"].shape == (64, 64) and a.shape == (32, 32, 4)
    assert len(np.unique(a.cpu().numpy().reshape(-1, 4), axis=0)) > 20


# ---- 6. refusal -------------------------------------------------------------------------------------------
def test_malformed_input_is_refused_and_costs_nothing(cuda):
    sc = SCENES["heptagon_hw8_64"]
    V = len(sc.xyz)
    cam = pixel_camera()
    bad_idx = sc.idx.copy()
    bad_idx[4] = V + 3
    bad = [
        (sc.off, bad_idx, 64, rf"indices\[4\] = {V + 3} is outside \[0, {V}\)"),
        (np.array([0, 5, 7, 10]), sc.idx, 64, r"polygon 1 has 2 ids, fewer than 3"),
        (np.array([1, 7, 10]), sc.idx, 64, r"offsets\[0\] = 1, not 0"),
        (sc.off, sc.idx, 9000, r"width = 9000 is outside \[1, 8192\]"),
    ]
    for off, idx, W, msg in bad:
        with pytest.raises(RuntimeError, match=msg):
            draw(sc.xyz, off, idx, cam, W, 64, sc.hw)
        # the next valid render in the same process is still exact
        r = draw(sc.xyz, sc.off, sc.idx, cam, sc.W, sc.H, sc.hw)
        check_exact(r, sc.off, sc.idx, sc.W, sc.H, sc.hw, f"after refusing {msg[:12]!r}")
    from tropical import _hip
    from tropical.utils.render import rasterize
    with pytest.raises(RuntimeError, match=r"edge_half_width = 300 is outside \[0, 256\]"):
        rasterize((sc.xyz, sc.off, sc.idx), cam, (64, 64), edge_half_width=300)
    assert _hip.lib().tnp_debug_render_path(7) == -1 and _hip.lib().tnp_debug_render_path(0) == 0
    assert C.sizeof(_hip.TnpRenderView) == 17 * 4 and C.sizeof(_hip.TnpRenderStats) == 7 * 8


def test_render_checks_before_it_computes_the_default_value(cuda, monkeypatch):
    """render() with the default value: the library's check comes first, so the
    torch gathers of the Newell normal never see an unchecked offset or id."""
    import tropical.utils.render as rd
    sc = SCENES["heptagon_hw8_64"]
    V = len(sc.xyz)
    calls = []
    real = rd.newell_normals
    monkeypatch.setattr(rd, "newell_normals", lambda *a: calls.append(1) or real(*a))
    bad_idx = sc.idx.copy()
    bad_idx[4] = V + 3
    far_idx = sc.idx.copy()
    far_idx[7] = 1 << 40
    for off, idx, size, msg in [
            (sc.off, bad_idx, (64, 64), rf"indices\[4\] = {V + 3} is outside \[0, {V}\)"),
            (sc.off, far_idx, (64, 64), rf"indices\[7\] = {1 << 40} is outside"),
            (np.array([0, 5, 7, 10]), sc.idx, (64, 64), r"polygon 1 has 2 ids, fewer than 3"),
            (np.array([1, 7, 10]), sc.idx, (64, 64), r"offsets\[0\] = 1, not 0"),
            (np.array([0, 12, 10]), sc.idx, (64, 64), r"offsets decrease at polygon 1"),
            (sc.off, sc.idx, (9000, 64), r"width = 36000 is outside \[1, 8192\]")]:
        with pytest.raises(RuntimeError, match=msg):
            rd.render((sc.xyz, off, idx), pixel_camera(), size=size, ssaa=4 if size[0] == 9000 else 1)
        assert calls == []
    # a valid soup, given as host int32 arrays and as device tensors: the same figure, normals computed once each
    a = rd.render((sc.xyz, sc.off.astype(np.int32), sc.idx.astype(np.int32)), pixel_camera(), size=(64, 64))
    t = [torch.from_numpy(x).to(cuda) for x in (sc.xyz, sc.off, sc.idx)]
    b, buf = rd.render((t[0], t[1], t[2], None), pixel_camera(), size=(64, 64), return_buffers=True)
    assert calls == [1, 1] and torch.equal(a, b)
    check_exact({**{k: buf[k].cpu().numpy() for k in ("prim", "tri", "edge")}, "stats": buf["stats"],
                 "screen": draw(sc.xyz, sc.off, sc.idx, pixel_camera(), 64, 64, 8)["screen"]},
                sc.off, sc.idx, 64, 64, 8, "render() after refusals")


# ---- the command line, end to end --------------------------------------------------------------------------
# (ssaa 1 for the run with edges: an unfiltered edge pixel is exactly the edge colour)
@pytest.mark.parametrize("dataset,extra", [("bunny", ["--ssaa", "1"]), ("dragon", ["--view", "20", "35", "--no-edges"])])
def test_visualize_writes_the_figures(cuda, tmp_path, capsys, dataset, extra):
    """A cube as `train --polygons` and `evaluate` would leave it: the polygon
    file is drawn with its six quads' edges, the marching meshes without."""
    import tropical.stanford.visualize as vz
    from tropical.utils.image import read_png
    from tropical.utils.mesh import Mesh, PolygonMesh
    V = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], dtype=np.float64) - 0.5
    Q = np.array([[0, 1, 3, 2], [4, 6, 7, 5], [0, 4, 5, 1], [2, 3, 7, 6], [0, 2, 6, 4], [1, 5, 7, 3]])
    pm = PolygonMesh(V, np.arange(0, 25, 4), Q.reshape(-1))
    d = tmp_path / "meshes" / dataset
    pm.export(str(d / "our_poly_mesh_small_45.ply"))
    Mesh(V, pm.triangles()).export(str(d / "our_mesh_small_45.ply"))
    Mesh(V * 0.8, pm.triangles()).export(str(d / "mc016_mesh_small_45.ply"))
    Mesh(V * 0.9, pm.triangles()).export(str(d / "mtet032_mesh_small_45.ply"))
    assert vz.main(["-d", dataset, "--out", str(tmp_path / "meshes"), "--png-dir", str(tmp_path / "outputs"),
                    "--size", "96", "64", "--ssaa", "2"] + extra) == 0
    out = capsys.readouterr().out
    names = ["small_ours.png", "small_mc016.png", "small_mtet032.png"]
    assert sorted(p.name for p in (tmp_path / "outputs" / dataset).iterdir()) == sorted(names)
    assert "our_poly_mesh_small_45.ply" in out and "(6 faces)" in out and "(12 faces)" in out
    img = {n: read_png(str(tmp_path / "outputs" / dataset / n)) for n in names}
    for n, a in img.items():
        assert a.shape == (64, 96, 4)
        assert (a[..., 3] == 0).sum() > 500 and (a[..., 3] == 255).sum() > 500       # transparent around the cube
        assert (a[0] == 0).all() and (a[:, 0] == 0).all()                               # the margin
    black = {n: int(((a[..., :3] == 0).all(-1) & (a[..., 3] == 255)).sum()) for n, a in img.items()}
    assert black["small_mc016.png"] == 0 and black["small_mtet032.png"] == 0          # plasma has no black
    assert (black["small_ours.png"] > 30) == ("--no-edges" not in extra)
    # one camera for the run: the smaller meshes cover fewer pixels
    cover = [int((img[n][..., 3] > 0).sum()) for n in names]
    assert cover[0] > cover[2] > cover[1]
