"""CPU: the host side of the renderer -- PNG files, the camera, the colour map,
the visualize command line -- and the numpy oracle of render_cases against
hand-counted cases (the GPU tests then hold the kernels to that oracle)."""
import os

import numpy as np
import pytest

from render_cases import (PIXEL_CAMERA, Scene, box_filter, fan, isqrt, lut_index64, project64, raster_oracle, scenes,
                          shade_oracle)


# ---- PNG ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (5, 17), (3, 2), (64, 33)])
def test_png_round_trip(tmp_path, shape):
    from tropical.utils.image import read_png, write_png
    rng = np.random.default_rng(shape[0] * 100 + shape[1])
    img = rng.integers(0, 256, shape + (4,), dtype=np.uint8)
    path = str(tmp_path / "sub" / "a.png")  # (the directory is made)
    write_png(path, img)
    assert open(path, "rb").read(8) == b"\x89PNG\r\n\x1a\n"
    back = read_png(path)
    assert back.dtype == np.uint8 and np.array_equal(back, img)


def test_png_is_read_by_pil(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from tropical.utils.image import write_png
    rng = np.random.default_rng(3)
    for shape in [(1, 1), (7, 13)]:
        img = rng.integers(0, 256, shape + (4,), dtype=np.uint8)
        path = str(tmp_path / f"{shape[0]}x{shape[1]}.png")
        write_png(path, img)
        with Image.open(path) as im:
            assert im.mode == "RGBA" and im.size == (shape[1], shape[0])
            assert np.array_equal(np.asarray(im), img)


def test_png_refuses_what_it_does_not_write(tmp_path):
    from tropical.utils.image import read_png, write_png
    with pytest.raises(ValueError, match="uint8"):
        write_png(str(tmp_path / "x.png"), np.zeros((2, 2, 3), np.uint8))
    with pytest.raises(ValueError, match="uint8"):
        write_png(str(tmp_path / "x.png"), np.zeros((2, 2, 4), np.float32))
    (tmp_path / "y.png").write_bytes(b"not a png at all")
    with pytest.raises(ValueError, match="not a PNG"):
        read_png(str(tmp_path / "y.png"))


def test_image_module_needs_no_imaging_library():
    import tropical.utils.colormap as cm
    import tropical.utils.image as im
    for mod in (im, cm):
        src = open(mod.__file__).read()
        code = src.split('"""', 2)[2]  # (the docstring may name them)
        assert "import PIL" not in code and "from PIL" not in code
        assert "import matplotlib" not in code and "from matplotlib" not in code


# ---- camera -------------------------------------------------------------------------
ANGLES = [(15, 120, 0, "z"), (15, -10, 10, "y"), (90, 30, 0, "z"), (-35, 200, -20, "x"), (0, 0, 0, "z"),
          (120, 45, 5, "z")]


@pytest.mark.parametrize("elev,azim,roll,axis", ANGLES)
def test_camera_rows_are_orthonormal(elev, azim, roll, axis):
    from tropical.utils.render import Camera
    R = Camera.from_angles(elev, azim, roll, axis).rotation()
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-12
    assert abs(np.linalg.det(R) - 1) < 1e-12  # right x up = toward


@pytest.mark.parametrize("axis", ["x", "y", "z"])
def test_camera_elevation_and_azimuth(axis):
    from tropical.utils.render import Camera
    k = "xyz".index(axis)
    e = np.eye(3)[k]
    top = Camera.from_angles(90, 40, 0, axis)
    assert np.abs(top.toward - e).max() < 1e-12      # looks down the vertical axis
    assert abs(top.right @ e) < 1e-12 and abs(top.up @ e) < 1e-12
    for elev in (0, 25):
        a, b = Camera.from_angles(elev, 10, 0, axis), Camera.from_angles(elev, 75, 0, axis)
        assert abs(a.toward @ e - np.sin(np.radians(elev))) < 1e-12  # the elevation is the angle above the plane
        # azim turns the viewer about the vertical axis by the difference of the angles
        pa, pb = a.toward - (a.toward @ e) * e, b.toward - (b.toward @ e) * e
        assert abs(b.toward @ e - a.toward @ e) < 1e-12
        assert np.abs(np.cross(pa, pb) - np.sin(np.radians(65)) * np.cos(np.radians(elev)) ** 2 * e).max() < 1e-12
        assert abs(a.up @ e - np.cos(np.radians(elev))) < 1e-12      # the vertical axis points up the image
        assert abs(a.right @ e) < 1e-12


@pytest.mark.parametrize("elev,azim,roll,axis", ANGLES)
def test_camera_is_matplotlibs(elev, azim, roll, axis):
    proj3d = pytest.importorskip("mpl_toolkits.mplot3d.proj3d")
    if not hasattr(proj3d, "_view_axes"):
        pytest.skip("this matplotlib has no proj3d._view_axes")
    from tropical.utils.render import Camera
    k = "xyz".index(axis)
    e, a = np.radians(elev), np.radians(azim)
    eye = np.roll([np.cos(e) * np.cos(a), np.cos(e) * np.sin(a), np.sin(e)], k - 2)  # axes3d.get_proj
    V = np.zeros(3)
    V[k] = -1 if abs(e) > np.pi / 2 else 1
    u, v, w = proj3d._view_axes(eye, np.zeros(3), V, np.radians(roll))
    cam = Camera.from_angles(elev, azim, roll, axis)
    assert np.abs(cam.rotation() - np.stack([u, v, w])).max() < 1e-12


@pytest.mark.parametrize("proj", ["ortho", "persp"])
def test_camera_fit_keeps_the_box_inside(proj):
    from tropical.utils.render import Camera
    rng = np.random.default_rng(4)
    pts = rng.uniform(-1, 1, (200, 3)) * [0.3, 1.7, 0.9] + [0.2, -0.4, 3.0]
    lo, hi = pts.min(0), pts.max(0)
    corners = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
    for W, H in [(130, 67), (64, 64), (17, 5)]:
        cam = Camera.from_angles(20, -50, 7, "y", proj).fit(pts, W, H, margin=0.05)
        assert (cam.persp_dist > 0) == (proj == "persp")
        sx, sy, sz, flag, q = project64(corners, cam.right, cam.up, cam.toward, cam.center, cam.scale, cam.persp_dist,
                                        cam.depth_half, W, H)
        assert not flag.any()
        assert (sx >= 0).all() and (sx <= 16 * W).all() and (sy >= 0).all() and (sy <= 16 * H).all()
        assert np.abs(q).max() < 1
        # and the box fills the image up to the margin in one direction
        fill = max((sx.max() - sx.min()) / (16 * W), (sy.max() - sy.min()) / (16 * H))
        # (to the rounding of a corner, 1/16 px; under perspective the scale allows for the nearest depth)
        assert (0.85 if proj == "ortho" else 0.7) <= fill <= 0.93
        vw = cam.view(W, H, 2)
        assert (vw.width, vw.height) == (W, H) and abs(vw.scale - 2 * cam.scale) <= 1e-6 * cam.scale


# ---- colour map ----------------------------------------------------------------------
def test_plasma_table():
    from tropical.utils.colormap import PLASMA, lut
    t = lut("plasma")
    assert t.shape == (256, 3) and t.dtype == np.uint8 and len(PLASMA) == 256
    assert tuple(t[0]) != tuple(t[-1])
    assert tuple(t[0]) == (12, 7, 134) and tuple(t[-1]) == (239, 248, 33)  # dark blue to yellow
    g = lut("gray")
    assert np.array_equal(g[:, 0], np.arange(256)) and np.array_equal(g[:, 0], g[:, 2])
    with pytest.raises(ValueError):
        lut("nope")


def test_plasma_table_is_matplotlibs():
    matplotlib = pytest.importorskip("matplotlib")
    from tropical.utils.colormap import lut
    want = matplotlib.colormaps["plasma"](np.arange(256), bytes=True)[:, :3]
    assert np.array_equal(lut("plasma"), want)


# ---- the oracle against hand-counted cases -----------------------------------------------
def _draw(sc, screen=None):
    if screen is None:  # the pixel camera is exact on multiples of 1/16
        sx, sy, sz, flag, _ = project64(sc.xyz, W=sc.W, H=sc.H, D=0.0, h=1.0,
                                        **{k: PIXEL_CAMERA[k] for k in ("right", "up", "toward", "center", "scale")})
        screen = np.stack([sx, sy, np.where(flag, -1, sz)], 1).astype(np.int64)
    return raster_oracle(screen, sc.off, sc.idx, sc.W, sc.H, sc.hw)


def test_oracle_quad_covers_each_centre_once():
    """A quad whose corners, edges and diagonal run through pixel centres,
    split on either diagonal: every centre the ownership rule gives the quad
    is covered by exactly one of the two triangles."""
    sc = scenes()["quad_diagonals_17x5"]
    prim, tri, edge, st = _draw(sc)
    counts = np.zeros((sc.H, sc.W), int)
    for T in range(4):
        counts += _draw(Scene(sc.W, sc.H, [sc.polys[T]]))[0] >= 0
    assert counts.max() == 1                       # no centre twice
    # ownership (clockwise on screen = positive A2 with y down): the top edge
    # (d.y = 0, d.x > 0) does not own its centres, the right edge (d.y > 0) does,
    # the bottom edge (d.y = 0, d.x < 0) does, the left edge (d.y < 0) does not:
    # quad A owns columns 2..4 of rows 1..3, quad B columns 9..11 of rows 1..3
    want = np.zeros((sc.H, sc.W), bool)
    want[1:4, 2:5] = True
    want[1:4, 9:12] = True
    assert np.array_equal(counts == 1, want)
    assert st["pixels_covered"] == 18 and st["n_drawn"] == 4
    # on the diagonal of quad A (centres (2.5, 2.5), (3.5, 3.5)): one triangle each, and a definite one
    assert prim[2, 2] in (0, 1) and prim[3, 3] in (0, 1)


def test_oracle_vertex_on_a_centre_and_zero_area():
    sc = scenes()["vertex_on_centre_17x5"]
    prim, _, _, st = _draw(sc)
    # triangle 0: (2.5, 2.5) -> (6.5, 1.5) -> (4.5, 4.5); the centre (2.5, 2.5) is its vertex: it lies on two
    # edges, 2->0 (d = (-2, -2): not owned) and 0->1 (d = (4, -1): not owned): not covered
    assert prim[2, 2] == -1
    assert prim[2, 4] == 0 and prim[3, 4] == 0     # (4.5, 2.5), (4.5, 3.5) inside
    assert st["pixels_covered"] == int((prim >= 0).sum()) > 0
    # the fan about a centre: the five triangles meet at (10.5, 10.5); exactly one of them covers it
    fan_sc = scenes()["fan_about_centre_64"]
    p, t, _, _ = _draw(fan_sc)
    hits = sum(int(_draw(Scene(64, 64, [poly]))[0][10, 10] >= 0) for poly in fan_sc.polys)
    assert hits == 1 and p[10, 10] >= 0
    sl = scenes()["slivers_64"]
    p, _, _, st = _draw(sl)
    assert (p == -1).all() and st["pixels_covered"] == 0
    assert (st["n_drawn"], st["n_degenerate"], st["n_dropped"]) == (3, 2, 0)


def test_oracle_depth_and_ties():
    sc = scenes()["coplanar_duplicates_64"]
    prim, tri, _, st = _draw(sc)
    assert set(np.unique(prim)) == {-1, 0}          # the lowest number wins every tie
    sc = scenes()["interpenetrating_64"]
    prim, _, _, _ = _draw(sc)
    only0, only1 = _draw(Scene(64, 64, [sc.polys[0]]))[0] >= 0, _draw(Scene(64, 64, [sc.polys[1]]))[0] >= 0
    both = only0 & only1
    assert both.sum() > 50 and (prim[both] == 0).any() and (prim[both] == 1).any()  # each is in front somewhere
    assert (prim[only0 & ~only1] == 0).all() and (prim[only1 & ~only0] == 1).all()
    # depth is the plane's: a flat triangle at q = 0.25 -> sz = floor(0.375 * 2^20) at every pixel
    sx, sy, sz, _, _ = project64([[0, 0, 0.25]], (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0), 1.0, 0.0, 1.0, 8, 8)
    assert int(sz[0]) == 393216 and (int(sx[0]), int(sy[0])) == (64, 64)


def test_oracle_threshold_and_edge_mask():
    sc = scenes()["threshold_130x67"]
    _, _, _, st = _draw(sc)
    assert st["n_large"] == 4 and st["n_triangles"] == 6
    ids, pid, t, deg = fan(np.array([0, 7, 10]), np.arange(10))
    assert len(ids) == 6 and list(pid) == [0] * 5 + [1] and list(t) == [0, 1, 2, 3, 4, 0] and list(deg) == [7] * 5 + [3]
    assert list(ids[4]) == [0, 5, 6] and list(ids[5]) == [7, 8, 9]
    thin, wide = (_draw(scenes()[k]) for k in ("heptagon_hw8_64", "heptagon_hw40_64"))
    assert np.array_equal(thin[0], wide[0])
    assert 0 < thin[2].sum() < wide[2].sum() and (thin[2] <= wide[2]).all()
    # the heptagon's centre region is far from its boundary: fan diagonals are not edges
    assert wide[0][31, 30] == 0 and wide[2][25:37, 24:36].sum() == 0
    # the triangle (a degree-3 polygon): all three sides are boundary; its pixels next to any side are marked
    assert (wide[2][wide[0] == 1] == 1).mean() > 0.5
    assert list(isqrt(np.array([0, 1, 3, 4, 24, 25, 26, (1 << 39) - 1, 1 << 38]))) == \
        [0, 1, 1, 2, 4, 5, 5, 741455, 1 << 19]


def test_oracle_shade_and_box_filter():
    prim = np.array([[-1, 0], [1, 1]], np.int32)
    edge = np.array([[0, 0], [1, 0]], np.uint8)
    idx = lut_index64([-1.0, 0.5, 2.0], -1, 1)
    assert list(idx) == [0, 191, 255]
    grey = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, 1)
    img = shade_oracle(prim, edge, idx, grey, (10, 20, 30, 255))
    assert img[0, 0].tolist() == [0, 0, 0, 0] and img[0, 1].tolist() == [0, 0, 0, 255]
    assert img[1, 0].tolist() == [10, 20, 30, 255] and img[1, 1].tolist() == [191, 191, 191, 255]
    out = box_filter(img, 2)
    assert out.shape == (1, 1, 4) and out[0, 0].tolist() == [(10 + 191 + 2) // 4, (20 + 191 + 2) // 4,
                                                              (30 + 191 + 2) // 4, (3 * 255 + 2) // 4]


# ---- command line -------------------------------------------------------------------------------
def test_visualize_cli_parsing_and_names(tmp_path, capsys):
    import tropical.stanford.visualize as vz
    a = vz.parse_args([])
    assert (a.dataset, a.seed, a.model_size, a.out, a.ssaa, a.no_edges, a.view, a.persp) == \
        ("dragon", 45, "small", "meshes", 2, False, None, False)
    a = vz.parse_args(["-d", "bunny", "-s", "31", "-m", "large", "--out", "m", "--size", "640", "480", "--ssaa", "4",
                       "--no-edges", "--view", "10", "-45.5", "--persp"])
    assert (a.dataset, a.seed, a.model_size, a.out, a.size, a.ssaa, a.no_edges, a.view, a.persp) == \
        ("bunny", 31, "large", "m", [640, 480], 4, True, [10.0, -45.5], True)
    with pytest.raises(SystemExit):
        vz.parse_args(["--ssaa", "3"])
    assert vz.output_name("outputs", "bunny", "large", "ours") == os.path.join("outputs", "bunny", "large_ours.png")
    assert vz.output_name("o", "dragon", "small", "mc016") == os.path.join("o", "dragon", "small_mc016.png")
    assert set(vz.VIEWS) == {"bunny", "dragon", "happy", "armadillo", "drill", "lucy"}
    # the plotted mesh's normal component that is the mesh's own: a triangle in the xy plane, normal +z,
    # plotted as (x, z, y) has the Newell normal -y; a stored normal vector becomes +y
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0.0]])[:, [0, 2, 1]]
    assert np.cross(tri[1] - tri[0], tri[2] - tri[0]).tolist() == [0, -1, 0]
    assert [vz.plotted_axis("z", True, True), vz.plotted_axis("z", True, False)] == ["-y", "y"]
    assert [vz.plotted_axis("-z", True, True), vz.plotted_axis("y", False, True), vz.plotted_axis("x", True, False)] \
        == ["y", "y", "x"]
    # what exists is found: the polygon file is preferred, marching meshes by method and resolution
    d = tmp_path / "meshes" / "bunny"
    d.mkdir(parents=True)
    assert vz.find_meshes(str(d), "small_45") == []
    for n in ("our_mesh_small_45", "mc128_mesh_small_45", "mc016_mesh_small_45", "mtet032_mesh_small_45",
              "mc016_mesh_small_46", "our_mesh_large_45"):
        (d / f"{n}.ply").write_bytes(b"")
    found = vz.find_meshes(str(d), "small_45")
    assert [(os.path.basename(p), s, poly) for p, s, poly in found] == [
        ("our_mesh_small_45.ply", "ours", False), ("mc016_mesh_small_45.ply", "mc016", False),
        ("mc128_mesh_small_45.ply", "mc128", False), ("mtet032_mesh_small_45.ply", "mtet032", False)]
    (d / "our_poly_mesh_small_45.ply").write_bytes(b"")
    assert [(os.path.basename(p), s, poly) for p, s, poly in vz.find_meshes(str(d), "small_45")][0] == \
        ("our_poly_mesh_small_45.ply", "ours", True)
    # nothing to draw: a message, as evaluate's, and no GPU needed
    assert vz.main(["-d", "lucy", "--out", str(tmp_path / "meshes")]) == 0
    assert "Mesh path is not found" in capsys.readouterr().out


def test_visualize_needs_a_gpu(tmp_path, monkeypatch):
    import torch

    import tropical.stanford.visualize as vz
    d = tmp_path / "meshes" / "bunny"
    d.mkdir(parents=True)
    (d / "our_mesh_small_45.ply").write_bytes(b"")
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit, match=r"tropical\.stanford\.visualize needs a ROCm GPU \(no CPU fallback\)"):
        vz.main(["-d", "bunny", "--out", str(tmp_path / "meshes")])
