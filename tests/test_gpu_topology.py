"""GPU: tnp_topology_* (components and boundary loops of a polygon soup)
against its numpy restatement (topology_cases.topology_ref), on synthetic
soups that are hard for a parallel labelling and on the extracted surfaces;
keep_components; the train / visualize flags."""
import re

import numpy as np
import pytest
import torch

from golden_io import load
from polygon_cases import polygon_stats
from topology_cases import COMP_INT, EDGE_COLS, LOOP_INT, reference, soups

pytestmark = pytest.mark.gpu
SOUPS = ["torus", "cylinder", "two_tets", "cube", "cube_reversed", "moebius", "two_fans", "one", "empty",
         "isolated_1000", "strip_4096", "book_1000", "strip_4096_vperm"]
SURFACES = {"small_torus": (1, 10, 8), "h8l3_sphere": (1, 2, 2), "small_sphere_curve": (59, 47, 35)}
_tol = {}


def _area_tol(name, v, off, idx):
    """The per-polygon fp32 tolerance of tests/test_gpu_polygons.py::_tolerances
    on these very inputs: 4 x the largest difference between the restated
    formula in float32 and in float64."""
    if name not in _tol:
        _, a64, _ = polygon_stats(v, off, idx, np.float64)
        _, a32, _ = polygon_stats(v, off, idx, np.float32)
        _tol[name] = 4 * float(np.abs(a32.astype(np.float64) - a64).max())
    return _tol[name]


def _check(name, connect, data=None, handle=None):
    """One build against the restatement: integers, labels and boxes exactly,
    the doubles within their derived bounds.  Returns the topology."""
    from tropical.utils.topology import polygon_topology
    v, off, idx = soups()[name] if data is None else data
    v = np.asarray(v, np.float32)
    ref = reference(name, connect, data)
    topo = polygon_topology(v, off, idx, connect=connect, handle=handle)
    c, lp, rc, rl = topo.components, topo.loops, ref["components"], ref["loops"]
    assert topo.labels.dtype == torch.int32 and topo.labels.is_cuda
    assert np.array_equal(topo.labels.cpu().numpy(), ref["labels"])
    assert (topo.n_components, topo.n_loops) == (len(rc["euler"]), len(rl["simple"]))
    for k in COMP_INT:
        assert np.array_equal(c[k], rc[k]), (name, connect, k)
    for k in LOOP_INT:
        assert np.array_equal(lp[k], rl[k]), (name, connect, k)
    assert np.array_equal(c["lo"], rc["lo"]) and np.array_equal(c["hi"], rc["hi"])
    assert (lp["reserved"] == 0).all()
    if len(off) > 1:
        tol_a = _area_tol(name, v, off, idx)
        ea = np.abs(c["area"] - rc["area"])
        ba = rc["n_polygons"] * tol_a
        ev = np.abs(c["volume"] - rc["volume"])
        bv = 2.0 ** -53 * (ref["n_tri"] + 8) * ref["det_abs"] / 6
        el = np.abs(lp["length"] - rl["length"])
        bl = 2.0 ** -52 * (rl["n_edges"] + 4) * rl["length"]
        print(f"{name}/{connect}: area err {ea.max():.3g} (bound {ba[ea.argmax()]:.3g}), volume err {ev.max():.3g} "
              f"(bound {bv[ev.argmax()]:.3g}), length err {el.max() if len(el) else 0:.3g} "
              f"(bound {bl[el.argmax()] if len(el) else 0:.3g})")
        assert (ea <= ba).all() and (ev <= bv).all() and (el <= bl).all()
    return topo


@pytest.mark.parametrize("connect", ["edge", "vertex"])
@pytest.mark.parametrize("name", SOUPS)
def test_soup_against_the_restatement(cuda, name, connect):
    topo = _check(name, connect)
    if name == "cube":
        assert topo.components["volume"].tolist() == [8.0] and topo.components["area"].tolist() == [24.0]
    if name == "cube_reversed":
        assert topo.components["volume"].tolist() == [-8.0]
    if name == "empty":
        assert (topo.n_components, topo.n_loops, topo.labels.numel()) == (0, 0, 0)
    if name == "two_tets":
        assert topo.n_components == (2 if connect == "edge" else 1)


def _surface(case, cuda):
    from test_gpu_polygons import run
    _, (_, verts, _, pm) = run(case, cuda)
    return verts.cpu().numpy(), pm


@pytest.mark.parametrize("connect", ["edge", "vertex"])
@pytest.mark.parametrize("case", list(SURFACES))
def test_extracted_surface(cuda, case, connect):
    from tropical.utils.mesh import polygon_report
    v, pm = _surface(case, cuda)
    topo = _check(case, connect, data=(v, pm.offsets, pm.indices))
    C, L, S = SURFACES[case]
    if connect == "edge":
        assert (topo.n_components, topo.n_loops, int(topo.loops["simple"].sum())) == (C, L, S)
    else:
        assert (topo.n_loops, int(topo.loops["simple"].sum())) == (L, S)
        assert topo.n_components == (23 if case == "small_sphere_curve" else 1)
    r = polygon_report(v, pm.offsets, pm.indices)
    for k in EDGE_COLS + ["n_polygons", "n_indices"]:
        assert int(topo.components[k].sum()) == r[k], k
    # the same P per-polygon areas, added in another order: each sum is off by at most (P - 1) 2^-53 of the total
    err, bound = abs(float(topo.components["area"].sum()) - r["area"]), len(pm) * 2.0 ** -52 * r["area"]
    print(f"{case}/{connect}: sum of component areas - report area = {err:.3g} (bound {bound:.3g})")
    assert err <= bound


def test_two_builds_give_the_same_bits(cuda):
    from tropical.utils.topology import polygon_topology
    v, pm = _surface("small_sphere_curve", cuda)
    a = polygon_topology(v, pm.offsets, pm.indices)
    b = polygon_topology(v, pm.offsets, pm.indices)
    assert torch.equal(a.labels, b.labels)
    assert a.components.tobytes() == b.components.tobytes() and a.loops.tobytes() == b.loops.tobytes()
    s = soups()["strip_4096_vperm"]
    a, b = polygon_topology(*s, connect="vertex"), polygon_topology(*s, connect="vertex")
    assert torch.equal(a.labels, b.labels)
    assert a.components.tobytes() == b.components.tobytes() and a.loops.tobytes() == b.loops.tobytes()


def test_a_second_build_replaces_the_first(cuda):
    from tropical.utils.topology import topology_handle
    h = topology_handle()
    try:
        big = _check("isolated_1000", "edge", handle=h)
        small = _check("cylinder", "edge", handle=h)
        assert (big.n_components, small.n_components, small.n_loops, small.labels.numel()) == (1000, 1, 2, 56)
        _check("empty", "edge", handle=h)
        _check("cube", "vertex", handle=h)
    finally:
        h.close()


def test_keep_the_largest_component(cuda):
    from tropical.utils.mesh import PolygonMesh, polygon_report
    from tropical.utils.topology import keep_components, largest_components, polygon_topology
    v, pm = _surface("small_sphere_curve", cuda)
    pm = PolygonMesh(v, pm.offsets, pm.indices, pm.normals)
    topo = polygon_topology(pm.vertices, pm.offsets, pm.indices)
    ids = largest_components(topo.components, 1)
    kept = keep_components(pm, topo.labels, ids)
    row = topo.components[ids[0]]
    assert len(kept) == 2103 == row["n_polygons"] and kept.normals.shape == (2103, 3)
    t2 = polygon_topology(kept.vertices, kept.offsets, kept.indices)
    assert t2.n_components == 1 and (t2.labels == 0).all()
    r = polygon_report(kept.vertices, kept.offsets, kept.indices)
    for k in EDGE_COLS + ["n_polygons", "n_indices", "euler"]:
        assert r[k] == row[k] == t2.components[0][k], k
    assert r["n_vertices_used"] == row["n_vertices"] == len(kept.vertices)
    assert t2.components[0]["area"].tobytes() == row["area"].tobytes()  # the same polygons in the same order


def test_train_and_visualize_flags(cuda, tmp_path, capsys):
    """The --components / --keep-largest report of train on a fixture net's
    surface (no dataset), then visualize --color component on what it wrote."""
    import tropical.stanford.train as tr
    import tropical.stanford.visualize as vz
    from tropical.utils.mesh import load_polygon_ply
    from tropical.utils.topology import keep_components, largest_components
    args = tr.parse_args(["--keep-largest", "1"])
    assert args.components and args.polygons and args.keep_largest == 1
    assert tr.parse_args(["--components"]).polygons and not tr.parse_args(["--polygons"]).components
    v, pm = _surface("small_sphere_curve", cuda)
    verts = v / tr.R
    out = tmp_path / "meshes" / "bunny"
    path = str(out / "our_poly_mesh_small_45.ply")
    capsys.readouterr()
    tr.export_polygons(pm, verts, path)
    topo = tr.export_components(pm, verts, path, keep_largest=1)
    lines = capsys.readouterr().out.splitlines()
    assert lines[0].startswith("Ours (polygons): ")
    g = re.fullmatch(r"Ours \(components\): (\d+) pieces \(edge-connected\), (\d+) boundary loops \((\d+) simple\), "
                     r"longest loop (\d+) edges / length (\S+)", lines[1])
    assert g, lines[1]
    assert [int(g.group(i)) for i in (1, 2, 3)] == [59, 47, 35]
    assert int(g.group(4)) == topo.loops["n_edges"].max() and float(g.group(5)) > 0
    rows = [l for l in lines[2:] if l.startswith("  component ")]
    assert len(rows) == 10 and lines[-1] == "  and 49 smaller components"
    top = re.fullmatch(r"  component (\d+): (\d+) polygons, area (\S+) \((\S+)%\), boundary edges (\d+), euler (-?\d+)"
                       r"(, volume \S+)?", rows[0])
    assert top and int(top.group(2)) == 2103
    for l in rows:  # a volume only for a closed, consistently oriented component
        c = topo.components[int(re.match(r"  component (\d+):", l).group(1))]
        closed = c["e_boundary"] == 0 and c["e_nonmanifold"] == 0 and c["e_misoriented"] == 0
        assert ("volume" in l) == bool(closed)
    big = load_polygon_ply(str(out / "our_poly_mesh_small_45_largest1.ply"))
    want = keep_components(load_polygon_ply(path), topo.labels, largest_components(topo.components, 1))
    assert np.array_equal(big.offsets, want.offsets) and np.array_equal(big.indices, want.indices)
    assert np.array_equal(big.vertices, want.vertices) and len(big) == 2103
    # visualize: one more image, the others byte for byte
    common = ["-d", "bunny", "--out", str(tmp_path / "meshes"), "--size", "160", "128", "--ssaa", "2"]
    assert vz.main(common + ["--png-dir", str(tmp_path / "a")]) == 0
    assert vz.main(common + ["--png-dir", str(tmp_path / "b"), "--color", "component"]) == 0
    a = sorted(p.name for p in (tmp_path / "a" / "bunny").iterdir())
    b = sorted(p.name for p in (tmp_path / "b" / "bunny").iterdir())
    assert a == ["small_ours.png"] and b == ["small_ours.png", "small_poly_components.png"]
    assert (tmp_path / "a" / "bunny" / "small_ours.png").read_bytes() == \
        (tmp_path / "b" / "bunny" / "small_ours.png").read_bytes()
    from tropical.utils.image import read_png
    img = read_png(str(tmp_path / "b" / "bunny" / "small_poly_components.png"))
    assert img.shape == (128, 160, 4) and (img[..., 3] > 0).any()
    assert len(np.unique(img[img[..., 3] == 255][:, :3], axis=0)) > 3  # several components, several colours
