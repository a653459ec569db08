"""GPU: tnp_simplify_* against its restatement (simplify_cases.simplify_ref) on
the synthetic soups and on the stored surfaces, bit for bit -- the map, the
position bytes, offsets, indices, source and every stat, max_shift by its bit
pattern -- then simplify() down the repair chain, train --simplify and the
training mesh's --mesh-cell."""
import re

import numpy as np
import pytest

from polygon_cases import FULL
from simplify_cases import DUPLICATES, MAX_CELLS, STAT_KEYS, grid_limit, reference, soups
from test_simplify_host import CELLS, INT_KEYS, TABLE
from test_weld_host import REPORT, surface

pytestmark = pytest.mark.gpu
SYMBOLS = ("tnp_simplify_create", "tnp_simplify_destroy", "tnp_simplify_build", "tnp_simplify_export",
           "tnp_debug_simplify_stages")


def _bits(x) -> int:
    return int(np.float32(x).view(np.uint32))


def _check(name, position="mean", data=None, cell=None, handle=None):
    """One build against the restatement, bitwise; returns the result."""
    from tropical.utils.simplify import cluster_vertices
    v, off, idx, h = soups()[name] if data is None else (*data, cell)
    v = np.asarray(v, np.float32)
    ref = reference(name, position, data, cell)
    res = cluster_vertices(v, off, idx, float(h), position, handle=handle)
    assert list(res.stats) == STAT_KEYS
    assert {k: res.stats[k] for k in INT_KEYS} == {k: ref["stats"][k] for k in INT_KEYS}, (name, res.stats, ref["stats"])
    for k, got in (("map", res.map), ("offsets", res.offsets), ("indices", res.indices), ("source", res.source)):
        assert got.dtype == np.int64 and np.array_equal(got, ref[k]), (name, position, k)
    assert res.positions.dtype == np.float32 and res.positions.shape == v.shape
    assert res.positions.tobytes() == ref["positions"].tobytes(), (name, position)
    assert _bits(res.stats["max_shift"]) == _bits(ref["stats"]["max_shift"]), (name, position, res.stats["max_shift"])
    return res


def test_the_abi_symbols_exist(cuda):
    from tropical import _hip
    lib = _hip.lib()
    for s in SYMBOLS:
        assert s in _hip.SIGNATURES and getattr(lib, s).argtypes == _hip.SIGNATURES[s][1], s
    assert [k for k, _ in _hip.TnpSimplifyStats._fields_] == STAT_KEYS


@pytest.mark.parametrize("name", list(soups()))
def test_synthetic_soup(cuda, name):
    from tropical.utils.mesh import polygon_report
    for position in ("mean", "nearest"):
        res = _check(name, position)
        if len(res):  # the output soup passes the soup checks
            r = polygon_report(res.positions, res.offsets, res.indices)
            assert (r["n_polygons"], r["n_indices"]) == (res.stats["n_polygons"], res.stats["n_indices"])
    st = res.stats
    if name in DUPLICATES:
        assert (st["n_polygons"], st["n_dropped_polygons"], st["n_duplicate_polygons"], st["n_folded"],
                st["n_pinched"]) == DUPLICATES[name][1]
    if name == "one_cell":
        assert (st["n_cells"], st["n_polygons"]) == (1, 0) and res.offsets.tolist() == [0]
    if name == "heavy":
        assert res.indices.tolist() == [0, 300, 500] and (st["max_cell"], st["n_duplicate_polygons"]) == (300, 57)
    if name == "same_1000":
        assert (st["n_polygons"], st["n_duplicate_polygons"]) == (1, 999)
    if name == "distinct_4096":
        assert (st["n_polygons"], st["n_duplicate_polygons"], st["n_folded"]) == (4096, 0, 0)
    if name == "cube_8_cells":
        r = polygon_report(res.positions, res.offsets, res.indices)
        assert (st["n_cells"], st["n_polygons"]) == (8, 6) and tuple(r[k] for k in REPORT) == (0, 0, 0, 2)
        assert st["n_dropped_polygons"] + st["n_duplicate_polygons"] == 90
    if name in ("no_polygons", "nothing"):
        assert st == dict.fromkeys(STAT_KEYS, 0) and res.offsets.tolist() == [0] and len(res.indices) == 0
    if name.startswith("grid_limit"):
        assert st["n_cells"] == 3 and res.map.tolist() == [0, 1, 2]


def test_weld_s_rewrite_cases(cuda):
    import weld_cases
    res, welds = _check("rewrite"), weld_cases.reference("rewrite")
    assert np.array_equal(res.offsets, welds["offsets"]) and np.array_equal(res.source, welds["source"])
    assert np.array_equal(res.indices, welds["indices"]) and np.array_equal(res.map, welds["map"])


def test_refusals(cuda):
    import ctypes as C

    import torch
    from tropical import _hip
    from tropical.utils.simplify import cluster_vertices, simplify_handle
    from topology_cases import CUBE_Q, CUBE_V, soup
    from weld_cases import bridge
    for axis in range(3):
        v, off, idx = grid_limit(axis, True)
        with pytest.raises(RuntimeError, match=rf"simplify: axis {'xyz'[axis]} needs {MAX_CELLS + 1} cells"):
            cluster_vertices(v, off, idx, 1.0)
    v, off, idx = bridge(used_nan=True)
    with pytest.raises(RuntimeError, match=r"simplify: vertex 4 has a coordinate that is not finite"):
        cluster_vertices(v, off, idx, 0.05)
    off, idx = soup(CUBE_Q)
    h = simplify_handle()
    try:
        lib, stream = _hip.lib(), C.c_void_p(_hip.stream_ptr(cuda))
        v, o, i = (torch.as_tensor(x, device=cuda) for x in (CUBE_V, off, idx))
        st = _hip.TnpSimplifyStats()
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            rc = lib.tnp_simplify_build(h.h, _hip.ptr(v), 8, _hip.ptr(o), _hip.ptr(i), 6, bad, 0, C.byref(st), stream)
            assert rc == -1 and b"simplify: cell = " in lib.tnp_last_error()
        for mode in (2, -1):
            rc = lib.tnp_simplify_build(h.h, _hip.ptr(v), 8, _hip.ptr(o), _hip.ptr(i), 6, 0.1, mode, C.byref(st), stream)
            assert rc == -1 and b"simplify: mode = " in lib.tnp_last_error()
        rc = lib.tnp_simplify_build(h.h, _hip.ptr(v), 1 << 31, _hip.ptr(o), _hip.ptr(i), 6, 0.1, 0, C.byref(st), stream)
        assert rc == -1 and b"below 2^31" in lib.tnp_last_error() and lib.tnp_last_error().startswith(b"simplify: ")
        rc = lib.tnp_simplify_build(None, _hip.ptr(v), 8, _hip.ptr(o), _hip.ptr(i), 6, 0.1, 0, C.byref(st), stream)
        assert rc == -1 and b"null handle" in lib.tnp_last_error()
    finally:
        h.close()
    bad = [
        (np.array([1, 4, 8, 12, 16, 20, 24]), idx, r"simplify: offsets\[0\] = 1, not 0"),
        (np.array([0, 4, 8, 6, 16, 20, 24]), idx,
         r"simplify: offsets decrease at polygon 2 \(offsets\[2\] = 8 > offsets\[3\] = 6\)"),
        (np.array([0, 4, 6, 12, 16, 20, 24]), idx, r"simplify: polygon 1 has 2 ids, fewer than 3"),
        (off, np.where(np.arange(24) == 5, 99, idx), r"simplify: indices\[5\] = 99 is outside \[0, 8\)"),
        (off, np.where(np.arange(24) == 9, idx[10], idx),
         r"simplify: indices\[9\] = 5 and the next id of its polygon are equal"),
        (off, np.where(np.arange(24) % 7 == 3, 1 << 40, idx), r"simplify: indices\[3\] = 1099511627776 is outside"),
    ]
    for o, i, msg in bad:
        with pytest.raises(RuntimeError, match=msg):
            cluster_vertices(CUBE_V, o, i, 0.1)
    # and the bad input cost nothing: a valid call still works
    res = cluster_vertices(CUBE_V, off, idx, 0.1)
    assert res.stats["n_cells"] == 8 and np.array_equal(res.indices, idx)


def test_two_builds_give_the_same_bits(cuda):
    from tropical.utils.simplify import simplify_handle
    h = simplify_handle()
    try:
        for name in ("heavy", "distinct_4096", "rewrite"):
            for position in ("mean", "nearest"):
                a, b = _check(name, position, handle=h), _check(name, position, handle=h)
                for k in ("map", "positions", "offsets", "indices", "source"):
                    assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), (name, k)
                assert a.stats == b.stats
        # a second build replaces the first
        _check("no_polygons", handle=h)
        _check("one_cell", handle=h)
        _check("same_1000", "nearest", handle=h)
    finally:
        h.close()


def test_stage_times(cuda):
    from tropical.utils.simplify import STAGES, cluster_vertices
    v, off, idx, cell = soups()["heavy"]
    res = cluster_vertices(v, off, idx, float(cell), "nearest", timed=True)
    assert list(res.stage_ms) == list(STAGES) and all(t >= 0 for t in res.stage_ms.values())
    assert sum(res.stage_ms.values()) > 0


@pytest.mark.parametrize("case", FULL)
def test_stored_surface(cuda, case):
    from tropical.utils.mesh import polygon_report
    data = surface(case)
    for cell in CELLS:
        for position in ("mean", "nearest"):
            res = _check(case, position, data, cell)
            assert tuple(res.stats[k] for k in INT_KEYS) == TABLE[case][cell][0]
            r = polygon_report(res.positions, res.offsets, res.indices)
            assert tuple(r[k] for k in REPORT) == TABLE[case][cell][1]


def test_simplify_a_polygon_mesh(cuda):
    from polygon_cases import fixture
    from tropical.utils.mesh import PolygonMesh, polygon_report
    from tropical.utils.simplify import simplify
    case, cell = "h8l3_sphere", 0.1
    v, off, idx = surface(case)
    pm = PolygonMesh(v, off, idx, fixture(case)["normals"])
    for position in ("mean", "nearest"):
        for compact in (True, False):
            out, st = simplify(pm, cell, position, compact=compact)
            r = polygon_report(out.vertices, out.offsets, out.indices)
            assert tuple(r[k] for k in REPORT) == TABLE[case][cell][1] == (0, 0, 0, 2)
            assert len(out.normals) == len(out) == st["n_polygons"] == TABLE[case][cell][0][3]
            assert len(out.vertices) == (r["n_vertices_used"] if compact else len(v))
            assert r["n_vertices_used"] <= st["n_cells"]  # (a class may lose all its polygons)


def test_the_training_mesh_is_clustered(cuda):
    """--mesh-cell: StanfordDataset.init clusters the normalised mesh (nearest, duplicates removed);
    without it the mesh goes through as it is."""
    from simplify_cases import int_cube
    from tropical.stanford.dataset import StanfordDataset
    from tropical.utils.mesh import Mesh
    from tropical.utils.simplify import cluster_triangles
    v, off, idx = int_cube(8)
    quads = idx.reshape(-1, 4)
    faces = np.concatenate([quads[:, [0, 1, 2]], quads[:, [0, 2, 3]]])

    def dataset(cell):
        d = StanfordDataset.__new__(StanfordDataset)
        d.R, d.name, d.device, d.mesh_cell = .8, "bunny", cuda, cell
        d.init(Mesh(v, faces))
        return d

    plain, coarse = dataset(None), dataset(0.5)
    norm = plain.vertices.numpy()
    assert norm.min() == -1 and norm.max() == 1 and np.array_equal(plain.faces.numpy(), faces)
    ref = reference("int_cube_8_triangles", "nearest", (norm, 3 * np.arange(len(faces) + 1), faces.reshape(-1)), 0.5)
    cv, cf, st = cluster_triangles(norm, faces, 0.5)
    assert st["n_polygons"] == ref["stats"]["n_polygons"] == len(cf) < len(faces) and st["n_cells"] == len(cv)
    assert np.array_equal(cv[cf.reshape(-1)], ref["positions"][ref["indices"]])
    assert np.array_equal(coarse.vertices.numpy(), cv) and np.array_equal(coarse.faces.numpy(), cf)
    assert coarse.V.shape == (len(cv), 3) and coarse.F.shape == (len(cf), 3)
    assert {tuple(p) for p in cv.tolist()} <= {tuple(p) for p in norm.tolist()}  # a subset of the input's vertices


def test_train_simplify_flag(cuda, tmp_path, capsys, monkeypatch):
    """train --weld --simplify on a fixture net's surface (the training is stood in for by the
    fixture's extraction): the _welded_simplified files and the line, behind the weld line and in front
    of the components."""
    import tropical.stanford.train as tr
    from test_gpu_polygons import run
    from tropical.utils.mesh import PolygonMesh, load_polygon_ply, polygon_report
    from tropical.utils.simplify import simplify
    from tropical.utils.weld import weld
    case, tol, cell = "h8l3_sphere", 1e-3 / tr.R, 0.1 / tr.R
    _, (faces, verts, fwi, pm) = run(case, cuda)
    monkeypatch.setattr(tr, "train_sdf", lambda net, args, path: (faces, verts, fwi, 0.0, pm))
    d = tmp_path / "out"
    assert tr.main(["-d", "bunny", "-c", "--keep-largest", "1", "--out", str(d), "--weld", repr(tol),
                    "--simplify", repr(cell), "--simplify-position", "nearest"]) == 0
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("Ours")]
    stem = "our_poly_mesh_small_45"
    assert sorted(p.name for p in (d / "bunny").iterdir()) == sorted(
        ["our_mesh_small_45.ply", f"{stem}.ply", f"{stem}_welded.ply", f"{stem}_welded_simplified.ply",
         f"{stem}_welded_simplified_largest1.ply"])
    kinds = [l.split(":")[0] for l in lines]
    assert kinds[:5] == ["Ours", "Ours (polygons)", "Ours (weld)", "Ours (simplify)", "Ours (components)"]
    g = re.fullmatch(r"Ours \(simplify\): cell (\S+) \(nearest\), (\d+) vertices -> (\d+) cells \(largest (\d+)\), "
                     r"polygons (\d+) -> (\d+) \((\d+) dropped, (\d+) duplicate, (\d+) folded, (\d+) pinched\), "
                     r"moved <= (\S+), boundary edges (\d+) -> (\d+), non-manifold (\d+) -> (\d+), "
                     r"misoriented (\d+) -> (\d+), Euler (-?\d+) -> (-?\d+)", lines[3])
    assert g, lines[3]
    before = PolygonMesh(verts.cpu().numpy() / tr.R, pm.offsets, pm.indices, pm.normals)
    welded, _ = weld(before, tol)
    want, st = simplify(welded, cell, "nearest")
    r0 = polygon_report(welded.vertices, welded.offsets, welded.indices)
    r1 = polygon_report(want.vertices, want.offsets, want.indices)
    assert float(g.group(1)) == pytest.approx(cell, rel=1e-5) and float(g.group(11)) == pytest.approx(st["max_shift"], rel=1e-2)
    assert [int(g.group(i)) for i in (2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 13, 14, 15, 16, 17, 18, 19)] == \
        [st["n_used"], st["n_cells"], st["max_cell"], len(welded), st["n_polygons"], st["n_dropped_polygons"],
         st["n_duplicate_polygons"], st["n_folded"], st["n_pinched"], r0["e_boundary"], r1["e_boundary"],
         r0["e_nonmanifold"], r1["e_nonmanifold"], r0["e_misoriented"], r1["e_misoriented"], r0["euler"], r1["euler"]]
    assert 0 < st["n_polygons"] < len(welded)
    got = load_polygon_ply(str(d / "bunny" / f"{stem}_welded_simplified.ply"))
    assert np.array_equal(got.offsets, want.offsets) and np.array_equal(got.indices, want.indices)
    assert np.array_equal(got.vertices, want.vertices.astype(np.float32).astype(np.float64))
    big = load_polygon_ply(str(d / "bunny" / f"{stem}_welded_simplified_largest1.ply"))
    assert 0 < len(big) <= len(got)
