"""GPU: tnp_weld_* against its restatement (weld_cases.weld_ref) on the
synthetic soups and on the stored surfaces -- maps, polygons and counts as
integers, mode-0 positions and max_shift bit for bit, mode-1 means within the
double sum's bound -- then weld() down the repair chain and train --weld."""
import math
import re

import numpy as np
import pytest

from polygon_cases import FULL
from test_weld_host import REPORT, TABLE, TOLS, surface
from weld_cases import CUBE_Q, STAT_KEYS, max_shift_of, reference, soups

pytestmark = pytest.mark.gpu
INT_KEYS = STAT_KEYS[:-1]


def _bits(x) -> int:
    return int(np.float32(x).view(np.uint32))


def _check(name, position="first", data=None, tol=None, handle=None):
    """One build against the restatement; returns the result."""
    from tropical.utils.weld import weld_vertices
    v, off, idx, t = soups()[name] if data is None else (*data, tol)
    v = np.asarray(v, np.float32)
    ref = reference(name, position, data, tol)
    res = weld_vertices(v, off, idx, t, position, handle=handle)
    assert list(res.stats) == STAT_KEYS
    assert {k: res.stats[k] for k in INT_KEYS} == {k: ref["stats"][k] for k in INT_KEYS}, (name, res.stats, ref["stats"])
    for k, got in (("map", res.map), ("offsets", res.offsets), ("indices", res.indices), ("source", res.source)):
        assert got.dtype == np.int64 and np.array_equal(got, ref[k]), (name, k)
    assert res.positions.dtype == np.float32 and res.positions.shape == v.shape
    if position == "first":
        assert res.positions.tobytes() == ref["positions"].tobytes(), name
        assert _bits(res.stats["max_shift"]) == _bits(ref["stats"]["max_shift"]), (name, res.stats["max_shift"])
        return res
    single = np.ones(len(v), bool)
    worst = 0.0
    for mem in ref["clusters"]:
        single[mem] = False
        m, p = len(mem), v[mem].astype(np.float64)
        assert (res.positions[mem].view(np.uint32) == res.positions[mem[0]].view(np.uint32)).all()
        for q in range(3):
            want = math.fsum(p[:, q]) / m
            err = abs(float(res.positions[mem[0], q]) - want)
            bound = float(np.spacing(np.float32(abs(want)))) + m * 2.0 ** -52 * float(np.abs(p[:, q]).max())
            worst = max(worst, err / bound)
            assert err <= bound, (name, mem[0], q, err, bound)
    assert res.positions[single].tobytes() == v[single].tobytes(), name
    assert _bits(res.stats["max_shift"]) == _bits(max_shift_of(v, res.positions, idx[:off[-1]])), name
    print(f"{name}/{position}: {len(ref['clusters'])} clusters, largest error / bound {worst:.3g}")
    return res


def test_distance_exactly_tol_is_close(cuda):
    at = _check("lattice_at_tol")
    assert (at.stats["n_pairs"], at.stats["max_cluster"]) == (54, 27) and (at.map == 0).all()
    below = _check("lattice_below_tol")
    assert (below.stats["n_pairs"], below.stats["n_merged"], below.stats["n_polygons"]) == (0, 0, 9)


def test_pairs_across_cell_borders(cuda):
    near, far = _check("borders_0.9"), _check("borders_1.1")
    n = len(near.map) // 2
    assert n == 30 and (near.stats["n_pairs"], near.stats["n_clusters"], near.stats["max_cluster"]) == (n, n, 2)
    assert np.array_equal(near.map, np.arange(2 * n) // 2 * 2)
    assert (far.stats["n_pairs"], far.stats["n_merged"]) == (0, 0) and np.array_equal(far.map, np.arange(2 * n))


@pytest.mark.parametrize("name,n", [("chain_1000", 1000), ("chain_257", 257)])
def test_a_chain_is_one_cluster(cuda, name, n):
    for position in ("first", "mean"):
        res = _check(name, position)
        assert (res.map == 0).all() and (res.stats["n_clusters"], res.stats["max_cluster"]) == (1, n)
        assert res.stats["n_pairs"] == n - 1 and res.stats["n_polygons"] == 0 and res.offsets.tolist() == [0]


def test_300_points_in_one_cell(cuda):
    for position in ("first", "mean"):
        res = _check("ball_300", position)
        assert (res.stats["n_pairs"], res.stats["max_cluster"], res.stats["n_merged"]) == (44850, 300, 299)


def test_unused_vertices_take_no_part(cuda):
    from tropical.utils.weld import weld_vertices
    from weld_cases import BRIDGE_TOL, bridge
    for name in ("bridge", "bridge_unused_nan"):
        for position in ("first", "mean"):
            res = _check(name, position)
            assert np.array_equal(res.map, np.arange(7)) and res.stats["n_used"] == 5
    v, off, idx = bridge(used_nan=True)
    with pytest.raises(RuntimeError, match=r"weld: vertex 4 has a coordinate that is not finite"):
        weld_vertices(v, off, idx, BRIDGE_TOL)


def test_tol_zero_welds_the_split_cube(cuda):
    from tropical.utils.mesh import PolygonMesh, polygon_report
    from tropical.utils.topology import polygon_topology
    from tropical.utils.weld import weld
    res = _check("split_cube")
    assert len(np.unique(res.map)) == 8 and res.stats["max_shift"] == 0.0
    v, off, idx, _ = soups()["split_cube"]
    welded, st = weld(PolygonMesh(v, off, idx), 0.0)
    assert len(welded.vertices) == 8 and len(welded) == 6 and st["n_merged"] == 16
    r = polygon_report(welded.vertices, welded.offsets, welded.indices)
    assert tuple(r[k] for k in REPORT) == (0, 0, 0, 2)
    topo = polygon_topology(welded.vertices, welded.offsets, welded.indices)
    assert topo.n_components == 1 and topo.n_loops == 0
    assert topo.components["volume"][0] > 0 and topo.components["volume"][0] == pytest.approx(1.0)
    assert len(CUBE_Q) == 6


def test_polygon_rewriting(cuda):
    for position in ("first", "mean"):
        res = _check("rewrite", position)
        assert res.source.tolist() == [0, 2, 4, 5, 6, 8] and np.diff(res.offsets).tolist() == [3, 3, 4, 3, 257, 4]
        assert (res.stats["n_dropped_polygons"], res.stats["n_pinched"]) == (3, 1)


@pytest.mark.parametrize("name", ["no_polygons", "nothing", "identical", "identical_tol", "far_box", "random_8192"])
def test_extremes(cuda, name):
    for position in ("first", "mean"):
        res = _check(name, position)
    if name in ("no_polygons", "nothing"):
        assert res.stats == dict.fromkeys(STAT_KEYS, 0) and res.offsets.tolist() == [0] and len(res.indices) == 0
    if name == "far_box":
        assert (res.stats["n_pairs"], res.stats["n_clusters"]) == (300, 300)
    if name == "random_8192":
        assert 200 <= res.stats["n_clusters"] <= 400


def test_two_builds_give_the_same_bits(cuda):
    from tropical.utils.weld import weld_handle
    h = weld_handle()
    try:
        for name in ("random_8192", "ball_300", "rewrite"):
            a, b = _check(name, "mean", handle=h), _check(name, "mean", handle=h)
            for k in ("map", "positions", "offsets", "indices", "source"):
                assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), (name, k)
            assert a.stats == b.stats
        # a second build replaces the first
        _check("no_polygons", handle=h)
        _check("chain_257", handle=h)
        _check("far_box", "mean", handle=h)
    finally:
        h.close()


def test_stage_times(cuda):
    from tropical.utils.weld import STAGES, weld_vertices
    v, off, idx, tol = soups()["random_8192"]
    res = weld_vertices(v, off, idx, tol, "mean", timed=True)
    assert list(res.stage_ms) == list(STAGES) and all(t >= 0 for t in res.stage_ms.values())
    assert sum(res.stage_ms.values()) > 0


def test_refusals(cuda):
    import ctypes as C

    import torch
    from tropical import _hip
    from tropical.utils.weld import weld_handle, weld_vertices
    from topology_cases import CUBE_V, soup
    off, idx = soup(CUBE_Q)
    for bad in (-1e-3, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(RuntimeError, match=r"weld: tol = \S+ \(finite, >= 0\)"):
            weld_vertices(CUBE_V, off, idx, bad)
    h = weld_handle()
    try:
        lib, stream = _hip.lib(), C.c_void_p(_hip.stream_ptr(cuda))
        v, o, i = (torch.as_tensor(x, device=cuda) for x in (CUBE_V, off, idx))
        st = _hip.TnpWeldStats()
        rc = lib.tnp_weld_build(h.h, _hip.ptr(v), 8, _hip.ptr(o), _hip.ptr(i), 6, 0.1, 2, C.byref(st), stream)
        assert rc == -1 and b"weld: mode = 2" in lib.tnp_last_error()
        rc = lib.tnp_weld_build(h.h, _hip.ptr(v), 1 << 31, _hip.ptr(o), _hip.ptr(i), 6, 0.1, 0, C.byref(st), stream)
        assert rc == -1 and b"below 2^31" in lib.tnp_last_error() and lib.tnp_last_error().startswith(b"weld: ")
        rc = lib.tnp_weld_build(None, _hip.ptr(v), 8, _hip.ptr(o), _hip.ptr(i), 6, 0.1, 0, C.byref(st), stream)
        assert rc == -1 and b"null handle" in lib.tnp_last_error()
    finally:
        h.close()
    bad = [
        (np.array([1, 4, 8, 12, 16, 20, 24]), idx, r"weld: offsets\[0\] = 1, not 0"),
        (np.array([0, 4, 8, 6, 16, 20, 24]), idx,
         r"weld: offsets decrease at polygon 2 \(offsets\[2\] = 8 > offsets\[3\] = 6\)"),
        (np.array([0, 4, 6, 12, 16, 20, 24]), idx, r"weld: polygon 1 has 2 ids, fewer than 3"),
        (off, np.where(np.arange(24) == 5, 99, idx), r"weld: indices\[5\] = 99 is outside \[0, 8\)"),
        (off, np.where(np.arange(24) == 17, -2, idx), r"weld: indices\[17\] = -2 is outside \[0, 8\)"),
        (off, np.where(np.arange(24) == 9, idx[10], idx),
         r"weld: indices\[9\] = 5 and the next id of its polygon are equal"),
        (off, np.where(np.arange(24) == 15, idx[12], idx), r"weld: indices\[15\] = 2 and the next id"),
        (off, np.where(np.arange(24) % 7 == 3, 1 << 40, idx), r"weld: indices\[3\] = 1099511627776 is outside"),
    ]
    for o, i, msg in bad:
        with pytest.raises(RuntimeError, match=msg):
            weld_vertices(CUBE_V, o, i, 0.1)
    # and the bad input cost nothing: a valid call still works
    res = weld_vertices(CUBE_V, off, idx, 0.1)
    assert res.stats["n_merged"] == 0 and np.array_equal(res.indices, idx)


@pytest.mark.parametrize("case", FULL)
def test_stored_surface(cuda, case):
    data = surface(case)
    for tol in TOLS + (0.0,):
        for position in ("first", "mean"):
            res = _check(case, position, data, tol)
            if tol:
                assert tuple(res.stats[k] for k in INT_KEYS) == TABLE[case][tol][0]
            else:
                assert np.array_equal(res.map, np.arange(len(data[0]))) and res.positions.tobytes() == data[0].tobytes()
                assert np.array_equal(res.indices, data[2]) and res.stats["n_merged"] == 0


@pytest.mark.parametrize("case,tol,want", [("h8l3_sphere", 1e-3, (0, 0, 0, 2)), ("small_torus", 2e-3, (0, 0, 0, 0))])
def test_welding_closes_the_fitted_surface(cuda, case, tol, want):
    from polygon_cases import fixture
    from tropical.utils.mesh import PolygonMesh, polygon_report
    from tropical.utils.topology import polygon_topology
    from tropical.utils.weld import weld
    v, off, idx = surface(case)
    pm = PolygonMesh(v, off, idx, fixture(case)["normals"])
    for position in ("first", "mean"):
        for compact in (True, False):
            welded, st = weld(pm, tol, position, compact=compact)
            r = polygon_report(welded.vertices, welded.offsets, welded.indices)
            assert tuple(r[k] for k in REPORT) == want, (position, compact)
            assert len(welded.normals) == len(welded) == st["n_polygons"] == TABLE[case][tol][0][5]
            assert len(welded.vertices) == (r["n_vertices_used"] if compact else len(v))
            assert r["n_vertices_used"] <= st["n_used"] - st["n_merged"]  # (a class may lose all its polygons)
    topo = polygon_topology(welded.vertices, welded.offsets, welded.indices)
    closed = topo.components[topo.components["e_boundary"] == 0]
    assert topo.n_loops == 0 and len(closed) == topo.n_components and abs(closed["volume"]).max() > 0


def test_weld_then_keep_then_fill(cuda):
    from polygon_cases import fixture
    from tropical.utils.mesh import PolygonMesh, polygon_report
    from tropical.utils.topology import fill_holes, keep_components, largest_components, polygon_topology
    from tropical.utils.weld import weld
    v, off, idx = surface("small_sphere")
    welded, st = weld(PolygonMesh(v, off, idx, fixture("small_sphere")["normals"]), 1e-3)
    assert tuple(st[k] for k in INT_KEYS) == TABLE["small_sphere"][1e-3][0]
    topo = polygon_topology(welded.vertices, welded.offsets, welded.indices)
    main = keep_components(welded, topo.labels, largest_components(topo.components, 1))
    filled, fst = fill_holes(main, max_edges=6)
    r0 = polygon_report(main.vertices, main.offsets, main.indices)
    r1 = polygon_report(filled.vertices, filled.offsets, filled.indices)  # (the soup front accepts it)
    assert r1["e_boundary"] == r0["e_boundary"] - fst["n_cycle_indices"] and len(filled) == len(main) + fst["n_capped"]
    assert len(filled.normals) == len(filled) and r0["e_boundary"] <= TABLE["small_sphere"][1e-3][1][0]


def test_train_weld_flag(cuda, tmp_path, capsys, monkeypatch):
    """train --weld on a fixture net's surface (the training is stood in for by
    the fixture's extraction): the _welded files and the line; without the flag
    the run writes what it wrote before."""
    import tropical.stanford.train as tr
    from golden_io import sha
    from polygon_cases import fixture
    from test_gpu_polygons import run
    from tropical.utils.mesh import PolygonMesh, load_polygon_ply, polygon_report
    from tropical.utils.weld import weld
    case, tol = "h8l3_sphere", 1e-3 / tr.R
    _, (faces, verts, fwi, pm) = run(case, cuda)
    monkeypatch.setattr(tr, "train_sdf", lambda net, args, path: (faces, verts, fwi, 0.0, pm))

    def outputs(d, extra):
        capsys.readouterr()
        assert tr.main(["-d", "bunny", "-c", "--keep-largest", "1", "--fill-holes", "6", "--out", str(d)] + extra) == 0
        lines = capsys.readouterr().out.splitlines()
        return [l for l in lines if l.startswith(("Ours", "  "))], sorted(p.name for p in (d / "bunny").iterdir())

    plain, plain_files = outputs(tmp_path / "a", [])
    lines, files = outputs(tmp_path / "b", ["--weld", repr(tol)])
    stem = "our_poly_mesh_small_45"
    assert plain_files == ["our_mesh_small_45.ply", f"{stem}.ply", f"{stem}_largest1.ply", f"{stem}_largest1_filled.ply"]
    assert files == sorted(["our_mesh_small_45.ply", f"{stem}.ply", f"{stem}_welded.ply", f"{stem}_welded_largest1.ply",
                            f"{stem}_welded_largest1_filled.ply"])
    for f in ("our_mesh_small_45.ply", f"{stem}.ply"):
        assert (tmp_path / "a" / "bunny" / f).read_bytes() == (tmp_path / "b" / "bunny" / f).read_bytes(), f
    poly = load_polygon_ply(str(tmp_path / "a" / "bunny" / f"{stem}.ply"))
    assert sha(poly.offsets, poly.indices) == fixture(case)["sha"]
    assert not any("weld" in l for l in plain) and plain[:2] == lines[:2]  # "Ours: ...", "Ours (polygons): ..."
    line = [l for l in lines if l.startswith("Ours (weld): ")]
    assert len(line) == 1 and lines.index(line[0]) == 2
    g = re.fullmatch(r"Ours \(weld\): tol (\S+), (\d+) of (\d+) vertices merged into (\d+) clusters \(largest (\d+), "
                     r"moved <= (\S+)\), (\d+) polygons dropped, boundary edges (\d+) -> (\d+), "
                     r"non-manifold (\d+) -> (\d+), Euler (-?\d+) -> (-?\d+)", line[0])
    assert g, line[0]
    before = PolygonMesh(verts.cpu().numpy() / tr.R, pm.offsets, pm.indices, pm.normals)
    want, st = weld(before, tol)
    r0 = polygon_report(before.vertices, before.offsets, before.indices)
    r1 = polygon_report(want.vertices, want.offsets, want.indices)
    assert float(g.group(1)) == pytest.approx(tol, rel=1e-5) and float(g.group(6)) == pytest.approx(st["max_shift"], rel=1e-2)
    assert [int(g.group(i)) for i in (2, 3, 4, 5, 7, 8, 9, 10, 11, 12, 13)] == \
        [st["n_merged"], st["n_used"], st["n_clusters"], st["max_cluster"], st["n_dropped_polygons"],
         r0["e_boundary"], r1["e_boundary"], r0["e_nonmanifold"], r1["e_nonmanifold"], r0["euler"], r1["euler"]]
    assert st["n_merged"] > 0 and r1["e_boundary"] < r0["e_boundary"]
    got = load_polygon_ply(str(tmp_path / "b" / "bunny" / f"{stem}_welded.ply"))
    assert np.array_equal(got.offsets, want.offsets) and np.array_equal(got.indices, want.indices)
    assert np.array_equal(got.vertices, want.vertices.astype(np.float32).astype(np.float64))
    # the later stages ran on the welded surface
    comp = [l for l in lines if l.startswith("Ours (components): ")]
    holes = [l for l in lines if l.startswith("Ours (holes): ")]
    assert len(comp) == 1 and len(holes) == 1 and lines.index(comp[0]) == 3
    big = load_polygon_ply(str(tmp_path / "b" / "bunny" / f"{stem}_welded_largest1.ply"))
    assert len(big) <= len(got) and f"boundary edges {polygon_report(big.vertices, big.offsets, big.indices)['e_boundary']} ->" in holes[0]
