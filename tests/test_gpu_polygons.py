"""GPU: the surface as polygons (tnp_engine_polygons) against the reference's
ordered rows (tests/golden/polygons.npz), and tnp_polygon_report against its
numpy restatement (polygon_cases.polygon_stats)."""
import re

import numpy as np
import pytest
import torch

from golden_io import golden_eps, load, sha
from helpers import product_net
from polygon_cases import ALL, FLAT, FULL, fan_t_major, fixture, polygon_stats

pytestmark = pytest.mark.gpu
INT_FIELDS = ["n_polygons", "n_indices", "max_degree", "n_vertices_used", "n_edges", "e_boundary", "e_manifold",
              "e_nonmanifold", "e_misoriented", "euler"]
_runs = {}


def run(case, cuda):
    """subpoly(..., polygons=True) of a fixture case, once per session."""
    if case not in _runs:
        import tropical.subpoly as sp
        d = load(case)
        net = product_net(d, cuda)
        _runs[case] = (d, sp.subpoly(net, 3, 1.2, golden_eps(d), force=str(d["kind"]) != "curve", polygons=True))
    return _runs[case]


@pytest.mark.parametrize("case", ALL)
def test_subpoly_polygons_are_the_reference_rows(cuda, case, capsys):
    d, (faces, verts, fwi, pm) = run(case, cuda)
    fx = fixture(case)
    # the three usual returns are untouched by polygons=True
    assert sha(verts.cpu().numpy()) == str(d["sha_surf"])
    assert sha(np.asarray(fwi, dtype=np.int64)) == str(d["sha_tri"])
    assert sha(np.asarray(faces, dtype=np.float32)) == str(d["sha_faces"])
    # the polygons: bitwise the rows the reference fans
    assert pm.offsets.dtype == np.int64 and pm.indices.dtype == np.int64
    assert (len(pm), len(pm.indices)) == (fx["stats"]["n_polygons"], fx["stats"]["n_indices"])
    assert int(pm.degrees().max()) == fx["stats"]["max_degree"] and int(pm.degrees().min()) >= 3
    assert sha(pm.offsets, pm.indices) == fx["sha"]
    assert sha(fan_t_major(pm.offsets, pm.indices)) == str(d["sha_tri"])
    assert np.array_equal(pm.vertices.astype(np.float32), verts.cpu().numpy())
    assert pm.normals.shape == (len(pm), 3)
    if case in FULL:
        assert np.array_equal(pm.offsets, fx["offsets"]) and np.array_equal(pm.indices, fx["indices"])
        # the bound of Net.normal against the reference (test_gpu_parity.py test_region_and_sdf)
        J_ref = fx["normals"]
        err, bound = np.abs(pm.normals - J_ref).max(), 1e-3 * max(1.0, float(np.abs(J_ref).max()))
        print(f"{case}: normals max err {err:.3g} (bound {bound:.3g})")
        assert err < bound
    if case in FLAT:
        # every polygon winds counter-clockwise about the normal that ordered it
        p = pm.vertices[pm.indices]
        nxt = np.arange(len(pm.indices)) + 1
        nxt[pm.offsets[1:] - 1] = pm.offsets[:-1]
        c = np.add.reduceat(p, pm.offsets[:-1], axis=0) / pm.degrees()[:, None]
        u = p - np.repeat(c, pm.degrees(), axis=0)
        N = 0.5 * np.add.reduceat(np.cross(u, u[nxt]), pm.offsets[:-1], axis=0)
        w = (N * pm.normals.astype(np.float64)).sum(1)
        print(f"{case}: Newell . normal > 0 for {(w > 0).sum()} of {len(w)}, min {w.min():.3g}")
        assert (w > 0).all()


def _tolerances(verts, off, idx):
    """What fp32 costs the header's formulas on these very inputs: the
    largest difference between their numpy restatement in float32 and in
    float64, x 4 for the order of the sums (the kernel adds a polygon's terms
    one by one, numpy's reduceat in its own order).  The total area differs
    by at most the sum of the per-polygon differences: P x that tolerance."""
    st64, a64, d64 = polygon_stats(verts, off, idx, np.float64)
    _, a32, d32 = polygon_stats(verts, off, idx, np.float32)
    tol_a = 4 * float(np.abs(a32.astype(np.float64) - a64).max())
    tol_d = 4 * float(np.abs(d32.astype(np.float64) - d64).max())
    return st64, a64, d64, tol_a, tol_d


def _check_report(verts, off, idx, want_int=None, label=""):
    from tropical.utils.mesh import polygon_report
    verts = np.asarray(verts, np.float32)
    st64, a64, d64, tol_a, tol_d = _tolerances(verts, off, idx)
    r = polygon_report(verts, off, idx, per_polygon=True)
    for k in INT_FIELDS:
        assert r[k] == st64[k], (k, r[k], st64[k])
        if want_int is not None:
            assert r[k] == want_int[k], (k, r[k], want_int[k])
    area, dev = r["polygon_area"].cpu().numpy().astype(np.float64), r["polygon_dev"].cpu().numpy().astype(np.float64)
    ea, ed = np.abs(area - a64).max(), np.abs(dev - d64).max()
    et, em = abs(r["area"] - st64["area"]), abs(r["max_dev"] - st64["max_dev"])
    print(f"{label}: area err {ea:.3g} (tol {tol_a:.3g}), dev err {ed:.3g} (tol {tol_d:.3g}), "
          f"total err {et:.3g} (tol {len(a64) * tol_a:.3g}), max_dev err {em:.3g}")
    assert ea <= tol_a and ed <= tol_d
    assert et <= len(a64) * tol_a and em <= tol_d
    # the total is reduced in a fixed order: the same bits on every call
    r2 = polygon_report(verts, off, idx)
    assert np.float64(r2["area"]).tobytes() == np.float64(r["area"]).tobytes()
    assert "polygon_area" not in r2 and r2["max_dev"] == r["max_dev"]
    return r


@pytest.mark.parametrize("case", ALL)
def test_polygon_report_on_the_fixture(cuda, case):
    fx = fixture(case)
    if case in FULL:
        verts, off, idx = load(case)["surf_V"], fx["offsets"], fx["indices"]
    else:  # stored as hashes: the engine's polygons, checked against them above
        _, (_, v, _, pm) = run(case, cuda)
        assert sha(pm.offsets, pm.indices) == fx["sha"]
        verts, off, idx = v.cpu().numpy(), pm.offsets, pm.indices
    r = _check_report(verts, off, idx, want_int=fx["stats"], label=case)
    if case == "small_sphere":
        assert (r["e_boundary"], r["e_nonmanifold"], r["euler"]) == (175, 42, -92)
    assert abs(r["area"] - fx["stats"]["area"]) <= 1e-5 * fx["stats"]["area"]


# ---- the lattice path, the row cache -----------------------------------------
def _lattice_engine(net, cuda):
    from tropical._engine import Engine
    eng = Engine(cuda).set_net(net)
    eng.lattice()
    eng.run_steps()
    eng.surface()
    return eng


@pytest.mark.parametrize("case", ["synth24", "synth16_h32l3"])
def test_lattice_polygons_and_the_row_cache(cuda, case):
    import tropical.subpoly as sp
    d = load(case)
    net = product_net(d, cuda)
    eng = sp.subpoly_lattice(net, faces=False)
    eng.surface()
    tri, fc = eng.faces()
    off, idx, nrm = eng.polygons()  # from the rows faces() left
    assert off.dtype == idx.dtype == torch.int64 and off.is_cuda and nrm.shape == (off.numel() - 1, 3)
    assert int(off[0]) == 0 and int(off[-1]) == idx.numel()
    assert sha(tri.cpu().numpy()) == str(d["sha_tri"])
    assert np.array_equal(fan_t_major(off.cpu().numpy(), idx.cpu().numpy()), tri.cpu().numpy())
    tri2, fc2 = eng.faces()  # and faces() after polygons() is unchanged
    assert torch.equal(tri, tri2) and torch.equal(fc, fc2)
    # polygons() first, on a fresh engine: it computes the rows itself
    eng2 = _lattice_engine(net, cuda)
    off2, idx2, nrm2 = eng2.polygons(host=True)
    assert not off2.is_cuda and off2.is_pinned()
    assert torch.equal(off2, off.cpu()) and torch.equal(idx2, idx.cpu()) and torch.equal(nrm2, nrm.cpu())
    tri3, _ = eng2.faces()
    assert torch.equal(tri3, tri)
    # another complex: the cached rows must not come back
    cube, pairs, _ = sp.get_hypercube(3, 0.35)
    eng2.load(cube, pairs)
    off3, idx3, _ = eng2.polygons()
    tri4, _ = eng2.faces()
    assert idx3.numel() != idx.numel()
    assert np.array_equal(fan_t_major(off3.cpu().numpy(), idx3.cpu().numpy()).reshape(-1, 3),
                          tri4.cpu().numpy().reshape(-1, 3))
    assert idx3.numel() == 0 or int(idx3.max()) < 8
    # an empty surface: no polygons, offsets [0]
    eng2.load(cube * 4.0, pairs)
    assert eng2.surface()[0] == 0
    off4, idx4, nrm4 = eng2.polygons()
    assert off4.tolist() == [0] and idx4.numel() == 0 and nrm4.shape == (0, 3)


def test_polygons_need_a_complex(cuda):
    from tropical._engine import Engine
    net = product_net(load("small_sphere"), cuda)
    with pytest.raises(RuntimeError, match="polygons: no consistent complex"):
        Engine(cuda).set_net(net).polygons()


def test_extract_polygons_is_extract_faces_unfanned(cuda):
    import tropical.subpoly as sp
    d, (_, verts, fwi, pm) = run("small_torus", cuda)
    net = product_net(d, cuda)
    edges = torch.tensor([[0, 1]], device=cuda)  # (the rows come from the vertices' regions alone)
    off, idx, nrm = sp.extract_polygons(verts, edges, net, eps=golden_eps(d))
    _, tri = sp.extract_faces(verts, edges, net, eps=golden_eps(d))
    assert len(off) > 1000 and nrm.shape == (len(off) - 1, 3) and off[-1] == len(idx)
    assert np.array_equal(fan_t_major(off, idx), tri)


# ---- hand-made soups ------------------------------------------------------------
CUBE_V = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], dtype=np.float32)  # id = 4x + 2y + z
CUBE_Q = [[0, 1, 3, 2], [4, 6, 7, 5], [0, 4, 5, 1], [2, 3, 7, 6], [0, 2, 6, 4], [1, 5, 7, 3]]  # outward


def _soup(polys):
    deg = [len(p) for p in polys]
    return np.concatenate([[0], np.cumsum(deg)]).astype(np.int64), np.concatenate(polys).astype(np.int64)


def test_report_cube(cuda):
    s = 1.5
    off, idx = _soup(CUBE_Q)
    r = _check_report(CUBE_V * s, off, idx, label="cube")
    assert (r["n_edges"], r["e_manifold"], r["e_boundary"], r["e_nonmanifold"], r["e_misoriented"]) == (12, 12, 0, 0, 0)
    assert (r["euler"], r["n_vertices_used"], r["max_degree"], r["max_dev"]) == (2, 8, 4, 0.0)
    assert r["area"] == 6 * s * s
    # one quad reversed: its four edges are now walked the same way from both sides
    off, idx = _soup([CUBE_Q[0][::-1]] + CUBE_Q[1:])
    r = _check_report(CUBE_V * s, off, idx, label="cube, one quad reversed")
    assert (r["e_misoriented"], r["e_manifold"], r["euler"]) == (4, 12, 2)
    # open: five quads
    off, idx = _soup(CUBE_Q[:5])
    r = _check_report(CUBE_V * s, off, idx, label="open cube")
    assert (r["e_boundary"], r["e_manifold"], r["n_edges"], r["euler"], r["e_misoriented"]) == (4, 8, 12, 1, 0)


def test_report_three_quads_on_one_edge(cuda):
    v = np.array([[0, 0, 0], [0, 0, 1], [1, 0, 0], [1, 0, 1], [0, 1, 0], [0, 1, 1], [-1, -1, 0], [-1, -1, 1]],
                 dtype=np.float32)
    off, idx = _soup([[0, 1, 3, 2], [0, 1, 5, 4], [0, 1, 7, 6]])
    r = _check_report(v, off, idx, label="fin")
    assert (r["e_nonmanifold"], r["e_boundary"], r["e_manifold"], r["n_edges"], r["e_misoriented"]) == (1, 9, 0, 10, 0)


def test_report_200_gons(cuda):
    """Degree above a wave: regular 200-gons in tilted planes (several, so the
    measured fp32 tolerance is the largest of a few and not one draw)."""
    rng = np.random.default_rng(5)
    a = np.linspace(0, 2 * np.pi, 200, endpoint=False)
    vs, polys = [], []
    for k in range(6):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        ring = np.stack([np.cos(a), np.sin(a), 0 * a], 1) * (0.3 + 0.2 * k)
        vs.append(ring @ q.T + rng.uniform(-1, 1, 3))
        polys.append(np.arange(200) + 200 * k)
    off, idx = _soup(polys)
    r = _check_report(np.concatenate(vs), off, idx, label="200-gons")
    assert (r["max_degree"], r["n_edges"], r["e_boundary"], r["n_vertices_used"]) == (200, 1200, 1200, 1200)
    want = sum(0.5 * 200 * np.sin(2 * np.pi / 200) * (0.3 + 0.2 * k) ** 2 for k in range(6))
    assert abs(r["area"] - want) < 1e-4 * want


def test_report_600_triangles_and_high_ids(cuda):
    rng = np.random.default_rng(6)
    v = rng.uniform(-1, 1, (1800, 3)).astype(np.float32)
    off, idx = _soup([[3 * t, 3 * t + 1, 3 * t + 2] for t in range(600)])  # polygons across workgroups
    r = _check_report(v, off, idx, label="600 triangles")
    assert (r["n_polygons"], r["n_edges"], r["e_boundary"], r["euler"]) == (600, 1800, 1800, 600)
    # a strip at the top of 70,000 vertices: ids past 16 bits, most vertices unused
    V = 70_000
    v = rng.uniform(-1, 1, (V, 3)).astype(np.float32)
    strip = [[V - 1 - t, V - 2 - t, V - 3 - t] if t % 2 == 0 else [V - 1 - t, V - 3 - t, V - 2 - t] for t in range(40)]
    off, idx = _soup(strip)
    r = _check_report(v, off, idx, label="strip")
    assert (r["n_vertices_used"], r["n_edges"], r["e_manifold"], r["e_boundary"], r["e_misoriented"]) == \
        (42, 81, 39, 42, 0)


def test_report_no_polygons(cuda):
    from tropical.utils.mesh import polygon_report
    r = polygon_report(np.zeros((5, 3), np.float32), np.zeros(1, np.int64), np.zeros(0, np.int64), per_polygon=True)
    assert all(r[k] == 0 for k in INT_FIELDS) and r["area"] == 0.0 and r["max_dev"] == 0.0
    assert r["polygon_area"].shape == (0,)


def test_report_refuses_malformed_input(cuda):
    import ctypes as C

    from tropical import _hip
    from tropical.utils.mesh import polygon_report
    off, idx = _soup(CUBE_Q)
    bad = [
        (np.array([1, 4, 8, 12, 16, 20, 24]), idx, r"offsets\[0\] = 1, not 0"),
        (np.array([0, 4, 8, 6, 16, 20, 24]), idx, r"offsets decrease at polygon 2 \(offsets\[2\] = 8 > offsets\[3\] = 6\)"),
        (np.array([0, 4, 6, 12, 16, 20, 24]), idx, r"polygon 1 has 2 ids, fewer than 3"),
        (off, np.where(np.arange(24) == 5, 99, idx), r"indices\[5\] = 99 is outside \[0, 8\)"),
        (off, np.where(np.arange(24) == 17, -2, idx), r"indices\[17\] = -2 is outside \[0, 8\)"),
        (off, np.where(np.arange(24) == 9, idx[10], idx), r"indices\[9\] = 5 and the next id of its polygon are equal"),
        # cyclic: the last id of polygon 3 equals its first
        (off, np.where(np.arange(24) == 15, idx[12], idx), r"indices\[15\] = 2 and the next id"),
        # the first offender is named when there are several
        (off, np.where(np.arange(24) % 7 == 3, 1 << 40, idx), r"indices\[3\] = 1099511627776 is outside"),
    ]
    for o, i, msg in bad:
        with pytest.raises(RuntimeError, match=msg):
            polygon_report(CUBE_V, o, i, per_polygon=True)
    st = _hip.TnpPolygonStats()
    o = torch.tensor([0, 3], device=cuda)
    rc = _hip.lib().tnp_polygon_report(None, 1 << 31, _hip.ptr(o), _hip.ptr(o), 1, C.byref(st), None, None,
                                       C.c_void_p(_hip.stream_ptr(cuda)))
    assert rc == -1 and b"below 2^31" in _hip.lib().tnp_last_error()
    # and the bad input cost nothing: a valid call still works
    r = polygon_report(CUBE_V, off, idx)
    assert (r["n_edges"], r["e_manifold"], r["euler"], r["area"]) == (12, 12, 2, 6.0)


# ---- train -e --polygons ----------------------------------------------------------
def test_train_cli_writes_and_reports_polygons(cuda, tmp_path, capsys, monkeypatch):
    """`train -c --mesh sphere.ply -e --polygons`.  Four epochs, as
    test_train_entry_point_fits_a_sphere: after one epoch the net has no zero
    set inside the canvas yet (0 faces), and `-e` cannot sample an empty mesh."""
    import tropical.stanford.train as tr
    from test_train import icosphere
    from tropical.utils.mesh import Mesh, load_ply, load_polygon_ply
    V, F = icosphere(4, r=0.37)
    Mesh(V, F).export(str(tmp_path / "sphere.ply"))
    monkeypatch.setattr(tr, "MC_SIZES", [64])
    assert tr.main(["-d", "bunny", "-c", "--mesh", str(tmp_path / "sphere.ply"), "--epochs", "4", "-e", "--polygons",
                    "--out", str(tmp_path / "meshes")]) == 0
    out = capsys.readouterr().out
    pm = load_polygon_ply(str(tmp_path / "meshes" / "bunny" / "our_poly_mesh_small_45.ply"))
    m = load_ply(str(tmp_path / "meshes" / "bunny" / "our_mesh_small_45.ply"), process=False)
    assert len(pm) > 0 and np.array_equal(fan_t_major(pm.offsets, pm.indices), m.faces)
    assert np.array_equal(pm.vertices, m.vertices)
    line = [l for l in out.splitlines() if l.startswith("Ours (polygons): ")]
    assert len(line) == 1
    g = re.fullmatch(r"Ours \(polygons\): (\d+) faces, mean degree (\d+\.\d\d), edges (\d+) \(boundary (\d+), "
                     r"non-manifold (\d+), misoriented (\d+)\), euler (-?\d+), max planarity dev (\S+)", line[0])
    assert g, line[0]
    st, _, _ = polygon_stats(pm.vertices.astype(np.float32), pm.offsets, pm.indices)
    assert [int(g.group(i)) for i in (1, 3, 4, 5, 6, 7)] == \
        [st[k] for k in ("n_polygons", "n_edges", "e_boundary", "e_nonmanifold", "e_misoriented", "euler")]
    assert g.group(2) == f"{len(pm.indices) / len(pm):.2f}" and float(g.group(8)) >= 0
    assert "Ours: " in out and "#samples, #vertices, CD, AD, time" in out
