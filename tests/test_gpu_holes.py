"""GPU: tnp_holes_* (ordered boundary cycles and the caps that close them)
against its restatement (holes_cases.holes_ref / caps_ref) on the synthetic
soups and on the extracted surfaces; fill_holes; train --fill-holes."""
import math
import re

import numpy as np
import pytest

from holes_cases import STAT_KEYS, caps_ref, reference, soups
from test_gpu_topology import SOUPS
from test_holes_host import TABLE

pytestmark = pytest.mark.gpu
EXTRA = ["ngons", "punched_grid", "flipped_cylinder"]


def _check(name, max_edges=0, data=None, handle=None, coords=True):
    """One build and both cap modes against the restatement, as integers; the
    star centres within the double sum's bound plus one fp32 rounding."""
    from tropical.utils.topology import boundary_cycles, cycle_caps, holes_handle
    v, off, idx = soups()[name] if data is None else data
    v = np.asarray(v, np.float32)
    ref = reference(name, max_edges, data)
    h = holes_handle() if handle is None else handle
    try:
        cyc = boundary_cycles(v if coords else len(v), off, idx, max_edges=max_edges, handle=h)
        assert cyc.status.dtype == np.int32 and cyc.vertices.dtype == np.int64
        assert cyc.stats == ref["stats"], (name, cyc.stats, ref["stats"])
        assert list(cyc.stats) == STAT_KEYS
        for k, got in (("status", cyc.status), ("cycle_loop", cyc.cycle_loop), ("offsets", cyc.offsets),
                       ("vertices", cyc.vertices)):
            assert np.array_equal(got, ref[k]), (name, k)
        poff, pidx, pnew = cycle_caps(h, cyc, "polygon")
        roff, ridx, _ = caps_ref(ref, "polygon", len(v))
        assert np.array_equal(poff, roff) and np.array_equal(pidx, ridx) and len(pnew) == 0
        soff, sidx, snew = cycle_caps(h, cyc, "star", v)
        roff, ridx, rnew = caps_ref(ref, "star", len(v), v)
        assert np.array_equal(soff, roff) and np.array_equal(sidx, ridx) and snew.shape == rnew.shape
    finally:
        if handle is None:
            h.close()
    worst, s = 0.0, 0
    for k in range(len(cyc.offsets) - 1):
        c = cyc.vertices[cyc.offsets[k]:cyc.offsets[k + 1]]
        m = len(c)
        if m < 4:
            continue
        p = v[c].astype(np.float64)
        for q in range(3):
            want = math.fsum(p[:, q]) / m
            err = abs(float(snew[s, q]) - want)
            bound = float(np.spacing(np.float32(abs(want)))) + m * 2.0 ** -52 * float(np.abs(p[:, q]).max())
            worst = max(worst, err / bound)
            assert err <= bound, (name, k, q, err, bound)
        s += 1
    assert s == len(snew)
    print(f"{name}/{max_edges}: {len(cyc)} cycles, {s} star centres, largest error / bound {worst:.3g}")
    return cyc, snew


@pytest.mark.parametrize("name", SOUPS + EXTRA)
def test_soup_against_the_restatement(cuda, name):
    from tropical.utils.topology import polygon_topology
    cyc, _ = _check(name)
    v, off, idx = soups()[name]
    loops = polygon_topology(v, off, idx).loops
    ref = reference(name)
    assert len(loops) == len(cyc.status)
    for k in ("first_vertex", "n_edges", "simple"):
        assert np.array_equal(loops[k], ref[k]), (name, k)
    assert np.array_equal(cyc.vertices[cyc.offsets[:-1]], loops["first_vertex"][cyc.cycle_loop])
    assert np.array_equal(np.diff(cyc.offsets), loops["n_edges"][cyc.cycle_loop])
    st = cyc.stats
    if name == "moebius":
        assert (st["n_loops"], st["n_unoriented"], st["n_capped"]) == (1, 1, 0)
    if name in ("two_fans", "book_1000"):
        assert (st["n_loops"], st["n_nonsimple"], st["n_capped"]) == (1, 1, 0)
    if name == "strip_4096_vperm":
        assert np.diff(cyc.offsets).tolist() == [8194] and st["longest_capped"] == 8194
    if name == "isolated_1000":
        assert (st["n_capped"], st["n_triangles"], st["n_cycle_indices"]) == (1000, 1000, 3000)
    if name in ("empty", "torus", "cube", "cube_reversed", "two_tets"):
        assert st["n_loops"] == 0 and len(cyc) == 0 and cyc.offsets.tolist() == [0] and len(cyc.vertices) == 0
    if name == "flipped_cylinder":
        assert cyc.status.tolist() == [2, 0]


def _surface(case, cuda):
    from test_gpu_polygons import run
    _, (_, verts, _, pm) = run(case, cuda)
    return verts.cpu().numpy(), pm


@pytest.mark.parametrize("case", list(TABLE))
def test_extracted_surface(cuda, case):
    from tropical.utils.mesh import PolygonMesh, polygon_report
    from tropical.utils.topology import fill_holes
    v, pm = _surface(case, cuda)
    L, K, (lo, hi), S, b0, b1, miso, e0, e1, nci, ntri, at4 = TABLE[case]
    cyc, _ = _check(case, data=(v, pm.offsets, pm.indices), coords=False)  # (no coordinates: build reads none)
    st = cyc.stats
    assert (st["n_loops"], st["n_capped"], st["n_nonsimple"], st["n_unoriented"], st["n_too_long"]) == (L, K, S, 0, 0)
    assert (st["n_cycle_indices"], st["n_triangles"], st["longest_capped"]) == (nci, ntri, hi)
    assert int(np.diff(cyc.offsets).min()) == lo
    mesh = PolygonMesh(v, pm.offsets, pm.indices, pm.normals)
    r0 = polygon_report(mesh.vertices, mesh.offsets, mesh.indices)
    assert (r0["e_boundary"], r0["e_misoriented"], r0["euler"]) == (b0, miso, e0)
    for mode in ("polygon", "star"):
        filled, fst = fill_holes(mesh, mode=mode)
        assert fst == st and len(filled.normals) == len(filled)
        r1 = polygon_report(filled.vertices, filled.offsets, filled.indices)
        assert (r1["e_boundary"], r1["e_misoriented"], r1["euler"]) == (b1, miso, e1), mode
        assert r1["e_nonmanifold"] == r0["e_nonmanifold"]
    f4, st4 = fill_holes(mesh, max_edges=4)
    assert (st4["n_capped"], st4["n_nonsimple"], st4["n_too_long"]) == at4 and len(f4) == len(mesh) + at4[0]


def test_two_builds_give_the_same_bits(cuda):
    v, pm = _surface("small_sphere_curve", cuda)
    for name, data in (("small_sphere_curve", (v, pm.offsets, pm.indices)), ("ngons", None)):
        (a, ca), (b, cb) = _check(name, data=data), _check(name, data=data)
        assert a.status.tobytes() == b.status.tobytes() and a.vertices.tobytes() == b.vertices.tobytes()
        assert a.offsets.tobytes() == b.offsets.tobytes() and a.cycle_loop.tobytes() == b.cycle_loop.tobytes()
        assert len(ca) > 0 and ca.tobytes() == cb.tobytes()


def test_a_second_build_replaces_the_first(cuda):
    from tropical.utils.topology import holes_handle
    h = holes_handle()
    try:
        big, _ = _check("ngons", handle=h)
        small, _ = _check("cylinder", handle=h)
        assert (len(big), len(small), small.stats["n_cycle_indices"]) == (16, 2, 16)
        _check("empty", handle=h)
        _check("cube", handle=h)
        _check("isolated_1000", handle=h)
    finally:
        h.close()


@pytest.mark.parametrize("max_edges", [4, 10, 0])
def test_max_edges_on_the_punched_grid(cuda, max_edges):
    cyc, _ = _check("punched_grid", max_edges)
    st = cyc.stats
    want = {4: (7, 1, 2), 10: (8, 1, 1), 0: (9, 1, 0)}[max_edges]
    assert (st["n_capped"], st["n_nonsimple"], st["n_too_long"]) == want
    assert st["longest_capped"] == {4: 4, 10: 10, 0: 96}[max_edges]


def test_train_fill_holes_flag(cuda, tmp_path, capsys):
    """train --fill-holes 6 --keep-largest 1 on a fixture net's surface (no
    dataset): the printed line, the file, and every other output unchanged."""
    import tropical.stanford.train as tr
    from tropical.utils.mesh import load_polygon_ply, polygon_report
    from tropical.utils.topology import fill_holes
    args = tr.parse_args(["--fill-holes", "6", "--keep-largest", "1"])
    assert args.components and args.polygons and (args.fill_holes, args.keep_largest) == (6, 1)
    v, pm = _surface("small_sphere_curve", cuda)
    verts = v / tr.R
    name = "our_poly_mesh_small_45.ply"

    def outputs(d, fill):
        path = str(d / name)
        tr.export_polygons(pm, verts, path)
        topo = tr.export_components(pm, verts, path, keep_largest=1)
        if fill:
            tr.export_filled(pm, verts, path, 6, topo, keep_largest=1)
        return capsys.readouterr().out.splitlines()

    capsys.readouterr()
    plain, with_fill = outputs(tmp_path / "a", False), outputs(tmp_path / "b", True)
    assert with_fill[:-1] == plain
    g = re.fullmatch(r"Ours \(holes\): (\d+) loops, (\d+) capped \(<= 6 edges\), (\d+) non-simple, (\d+) unoriented, "
                     r"(\d+) longer; boundary edges (\d+) -> (\d+), closed components (\d+) -> (\d+)", with_fill[-1])
    assert g, with_fill[-1]
    got = [int(x) for x in g.groups()]
    big = load_polygon_ply(str(tmp_path / "b" / "our_poly_mesh_small_45_largest1.ply"))
    want, st = fill_holes(big, max_edges=6)
    b0 = polygon_report(big.vertices, big.offsets, big.indices)["e_boundary"]
    b1 = polygon_report(want.vertices, want.offsets, want.indices)["e_boundary"]
    assert got[:7] == [st["n_loops"], st["n_capped"], st["n_nonsimple"], st["n_unoriented"], st["n_too_long"], b0, b1]
    assert b0 - b1 == st["n_cycle_indices"] and st["n_capped"] > 0 and st["longest_capped"] <= 6
    assert got[7] <= got[8] <= 1
    filled = load_polygon_ply(str(tmp_path / "b" / "our_poly_mesh_small_45_largest1_filled.ply"))
    assert np.array_equal(filled.offsets, want.offsets) and np.array_equal(filled.indices, want.indices)
    assert len(filled) == len(big) + st["n_capped"]
    files = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert sorted(p.name for p in (tmp_path / "b").iterdir()) == sorted(files + ["our_poly_mesh_small_45_largest1_filled.ply"])
    for f in files:
        assert (tmp_path / "a" / f).read_bytes() == (tmp_path / "b" / f).read_bytes(), f
