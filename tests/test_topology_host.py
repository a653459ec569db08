"""CPU: the numpy restatement of tnp_topology_* (topology_cases.topology_ref)
on soups whose answers are known and on the stored polygon rows, and
keep_components / largest_components on numpy input."""
import numpy as np
import pytest

from golden_io import load
from polygon_cases import FULL, fixture
from topology_cases import EDGE_COLS, reference, soups

# case: (components by edge, by vertex, loops, simple loops)
FIXTURE_COUNTS = {"small_sphere": (1, 1, 37, 34), "small_torus": (1, 1, 10, 8), "h8l3_sphere": (1, 1, 2, 2),
                  "small_sphere_curve": (59, 23, 47, 35)}


def test_torus_is_one_closed_component():
    for connect in ("edge", "vertex"):
        r = reference("torus", connect)
        c = r["components"]
        assert len(c["euler"]) == 1 and c["euler"][0] == 0 and len(r["loops"]["n_edges"]) == 0
        assert (c["n_polygons"][0], c["n_vertices"][0], c["n_edges"][0], c["e_manifold"][0]) == (64, 64, 128, 128)
        assert c["e_misoriented"][0] == 0 and c["first_polygon"][0] == 0 and (r["labels"] == 0).all()


def test_open_cylinder_has_two_simple_loops():
    lp = reference("cylinder", "edge")["loops"]
    assert lp["n_edges"].tolist() == [8, 8] and lp["n_vertices"].tolist() == [8, 8] and lp["simple"].tolist() == [1, 1]
    assert lp["first_vertex"].tolist() == [0, 7] and lp["component"].tolist() == [0, 0]
    want = 8 * 2 * np.sin(np.pi / 8)  # a regular octagon of circumradius 1
    assert np.allclose(lp["length"], want, rtol=1e-6)


def test_two_tetrahedra_sharing_a_vertex():
    e, v = reference("two_tets", "edge"), reference("two_tets", "vertex")
    assert e["labels"].tolist() == [0] * 4 + [1] * 4 and v["labels"].tolist() == [0] * 8
    assert e["components"]["euler"].tolist() == [2, 2] and e["components"]["n_vertices"].tolist() == [4, 4]
    assert v["components"]["euler"].tolist() == [3] and v["components"]["n_vertices"].tolist() == [7]
    assert e["components"]["first_polygon"].tolist() == [0, 4]
    assert np.allclose(e["components"]["volume"], [-0.7 ** 3 / 6, 1 / 6])


def test_cube_volume_is_exact():
    c, r = reference("cube", "edge")["components"], reference("cube_reversed", "edge")["components"]
    assert c["volume"].tolist() == [8.0] and r["volume"].tolist() == [-8.0]
    assert c["area"].tolist() == [24.0] and r["area"].tolist() == [24.0]
    assert c["lo"].tolist() == [[0, 0, 0]] and c["hi"].tolist() == [[2, 2, 2]]
    assert (c["e_boundary"][0], c["e_misoriented"][0], c["euler"][0]) == (0, 0, 2)


def test_moebius_strip():
    r = reference("moebius", "edge")
    assert len(r["components"]["euler"]) == 1 and r["components"]["e_misoriented"][0] >= 1
    assert r["loops"]["simple"].tolist() == [1] and r["loops"]["n_edges"].tolist() == [16]
    assert r["components"]["euler"][0] == 0


def test_two_fans_meeting_at_a_boundary_vertex():
    e, v = reference("two_fans", "edge"), reference("two_fans", "vertex")
    assert e["loops"]["simple"].tolist() == [0] and e["loops"]["n_edges"].tolist() == [8]
    assert e["loops"]["n_vertices"].tolist() == [7] and e["loops"]["component"].tolist() == [0]
    assert len(e["components"]["euler"]) == 2 and len(v["components"]["euler"]) == 1


def test_the_hard_shapes_have_the_expected_classes():
    assert len(reference("isolated_1000", "edge")["components"]["euler"]) == 1000
    assert reference("isolated_1000", "edge")["loops"]["n_edges"].tolist() == [3] * 1000
    for name in ("strip_4096", "strip_4096_vperm"):
        r = reference(name, "edge")
        assert r["components"]["n_polygons"].tolist() == [4096]
        assert r["loops"]["n_edges"].tolist() == [8194] and r["loops"]["simple"].tolist() == [1]
    b = reference("book_1000", "edge")
    assert b["components"]["n_polygons"].tolist() == [1000] and b["components"]["e_nonmanifold"].tolist() == [1]
    assert b["loops"]["n_edges"].tolist() == [2000] and b["loops"]["simple"].tolist() == [0]
    assert len(reference("empty", "edge")["labels"]) == 0 and len(reference("one", "vertex")["labels"]) == 1


@pytest.mark.parametrize("case", FULL)
def test_counts_on_the_stored_rows(case):
    fx = fixture(case)
    data = (load(case)["surf_V"], fx["offsets"], fx["indices"])
    e, v = reference(case, "edge", data), reference(case, "vertex", data)
    got = (len(e["components"]["euler"]), len(v["components"]["euler"]), len(e["loops"]["simple"]),
           int(e["loops"]["simple"].sum()))
    assert got == FIXTURE_COUNTS[case]
    for r in (e, v):
        c = r["components"]
        for k in EDGE_COLS:  # every undirected edge lies in exactly one component
            assert int(c[k].sum()) == fx["stats"][k], k
        assert int(c["n_polygons"].sum()) == fx["stats"]["n_polygons"]
        assert int(c["n_indices"].sum()) == fx["stats"]["n_indices"]
        assert int(r["loops"]["n_edges"].sum()) == fx["stats"]["e_boundary"]
        assert (np.diff(c["first_polygon"]) > 0).all() and r["labels"].max() == len(c["euler"]) - 1
    # the loops are the same in both modes; vertex classes are unions of edge classes
    assert v["loops"]["n_edges"].tolist() == e["loops"]["n_edges"].tolist()
    assert len(np.unique(e["labels"].astype(np.int64) * (1 << 32) + v["labels"])) == len(e["components"]["euler"])


def test_keep_components_on_numpy_input():
    from tropical.utils.mesh import PolygonMesh
    from tropical.utils.topology import COMPONENT_DTYPE, keep_components, largest_components
    v, off, idx = soups()["two_tets"]
    nrm = np.arange(24, dtype=np.float32).reshape(8, 3)
    pm = PolygonMesh(v, off, idx, nrm)
    labels = reference("two_tets", "edge")["labels"]
    k = keep_components(pm, labels, [1])
    assert len(k) == 4 and k.offsets.tolist() == [0, 3, 6, 9, 12]
    # vertices 0, 1, 2 are dropped: 3 .. 6 become 0 .. 3 in their order
    assert np.array_equal(k.vertices, pm.vertices[3:]) and np.array_equal(k.indices, idx[12:] - 3)
    assert np.array_equal(k.normals, nrm[4:])
    k0 = keep_components(pm, labels, [0])
    assert np.array_equal(k0.vertices, pm.vertices[:4]) and np.array_equal(k0.indices, idx[:12])
    both = keep_components(pm, labels, [1, 0])  # every component: the identity, in the polygons' order
    assert np.array_equal(both.vertices, pm.vertices) and np.array_equal(both.offsets, pm.offsets)
    assert np.array_equal(both.indices, pm.indices) and np.array_equal(both.normals, pm.normals)
    assert keep_components(PolygonMesh(v, off, idx), labels, [1]).normals is None
    with pytest.raises(ValueError, match="labels"):
        keep_components(pm, labels[:3], [0])
    comps = np.zeros(4, COMPONENT_DTYPE)
    comps["area"] = [1.0, 3.0, 3.0, 2.0]
    comps["n_polygons"] = [9, 1, 1, 1]
    assert largest_components(comps, 2).tolist() == [1, 2]  # ties go to the lower id
    assert largest_components(comps, 10).tolist() == [1, 2, 3, 0]
    assert largest_components(comps, 1, by="n_polygons").tolist() == [0]
