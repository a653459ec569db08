"""CPU: the polygon fixture (tests/golden/polygons.npz) against the triangle
goldens it was captured with, and the PolygonMesh container / PLY I/O."""
import os

import numpy as np
import pytest

from golden_io import GOLDEN, load, sha
from polygon_cases import FLAT, FULL, fan_t_major, fixture


@pytest.mark.parametrize("case", FULL)
def test_fixture_fans_to_the_golden_triangles(case):
    """The t-major fan of the stored polygons is the case's own faces_with_indices."""
    d, g = fixture(case), load(case)
    tri = fan_t_major(d["offsets"], d["indices"])
    assert tri.dtype == np.int64 and sha(tri) == str(g["sha_tri"])
    assert np.array_equal(tri, g["tri"])
    assert sha(d["offsets"], d["indices"]) == d["sha"]
    assert d["normals"].shape == (len(d["offsets"]) - 1, 3)
    assert d["stats"]["n_polygons"] == len(d["offsets"]) - 1 and d["stats"]["n_indices"] == len(d["indices"])


def test_fixture_is_small_and_records_the_reference_counts():
    assert os.path.getsize(os.path.join(GOLDEN, "polygons.npz")) < 1 << 20
    s = fixture("small_sphere")["stats"]
    assert (s["n_polygons"], s["n_edges"], s["e_boundary"], s["e_nonmanifold"], s["euler"]) == \
        (5046, 10159, 175, 42, -92)
    w = fixture("h32l3_rand")
    assert "offsets" not in w and w["stats"]["n_polygons"] == 95847 and w["stats"]["max_degree"] == 20
    assert w["stats"]["e_misoriented"] == 13610
    assert set(FLAT) < set(FULL)


def _mesh(case):
    from tropical.utils.mesh import PolygonMesh
    d, g = fixture(case), load(case)
    return PolygonMesh(g["surf_V"], d["offsets"], d["indices"], d["normals"])


def test_export_reads_back_as_its_fan(tmp_path):
    from tropical.utils.mesh import load_ply
    pm = _mesh("small_torus")
    assert np.array_equal(pm.degrees(), np.diff(pm.offsets)) and len(pm) == len(pm.offsets) - 1
    tri = pm.triangles()
    assert tri.shape == (int((pm.degrees() - 2).sum()), 3)
    # polygon-major: the same triangles as the fan-position-major list, another order
    assert np.array_equal(np.unique(tri, axis=0), np.unique(fan_t_major(pm.offsets, pm.indices), axis=0))
    pm.export(str(tmp_path / "p.ply"))
    m = load_ply(str(tmp_path / "p.ply"), process=False)
    assert np.array_equal(m.faces, tri)
    assert np.array_equal(m.vertices.astype(np.float32), pm.vertices.astype(np.float32))


def test_polygon_ply_round_trip(tmp_path):
    from tropical.utils.mesh import PolygonMesh, load_polygon_ply
    pm = _mesh("h8l3_sphere")
    pm.export(str(tmp_path / "p.ply"))
    assert b"property list uchar int vertex_indices" in open(tmp_path / "p.ply", "rb").read(400)
    back = load_polygon_ply(str(tmp_path / "p.ply"))
    assert np.array_equal(back.offsets, pm.offsets) and np.array_equal(back.indices, pm.indices)
    assert np.array_equal(back.vertices.astype(np.float32), pm.vertices.astype(np.float32))
    # a 300-gon: the count no longer fits a uchar
    a = np.linspace(0, 2 * np.pi, 300, endpoint=False)
    big = PolygonMesh(np.stack([np.cos(a), np.sin(a), 0 * a], 1), [0, 300, 303], list(range(300)) + [0, 5, 9])
    big.export(str(tmp_path / "big.ply"))
    assert b"property list int int vertex_indices" in open(tmp_path / "big.ply", "rb").read(400)
    back = load_polygon_ply(str(tmp_path / "big.ply"))
    assert np.array_equal(back.offsets, [0, 300, 303]) and np.array_equal(back.indices, big.indices)
    assert big.triangles().shape == (299, 3)
    # no polygons at all
    empty = PolygonMesh(np.zeros((0, 3)), [0], [])
    empty.export(str(tmp_path / "e.ply"))
    back = load_polygon_ply(str(tmp_path / "e.ply"))
    assert len(back) == 0 and back.triangles().shape == (0, 3)
    with pytest.raises(ValueError):
        PolygonMesh(np.zeros((3, 3)), [0, 2], [0, 1, 2])


def test_polygon_ply_ascii(tmp_path):
    from tropical.utils.mesh import load_polygon_ply
    (tmp_path / "a.ply").write_text(
        "ply\nformat ascii 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\n"
        "element face 2\nproperty list uchar int vertex_indices\nend_header\n"
        "0 0 0\n1 0 0\n1 1 0\n0 1 0\n4 0 1 2 3\n3 0 2 3\n")
    m = load_polygon_ply(str(tmp_path / "a.ply"))
    assert m.offsets.tolist() == [0, 4, 7] and m.indices.tolist() == [0, 1, 2, 3, 0, 2, 3]
    assert m.vertices[2].tolist() == [1, 1, 0]


def test_train_cli_has_the_polygons_flag():
    from tropical.stanford.train import parse_args
    assert parse_args([]).polygons is False
    assert parse_args(["-e", "--polygons"]).polygons is True
