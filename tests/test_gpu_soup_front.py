"""GPU: the front the four polygon-soup entry points share (csrc/soup_host.h)
-- tnp_polygon_report, tnp_render_raster, tnp_topology_build, tnp_holes_build:
all refuse the same malformed soups in the same words, a refusal costs the
next call nothing, and each is driven through the smallest soups at which the
front can go wrong."""
import numpy as np
import pytest

from holes_cases import reference as holes_reference
from test_gpu_polygons import INT_FIELDS, _check_report
from test_gpu_render import check_exact, draw
from topology_cases import EDGE_COLS, reference, soups

pytestmark = pytest.mark.gpu
# P = 0; no boundary (B = L = 0: the holes build's early return); P = 1, n = 3; n over several 256-thread blocks and
# one class per polygon
EDGE_SOUPS = ["empty", "cube", "one", "isolated_1000"]
PREFIX = {"report": "tnp_polygon_report: polygon_report: ", "render": "tnp_render_raster: render: ",
          "topology": "tnp_topology_build: topology: ", "holes": "tnp_holes_build: holes: "}


def _camera(v, W=64, H=64):
    from tropical.utils.render import Camera
    return Camera.from_angles(15, 120).fit(v, W, H)


def test_malformed_soups_raise_alike_at_all_four_entry_points(cuda):
    from tropical.utils.mesh import polygon_report
    from tropical.utils.topology import boundary_cycles, holes_handle, polygon_topology, topology_handle
    v, off, idx = soups()["cube"]
    cyl = soups()["cylinder"]
    at = np.arange(24)
    bad = [
        (np.array([1, 4, 8, 12, 16, 20, 24]), idx, r"offsets\[0\] = 1, not 0"),
        (np.array([0, 4, 8, 6, 16, 20, 24]), idx,
         r"offsets decrease at polygon 2 \(offsets\[2\] = 8 > offsets\[3\] = 6\)"),
        (np.array([0, 4, 6, 12, 16, 20, 24]), idx, r"polygon 1 has 2 ids, fewer than 3"),
        (off, np.where(at == 5, 99, idx), r"indices\[5\] = 99 is outside \[0, 8\)"),
        (off, np.where(at == 17, -2, idx), r"indices\[17\] = -2 is outside \[0, 8\)"),
        (off, np.where(at == 9, idx[10], idx), r"indices\[9\] = 5 and the next id of its polygon are equal"),
        # cyclic: the last id of polygon 3 equals its first
        (off, np.where(at == 15, idx[12], idx), r"indices\[15\] = 2 and the next id"),
        # the first offender is named when there are several
        (off, np.where(at % 7 == 3, 1 << 40, idx), r"indices\[3\] = 1099511627776 is outside"),
    ]
    cam = _camera(v)
    th, hh = topology_handle(), holes_handle()
    try:
        good = draw(v, off, idx, cam, 64, 64, 8)
        check_exact(good, off, idx, 64, 64, 8, "cube")
        assert good["stats"]["pixels_covered"] > 500
        calls = {"report": lambda o, i: polygon_report(v, o, i, per_polygon=True),
                 "render": lambda o, i: draw(v, o, i, cam, 64, 64, 8),
                 "topology": lambda o, i: polygon_topology(v, o, i, handle=th),
                 "holes": lambda o, i: boundary_cycles(v, o, i, handle=hh)}
        for o, i, msg in bad:
            rest = {}
            for who, call in calls.items():
                with pytest.raises(RuntimeError, match=msg) as e:
                    call(o, i)
                assert str(e.value).startswith(PREFIX[who]), (who, str(e.value))
                rest[who] = str(e.value)[len(PREFIX[who]):]
            assert len(set(rest.values())) == 1, rest
            # and the bad input cost nothing: a valid call right afterwards, on the same handle, gives the known answer
            r = polygon_report(v, off, idx)
            assert (r["n_edges"], r["e_manifold"], r["euler"], r["area"]) == (12, 12, 2, 24.0)
            again = draw(v, off, idx, cam, 64, 64, 8)
            assert all(np.array_equal(again[k], good[k]) for k in ("screen", "prim", "tri", "edge"))
            assert again["stats"] == good["stats"]
            assert polygon_topology(v, off, idx, handle=th).components["volume"].tolist() == [8.0]
            assert boundary_cycles(v, off, idx, handle=hh).stats["n_loops"] == 0
            assert boundary_cycles(*cyl, handle=hh).stats["n_capped"] == 2
        with pytest.raises(ValueError, match="connect"):
            polygon_topology(v, off, idx, connect="face", handle=th)
        with pytest.raises(RuntimeError, match="max_edges"):
            boundary_cycles(v, off, idx, max_edges=-1, handle=hh)
        assert polygon_topology(v, off, idx, handle=th).components["volume"].tolist() == [8.0]
        assert boundary_cycles(*cyl, handle=hh).stats["n_capped"] == 2
    finally:
        th.close()
        hh.close()


@pytest.mark.parametrize("name", EDGE_SOUPS)
def test_report_and_raster_on_the_fronts_edge_soups(cuda, name):
    """The topology's and the holes' own suites run every soup of
    test_gpu_topology.SOUPS, these four among them; here the report and the
    rasteriser take the same four, the report against the topology's
    restatement as well as its own."""
    from tropical.utils.mesh import polygon_report
    v, off, idx = soups()[name]
    ref = reference(name, "edge")["components"]
    if name == "empty":
        r = polygon_report(v, off, idx, per_polygon=True)
        assert all(r[k] == 0 for k in INT_FIELDS) and r["area"] == 0.0 and r["polygon_area"].shape == (0,)
    else:
        r = _check_report(v, off, idx, label=name)
    for k in EDGE_COLS + ["n_polygons", "n_indices"]:
        assert r[k] == int(ref[k].sum()), k
    assert r["e_boundary"] == int(holes_reference(name)["n_edges"].sum())
    res = draw(v, off, idx, _camera(v), 64, 64, 8)
    _, _, _, st = check_exact(res, off, idx, 64, 64, 8, name)
    assert (st["n_polygons"], st["n_dropped"]) == (len(off) - 1, 0)
    assert (st["pixels_covered"] > 0) == (len(off) > 1)
