"""CPU: the restatement of tnp_holes_* (holes_cases.holes_ref) on the stored
polygon rows and on the synthetic soups, the host parts of fill_holes, and the
--fill-holes argparse rules."""
import numpy as np
import pytest

from golden_io import load
from holes_cases import CAPPED, NONSIMPLE, TOO_LONG, UNORIENTED, NGON_SIZES, caps_ref, filled_soup, holes_ref, \
    reference, soups
from polygon_cases import FULL, fixture, polygon_stats
from topology_cases import topology_ref

# case: loops, capped, (shortest, longest capped), non-simple, e_boundary before / after, e_misoriented,
#       euler before / after, n_cycle_indices, n_triangles; then capped / non-simple / too long at max_edges = 4
TABLE = {"small_sphere": (37, 34, (3, 6), 3, 175, 26, 0, -92, -58, 149, 3, (23, 3, 11)),
         "small_torus": (10, 8, (4, 8), 2, 62, 16, 2, -24, -16, 46, 0, (2, 2, 6)),
         "h8l3_sphere": (2, 2, (4, 4), 0, 8, 0, 0, -2, 0, 8, 0, (2, 0, 0)),
         "small_sphere_curve": (47, 35, (3, 25), 12, 1892, 1609, 2, -29, 6, 283, 6, (12, 12, 23))}
SYNTHETIC = ["torus", "cylinder", "two_tets", "cube", "cube_reversed", "moebius", "two_fans", "one", "empty",
             "isolated_1000", "strip_4096", "book_1000", "strip_4096_vperm", "ngons", "punched_grid",
             "flipped_cylinder"]


def _surface(case):
    fx = fixture(case)
    return load(case)["surf_V"], fx["offsets"], fx["indices"]


@pytest.mark.parametrize("case", FULL)
def test_the_stored_surfaces_give_the_table(case):
    v, off, idx = _surface(case)
    L, K, (lo, hi), S, b0, b1, miso, e0, e1, nci, ntri, at4 = TABLE[case]
    ref = reference(case, 0, (v, off, idx))
    st = ref["stats"]
    lens = np.diff(ref["offsets"])
    assert (st["n_loops"], st["n_capped"], st["n_nonsimple"], st["n_unoriented"], st["n_too_long"]) == (L, K, S, 0, 0)
    assert (int(lens.min()), int(lens.max()), st["longest_capped"]) == (lo, hi, hi)
    assert (st["n_cycle_indices"], st["n_triangles"]) == (nci, ntri)
    before, _, _ = polygon_stats(v, off, idx)
    assert (before["e_boundary"], before["e_misoriented"], before["euler"]) == (b0, miso, e0)
    for mode in ("polygon", "star"):
        fv, foff, fidx = filled_soup(v, off, idx, *caps_ref(ref, mode, len(v), v))
        after, _, _ = polygon_stats(fv, foff, fidx)
        assert (after["e_boundary"], after["e_misoriented"], after["euler"]) == (b1, miso, e1), mode
    r4 = reference(case, 4, (v, off, idx))["stats"]
    assert (r4["n_capped"], r4["n_nonsimple"], r4["n_too_long"]) == at4


@pytest.mark.parametrize("name", SYNTHETIC + FULL)
def test_filling_lowers_the_boundary_by_the_cycle_indices(name):
    v, off, idx = soups()[name] if name in SYNTHETIC else _surface(name)
    ref = reference(name, 0, (v, off, idx))
    st = ref["stats"]
    assert st["n_capped"] + st["n_nonsimple"] + st["n_unoriented"] + st["n_too_long"] == st["n_loops"]
    if len(off) == 1:
        assert st["n_loops"] == 0 and len(ref["vertices"]) == 0 and ref["offsets"].tolist() == [0]
        return
    before, _, _ = polygon_stats(v, off, idx)
    tb = topology_ref(v, off, idx)
    assert np.array_equal(tb["loops"]["first_vertex"], ref["first_vertex"])
    assert np.array_equal(tb["loops"]["n_edges"], ref["n_edges"]) and np.array_equal(tb["loops"]["simple"], ref["simple"])
    open_ = ref["status"] != CAPPED
    for mode in ("polygon", "star"):
        coff, cidx, new = caps_ref(ref, mode, len(v), v)
        fv, foff, fidx = filled_soup(v, off, idx, coff, cidx, new)
        after, _, _ = polygon_stats(fv, foff, fidx)
        assert after["e_boundary"] == before["e_boundary"] - st["n_cycle_indices"], mode
        assert after["e_misoriented"] == before["e_misoriented"] and after["e_nonmanifold"] == before["e_nonmanifold"]
        ta = topology_ref(fv, foff, fidx)
        # exactly the uncapped loops are left, and a cap joins the component of its loop
        for k in ("first_vertex", "n_edges", "simple"):
            assert np.array_equal(ta["loops"][k], tb["loops"][k][open_]), (mode, k)
        assert np.array_equal(ta["labels"][:len(off) - 1], tb["labels"])
        assert len(ta["components"]["euler"]) == len(tb["components"]["euler"])
        n_caps = len(coff) - 1
        if mode == "polygon":
            assert np.array_equal(ta["labels"][len(off) - 1:], tb["loops"]["component"][ref["cycle_loop"]])
            assert n_caps == st["n_capped"] and len(new) == 0
        else:
            assert n_caps == st["n_cycle_indices"] - 2 * st["n_triangles"] and (np.diff(coff) == 3).all()
            assert len(new) == st["n_capped"] - st["n_triangles"]


def test_the_synthetic_soups_have_the_expected_status():
    assert reference("moebius")["status"].tolist() == [UNORIENTED]
    assert reference("two_fans")["status"].tolist() == [NONSIMPLE]
    assert reference("book_1000")["status"].tolist() == [NONSIMPLE]
    assert reference("flipped_cylinder")["status"].tolist() == [UNORIENTED, CAPPED]
    assert reference("flipped_cylinder")["vertices"].tolist() == [7 + 8 * i for i in range(8)]
    assert np.diff(reference("strip_4096_vperm")["offsets"]).tolist() == [8194]
    assert reference("isolated_1000")["stats"]["n_triangles"] == 1000
    for closed in ("torus", "cube", "cube_reversed", "two_tets", "empty"):
        assert reference(closed)["stats"]["n_loops"] == 0
    ng = reference("ngons")
    assert sorted(np.diff(ng["offsets"]).tolist()) == NGON_SIZES and (ng["status"] == CAPPED).all()
    # a cylinder's cap runs against its rim: the cycle from vertex 0 goes down the i's
    cyl = reference("cylinder")
    assert cyl["vertices"][:8].tolist() == [0] + [8 * i for i in range(7, 0, -1)]


def test_max_edges_on_the_punched_grid():
    g0, g4, g10 = reference("punched_grid", 0), reference("punched_grid", 4), reference("punched_grid", 10)
    assert sorted(g0["n_edges"].tolist()) == [4] * 7 + [8, 10, 96]
    for g, want in ((g0, (9, 1, 0)), (g4, (7, 1, 2)), (g10, (8, 1, 1))):
        st = g["stats"]
        assert (st["n_capped"], st["n_nonsimple"], st["n_too_long"]) == want and st["n_unoriented"] == 0
    assert g0["stats"]["longest_capped"] == 96 and g10["stats"]["longest_capped"] == 10
    assert g4["status"][g4["n_edges"] == 8].tolist() == [NONSIMPLE]  # the pinch wins over the length
    assert set(g4["status"][g4["n_edges"] > 8].tolist()) == {TOO_LONG}


def test_fill_holes_host_parts():
    from tropical.utils.mesh import PolygonMesh
    from tropical.utils.topology import append_caps, fill_holes, newell_normals
    v, off, idx = soups()["cylinder"]
    ref = reference("cylinder")
    nrm = np.tile(np.float32([1, 0, 0]), (len(off) - 1, 1))
    pm = PolygonMesh(v, off, idx, nrm)
    coff, cidx, _ = caps_ref(ref, "polygon", len(v))
    f = append_caps(pm, coff, cidx)
    assert len(f) == len(pm) + 2 and np.array_equal(f.vertices, pm.vertices)
    assert np.array_equal(f.offsets[:len(pm.offsets)], pm.offsets) and np.array_equal(f.indices[:len(idx)], idx)
    assert f.offsets[-3:].tolist() == [len(idx), len(idx) + 8, len(idx) + 16] and np.array_equal(f.indices[len(idx):], cidx)
    assert np.array_equal(f.normals[:len(pm)], nrm)
    # the cylinder's quads wind outward: the caps' normals point out of its two ends
    assert np.allclose(f.normals[-2:], [[0, 0, -1], [0, 0, 1]], atol=1e-6)
    soff, sidx, new = caps_ref(ref, "star", len(v), v)
    g = append_caps(pm, soff, sidx, new)
    assert len(g) == len(pm) + 16 and len(g.vertices) == len(v) + 2 and g.normals.shape == (len(g), 3)
    assert np.array_equal(g.vertices[-2:], new.astype(np.float64)) and np.allclose(new, [[0, 0, 0], [0, 0, 1.75]], atol=1e-6)
    assert np.allclose(g.normals[len(pm):len(pm) + 8], [0, 0, -1], atol=1e-6)
    assert append_caps(PolygonMesh(v, off, idx), coff, cidx).normals is None
    assert newell_normals(v, [0], []).shape == (0, 3)
    # no caps: the identity
    e = append_caps(pm, [0], np.zeros(0, np.int64), np.zeros((0, 3), np.float32))
    assert np.array_equal(e.offsets, pm.offsets) and np.array_equal(e.indices, pm.indices) and len(e.normals) == len(pm)
    with pytest.raises(ValueError, match="mode"):
        fill_holes(pm, mode="fan")


def test_fill_holes_flag_rules(capsys):
    import tropical.stanford.train as tr
    a = tr.parse_args(["--fill-holes", "6"])
    assert a.fill_holes == 6 and a.components and a.polygons and a.keep_largest == 0
    a = tr.parse_args(["--fill-holes", "3", "--keep-largest", "2"])
    assert (a.fill_holes, a.keep_largest) == (3, 2)
    d = tr.parse_args([])
    assert d.fill_holes == 0 and not d.components and not d.polygons
    assert tr.parse_args(["--fill-holes", "0"]).components is False
    for bad in ("-1", "1", "2"):
        with pytest.raises(SystemExit):
            tr.parse_args(["--fill-holes", bad])
        assert "--fill-holes" in capsys.readouterr().err
