"""CPU: the restatement of tnp_weld_* (weld_cases.weld_ref) -- its grid search
against the plain all-pairs search, its table on the stored surfaces, what the
synthetic soups are built to give -- and the --weld argparse rules."""
import numpy as np
import pytest

from golden_io import load
from polygon_cases import FULL, fixture, polygon_stats
from weld_cases import (DIRECTIONS, STAT_KEYS, close_pairs, close_pairs_brute, reference, soups, weld_ref,
                        welded_soup)

TOLS = (1e-3, 2e-3)
# case: at each tolerance (n_used, n_pairs, n_clusters, n_merged, max_cluster, n_polygons, n_indices,
#       n_dropped_polygons, n_pinched), then (e_boundary, e_nonmanifold, e_misoriented, euler) after welding;
#       "before": the same four columns of the input
TABLE = {
    "small_sphere": {"before": (175, 42, 0, -92),
                     1e-3: ((5021, 324, 261, 295, 4, 4844, 19201, 202, 0), (129, 24, 0, -77)),
                     2e-3: ((5021, 597, 441, 527, 5, 4567, 18168, 479, 0), (101, 15, 0, -64))},
    "small_torus": {"before": (62, 30, 2, -24),
                    1e-3: ((2993, 190, 147, 169, 5, 2868, 11397, 141, 0), (23, 11, 0, -10)),
                    2e-3: ((2993, 446, 308, 372, 7, 2686, 10614, 323, 0), (0, 0, 0, 0))},
    "h8l3_sphere": {"before": (8, 2, 0, -2),
                    1e-3: ((1425, 8, 8, 8, 2, 1423, 5676, 8, 0), (0, 0, 0, 2)),
                    2e-3: ((1425, 20, 12, 16, 3, 1420, 5654, 11, 0), (0, 0, 0, 2))},
    "small_sphere_curve": {"before": (1892, 6, 2, -29),
                           1e-3: ((3614, 269, 215, 242, 4, 2998, 10987, 156, 0), (1810, 2, 0, -27)),
                           2e-3: ((3614, 420, 326, 375, 5, 2843, 10451, 311, 0), (1766, 2, 0, -26))},
}
REPORT = ("e_boundary", "e_nonmanifold", "e_misoriented", "euler")


def surface(case):
    fx = fixture(case)
    return np.asarray(load(case)["surf_V"], np.float32), fx["offsets"], fx["indices"]


def report_of(soup):
    st, _, _ = polygon_stats(*soup)
    return tuple(st[k] for k in REPORT)


@pytest.mark.parametrize("name", list(soups()))
def test_the_grid_search_finds_the_all_pairs_search_pairs(name):
    v, off, idx, tol = soups()[name]
    assert np.array_equal(close_pairs(v, idx, tol), close_pairs_brute(v, idx, tol)), name


@pytest.mark.parametrize("tol", TOLS + (0.0, 0.05))
def test_the_grid_search_on_a_stored_surface(tol):
    v, off, idx = surface("h8l3_sphere")
    got = close_pairs(v, idx, tol)
    assert np.array_equal(got, close_pairs_brute(v, idx, tol))
    assert tol != 0.05 or len(got) > 1000  # (many vertices per cell)


@pytest.mark.parametrize("case", FULL)
def test_the_stored_surfaces_give_the_table(case):
    data = surface(case)
    assert report_of(data) == TABLE[case]["before"]
    for tol in TOLS:
        ref = reference(case, "first", data, tol)
        want_stats, want_report = TABLE[case][tol]
        assert tuple(ref["stats"][k] for k in STAT_KEYS[:-1]) == want_stats, (case, tol)
        assert report_of(welded_soup(ref)) == want_report, (case, tol)
        assert 0 < ref["stats"]["max_shift"] <= want_stats[4] * tol  # (a chain of m members is shorter than m tol)
        mean = reference(case, "mean", data, tol)
        for k in ("map", "offsets", "indices", "source"):
            assert np.array_equal(mean[k], ref[k])
        assert report_of(welded_soup(mean)) == want_report


def test_welding_closes_the_fitted_sphere_and_torus():
    sphere = reference("h8l3_sphere", "first", surface("h8l3_sphere"), 1e-3)
    assert report_of(welded_soup(sphere)) == (0, 0, 0, 2)
    torus = reference("small_torus", "first", surface("small_torus"), 2e-3)
    assert report_of(welded_soup(torus)) == (0, 0, 0, 0)


@pytest.mark.parametrize("case", FULL)
def test_tol_zero_changes_nothing_on_the_stored_surfaces(case):
    v, off, idx = surface(case)
    for position in ("first", "mean"):
        ref = reference(case, position, (v, off, idx), 0.0)
        assert np.array_equal(ref["map"], np.arange(len(v))) and ref["positions"].tobytes() == v.tobytes()
        assert np.array_equal(ref["offsets"], off) and np.array_equal(ref["indices"], idx)
        assert np.array_equal(ref["source"], np.arange(len(off) - 1))
        st = ref["stats"]
        assert (st["n_pairs"], st["n_merged"], st["n_dropped_polygons"], st["max_shift"]) == (0, 0, 0, 0.0)


def test_the_synthetic_soups_give_what_they_are_built_for():
    st = {name: reference(name)["stats"] for name in soups()}
    assert (st["lattice_at_tol"]["n_pairs"], st["lattice_at_tol"]["max_cluster"]) == (54, 27)
    assert (st["lattice_below_tol"]["n_pairs"], st["lattice_below_tol"]["n_merged"]) == (0, 0)
    n_pairs = len(DIRECTIONS) + 4
    near = reference("borders_0.9")
    assert (st["borders_0.9"]["n_pairs"], st["borders_0.9"]["n_clusters"], st["borders_0.9"]["max_cluster"]) == \
        (n_pairs, n_pairs, 2)
    assert np.array_equal(near["map"], np.arange(2 * n_pairs) // 2 * 2)
    assert (st["borders_1.1"]["n_pairs"], st["borders_1.1"]["n_merged"]) == (0, 0)
    v = soups()["borders_0.9"][0]
    assert v.min() == -1 and v.max() == 1 and (v < 0).any() and (v > 0).any()
    for name, n in (("chain_1000", 1000), ("chain_257", 257)):
        assert (st[name]["n_pairs"], st[name]["n_clusters"], st[name]["max_cluster"]) == (n - 1, 1, n)
        assert (reference(name)["map"] == 0).all()
    assert (st["ball_300"]["n_pairs"], st["ball_300"]["max_cluster"]) == (44850, 300)
    for name in ("bridge", "bridge_unused_nan"):
        assert st[name]["n_merged"] == 0 and st[name]["n_used"] == 5
    cube = reference("split_cube")
    assert (st["split_cube"]["n_merged"], st["split_cube"]["max_cluster"], st["split_cube"]["n_polygons"]) == (16, 3, 6)
    assert report_of(welded_soup(cube)) == (0, 0, 0, 2) and len(np.unique(cube["map"])) == 8
    assert (st["identical"]["n_pairs"], st["identical_tol"]["max_cluster"]) == (780, 40)
    assert (st["far_box"]["n_pairs"], st["far_box"]["n_clusters"], st["far_box"]["max_cluster"]) == (300, 300, 2)
    assert 200 <= st["random_8192"]["n_clusters"] <= 400
    assert st["no_polygons"] == st["nothing"] == dict.fromkeys(STAT_KEYS, 0)


def test_the_rewritten_polygons():
    v, off, idx, tol = soups()["rewrite"]
    ref = reference("rewrite")
    st = ref["stats"]
    assert ref["source"].tolist() == [0, 2, 4, 5, 6, 8]  # dropped: 1 (two ids left), 3 (one), 7 (two)
    assert np.diff(ref["offsets"]).tolist() == [3, 3, 4, 3, 257, 4]
    assert (st["n_polygons"], st["n_indices"], st["n_dropped_polygons"], st["n_pinched"]) == (6, 274, 3, 1)
    p = [ref["indices"][a:b].tolist() for a, b in zip(ref["offsets"][:-1], ref["offsets"][1:])]
    q = [idx[a:b].tolist() for a, b in zip(off[:-1], off[1:])]
    assert p[0] == [q[0][0], q[0][2], q[0][4]]
    assert p[1] == [q[2][1], q[2][2], q[2][0]]  # the run (last, first) wraps: the first position goes
    assert p[2] == [q[4][0], q[4][1], q[4][0], q[4][3]]  # pinched
    assert p[3] == q[5] and p[5] == q[8]
    assert p[4] == q[6][0:512:2] + [q[6][512]]
    # the same by a restatement without the close pairs handed in
    again = weld_ref(v, off, idx, tol)
    assert all(np.array_equal(again[k], ref[k]) for k in ("map", "offsets", "indices", "source"))


def test_a_mean_lies_between_its_members():
    for name in ("ball_300", "rewrite", "random_8192"):
        v = soups()[name][0]
        first, mean = reference(name, "first"), reference(name, "mean")
        assert np.array_equal(first["map"], mean["map"]) and len(mean["clusters"]) == mean["stats"]["n_clusters"]
        single = np.ones(len(v), bool)
        for mem in mean["clusters"]:
            single[mem] = False
            assert (mean["positions"][mem] == mean["positions"][mem[0]]).all()
            assert (mean["positions"][mem[0]] >= v[mem].min(0)).all() and (mean["positions"][mem[0]] <= v[mem].max(0)).all()
        assert mean["positions"][single].tobytes() == v[single].tobytes()


def test_weld_flag_rules(capsys):
    import tropical.stanford.train as tr
    a = tr.parse_args(["--weld", "1e-3"])
    assert a.weld == 1e-3 and a.components and a.polygons and (a.keep_largest, a.fill_holes) == (0, 0)
    a = tr.parse_args(["--weld", "0.002", "--keep-largest", "1", "--fill-holes", "6"])
    assert (a.weld, a.keep_largest, a.fill_holes) == (0.002, 1, 6)
    d = tr.parse_args([])
    assert d.weld == 0 and not d.components and not d.polygons
    assert tr.parse_args(["--weld", "0"]).components is False
    for bad in ("-1e-3", "nan", "inf"):
        with pytest.raises(SystemExit):
            tr.parse_args(["--weld", bad])
        assert "--weld" in capsys.readouterr().err


def test_weld_refuses_bad_arguments_on_the_host():
    from tropical.utils.mesh import PolygonMesh
    from tropical.utils.weld import weld, weld_vertices
    v, off, idx, _ = soups()["bridge"]
    with pytest.raises(ValueError, match="position"):
        weld_vertices(v, off, idx, 0.1, position="median")
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="tol"):
            weld(PolygonMesh(v, off, idx), bad)
