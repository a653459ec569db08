"""CPU: the restatement of tnp_simplify_* (simplify_cases.simplify_ref) -- what
the synthetic soups are built to give, its table on the stored surfaces, the
drift bound -- and the --simplify / --mesh-cell argparse rules and the host-side
refusals of tropical.utils.simplify."""
import math

import numpy as np
import pytest

import tropical.utils.simplify as simplify_py  # (every test here needs the feature)
from polygon_cases import FULL, polygon_stats
from simplify_cases import (DUPLICATES, MAX_CELLS, STAT_KEYS, canonical, cells_of, fixed_shape_sums, fsum_mean,
                            grid_limit, reference, simplified_soup, simplify_ref, soups)
from test_weld_host import REPORT, surface

CELLS = (0.05, 0.1)
INT_KEYS = STAT_KEYS[:-1]
# case, (cell, position): (n_used, n_cells, max_cell, n_polygons, n_indices, n_dropped_polygons,
#   n_duplicate_polygons, n_folded, n_pinched), then (e_boundary, e_nonmanifold, e_misoriented, euler) of the
#   output; the two positions share every integer.  Recorded from the restatement.
TABLE = {
    "small_sphere": {0.05: ((5021, 1624, 16, 2095, 7470, 2950, 1, 1, 8), (21, 49, 0, 6)),
                     0.1: ((5021, 557, 24, 768, 2659, 4274, 4, 2, 5), (1, 15, 0, 9))},
    "small_torus": {0.05: ((2993, 1318, 12, 1543, 5722, 1466, 0, 0, 0), (0, 0, 0, 0)),
                    0.1: ((2993, 483, 21, 603, 2180, 2406, 0, 0, 0), (0, 4, 0, 0))},
    "h8l3_sphere": {0.05: ((1425, 823, 7, 874, 3392, 557, 0, 0, 0), (4, 1, 0, 0)),
                    0.1: ((1425, 439, 8, 579, 2032, 852, 0, 0, 0), (0, 0, 0, 2))},
    "small_sphere_curve": {0.05: ((3614, 1469, 12, 1325, 4542, 1829, 0, 0, 0), (1171, 1, 0, -81)),
                           0.1: ((3614, 538, 16, 497, 1681, 2657, 0, 0, 0), (565, 0, 0, -97))},
}


def report_of(soup):
    st, _, _ = polygon_stats(*soup)
    return tuple(st[k] for k in REPORT)


def within_bound(ref, cell):
    return ref["stats"]["max_shift"] <= math.sqrt(3.0) * float(np.float32(cell)) * (1 + 2.0 ** -20)


def ints(ref):
    return tuple(ref["stats"][k] for k in INT_KEYS)


def test_the_module_names_the_modes_and_stages():
    assert simplify_py.POSITIONS == {"mean": 0, "nearest": 1} and len(simplify_py.STAGES) == 7


@pytest.mark.parametrize("name", list(soups()))
def test_every_soup_stays_within_the_drift_bound_and_states_weld_s_mean(name):
    v, off, idx, cell = soups()[name]
    mean, near = reference(name, "mean"), reference(name, "nearest")
    assert within_bound(mean, cell) and within_bound(near, cell), name
    assert ints(mean) == ints(near)
    for k in ("map", "offsets", "indices", "source"):
        assert np.array_equal(mean[k], near[k])
    assert mean["stats"]["n_polygons"] + mean["stats"]["n_dropped_polygons"] + \
        mean["stats"]["n_duplicate_polygons"] == len(off) - 1
    single = np.ones(len(v), bool)
    for mem in mean["classes"]:
        single[mem] = False
        assert mean["positions"][mem[0]].tobytes() == fsum_mean(v, mem).tobytes()  # weld_cases' statement of the mean
        assert (mean["positions"][mem].view(np.uint32) == mean["positions"][mem[0]].view(np.uint32)).all()
        pick = near["positions"][mem[0]]
        assert any(pick.tobytes() == v[i].tobytes() for i in mem)  # a member's bits
    assert mean["positions"][single].tobytes() == near["positions"][single].tobytes() == \
        np.asarray(v, np.float32)[single].tobytes()


def test_the_fixed_shape_sum_rounds_where_fsum_does_not():
    """Three values whose exact sum needs more than 53 bits: the restated shape adds left to right."""
    vals = np.array([[1.0, 2.0 ** -60, -1.0]] * 3).T.copy()
    assert fixed_shape_sums(vals, np.array([0, 3]))[0].tolist() == [0.0, 0.0, 0.0]
    assert math.fsum(vals[:, 0]) == 2.0 ** -60


def test_border_vertices_fall_where_np_floor_puts_them():
    v, off, idx, cell = soups()["borders"]
    ref = reference("borders")
    u, c = ref["cells"]
    assert len(u) == len(v) == 19 and c[0].tolist() == [0, 0, 0]
    h = float(np.float32(cell))
    for i in range(1, 19):
        q, k, below = (i - 1) // 6, (i - 1) % 6 // 2 + 1, (i - 1) % 2
        want = int(np.floor((float(v[i, q]) - 1000.0) / h))
        assert c[i, q] == want and want in (k - 1, k) and (c[i, np.arange(3) != q] == 0).all()
        if below:
            assert want <= c[i - 1, q]
    assert ref["stats"]["n_cells"] == len({tuple(r) for r in c.tolist()})
    assert float(np.float32(cell)) != 0.3 and math.frexp(float(np.float32(cell)))[0] != 0.5


def test_the_grid_limit():
    for name in ("grid_limit_x", "grid_limit_z"):
        ref = reference(name)
        assert ref["cells"][1].max() == MAX_CELLS - 1 and ref["stats"]["n_cells"] == 3
    for axis in range(3):
        v, off, idx = grid_limit(axis, True)
        with pytest.raises(ValueError, match=f"axis {'xyz'[axis]} needs {MAX_CELLS + 1} cells"):
            cells_of(v, idx, 1.0)


def test_one_cell_drops_everything():
    st = reference("one_cell")["stats"]
    assert (st["n_cells"], st["max_cell"], st["n_polygons"], st["n_dropped_polygons"]) == (1, 98, 0, 96)
    assert reference("one_cell")["offsets"].tolist() == [0] and len(reference("one_cell")["source"]) == 0


def test_heavy_classes_and_the_513_gon():
    ref = reference("heavy")
    st = ref["stats"]
    assert sorted(len(m) for m in ref["classes"]) == [13, 257, 300] and (st["n_cells"], st["max_cell"]) == (3, 300)
    assert ref["indices"].tolist() == [0, 300, 500] and ref["source"].tolist() == [0]
    assert (st["n_dropped_polygons"], st["n_duplicate_polygons"], st["n_folded"]) == (0, 57, 0)


def test_nearest_ties_go_to_the_smaller_id():
    v = soups()["ties"][0]
    near = reference("ties", "nearest")
    assert near["map"].tolist() == [0, 0, 0, 0, 4, 4, 4, 4, 8, 8]
    assert near["positions"][0:4].tobytes() == np.tile(v[2], (4, 1)).tobytes()  # 2 and 3 tie
    assert near["positions"][4:8].tobytes() == np.tile(v[4], (4, 1)).tobytes()  # 4 and 5 tie
    pick = near["positions"][8]
    assert pick.tobytes() in (v[8].tobytes(), v[9].tobytes()) and near["positions"][9].tobytes() == pick.tobytes()


@pytest.mark.parametrize("name", list(DUPLICATES))
def test_duplicates_by_the_smallest_rotation(name):
    st = reference(name)["stats"]
    assert (st["n_polygons"], st["n_dropped_polygons"], st["n_duplicate_polygons"], st["n_folded"],
            st["n_pinched"]) == DUPLICATES[name][1], name


def test_canonical_forms():
    assert canonical([5, 2, 9]) == (2, 9, 5) and canonical([1, 2, 1, 3]) == canonical([1, 3, 1, 2]) == (1, 2, 1, 3)
    assert canonical([0, 1, 2, 3]) != canonical([0, 2, 1, 3]) and canonical([3, 1, 2, 1]) == (1, 2, 1, 3)
    assert canonical([2, 0, 1][::-1]) == (0, 2, 1)


def test_runs_of_duplicates_and_none():
    same, distinct = reference("same_1000"), reference("distinct_4096")
    assert (same["stats"]["n_polygons"], same["stats"]["n_duplicate_polygons"]) == (1, 999)
    assert same["source"].tolist() == [0]
    st = distinct["stats"]
    assert (st["n_polygons"], st["n_duplicate_polygons"], st["n_cells"]) == (4096, 0, 64)
    assert np.array_equal(distinct["indices"], soups()["distinct_4096"][2])
    assert len({canonical(t) for t in distinct["indices"].reshape(-1, 3)}) == 4096


def test_weld_s_rewrite_cases_come_out_as_weld_gives_them():
    import weld_cases
    ours, welds = reference("rewrite"), weld_cases.reference("rewrite")
    for k in ("map", "offsets", "indices", "source"):
        assert np.array_equal(ours[k], welds[k]), k
    st = ours["stats"]
    assert (st["n_dropped_polygons"], st["n_pinched"], st["n_duplicate_polygons"]) == (3, 1, 0)
    assert ours["source"].tolist() == [0, 2, 4, 5, 6, 8]


def test_an_unused_nan_is_accepted_and_a_used_one_named():
    from weld_cases import bridge
    ref = reference("bridge_unused_nan")
    assert ref["stats"]["n_used"] == 5 and np.array_equal(ref["map"], np.arange(7))
    assert np.isnan(ref["positions"][5, 0])
    v, off, idx = bridge(used_nan=True)
    with pytest.raises(ValueError, match="simplify: vertex 4 has a coordinate that is not finite"):
        simplify_ref(v, off, idx, 0.05)


def test_the_subdivided_cube():
    """The integer cube [0, 4]^3, each face 4 x 4 quads.  Its vertices' coordinates are 0 .. 4, so a
    cell of 2 gives three cells per axis (0-1, 2-3, 4): 26 cells and a closed surface of 24 quads.
    Two cells per axis -- 8 cells, 6 quads, 90 of 96 gone -- need 2 < cell <= 4 ... 2.5 here."""
    ref = reference("cube_8_cells")
    st = ref["stats"]
    assert (st["n_cells"], st["n_polygons"], st["n_indices"]) == (8, 6, 24)
    assert st["n_dropped_polygons"] + st["n_duplicate_polygons"] == 90
    assert (st["n_dropped_polygons"], st["n_duplicate_polygons"]) == (90, 0)  # the restatement's split
    assert report_of(simplified_soup(ref)) == (0, 0, 0, 2)
    two = reference("cube_cell_2")
    assert (two["stats"]["n_cells"], two["stats"]["n_polygons"], two["stats"]["n_dropped_polygons"]) == (26, 24, 72)
    assert report_of(simplified_soup(two)) == (0, 0, 0, 2)


@pytest.mark.parametrize("name", ["no_polygons", "nothing"])
def test_tiny(name):
    v = soups()[name][0]
    for position in ("mean", "nearest"):
        ref = reference(name, position)
        assert ref["stats"] == dict.fromkeys(STAT_KEYS, 0) and ref["offsets"].tolist() == [0]
        assert np.array_equal(ref["map"], np.arange(len(v))) and ref["positions"].tobytes() == v.tobytes()


@pytest.mark.parametrize("case", FULL)
def test_the_stored_surfaces_give_the_table(case):
    data = surface(case)
    for cell in CELLS:
        want_stats, want_report = TABLE[case][cell]
        for position in ("mean", "nearest"):
            ref = reference(case, position, data, cell)
            assert ints(ref) == want_stats, (case, cell, position)
            assert report_of(simplified_soup(ref)) == want_report, (case, cell, position)
            assert 0 < ref["stats"]["max_shift"] and within_bound(ref, cell)
            if position == "mean":
                for mem in ref["classes"]:
                    assert ref["positions"][mem[0]].tobytes() == fsum_mean(data[0], mem).tobytes()


def test_simplify_flag_rules(capsys):
    import tropical.stanford.train as tr
    a = tr.parse_args(["--simplify", "0.05"])
    assert a.simplify == 0.05 and a.simplify_position == "mean" and a.components and a.polygons
    a = tr.parse_args(["--weld", "1e-3", "--simplify", "0.1", "--simplify-position", "nearest", "--keep-largest", "1"])
    assert (a.weld, a.simplify, a.simplify_position, a.keep_largest) == (1e-3, 0.1, "nearest", 1)
    d = tr.parse_args([])
    assert d.simplify is None and d.mesh_cell is None and not d.components and not d.polygons
    for bad in ("0", "-0.05", "nan", "inf", "1e-60", "1e60", "fine"):
        with pytest.raises(SystemExit):
            tr.parse_args(["--simplify", bad])
        assert "--simplify" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        tr.parse_args(["--simplify", "0.1", "--simplify-position", "median"])
    assert "--simplify-position" in capsys.readouterr().err
    a = tr.parse_args(["--mesh", "scan.ply", "--mesh-cell", "0.01"])
    assert a.mesh_cell == 0.01 and not a.polygons
    for bad in (["--mesh", "scan.ply", "--mesh-cell", "0"], ["--mesh-cell", "0.01"]):
        with pytest.raises(SystemExit):
            tr.parse_args(bad)
        assert "--mesh-cell" in capsys.readouterr().err


def test_simplify_refuses_bad_arguments_on_the_host():
    from tropical.utils.mesh import PolygonMesh
    from tropical.utils.simplify import cluster_triangles, cluster_vertices, simplify
    v, off, idx, _ = soups()["heavy"]
    for position in ("first", "median", 0):
        with pytest.raises(ValueError, match="position"):
            cluster_vertices(v, off, idx, 0.1, position=position)
        with pytest.raises(ValueError, match="position"):
            simplify(PolygonMesh(v, off, idx), 0.1, position=position)
    for bad in (0, 0.0, -1.0, float("nan"), float("inf"), 1e-60, 1e60, "0.1", None, True):
        with pytest.raises(ValueError, match="cell"):
            cluster_vertices(v, off, idx, bad)
        with pytest.raises(ValueError, match="cell"):
            simplify(PolygonMesh(v, off, idx), bad)
        with pytest.raises(ValueError, match="cell"):
            cluster_triangles(v, np.zeros((1, 3), np.int64), bad)
