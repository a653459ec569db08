"""CPU: the inputs of test_gpu_eval_kernels.py (eval_cases.py) satisfy the
conditions its assertions rest on.  Only the float64 references run here,
never the kernels: the 256 case volumes hit their cases, the on-level volume
makes the degenerate triangles it is meant to, at most 1 % of a ray family is
excluded, every Voronoi region of a triangle is the nearest feature of enough
points, and the signed-distance launches have the stated shapes."""
import numpy as np
import pytest

import eval_cases as ec


# ---------------------------------------------------------------------------
# marching cubes
# ---------------------------------------------------------------------------
def test_mc_shapes_have_three_distinct_extents_or_are_minimal():
    for s in ec.MC_SHAPES:
        assert len(set(s)) == 3 or s == (2, 2, 2)
        vol = ec.mc_noise_volume(s)
        V, F = ec.mc_reference(vol, 0.0)
        assert vol.shape == s and len(F) > 0
        if min(s) > 2:  # the surface reaches the volume's faces: no outside border
            on_face = ((V == 0) | (V == np.array(s) - 1.0)).any(1)
            assert on_face.any()


def test_mc_case_volumes_hit_every_case():
    from tropical.utils.mc_table import case_table
    total = 0
    for c in range(256):
        vol = ec.mc_corner_case(c)
        inside = vol < 0
        got = sum(int(inside[x, y, z]) << i
                  for i, (x, y, z) in enumerate([(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0),
                                                 (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)]))
        assert got == c and set(np.unique(vol)) <= {-1.0, 1.0}
        V, F = ec.mc_reference(vol, 0.0)
        assert len(F) == ec.mc_table_count(c)
        total += len(F)
    assert total == int((case_table() >= 0).sum()) // 3
    strip = ec.mc_case_strip()
    assert strip.shape == (512, 2, 2)
    for c in (0, 1, 77, 255):
        np.testing.assert_array_equal(strip[2 * c:2 * c + 2], ec.mc_corner_case(c))


def test_mc_iso_levels_cut_the_noise_volume():
    vol = ec.mc_noise_volume(ec.MC_ISO_SHAPE)
    counts = {iso: len(ec.mc_reference(vol, iso)[1]) for iso in [0.0] + ec.MC_ISOS}
    assert all(n > 0 for n in counts.values()) and len(set(counts.values())) > 1


def test_mc_on_level_volume_makes_twin_vertex_triangles():
    vol = ec.mc_on_level_volume()
    assert set(np.unique(vol)) == {-1.0, 0.0, 1.0}
    assert (np.signbit(vol) & (vol == 0)).any() and (~np.signbit(vol) & (vol == 0)).any()
    V, F = ec.mc_reference(vol, 0.0)
    frac = V - np.floor(V)
    assert np.isin(frac, [0.0, 0.5]).all()  # t is exactly 0, 1/2 or 1
    n_deg, twins = ec.degenerate_have_twin_vertices(V, F)
    assert n_deg >= 20 and twins


def test_mc_empty_volumes_are_empty():
    for _, vol, iso in ec.mc_empty_volumes():
        V, F = ec.mc_reference(vol, iso)
        assert V.shape == (0, 3) and F.shape == (0, 3)


# ---------------------------------------------------------------------------
# ray caster
# ---------------------------------------------------------------------------
def test_ray_meshes():
    V, F = ec.ray_mesh("noise")
    assert V.dtype == np.float32 and np.abs(V).max() <= 1 and (len(V), len(F)) == (1680, 3488)
    Vt, Ft = ec.ray_mesh("thin")
    assert np.array_equal(Ft, F) and np.abs(Vt[:, 2]).max() <= 0.01 + 1e-9
    Vp, Fp = ec.ray_mesh("planar")
    assert Fp.shape == (128, 3) and np.ptp(Vp[:, 2]) == 0 and Vp[0, 2] == 0.25
    assert ec.ray_mesh("triangle")[1].shape == (1, 3) and ec.ray_mesh("empty")[1].shape == (0, 3)


@pytest.mark.parametrize("name", ec.RAY_FAMILIES)
def test_ray_family_excludes_at_most_one_percent(name):
    fam = ec.ray_family(name)
    assert 500 <= len(fam.o) <= 2000 and fam.o.dtype == fam.d.dtype == np.float32
    assert fam.excluded.mean() <= 0.01, (name, int(fam.excluded.sum()))
    hit = fam.f1 >= 0
    if name == "miss_box":
        assert not hit.any()
        # the rays miss the box [-1, 1]^3 itself, not only the mesh
        o, d = fam.o.astype(np.float64), fam.d.astype(np.float64)
        with np.errstate(divide="ignore"):
            ta, tb = (-1 - o) / d, (1 - o) / d
        t0 = np.maximum(np.minimum(ta, tb).max(1), 0)
        assert (t0 > np.maximum(ta, tb).min(1)).all()
    else:
        assert hit.mean() > 0.1


def test_ray_family_directions_are_what_they_say():
    d = ec.ray_family("axis").d
    assert ((d == 0).sum(1) == 2).all() and (np.abs(d).sum(1) == 1).all()
    o = ec.ray_family("axis").o
    assert (np.abs(o).max(1) == 2).all()  # outside the box
    d = ec.ray_family("signed_zero").d
    small = np.abs(d) <= 1e-30
    assert (small.sum(1) == 1).all()
    s = d[small]
    assert (np.signbit(s) & (s == 0)).any() and (~np.signbit(s) & (s == 0)).any()
    assert (s == np.float32(1e-30)).any() and (s == np.float32(-1e-30)).any()
    n = np.linalg.norm(ec.ray_family("nonunit").d.astype(np.float64), axis=1)
    assert np.allclose(n[0::2], 0.01, rtol=1e-6) and np.allclose(n[1::2], 100, rtol=1e-6)
    assert (np.abs(ec.ray_family("planar_grazing").d[:, 2]) <= 0.02).all()
    assert np.abs(ec.ray_family("shift100").V - 100).max() <= 1.0
    for name, s in (("scale1e-3", 1e-3), ("scale1e-5", 1e-5), ("scale1e3", 1e3)):
        fam = ec.ray_family(name)
        assert fam.L == s and np.abs(fam.V).max() <= s * (1 + 1e-6)


def test_ray_classification_on_a_known_triangle():
    V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    F = np.array([[0, 1, 2]])
    o = np.array([[0.25, 0.25, 1], [0.5, 0.5, 1], [2, 2, 1], [0.25, 0.25, -1], [0.25, 0.25, 0]], np.float32)
    d = np.tile(np.array([[0, 0, -1]], np.float32), (5, 1))
    r = ec.classify_rays(V, F, o, d)
    # interior hit; on the hypotenuse; beside; behind; starting on the surface (t = 0)
    assert r.excluded.tolist() == [False, True, False, False, True]
    assert r.f1.tolist() == [0, -1, -1, -1, -1] and r.t1[0] == 1.0 and np.isinf(r.t2).all()


# ---------------------------------------------------------------------------
# nearest neighbour
# ---------------------------------------------------------------------------
def test_nn_cases():
    assert (1, 1025) in ec.NN_SIZES and (256, 1024) in ec.NN_SIZES and (1000, 2049) in ec.NN_SIZES
    a, b = ec.nn_case("own_rows")
    assert (ec.nn_reference(a, b) == 0).all()
    a, b = ec.nn_case("shift100")
    assert a.min() >= 100 and ec.nn_length(a, b) > 100
    a, b = ec.nn_case("outlier")
    assert np.abs(b).max() == 50 and ec.nn_reference(a, b).max() < 1


# ---------------------------------------------------------------------------
# mesh signed distance
# ---------------------------------------------------------------------------
def test_sd_launch_shapes():
    assert len(ec.sd_mesh("sphere80")[1]) == 80 and ec.sd_launch_shape(len(ec.sd_points("random")), 80)[1:] == (1, [80])
    V, F = ec.sd_mesh("sphere1325")
    P, idx = ec.sd_big_points()
    assert len(F) == 1325 and len(P) == 200000
    assert ec.sd_launch_shape(200000, 1325) == (782, 3, [512, 512, 301])
    assert idx[0] == 0 and idx[-1] == 199999 and len(np.unique(idx)) == len(idx)
    assert set(range(256)) <= set(idx.tolist()) and set(range(200000 - 256, 200000)) <= set(idx.tolist())
    for n in (1, 255, 256, 257):
        assert ec.sd_launch_shape(n, 320) == ((n + 255) // 256, 2, [256, 64])
    n_all = len(ec.sd_points("all"))
    assert ec.sd_launch_shape(n_all, 365)[1:] == (2, [256, 109])


def test_sd_degenerate_triangles_lie_on_the_mesh_edges():
    V0, F0 = ec.sd_mesh("sphere")
    V, F = ec.sd_mesh("sphere_degenerate")
    extra = F[len(F0):]
    assert len(extra) == 45 and (F[:len(F0)] == F0).all() and (V[:len(V0)] == V0).all()
    edges = {tuple(e) for e in ec._edges(F0).tolist()}
    patterns = set()
    for t in extra.tolist():
        old = sorted({i for i in t if i < len(V0)})
        new = [i for i in t if i >= len(V0)]
        assert len(old) == 1 or tuple(old) in edges
        if new:  # the inserted point lies on the edge, up to float32 rounding
            a, b = V[old[0]].astype(np.float64), V[old[1]].astype(np.float64)
            m = V[new[0]].astype(np.float64)
            assert np.linalg.norm(np.cross(m - a, b - a)) / np.linalg.norm(b - a) < 1e-7
            patterns.add("amb")
        else:
            patterns.add("".join("ab"[old.index(i)] for i in t))
    assert patterns == {"aab", "aba", "baa", "abb", "bab", "bba", "aaa", "amb"}
    tri = V.astype(np.float64)[extra]
    area = np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    assert area.max() < 1e-7


def test_sd_every_region_is_nearest_for_twenty_points():
    V, F = ec.sd_mesh("sphere")
    reg = ec.sd_regions(V, F, ec.sd_points("all"))
    counts = np.bincount(reg, minlength=7)
    assert (reg >= 0).all() and (counts >= 20).all(), counts.tolist()


def test_sd_reference_on_the_meshes():
    P = ec.sd_points("all")
    sign_ok = ec.sd_sign_ok_mask(len(P))
    ref, wind = ec.sd_reference("sphere", "all")
    assert np.isfinite(ref).all()
    r = np.linalg.norm(P.astype(np.float64), axis=1)
    assert (ref[r < 0.97 * ec.SD_RADIUS] > 0).all() and (ref[r > 1.001 * ec.SD_RADIUS] < 0).all()
    assert np.abs(ref).max() > 25                    # the far points
    decided = sign_ok & (np.abs(ref) > ec.SD_SIGN_MIN) & (np.abs(np.abs(wind) - 0.5) > ec.SD_WIND_GAP)
    assert decided.sum() > 0.9 * sign_ok.sum()
    # flipped: same distances, winding number negated, same sign
    ref_f, wind_f = ec.sd_reference("flipped", "all")
    assert np.allclose(ref_f, ref, rtol=0, atol=1e-12) and np.allclose(wind_f[sign_ok], -wind[sign_ok], atol=1e-12)
    # degenerate triangles on the sphere's own edges change nothing
    ref_d, wind_d = ec.sd_reference("sphere_degenerate", "all")
    assert np.isfinite(ref_d).all() and np.allclose(np.abs(ref_d), np.abs(ref), rtol=0, atol=1e-7)
    # the open hemisphere has fractional winding numbers on both sides of 1/2
    ref_h, wind_h = ec.sd_reference("hemisphere", "random")
    assert (np.abs(wind_h) > 0.55).any() and (np.abs(wind_h) < 0.45).any()
    # a single triangle never encloses anything
    ref_t, wind_t = ec.sd_reference("triangle", "random")
    assert (np.abs(wind_t) < 0.5).all() and (ref_t <= 0).all()
