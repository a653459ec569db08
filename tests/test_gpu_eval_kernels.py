"""GPU: the evaluation and training-data kernels at their edges, each against
a float64 reference of the same operation (eval_cases.py; the inputs'
conditions are checked on the CPU by test_eval_cases_host.py).

- Marching cubes (csrc/evaluate.hip tnp_mc_count / tnp_mc_emit) equals
  oracle/marching_cubes.py bitwise on non-cubic volumes without a border, on
  all 256 corner cases, at other iso levels, on samples exactly on the level
  and on volumes that mesh to nothing; the Python wrapper's conversions.
- The ray caster (tnp_raycaster_*) equals a brute-force Moller-Trumbore on
  rays from inside and outside the grid, axis-parallel and signed-zero
  directions, non-unit directions, rays that miss the box, a mesh far from the
  origin, meshes scaled by 1e-3, 1e-5 and 1e3, and thin, flat, single-triangle
  and empty meshes.  Rays the float64 classification cannot decide are left
  out of the equality checks but not of the soundness checks.
- Nearest neighbours (tnp_nn_min_dist) equal a float64 all-pairs minimum below
  one tile, at exact multiples of the block and the tile, and one past them.
- The mesh signed distance (csrc/train.hip k_mesh_sd) equals
  oracle.train.signed_distance with one partial tile, two tiles per chunk and
  a partial last one, on all seven Voronoi regions of a triangle, on flipped,
  open and degenerate meshes.

PyMCubes / cubvh / sklearn (the reference's helpers) are absent here: parity
with them is unpinned; these tests pin the kernels to restatements of the
same formulas.  Every test prints the figures it asserts on."""
import numpy as np
import pytest
import torch

import eval_cases as ec

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------
# marching cubes
# ---------------------------------------------------------------------------
def _mc(vol, iso, cuda):
    from tropical.utils.marching_cubes import marching_cubes_torch
    V, F = marching_cubes_torch(torch.from_numpy(np.ascontiguousarray(vol)).to(cuda), iso)
    assert V.dtype == torch.float64 and F.dtype == torch.int64
    return V.cpu().numpy(), F.cpu().numpy()


def _assert_mc_equal(vol, iso, cuda):
    V, F = _mc(vol, iso, cuda)
    rV, rF = ec.mc_reference(vol, iso)
    np.testing.assert_array_equal(V, rV)
    np.testing.assert_array_equal(F, rF)
    return V, F


@pytest.mark.parametrize("shape", ec.MC_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_mc_non_cubic_volume(cuda, shape):
    _assert_mc_equal(ec.mc_noise_volume(shape), 0.0, cuda)


def test_mc_all_256_corner_cases(cuda):
    for case in range(256):
        _, F = _assert_mc_equal(ec.mc_corner_case(case), 0.0, cuda)
        assert len(F) == ec.mc_table_count(case), case
    _assert_mc_equal(ec.mc_case_strip(), 0.0, cuda)


@pytest.mark.parametrize("iso", ec.MC_ISOS)
def test_mc_other_iso_levels(cuda, iso):
    _assert_mc_equal(ec.mc_noise_volume(ec.MC_ISO_SHAPE), iso, cuda)


def test_mc_samples_exactly_on_the_level(cuda):
    V, F = _assert_mc_equal(ec.mc_on_level_volume(), 0.0, cuda)
    n_deg, twins = ec.degenerate_have_twin_vertices(V, F)
    print(f"on-level volume: {len(F)} triangles, {n_deg} degenerate")
    assert n_deg > 0 and twins


@pytest.mark.parametrize("name,vol,iso", ec.mc_empty_volumes(), ids=[c[0] for c in ec.mc_empty_volumes()])
def test_mc_empty_result(cuda, name, vol, iso):
    from tropical.utils.marching_cubes import marching_cubes_torch
    V, F = marching_cubes_torch(torch.from_numpy(vol).to(cuda), iso)
    assert tuple(V.shape) == (0, 3) and V.dtype == torch.float64
    assert tuple(F.shape) == (0, 3) and F.dtype == torch.int64


def test_mc_wrapper(cuda):
    from tropical.utils.marching_cubes import marching_cubes, marching_cubes_torch
    vol = ec.mc_noise_volume((7, 3, 5))
    t = torch.from_numpy(vol).to(cuda)
    # a transposed view against its contiguous copy
    view = t.permute(2, 0, 1)
    assert not view.is_contiguous()
    Vv, Fv = marching_cubes_torch(view, 0.0)
    Vc, Fc = marching_cubes_torch(view.contiguous(), 0.0)
    assert torch.equal(Vv, Vc) and torch.equal(Fv, Fc)
    rV, rF = ec.mc_reference(np.ascontiguousarray(vol.transpose(2, 0, 1)), 0.0)
    np.testing.assert_array_equal(Vv.cpu().numpy(), rV)
    np.testing.assert_array_equal(Fv.cpu().numpy(), rF)
    # float64 samples against their float32 cast
    t64 = torch.from_numpy(np.random.RandomState(5).randn(5, 4, 6)).to(cuda)
    V64, F64 = marching_cubes_torch(t64, 0.1)
    V32, F32 = marching_cubes_torch(t64.float(), 0.1)
    assert t64.dtype == torch.float64 and torch.equal(V64, V32) and torch.equal(F64, F32) and len(F64) > 0
    # numpy in, numpy out
    V, F = marching_cubes(vol, 0.0)
    assert isinstance(V, np.ndarray) and V.dtype == np.float64 and isinstance(F, np.ndarray) and F.dtype == np.int64
    rV, rF = ec.mc_reference(vol, 0.0)
    np.testing.assert_array_equal(V, rV)
    np.testing.assert_array_equal(F, rF)
    # an extent of 1 is refused before any launch
    for shape in ((1, 4, 4), (4, 1, 4), (4, 4, 1)):
        with pytest.raises(RuntimeError):
            marching_cubes_torch(torch.zeros(shape, device=cuda), 0.0)


# ---------------------------------------------------------------------------
# ray caster
# ---------------------------------------------------------------------------
def _cast(fam):
    from tropical.utils.chamfer_distance import RayCaster
    pos, fid, depth = RayCaster(fam.V, fam.F).ray_trace(torch.from_numpy(fam.o), torch.from_numpy(fam.d))
    assert fid.dtype == torch.int64
    return pos.cpu().numpy(), fid.cpu().numpy(), depth.cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("name", ec.RAY_FAMILIES)
def test_ray_family(cuda, name):
    """Clear rays: the same hit mask, depth and (where the next surface is
    far enough behind) face as the float64 brute force.  All rays: whatever
    is reported is a real hit of that face, not behind the nearest clear hit,
    and a miss is (-1, 0).

    Two families failed on the kernel as it was: with ray_tri's absolute
    `|det| < 1e-12` the mesh scaled by 1e-5 lost 7 of 493 hits and 69 rays
    reported a surface behind, and the planar mesh lay outside its own grid,
    so 9 of 500 grazing rays missed it."""
    fam = ec.ray_family(name)
    pos, f, depth = _cast(fam)
    clear, ref_hit = ~fam.excluded, fam.f1 >= 0
    hit = f >= 0
    both = clear & ref_hit & hit
    with np.errstate(invalid="ignore"):  # inf - inf where there is no reference hit
        tol = ec.ray_tol(fam, fam.t1)
        sure = both & (fam.t2 - fam.t1 > 2 * tol)
    err = np.abs(depth[both] - fam.t1[both])
    rel = (err / tol[both]).max() if both.any() else 0.0
    # soundness figures, on the base geometry (depths carried to the family's scale)
    u, v, w, t = ec.ray_face_hit(fam.V0, fam.F, fam.o0, fam.d, np.where(hit, f, 0)) if len(fam.F) else (np.zeros(0),) * 4
    bary = np.minimum(np.minimum(u, v), w)[hit] if hit.any() else np.zeros(0)
    print(f"{name}: {len(f)} rays, {int(fam.excluded.sum())} excluded, {int(ref_hit.sum())} reference hits, "
          f"{int(hit.sum())} kernel hits, mask mismatches on clear rays {int((hit != ref_hit)[clear].sum())}, "
          f"worst depth error {err.max() if both.any() else 0.0:.3e} (= {rel:.3f} of the tolerance, L = {fam.L:g}), "
          f"face mismatches {int((f != fam.f1)[sure].sum())} of {int(sure.sum())}, "
          f"lowest barycentric coordinate of a reported face {bary.min() if len(bary) else 0.0:.3e}")
    # clear rays
    assert (hit == ref_hit)[clear].all()
    assert (err <= tol[both]).all()
    assert (f[sure] == fam.f1[sure]).all()
    # all rays
    assert (f[~hit] == -1).all() and (depth[~hit] == 0).all()
    if hit.any():
        assert (bary >= -ec.RAY_BAND).all()
        t_face = t[hit] * fam.scale
        assert (np.abs(depth[hit] - t_face) <= ec.ray_tol(fam, t_face)).all()
        assert (depth[hit] <= fam.t1[hit] + ec.ray_tol(fam, fam.t1[hit])).all()
        want = fam.o.astype(np.float64) + fam.d.astype(np.float64) * depth[:, None]
        np.testing.assert_allclose(pos[hit], want[hit], rtol=1e-6, atol=1e-6 * fam.L)
    assert np.array_equal(pos[~hit], fam.o[~hit])


def test_ray_empty_mesh_misses_everything(cuda):
    from tropical.utils.chamfer_distance import RayCaster
    V, F = ec.ray_mesh("empty")
    fam = ec.ray_family("outside")
    _, f, depth = RayCaster(V, F).ray_trace(fam.o, fam.d)
    assert (f == -1).all() and (depth == 0).all()


def test_sample_surface_from_rays_with_normals(cuda):
    from tropical.utils.chamfer_distance import sample_surface_from_rays
    from tropical.utils.mesh import Mesh
    # face 0 in the plane z = 0, face 1 tilted; neither is unit-sized
    V = np.array([[0, 0, 0], [2e-4, 0, 0], [0, 2e-4, 0], [1, 0, 0], [1, 1, 0.5], [0, 1, 0.5]], np.float64)
    F = np.array([[0, 1, 2], [3, 4, 5]])
    mesh = Mesh(V, F)
    o = np.array([[5e-5, 5e-5, 1], [0.7, 0.6, 1], [3, 3, 1], [0.8, 0.7, 1], [-1, -1, 1]], np.float32)
    d = np.tile(np.array([[0, 0, -1]], np.float32), (5, 1))
    pos, normals, mask = sample_surface_from_rays(torch.from_numpy(o), torch.from_numpy(d), mesh, return_normal=True)
    assert mask.tolist() == [True, True, False, True, False]
    assert pos.shape == (3, 3)
    np.testing.assert_allclose(pos[:, :2], o[mask][:, :2], atol=1e-6)
    np.testing.assert_allclose(pos[0, 2], 0.0, atol=1e-6)
    c = np.cross(V[F[:, 1]] - V[F[:, 0]], V[F[:, 2]] - V[F[:, 0]])
    want = c / (np.linalg.norm(c, axis=-1, keepdims=True) + 1e-9)
    # |c0| = 4e-8: the 1e-9 shortens face 0's normal by 2.4 %, face 1's by 1e-9
    assert abs(np.linalg.norm(want[0]) - 4e-8 / 4.1e-8) < 1e-9
    np.testing.assert_allclose(normals, want[[0, 1, 0, 1, 0]], rtol=1e-12, atol=0)
    assert sample_surface_from_rays(torch.from_numpy(o), torch.from_numpy(d), mesh).shape == (3, 3)


# ---------------------------------------------------------------------------
# nearest neighbour
# ---------------------------------------------------------------------------
def _assert_nn(a, b, what):
    from tropical.utils.chamfer_distance import nn_min_dist
    got = nn_min_dist(a, b).cpu().numpy().astype(np.float64)
    ref = ec.nn_reference(a, b)
    L = ec.nn_length(a, b)
    tol = ec.NN_RTOL * ref + ec.NN_ATOL * L
    err = np.abs(got - ref)
    print(f"nn {what}: worst error {err.max():.3e} (= {(err / tol).max():.3f} of the tolerance, L = {L:g})")
    assert got.shape == ref.shape and (err <= tol).all()
    return got


@pytest.mark.parametrize("na,nb", ec.NN_SIZES)
def test_nn_sizes(cuda, na, nb):
    _assert_nn(*ec.nn_clouds(na, nb), f"{na} x {nb}")


def test_nn_special_clouds(cuda):
    got = _assert_nn(*ec.nn_case("own_rows"), "own rows")
    assert (got == 0.0).all()
    _assert_nn(*ec.nn_case("shift100"), "shifted by 100")
    _assert_nn(*ec.nn_case("outlier"), "one far outlier")


def test_nn_empty_sides(cuda):
    from tropical.utils.chamfer_distance import nn_min_dist
    a, b = ec.nn_clouds(7, 9)
    out = nn_min_dist(np.zeros((0, 3), np.float32), b)
    assert tuple(out.shape) == (0,) and out.dtype == torch.float32
    with pytest.raises(RuntimeError):
        nn_min_dist(a, np.zeros((0, 3), np.float32))


def test_chamfer_is_symmetric_and_zero_on_itself(cuda):
    from tropical.utils.chamfer_distance import chamfer_distance
    a, b = ec.nn_clouds(257, 1025)
    ab, ba = chamfer_distance(a, b), chamfer_distance(b, a)
    ref = (ec.nn_reference(a, b).mean() + ec.nn_reference(b, a).mean()) / 2
    print(f"chamfer: {ab!r} / {ba!r}, float64 {ref!r}")
    assert ab == ba and abs(ab - ref) < 1e-6
    assert chamfer_distance(a, a) == 0.0


# ---------------------------------------------------------------------------
# mesh signed distance
# ---------------------------------------------------------------------------
def _sd(mesh, P, cuda):
    from tropical.stanford.sdf_train import mesh_signed_distance
    V, F = ec.sd_mesh(mesh)
    return mesh_signed_distance(torch.from_numpy(V).to(cuda), torch.from_numpy(F).to(cuda),
                                torch.from_numpy(P).to(cuda)).cpu().numpy().astype(np.float64)


def _assert_sd(got, ref, wind, what, sign_ok=None):
    assert got.shape == ref.shape and np.isfinite(got).all()
    scale = np.maximum(1.0, np.abs(ref))
    err = np.abs(np.abs(got) - np.abs(ref)) / scale
    decided = (np.abs(ref) > ec.SD_SIGN_MIN) & (np.abs(np.abs(wind) - 0.5) > ec.SD_WIND_GAP)
    if sign_ok is not None:
        decided &= sign_ok
    wrong = int((np.sign(got) != np.sign(ref))[decided].sum())
    print(f"sd {what}: {len(got)} points, worst |d| error / max(1, |ref|) {err.max():.3e}, "
          f"signs compared {int(decided.sum())}, wrong {wrong}")
    assert (err <= ec.SD_MAG_TOL).all()
    assert wrong == 0


@pytest.mark.parametrize("mesh", ["sphere", "flipped", "sphere_degenerate"])
def test_sd_all_points(cuda, mesh):
    """Random, on-feature, off-feature and far points: all seven regions of
    tri_dist2 decide a point's distance (test_eval_cases_host.py)."""
    P = ec.sd_points("all")
    ref, wind = ec.sd_reference(mesh, "all")
    _assert_sd(_sd(mesh, P, cuda), ref, wind, mesh, ec.sd_sign_ok_mask(len(P)))


def test_sd_flipped_sphere_agrees_with_the_sphere(cuda):
    P = ec.sd_points("all")
    a, b = _sd("sphere", P, cuda), _sd("flipped", P, cuda)
    ref, wind = ec.sd_reference("sphere", "all")
    ok = ec.sd_sign_ok_mask(len(P)) & (np.abs(ref) > ec.SD_SIGN_MIN) & (np.abs(np.abs(wind) - 0.5) > ec.SD_WIND_GAP)
    err = np.abs(np.abs(a) - np.abs(b)) / np.maximum(1.0, np.abs(ref))
    print(f"sd flipped against unflipped: worst |d| difference {err.max():.3e}")
    assert (err <= 2 * ec.SD_MAG_TOL).all() and (np.sign(a) == np.sign(b))[ok].all()


@pytest.mark.parametrize("mesh", ["sphere80", "hemisphere", "triangle"])
def test_sd_random_points(cuda, mesh):
    ref, wind = ec.sd_reference(mesh, "random")
    _assert_sd(_sd(mesh, ec.sd_points("random"), cuda), ref, wind, mesh)


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_sd_point_counts_around_one_block(cuda, n):
    ref, wind = ec.sd_reference("sphere", n)
    _assert_sd(_sd("sphere", ec.sd_points("random")[:n], cuda), ref[:n], wind[:n], f"sphere, n = {n}")


def test_sd_two_tiles_per_chunk_and_a_partial_last(cuda):
    """1325 faces x 200 000 points: a 782 x 3 grid, chunks of 512 / 512 / 301
    triangles.  The kernel runs on every point, the oracle on the first and
    last block and every 101st point between."""
    P, idx = ec.sd_big_points()
    assert ec.sd_launch_shape(len(P), len(ec.sd_mesh("sphere1325")[1])) == (782, 3, [512, 512, 301])
    got = _sd("sphere1325", P, cuda)
    assert np.isfinite(got).all()
    ref, wind = ec.sd_reference("sphere1325", "big")
    _assert_sd(got[idx], ref, wind, "sphere1325")
