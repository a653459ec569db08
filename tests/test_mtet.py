"""Marching tetrahedra (tropical.utils.mtet, csrc/mtet.hip) and the evaluate
CLI (tropical.stanford.evaluate) against the joined reference's recorded
outputs (tests/golden/mtet_cases.npz, written by make_mtet_golden.py)."""
import contextlib
import io
import os

import numpy as np
import pytest
import torch

from golden_io import GOLDEN, sha

CASES = ["sphere12", "noise10", "soup", "sphere40", "allpos"]
EDGES = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(GOLDEN, "mtet_cases.npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def _grid_points(n):
    s = np.linspace(-1.2, 1.2, n)
    return np.stack(np.meshgrid(s, s, s, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)


def _sphere_sdf(p):
    q = p.astype(np.float64)
    return (np.sqrt((q * q).sum(-1)) - 0.8).astype(np.float32)


def _inputs(gold, name):
    """(vertices fp32 [N, 3], tets int64 [T, 4], sdf fp32 [N]) of a case."""
    if f"{name}:vertices" in gold:
        return gold[f"{name}:vertices"], gold[f"{name}:tets"].astype(np.int64), gold[f"{name}:sdf"]
    import tropical.stanford.evaluate as ev
    assert name == "sphere40"
    v = _grid_points(40)
    tets = ev.generate_tetrahedra_indices(40).numpy()
    sdf = _sphere_sdf(v)
    assert sha(v, sdf, tets) == str(gold[f"{name}:in_sha"])  # the generator's inputs
    return v, tets, sdf


def _check(gold, name, tets_in, verts, faces, tet_idx, tets_after):
    nT, nV, nF = (int(x) for x in gold[f"{name}:counts"])
    assert verts.shape == (nV, 3) and verts.dtype == np.float32
    assert faces.shape == (nF, 3) and faces.dtype == np.int64
    assert tet_idx.shape == (nF,) and tet_idx.dtype == np.int64
    assert tets_after.shape == (nT, 4)
    if f"{name}:verts" in gold:
        assert np.array_equal(verts.view(np.uint32), gold[f"{name}:verts"].view(np.uint32))
        assert np.array_equal(faces, gold[f"{name}:faces"])
        assert np.array_equal(tet_idx, gold[f"{name}:tet_idx"])
        flips = np.unpackbits(gold[f"{name}:flips"])[:nT].astype(bool)
        want = tets_in.copy()
        want[flips, 0], want[flips, 1] = tets_in[flips, 1], tets_in[flips, 0]
        assert np.array_equal(tets_after, want)
    else:
        assert sha(verts) == str(gold[f"{name}:verts_sha"])
        assert sha(faces) == str(gold[f"{name}:faces_sha"])
        assert sha(tet_idx) == str(gold[f"{name}:tet_idx_sha"])
        assert sha(tets_after) == str(gold[f"{name}:tets_after_sha"])


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
def test_modules_import_and_cli_defaults():
    import tropical.stanford.evaluate as ev
    import tropical.utils.mtet as mt
    assert callable(mt.marching_tetrahedras) and callable(ev.main)
    a = ev.parse_args([])
    assert (a.dataset, a.seed, a.model_size, a.method) == ("dragon", 45, "small", "mc")
    assert (a.weights, a.out) == (None, "meshes")
    assert ev.parse_args(["-t", "mc"]).method == "mc"
    assert ev.parse_args(["-t", "mtet"]).method == "mtet"
    for bad in ("cubes", "MC", "tet", ""):
        with pytest.raises(SystemExit):
            ev.parse_args(["-t", bad])
    assert ev.GT_RES == {"small": 256, "medium": 512, "large": 512}
    assert ev.RESOLS[("mc", "small")] == [256, 16, 24, 32, 40, 48, 56, 64, 128, 192, 224]
    assert ev.RESOLS[("mtet", "medium")] == [512, 16, 32, 48, 64, 96]
    assert ev.RESOLS[("mtet", "large")] == [512, 16, 32, 48, 64, 96, 128, 192]


def test_tet_grid_is_the_references(gold):
    import tropical.stanford.evaluate as ev
    t4 = ev.generate_tetrahedra_indices(4)
    assert t4.dtype == torch.int64 and t4.device.type == "cpu"
    assert np.array_equal(t4.numpy(), gold["tets_n4"])
    assert sha(ev.generate_tetrahedra_indices(12, device="cpu").numpy()) == str(gold["tets_n12_sha"])
    assert sha(ev.generate_tetrahedra_indices(40).numpy()) == str(gold["tets_n40_sha"])


def test_cpu_tensors_are_refused(gold):
    from tropical.utils.mtet import marching_tetrahedras
    v, tets, sdf = (torch.from_numpy(x) for x in _inputs(gold, "sphere12"))
    before = tets.clone()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        marching_tetrahedras(v, tets, sdf)
    assert torch.equal(tets, before)


def test_triangle_table_uses_exactly_the_crossed_edges(gold):
    table, ntri = gold["triangle_table"], gold["num_triangles"]
    assert table.shape == (16, 6) and ntri.shape == (16,)
    for c in range(16):
        occ = [(c >> i) & 1 for i in range(4)]
        crossed = {e for e, (i, j) in enumerate(EDGES) if occ[i] != occ[j]}
        row = table[c]
        used = row[row >= 0]
        assert set(used.tolist()) == crossed
        assert len(used) == 3 * ntri[c] and (row[len(used):] == -1).all()
        assert ntri[c] == {0: 0, 1: 1, 2: 2, 3: 1, 4: 0}[sum(occ)]
        for k in range(int(ntri[c])):
            assert len(set(row[3 * k:3 * k + 3].tolist())) == 3
    # a case and its complement: the same triangles, opposite winding
    for c in (1, 2, 4, 8):
        a, b = table[c][:3].tolist(), table[15 - c][:3].tolist()
        assert sorted(a) == sorted(b)
        assert b in ([a[0], a[2], a[1]], [a[2], a[1], a[0]], [a[1], a[0], a[2]])


def test_missing_files_print_the_references_messages(tmp_path, capsys):
    import tropical.stanford.evaluate as ev
    assert ev.main(["--weights", str(tmp_path / "none.pth"), "--out", str(tmp_path)]) == 0
    assert f"Model path is not found: {tmp_path / 'none.pth'}" in capsys.readouterr().out
    w = tmp_path / "w.pth"
    w.write_bytes(b"")
    assert ev.main(["-d", "bunny", "--weights", str(w), "--out", str(tmp_path)]) == 0
    want = os.path.join(str(tmp_path), "bunny", "our_mesh_small_45.ply")
    assert f"Mesh path is not found: {want}" in capsys.readouterr().out


def test_count_vertices_near_values():
    import tropical.stanford.evaluate as ev
    v = np.array([[0.5, 0.1, 0.2], [0.3, 0.25 + 5e-5, 0.9], [0.3, 0.25 + 2e-4, 0.9], [0.0, 0.0, 1.0]])
    marks = np.array([0.0, 0.25, 0.5])
    assert ev.count_vertices_near_values(v, marks) == 3
    assert ev.count_vertices_near_values(v, marks, chunk=1) == 3
    assert ev.count_vertices_near_values(np.zeros((0, 3)), marks) == 0


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_gpu_matches_the_joined_reference(cuda, gold, name):
    from tropical.utils.mtet import marching_tetrahedras
    v_np, tets_np, sdf_np = _inputs(gold, name)
    v, sdf = torch.from_numpy(v_np).to(cuda), torch.from_numpy(sdf_np).to(cuda)
    tets = torch.from_numpy(tets_np).to(cuda)
    verts, faces, tet_idx = marching_tetrahedras(v, tets, sdf, True)
    assert verts.device == v.device and faces.device == v.device and tet_idx.device == v.device
    after = tets.cpu().numpy()
    _check(gold, name, tets_np, verts.cpu().numpy(), faces.cpu().numpy(), tet_idx.cpu().numpy(), after)
    # the flipped tets flip no more, and the result is the same
    out = marching_tetrahedras(v, tets, sdf)
    assert isinstance(out, tuple) and len(out) == 2
    assert np.array_equal(tets.cpu().numpy(), after)
    assert torch.equal(out[0].view(torch.int32), verts.view(torch.int32)) and torch.equal(out[1], faces)


@pytest.mark.gpu
def test_gpu_flips_a_strided_view_of_the_callers_tets(cuda, gold):
    from tropical.utils.mtet import marching_tetrahedras
    v_np, tets_np, sdf_np = _inputs(gold, "sphere12")
    v, sdf = torch.from_numpy(v_np).to(cuda), torch.from_numpy(sdf_np).to(cuda)
    wide = torch.full((len(tets_np), 5), -7, dtype=torch.int64, device=cuda)
    wide[:, 1:] = torch.from_numpy(tets_np).to(cuda)
    tets = wide[:, 1:]
    verts, faces, tet_idx = marching_tetrahedras(v, tets, sdf, True)
    _check(gold, "sphere12", tets_np, verts.cpu().numpy(), faces.cpu().numpy(), tet_idx.cpu().numpy(),
           wide[:, 1:].cpu().numpy())
    assert (wide[:, 0] == -7).all()


@pytest.mark.gpu
def test_gpu_index_out_of_range_raises(cuda, gold):
    from tropical.utils.mtet import marching_tetrahedras
    v_np, tets_np, sdf_np = _inputs(gold, "sphere12")
    v, sdf = torch.from_numpy(v_np).to(cuda), torch.from_numpy(sdf_np).to(cuda)
    for bad in (len(v_np), -1):
        t = tets_np.copy()
        t[len(t) // 2, 2] = bad
        with pytest.raises(IndexError):
            marching_tetrahedras(v, torch.from_numpy(t).to(cuda), sdf)
    tets = torch.from_numpy(tets_np).to(cuda)
    verts, faces, tet_idx = marching_tetrahedras(v, tets, sdf, True)
    _check(gold, "sphere12", tets_np, verts.cpu().numpy(), faces.cpu().numpy(), tet_idx.cpu().numpy(),
           tets.cpu().numpy())


def _formula(vertices, sdf, interp_v):
    a, b = interp_v[:, 0], interp_v[:, 1]
    sa, sb = sdf[a], sdf[b]
    n = -sb
    den = sa + n
    return vertices[a] * (n / den)[:, None] + vertices[b] * (sa / den)[:, None]


def _grads(v_np, sdf_np, interp_v, dtype):
    v = torch.from_numpy(v_np).to(dtype).requires_grad_(True)
    s = torch.from_numpy(sdf_np).to(dtype).requires_grad_(True)
    _formula(v, s, torch.from_numpy(interp_v)).square().sum().backward()
    return v.grad.numpy(), s.grad.numpy()


# largest error of the formula's fp32 CPU autograd against its float64
# autograd on sphere12, relative to the largest float64 gradient entry
# (measured on the CPU: d/d vertices 1.17e-7, d/d sdf 7.03e-7); the GPU's
# scatter-add sums in another order: 4x that is allowed
AUTOGRAD_REL = {"vertices": 4 * 1.17e-7, "sdf": 4 * 7.03e-7}


def _rel(g, ref):
    return float(np.abs(g.astype(np.float64) - ref).max() / np.abs(ref).max())


def test_autograd_tolerance_is_the_measured_cpu_error(gold):
    """The fp32 CPU error the GPU tolerance is 4x of: measured 1.17e-7
    (vertices) and 7.03e-7 (sdf) on sphere12."""
    v_np, _, sdf_np = _inputs(gold, "sphere12")
    iv = gold["sphere12:interp_v"].astype(np.int64)
    g32, g64 = _grads(v_np, sdf_np, iv, torch.float32), _grads(v_np, sdf_np, iv, torch.float64)
    for k, name in enumerate(("vertices", "sdf")):
        r = _rel(g32[k], g64[k])
        print(f"fp32 CPU autograd, d/d {name}: relative error {r:.3g}")
        assert 0 < r <= AUTOGRAD_REL[name]


@pytest.mark.gpu
def test_gpu_autograd_matches_float64(cuda, gold):
    """Forward with requires_grad: bitwise the kernel's vertices.  Gradients
    of verts.square().sum() against float64 CPU autograd of the same formula
    over the fixture's interp_v, within 4x the fp32 CPU autograd's own error
    (1.17e-7 for vertices, 7.03e-7 for sdf, relative to the largest entry)."""
    from tropical.utils.mtet import marching_tetrahedras
    v_np, tets_np, sdf_np = _inputs(gold, "sphere12")
    iv = gold["sphere12:interp_v"].astype(np.int64)
    v = torch.from_numpy(v_np).to(cuda).requires_grad_(True)
    sdf = torch.from_numpy(sdf_np).to(cuda).requires_grad_(True)
    verts, faces = marching_tetrahedras(v, torch.from_numpy(tets_np).to(cuda), sdf)
    assert verts.requires_grad
    assert np.array_equal(verts.detach().cpu().numpy().view(np.uint32), gold["sphere12:verts"].view(np.uint32))
    assert np.array_equal(faces.cpu().numpy(), gold["sphere12:faces"])
    verts.square().sum().backward()
    g64 = _grads(v_np, sdf_np, iv, torch.float64)
    for g, ref, name in ((v.grad, g64[0], "vertices"), (sdf.grad, g64[1], "sdf")):
        r = _rel(g.cpu().numpy(), ref)
        print(f"GPU autograd, d/d {name}: relative error {r:.3g} (allowed {AUTOGRAD_REL[name]:.3g})")
        assert r <= AUTOGRAD_REL[name]
    # without requires_grad the kernel's own vertices come back, no graph
    plain, _ = marching_tetrahedras(v.detach(), torch.from_numpy(tets_np).to(cuda), sdf.detach())
    assert not plain.requires_grad and torch.equal(plain.view(torch.int32), verts.detach().view(torch.int32))


def _rows(out):
    """{first field: [fields]} of the table lines after the header."""
    lines = out.splitlines()
    start = lines.index("#samples, #vertices, CD, AD, time")
    rows = {}
    for l in lines[start + 1:]:
        f = [x.strip() for x in l.split(",")]
        if len(f) == 5:
            rows[f[0]] = f
    return rows


@pytest.fixture(scope="module")
def trained(cuda, tmp_path_factory):
    """`train -e` on the stand-in small net with MC size 64 first: the
    weights, the mesh directory and the table it printed."""
    import tropical.stanford.train as tr
    from golden_io import load
    from helpers import product_net
    tmp = tmp_path_factory.mktemp("mtet_cli")
    net = product_net(load("small_sphere"), cuda)
    w = tmp / "bunny_sdf_small_45.pth"
    torch.save(net.state_dict(), w)
    sizes, tr.MC_SIZES = tr.MC_SIZES, [64]
    buf = io.StringIO()
    try:
        with contextlib.redirect_stdout(buf):
            assert tr.main(["-d", "bunny", "-m", "small", "-e", "--weights", str(w), "--out", str(tmp)]) == 0
    finally:
        tr.MC_SIZES = sizes
    return net, w, tmp, _rows(buf.getvalue())


@pytest.mark.gpu
@pytest.mark.parametrize("method", ["mtet", "mc"])
def test_gpu_evaluate_cli_end_to_end(trained, monkeypatch, capsys, method):
    import tropical.stanford.evaluate as ev
    import tropical.stanford.train as tr
    net, w, tmp, train_rows = trained
    monkeypatch.setitem(ev.GT_RES, "small", 64)
    monkeypatch.setitem(ev.RESOLS, (method, "small"), [64, 16, 32])
    assert ev.main(["-d", "bunny", "-m", "small", "-t", method, "--weights", str(w), "--out", str(tmp)]) == 0
    out = capsys.readouterr().out
    name = {"mtet": "Tetrahedra", "mc": "Cubes"}[method]
    assert f"Marching {name} Results:" in out and "#samples, #vertices, CD, AD, time" in out
    assert "Number of vertices near the grid marks: " in out
    rows = _rows(out)
    assert list(rows) == ["Ours", "64", "16", "32"]
    for i in (64, 16, 32):
        assert (tmp / "bunny" / f"{method}{i:03d}_mesh_small_45.ply").is_file()
    # the pseudo ground truth is marching cubes whatever the method
    assert int(rows["64"][1]) == tr.run_marching_cubes(net, 64).vertices.shape[0]
    run = ev.run_marching_tetrahedras if method == "mtet" else tr.run_marching_cubes
    for i in (16, 32):
        assert int(rows[str(i)][1]) == run(net, i).vertices.shape[0] > 0
    assert float(rows["32"][2]) < float(rows["16"][2])
    # the same rays, mesh and ground truth as train -e: the same Ours row but its time
    assert rows["Ours"][1:4] == train_rows["Ours"][1:4]
    assert rows["Ours"][4] == "-1.00"
    assert rows["64"][1:4] == train_rows["64"][1:4]
