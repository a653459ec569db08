"""GPU parity: the HIP path against the reference's golden fixtures and the
oracle (bit-exact integer outputs and vertices; the north-star tolerance for
vertex coordinates is 1e-5 abs, but the design target -- and what these
tests require -- is bitwise equality, see DESIGN.md "Bitwise contract")."""
import numpy as np
import pytest
import torch

from golden_io import cases, golden_eps, load, sha
from helpers import engine_steps, oracle_net, product_net

pytestmark = pytest.mark.gpu

VERTEX_TOL = 1e-5  # north_star: vertex coords within 1e-5 abs


def _rand_points(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, 3, generator=g) * 2 - 1


# net shapes beyond 3 layers x 16 hidden x {2,4} levels (reference Net is
# generic, model.py:19-50): 4 layers (K = 49), 32 hidden, 8 hidden x 3
# levels, 8 levels, and lattices of 4 layers x 8 hidden / 2 layers x 32
SHAPES = [n for n in ("small4l_sphere", "h32_torus", "h8l3_sphere", "lv8_rand", "synth24_l4h8", "synth20_h32")
          if n in cases()]
# K > 63 planes (two-word sign keys): 3 x 32 and 5 x 16 (K = 65), 4 x 32 (K = 97)
WIDE = [n for n in ("h32l3_rand", "h16l5_sphere", "synth16_h32l3", "synth8_h32l4") if n in cases()]


@pytest.mark.parametrize("name", ["small_sphere", "synth32", "small_rand"] + SHAPES + WIDE)
def test_forward_bitwise(cuda, name):
    d = load(name)
    net, ref = product_net(d, cuda), oracle_net(d)
    x = _rand_points(20000, 1)
    # include exact lattice points (grid-plane ties) and the box corners
    mk = torch.as_tensor(d["marks"])
    lat = torch.stack(torch.meshgrid(mk[::3], mk[::5], mk[::7], indexing="ij"), -1).reshape(-1, 3) * 2 - 1
    x = torch.cat([x, lat, torch.tensor([[-1.0, -1, -1], [1, 1, 1]])])
    with torch.no_grad():
        want = torch.cat(ref(x, gather=True)[1], -1)
        out_ref = ref(x)
    out, pre = net(x.to(cuda), gather=True)
    got = torch.cat(pre, -1).cpu()
    assert torch.equal(got, want), f"max |diff| {(got - want).abs().max()}"
    assert torch.equal(out.cpu(), out_ref)


@pytest.mark.parametrize("name", ["small_sphere"] + SHAPES + WIDE)
@pytest.mark.parametrize("n", [1, 2, 3, 5, 7, 8, 15, 16, 17, 64])
def test_forward_small_batches_bitwise(cuda, name, n):
    """A call's row count selects the reference's MKL summation schedule
    (1 row; 2..15 rows for the 2-output layer, 2..7 for an 8-output layer of
    <= 8 inputs; zero-padded lanes for odd level counts; the row parity for
    a 32-input layer): the HIP MLP follows it for every net shape."""
    d = load(name)
    net, ref = product_net(d, cuda), oracle_net(d)
    x = _rand_points(n * 37, 7)
    for c in x.split(n):
        with torch.no_grad():
            want = torch.cat(ref(c, gather=True)[1], -1)
        got = torch.cat(net(c.to(cuda), gather=True)[1], -1).cpu()
        assert torch.equal(got, want)


@pytest.mark.parametrize("name", [n for n in ("synth32u", "synth32h", "synth64h", "large_sphere")
                                  if n in cases()])
def test_encoding_bitwise(cuda, name):
    """Dense levels (synth32u) and prime-XOR hashed levels (synth32h: 31^3 >
    2^14; synth64h; large_sphere level 3: 128^3 > 2^19)."""
    d = load(name)
    net, ref = product_net(d, cuda), oracle_net(d)
    x = (_rand_points(5000, 2) + 1) / 2
    got = net.enc(x.to(cuda)).cpu()
    with torch.no_grad():
        want = ref.enc(x)
    assert torch.equal(got, want)


@pytest.mark.parametrize("name", ["small_sphere", "synth24"] + WIDE[:1])
def test_region_and_sdf(cuda, name):
    d = load(name)
    net, ref = product_net(d, cuda), oracle_net(d)
    x = _rand_points(4000, 3)
    mk = torch.as_tensor(d["marks"])
    x[:500, 0] = mk[torch.arange(500) % len(mk)] * 2 - 1  # on grid planes
    m, off, _ = net.region(x.to(cuda))
    with torch.no_grad():
        m_ref, off_ref, _ = ref.region(x)
        sdf_ref = ref.sdf(x)
    assert torch.equal(m.cpu(), m_ref)
    assert torch.equal(off.cpu(), off_ref)
    assert (net.sdf(x.to(cuda)).cpu() - sdf_ref).abs().max() < 1e-5
    J = net.normal(x[:64].to(cuda)).cpu()
    J_ref = ref.normal(x[:64].clone())
    assert (J - J_ref).abs().max() < 1e-3 * max(1.0, J_ref.abs().max().item())


@pytest.mark.parametrize("name", cases("lattice"))
def test_lattice_steps_bitwise(cuda, name):
    """Every one of the 33 subpoly_ steps on the full lattice, hashed
    against the reference's (vertices, edges, cache) after each call."""
    from tropical._engine import engine_for
    d = load(name)
    net = product_net(d, cuda)
    eng = engine_for(net)
    eng.lattice(keep_all=True)
    got = engine_steps(eng)
    for i, (g, V, E, s) in enumerate(zip(got, d["step_V"], d["step_E"], d["step_sha"])):
        assert (g[0], g[1]) == (V, E), f"step {i}: V/E {g[:2]} != {(V, E)}"
        assert g[2] == s, f"step {i}: state hash differs"
    _check_surface_faces(eng, d)


def _check_surface_faces(eng, d):
    sV, sE = eng.surface()
    assert sV == int(d["n_surf"][0])
    if sV == 0:
        return
    v, e, _ = eng.export()
    tri, fc = eng.faces()
    if "sha_surf_E" in d:
        assert sha(e.cpu().numpy()) == str(d["sha_surf_E"])
    if "surf_V" in d:
        assert np.abs(v.cpu().numpy() - d["surf_V"]).max() <= VERTEX_TOL
        assert tri.shape[0] == d["tri"].shape[0]
        np.testing.assert_array_equal(tri.cpu().numpy(), d["tri"])
        np.testing.assert_array_equal(fc.cpu().numpy(), d["faces"])
    assert sha(v.cpu().numpy()) == str(d["sha_surf"])
    assert tri.shape[0] == int(d["n_surf"][1])
    assert sha(tri.cpu().numpy()) == str(d["sha_tri"])
    assert sha(fc.cpu().numpy()) == str(d["sha_faces"])


@pytest.mark.parametrize("name", cases("subpoly"))
def test_skeleton_bitwise(cuda, name):
    from tropical._engine import engine_for
    d = load(name)
    net = product_net(d, cuda)
    eng = engine_for(net)
    V, E = eng.skeleton(128, 1.2)
    v, e, _ = eng.export()
    if "skel_V" in d:
        np.testing.assert_array_equal(v.cpu().numpy(), d["skel_V"])
        np.testing.assert_array_equal(e.cpu().numpy(), d["skel_E"])
    else:
        assert sha(v.cpu().numpy(), e.cpu().numpy()) == str(d["sha_skel"])
    if "skel_dups" in d:
        # a multi-tile skeleton (> 128 marks): the 127-stride tile overlap
        # duplicates edges (reference tropical.py:176-181); they are kept, as
        # the reference does
        if len(d["marks"]) > 128:
            assert int(d["skel_dups"]) > 0
        assert e.shape[0] - torch.unique(e, dim=0).shape[0] == int(d["skel_dups"])


@pytest.mark.parametrize("name,unit", [("small_sphere", 128), ("small_sphere", 16), ("small_rand", 16)])
def test_skeleton_sign_mode_matches_oracle(cuda, name, unit):
    """The reference's dormant PRUNING_MODE="sign" (tropical.py:198-202 ->
    _skeleton, :80-100), against the oracle's restatement (the reference
    never runs it, so no golden exists): vertices and edges bitwise, tile
    overlaps (unit 16) included."""
    import oracle.subdivide as od
    from tropical._engine import engine_for
    d = load(name)
    net = product_net(d, cuda)
    eng = engine_for(net)
    eng.skeleton(unit, 1.2, mode="sign")
    v, e, _ = eng.export()
    rv, re = od.skeleton(oracle_net(d), unit, mode="sign")
    assert e.shape[0] > 0
    np.testing.assert_array_equal(v.cpu().numpy(), rv.numpy())
    np.testing.assert_array_equal(e.cpu().numpy(), re.numpy())
    # distance mode is unaffected by the mode switch
    eng.skeleton(unit, 1.2, mode="distance")
    v2, e2, _ = eng.export()
    dv, de = od.skeleton(oracle_net(d), unit)
    np.testing.assert_array_equal(v2.cpu().numpy(), dv.numpy())
    np.testing.assert_array_equal(e2.cpu().numpy(), de.numpy())


@pytest.mark.parametrize("name", cases("subpoly"))
def test_subpoly_steps_bitwise(cuda, name):
    from tropical._engine import engine_for
    d = load(name)
    net = product_net(d, cuda)
    eng = engine_for(net)
    eng.skeleton(128, 1.2)
    v0, e0, _ = eng.export()
    eng.load(v0, e0, keep_all=True)
    eng.set_eps(golden_eps(d))  # subpoly's eps argument (the eps goldens: != net.eps)
    got = engine_steps(eng)
    for i, (g, V, E, s) in enumerate(zip(got, d["step_V"], d["step_E"], d["step_sha"])):
        assert (g[0], g[1]) == (V, E), f"step {i}: V/E {g[:2]} != {(V, E)}"
        assert g[2] == s, f"step {i}: state hash differs"
    _check_surface_faces(eng, d)


@pytest.mark.parametrize("name", cases("subpoly"))
def test_subpoly_dropin(cuda, name, capsys):
    """The drop-in call surface: subpoly(net, 3, 1.2, eps, force=True) (eps:
    the golden's argument -- Net's 1e-4, or another value for the eps
    goldens, where the reference mixes the argument and Net.eps)."""
    import tropical.subpoly as sp
    d = load(name)
    net = product_net(d, cuda)
    stats = []
    faces, verts, fwi = sp.subpoly(net, 3, 1.2, golden_eps(d), force=True, stats=stats)
    out = capsys.readouterr().out
    assert "# of vertices and edges = " in out and " faces, " in out
    assert verts.shape[0] == int(d["n_surf"][0])
    assert sha(verts.cpu().numpy()) == str(d["sha_surf"])
    assert sha(np.asarray(fwi, dtype=np.int64)) == str(d["sha_tri"])
    assert sha(np.asarray(faces, dtype=np.float32)) == str(d["sha_faces"])
    assert sum(s["S"] for s in stats) > 0


def test_subpoly_step_dropin(cuda):
    """subpoly_(vertices, edges, net, l, h, eps, outputs_) one call at a time
    reproduces the reference's per-step states."""
    import tropical.subpoly as sp
    from tropical.synthetic import lattice_edges, lattice_vertices
    d = load("synth24")
    net = product_net(d, cuda)
    n = int(d["lattice_n"])
    V = torch.from_numpy(lattice_vertices(d["marks"])).to(cuda)
    E = torch.from_numpy(lattice_edges(n)).to(cuda)
    o = None
    for step, idx in enumerate(d["step_idx"][:12]):
        l, h = divmod(int(idx), net.num_hidden)
        V, E, o = sp.subpoly_(V, E, net, l, h, 1e-4, o, force=True)
        assert sha(V.cpu().numpy(), E.cpu().numpy(), o.cpu().numpy()) == str(d["step_sha"][step])


@pytest.mark.parametrize("name", [n for n in ("small_sphere_eps3", "small_torus_eps05") if n in cases()])
def test_subpoly_step_dropin_other_eps(cuda, name):
    """subpoly_(..., eps, ...) one call at a time from the skeleton with eps
    != net.eps (3e-4 / 5e-5 against Net's 1e-4): sign test, split point,
    hits and failover at the argument, regions and pruning at net.eps --
    every step's state hash equals the reference's, then extract_skeleton
    and extract_faces at the argument give its surface and faces."""
    import tropical.subpoly as sp
    from tropical._engine import engine_for
    d = load(name)
    eps = golden_eps(d)
    assert eps != 1e-4
    net = product_net(d, cuda)
    eng = engine_for(net)
    eng.skeleton(128, 1.2)
    V, E, _ = eng.export()
    o = None
    # subpoly.py:60-69: every (l, h), then the output plane (l = L-2, h = H)
    calls = [(l, h) for l in range(net.num_layers - 1) for h in range(net.num_hidden)]
    calls.append((net.num_layers - 2, net.num_hidden))
    for step, (l, h) in enumerate(calls):
        V, E, o = sp.subpoly_(V, E, net, l, h, eps, o, force=True)
        assert sha(V.cpu().numpy(), E.cpu().numpy().astype(np.int64), o.cpu().numpy()) == \
            str(d["step_sha"][step]), f"step {step}"
    assert len(calls) == len(d["step_sha"])
    Vs, Es, used = sp.extract_skeleton(V, E, net, eps, o)
    assert sha(Vs.cpu().numpy()) == str(d["sha_surf"])
    faces, fwi = sp.extract_faces(Vs, Es, net, o[used], eps)
    assert sha(np.asarray(fwi, dtype=np.int64)) == str(d["sha_tri"])
    assert sha(np.asarray(faces, dtype=np.float32)) == str(d["sha_faces"])


def test_tied_levels_layout(cuda, monkeypatch):
    """The synthetic lattice nets have identical levels (r_min == r_max), so
    the engine runs on its level-interleaved table copy (NetDev::tied); the
    complex must be bitwise the one the per-level tcnn layout gives."""
    from tropical._engine import engine_for
    d = load("synth32")
    net = product_net(d, cuda)
    runs = []
    for untied in (False, True):
        if untied:
            monkeypatch.setenv("TNP_NO_TIED", "1")
        eng = engine_for(net)
        eng.lattice(keep_all=True)
        runs.append(engine_steps(eng))
    assert runs[0] == runs[1]
    assert runs[0][-1][:2] == (int(d["step_V"][-1]), int(d["step_E"][-1]))


def test_lookback_recompute_path(cuda):
    """The split and the prune number tiles by blockIdx and, after a bounded
    wait, recompute an unpublished predecessor tile's aggregate
    (common.h lb_prefix_rc).  In-order dispatch makes that path rare, so a
    poll count of 0 forces it on every unpublished predecessor: the
    recompute must really run (its counter moves) and the per-step states
    must stay bitwise the reference's."""
    from tropical._engine import engine_for
    d = load("synth32")
    net = product_net(d, cuda)
    runs, recomputes = [], []
    eng = engine_for(net)
    try:
        for spin in (-1, 0):
            eng.debug_lb(spin)
            eng.lattice(keep_all=True)
            runs.append(engine_steps(eng))
            recomputes.append(eng.debug_lb())
    finally:
        eng.debug_lb(-1)
    assert recomputes[1] > 0, recomputes
    assert runs[0] == runs[1]
    for g, V, E, s in zip(runs[1], d["step_V"], d["step_E"], d["step_sha"]):
        assert (g[0], g[1], g[2]) == (V, E, s)


@pytest.mark.parametrize("name", ["synth32", "synth64h"])
def test_lds_record_path(cuda, name):
    """The grouping kernel keeps the records of buckets above 256 entries out
    of memory (csrc/bucket.hip wave_windows: the entry words in cell order in
    memory, each wave building its windows' records in a private 64-record
    LDS stage, pipelined two deep); every step state must be bitwise the same
    with the path off (records through memory) and equal to the reference's
    step records (synth64h: buckets of thousands of entries, many windows
    per wave)."""
    from tropical._engine import engine_for
    d = load(name)
    net = product_net(d, cuda)
    eng = engine_for(net)
    runs = []
    try:
        for on in (True, False):
            eng.debug_lds_records(on)
            eng.lattice(keep_all=True)
            runs.append(engine_steps(eng))
    finally:
        eng.debug_lds_records(True)
    assert runs[0] == runs[1]
    for g, V, E, s in zip(runs[0], d["step_V"], d["step_E"], d["step_sha"]):
        assert (g[0], g[1], g[2]) == (V, E, s)


@pytest.mark.parametrize("force", [True, False])
def test_subpoly_step_rewrites_caller_edges(cuda, force):
    """subpoly.py:209-212: a splitting step rewrites the caller's edges[:, 1]
    in place (masked_scatter_ of the new vertex ids).  With pruning=False the
    returned edge list is [rewritten edges; e_new; c_new], so its head must
    equal the caller's tensor after the call."""
    import tropical.subpoly as sp
    from tropical.synthetic import lattice_edges, lattice_vertices
    d = load("synth24")
    net = product_net(d, cuda)
    V = torch.from_numpy(lattice_vertices(d["marks"])).to(cuda)
    E = torch.from_numpy(lattice_edges(int(d["lattice_n"]))).to(cuda)
    o = None
    for idx in range(net.K):
        l, h = divmod(idx, net.num_hidden)
        E_in = E.clone()
        V2, E2, o2 = sp.subpoly_(V, E, net, l, h, 1e-4, o, pruning=False, force=force)
        if V2.shape[0] == V.shape[0]:
            assert torch.equal(E, E_in)  # nothing split: untouched
            V, E, o = V2, E2, o2
            continue
        changed = (E != E_in).any(dim=1)
        assert changed.any() and torch.equal(E[:, 0], E_in[:, 0])
        assert torch.equal(E2[:E.shape[0]], E)
        assert int(E[changed, 1].min()) >= V.shape[0]
        break


@pytest.mark.parametrize("name", ["small_sphere", "synth32"])
def test_row_order_fast_path_is_the_full_sort(cuda, name, monkeypatch):
    """Faces F4: rows without an exact key tie are ordered in registers
    (faces.hip k_row_fast); TNP_ROW_SORT_FULL=1 runs the padded introsort on
    every row.  Both give the same triangles and float faces, bitwise."""
    from tropical._engine import engine_for
    d = load(name)
    net = product_net(d, cuda)
    eng = engine_for(net)
    outs = []
    for full in ("0", "1"):
        monkeypatch.setenv("TNP_ROW_SORT_FULL", full)
        if d["kind"] == "lattice":
            eng.lattice(keep_all=True)
        else:
            eng.skeleton(128, 1.2)
            v0, e0, _ = eng.export()
            eng.load(v0, e0, keep_all=True)
        engine_steps(eng, record=False)
        eng.surface()
        tri, fc = eng.faces()
        outs.append((tri.cpu().numpy(), fc.cpu().numpy()))
    np.testing.assert_array_equal(outs[0][0], outs[1][0])
    np.testing.assert_array_equal(outs[0][1], outs[1][1])
    assert sha(outs[0][0]) == str(d["sha_tri"]) and sha(outs[0][1]) == str(d["sha_faces"])


@pytest.mark.timeout(300)
@pytest.mark.parametrize("G", [128, 203])
def test_engine_footprint_is_steady_across_passes(cuda, G):
    """bench.py's loop on one engine (the 128^3 headline lattice and the 203^3
    one round 4's 4-block run blew up on): 8 passes of the same workload;
    after the first, the engine's device footprint (every buffer,
    tnp_engine_scratch_bytes) and its connect key buffer do not change, and
    every pass extracts the same complex."""
    import bench
    from tropical.distributed import complex_hash
    from tropical._engine import engine_for
    net = bench.make_net(G, cuda, 6)
    eng = engine_for(net)
    eng.set_owned()
    eng.set_shards(1)
    foot, got = [], []
    for _ in range(8):
        eng.lattice()
        eng.run_steps([])
        foot.append(eng.scratch_bytes())
        V, E = eng.sizes()
        got.append((V, E))
    assert all(f == foot[1] for f in foot[1:]), [f["bytes"] for f in foot]
    assert len(set(got)) == 1
    assert foot[0]["key_bytes"] > 0 and foot[0]["buffers"] > 10


@pytest.mark.timeout(300)
@pytest.mark.parametrize("G", [48, 128])
def test_run_steps_deferred_counts_match_host_loop(cuda, G):
    """tnp_engine_run_steps leaves a pruning step's live counts to the next
    split's hit workers (engine.cpp resolve_counts): its per-step stats (V_out,
    E_out included) and the extracted complex equal the host loop's, which
    counts them in the finish (split / finish through the same entry points)."""
    import bench
    from tropical._engine import engine_for
    net = bench.make_net(G, cuda, 6)
    eng = engine_for(net)
    eng.set_owned()
    eng.set_shards(1)
    outs = []
    for host in (False, True):
        eng.lattice()
        st = []
        if host:
            eng._run_steps_host(st, lambda v, op: v)
        else:
            eng.run_steps(st)
        v, e, _ = eng.export()
        outs.append((st, eng.sizes(), v.cpu().numpy(), e.cpu().numpy()))
    assert outs[0][0] == outs[1][0]
    assert outs[0][1] == outs[1][1]
    np.testing.assert_array_equal(outs[0][2], outs[1][2])
    np.testing.assert_array_equal(outs[0][3], outs[1][3])
    assert any(s["E_out"] < s["E_in"] + s["X"] for s in outs[0][0])


@pytest.mark.parametrize("name", ["large_sphere", "small_sphere"])
def test_skeleton_box_is_the_restricted_skeleton(cuda, name):
    """The sharded skeleton (tnp_engine_skeleton_gmax / _box): the tiles' max
    |grad sdf| computed on 3 'ranks' (every third tile each) and MAX-reduced
    equal the one-rank values, and the skeleton built on a box -- tile & box
    only, with those maxima -- is exactly box_restrict of the whole skeleton
    (vertices bitwise, edges in order, tile-overlap duplicates included), on
    boxes that cut the tiles and one that misses the surface."""
    from tropical.distributed import box_restrict
    from tropical._engine import engine_for
    d = load(name)
    net = product_net(d, cuda)
    eng = engine_for(net)
    g1, l1 = eng.skeleton_gmax(128, 0, 1)
    parts = [eng.skeleton_gmax(128, r, 3) for r in range(3)]
    gm = np.maximum.reduce([g for g, _ in parts])
    assert np.array_equal(gm, g1) and (g1 > 0).all()
    assert np.array_equal(sum(ld for _, ld in parts), l1) and l1.sum() > 0
    eng.skeleton(128, 1.2)
    v, e, _ = eng.export()
    marks = net.enc.marks
    L = int(marks.shape[0])
    boxes = [([0, 0, 0], [L - 1, L - 1, L - 1]), ([L // 3, 2, L // 2 - 3], [L - 4, L // 2 + 7, L - 1]),
             ([L // 2 - 3, L // 2 - 3, L // 2 - 3], [L // 2 + 3, L // 2 + 3, L // 2 + 3]), ([0, 0, 0], [2, 2, 2])]
    for lo, hi in boxes:
        vw, ew = box_restrict(v, e, marks, lo, hi, net.eps)
        V, E = eng.skeleton_box(lo, hi, g1)
        vb, eb, _ = eng.export()
        assert (V, E) == (vw.shape[0], ew.shape[0]), (lo, hi)
        assert torch.equal(vb, vw) and torch.equal(eb, ew), (lo, hi)


@pytest.mark.timeout(300)
def test_early_forward_bound_keeps_the_vertex_set_small(cuda, monkeypatch):
    """the early k_forward_new (launched before the
    split count reaches the host) sized the vertex set by the edge-SLOT count
    E, lazily deleted slots included, so the cache kept ~V + E rows.  Its
    bound is now the largest split count seen (+25 %); a step above it runs
    the forward again once S is known.  On fresh engines over the 128^3
    headline lattice: the complex is the reference's (bench128 fingerprint),
    the redo happens only while the engine learns the split counts (never in
    a later pass), and the vertex set holds no more rows than with the
    edge-slot bound (TNP_EARLY_BOUND=0, round 5's sizing).  (At 128^3 both
    end at the last step's V + S -- 12,957,696 rows on the box: the bound
    matters where the dead edge slots outnumber the splits.)"""
    import bench
    from tropical._engine import Engine
    from tropical.distributed import complex_hash
    net = bench.make_net(128, cuda, 6)
    ref = bench.reference_fingerprint(128, 6)
    rows = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("TNP_EARLY_BOUND", mode)
        eng = Engine(cuda)
        eng.set_net(net)
        redo = []
        for _ in range(3):
            eng.lattice()
            eng.run_steps([])
            redo.append(eng.vertex_capacity()["early_redo"])
        V, E, _ = eng.export()
        assert (V.shape[0], E.shape[0]) + complex_hash(V, E) == ref
        rows[mode] = eng.vertex_capacity()["rows"]
        if mode == "1":
            assert redo[1] == redo[0] and redo[2] == redo[0], redo  # steady after the first pass
        del eng
    assert rows["1"] <= rows["0"], rows


@pytest.mark.timeout(300)
@pytest.mark.parametrize("run", ["2", "32"])
def test_two_stage_key_sort_keeps_the_reference_complex(cuda, monkeypatch, run):
    """VERDICT r05 #4 (pair_sort): the connecting-edge keys lo << nb | hi
    sorted as the lo half (onesweep on bits [nb, 2nb)) plus one pass that
    orders each run of equal lo by hi (sort.hip sort_keys_lex,
    TNP_SORT_RUN=R: runs of <= R keys in the pass, longer ones one workgroup
    each).  R = 2 sends most runs through the long-run kernel.  The order
    must be c_new.sort(-1).unique(dim=0)'s (subpoly.py:243-244): the 128^3
    headline complex equals the reference's bench128 fingerprint, and every
    step's record equals the one-stage sort's."""
    import bench
    from tropical._engine import Engine
    from tropical.distributed import complex_hash
    net = bench.make_net(128, cuda, 6)
    ref = bench.reference_fingerprint(128, 6)
    stats = {}
    for mode in ("0", run):
        monkeypatch.setenv("TNP_SORT_RUN", mode)
        eng = Engine(cuda)
        eng.set_net(net)
        for _ in range(2):
            st = []
            eng.lattice()
            eng.run_steps(st)
        V, E, _ = eng.export()
        assert (V.shape[0], E.shape[0]) + complex_hash(V, E) == ref, mode
        stats[mode] = st
        del eng
    assert stats["0"] == stats[run]


@pytest.mark.timeout(300)
def test_early_forward_footprint(cuda, monkeypatch):
    """ADVICE r05 (medium), the footprint half: the device memory the engine
    holds after two 128^3 passes with the early k_forward_new
    (TNP_EARLY_FWD=1, the default, sized by the largest split count seen)
    against the late launch (0, sized by the split count read back).  On
    the box: 6.75 vs 6.46 GB, 15.95 M vs 14.40 M vertex rows (the bound's
    25 % margin meets the set's 1.5x growth one step earlier;
    profiles/r06_early_forward_footprint.log).  Pinned at <= 10 % more bytes
    and <= 15 % more rows (round 5's edge-slot bound held ~V + E rows)."""
    import json
    import bench
    from tropical._engine import Engine
    net = bench.make_net(128, cuda, 6)
    got = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("TNP_EARLY_FWD", mode)
        eng = Engine(cuda)
        eng.set_net(net)
        for _ in range(2):
            eng.lattice()
            eng.run_steps([])
        got[mode] = dict(eng.scratch_bytes(), rows=eng.vertex_capacity()["rows"])
        del eng
    print("footprint", json.dumps(got))
    assert got["1"]["rows"] <= got["0"]["rows"] * 1.15, got
    assert got["1"]["bytes"] <= got["0"]["bytes"] * 1.10, got
