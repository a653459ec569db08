"""Training and autograd on the wide net shapes (K = 65 / 97 planes: 5 x 16,
3 x 32, 4 x 32; csrc/train_wide.h, one wave per 64 points on the matrix
cores) against the float64 oracle of oracle/train.py, with the tolerances
of test_train.py; the `train` entry point's --layers / --hidden.

The additive floors of the gradient tolerances (1e-9 / 1e-7) must not
swallow a comparison: every config below is chosen so that the oracle's
max |g| is >= 1e-4 for every parameter tensor, and each test asserts that on
the reference values alone.  Default nn.Linear init starves a layer of the
4 x 32 net (max |g| ~ 1e-7), so its fc weights are scaled by FC_SCALE.

The kernels' workgroup is 128 points (2 waves), an MFMA row block 16."""
import pytest
import torch

from test_train import _double_backward_ref, _fc, _names, _small_net, icosphere

G_MIN = 1e-4   # the oracle's max |g| of every parameter tensor is at least this
FC_SCALE = 2.0  # 4 x 32: fc weights (not biases) times this

WIDE = {
    "3x32": dict(levels=4, r_min=2, r_max=32, T=19, num_layers=3, num_hidden=32),
    "5x16": dict(levels=5, r_min=2, r_max=32, T=19, num_layers=5, num_hidden=16),
    "4x32": dict(levels=3, r_min=4, r_max=64, T=12, num_layers=4, num_hidden=32),  # hashed levels
}
EDGES = [1, 15, 16, 17, 63, 64, 65, 127, 128, 129]


def wide_net(name):
    net = _small_net(**WIDE[name])
    if name == "4x32":
        with torch.no_grad():
            for lin in net.fc:
                lin.weight.mul_(FC_SCALE)
    return net


def train_inputs(n, seed=1):
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(n, 3, generator=g) * 2 - 1) * 0.95
    gt = (torch.rand(n, generator=g) * 2 - 1) * 0.3
    return x, gt


def train_ref(net, x, gt):
    from oracle.train import train_loss_grads
    from tropical.stanford.sdf_train import EIK_W
    return train_loss_grads(net.enc.module.params.detach().cpu(), _fc(net), net.enc.meta, x, gt,
                            eik_w=EIK_W, batch_size=1000)


def assert_ref_above_floor(names, ref):
    for name, b in zip(names, ref):
        assert float(b.abs().max()) >= G_MIN, (name, float(b.abs().max()))


def check_train_grads(cuda, name, n, seed=1):
    from tropical.stanford.sdf_train import SDFTrainer
    net = wide_net(name)
    x, gt = train_inputs(n, seed)
    rl1, reik, ref = train_ref(net, x, gt)
    assert_ref_above_floor(_names(net), ref)
    net = net.to(cuda)
    tr = SDFTrainer(net)
    l1, eik = tr.data_grads(x.to(cuda), gt.to(cuda))
    assert abs(float(l1) - float(rl1)) <= 1e-5 * max(1.0, float(rl1))
    assert abs(float(eik) - float(reik)) <= 1e-4 * max(1e-3, float(reik))
    got = [tr.g_table.cpu()]
    off = 0
    for t in _fc(net):
        got.append(tr.g_w[off:off + t.numel()].view_as(t).cpu())
        off += t.numel()
    for pname, a, b in zip(_names(net), got, ref):
        scale = float(b.abs().max())
        err = float((a.double() - b).abs().max())
        assert err <= 2e-4 * scale + 1e-9, (pname, err, scale)


# ---------------------------------------------------------------- CPU -----

def test_cli_shape_flags(capsys):
    import os
    from tropical.stanford.train import model_path, net_config, parse_args, supported_shapes
    a = parse_args([])
    assert (a.layers, a.hidden) == (3, 16)
    b = parse_args(["--layers", "3", "--hidden", "32"])
    assert (b.layers, b.hidden) == (3, 32)
    assert net_config("small", "x") == dict(num_layers=3, num_hidden=16, levels=4, r_min=2, r_max=32, T=19)
    c = net_config("small", "x", num_layers=4, num_hidden=32)
    assert (c["num_layers"], c["num_hidden"], c["levels"]) == (4, 32, 4)
    p = model_path("bunny", "small", 45)
    assert p.replace(os.sep, "/").endswith("tropical/stanford/models/bunny/bunny_sdf_small_45.pth")
    assert model_path("bunny", "small", 45, 3, 16) == p
    assert model_path("bunny", "small", 45, 3, 32) == p[:-len(".pth")] + "_l3h32.pth"
    # the supported list: the library's own (csrc/net_device.h), wide shapes included
    shapes = supported_shapes()
    assert {(3, 16), (5, 16), (3, 32), (4, 32)} <= set(shapes) and (3, 64) not in shapes
    with pytest.raises(SystemExit):
        parse_args(["--hidden", "64"])
    err = capsys.readouterr().err
    assert "3 layers x 64 hidden" in err
    assert all(f"{nl} x {h}" in err for nl, h in shapes)
    with pytest.raises(ValueError, match="4 x 32"):
        net_config("small", "x", num_layers=6, num_hidden=16)


# ---------------------------------------------------------------- GPU -----

@pytest.mark.gpu
@pytest.mark.parametrize("name", list(WIDE))
def test_wide_train_grads_match_oracle(cuda, name):
    check_train_grads(cuda, name, 777)


@pytest.mark.gpu
@pytest.mark.parametrize("n", EDGES)
def test_wide_train_grads_batch_edges(cuda, n):
    """The edges of an MFMA row block (16), a wave (64) and a workgroup (128):
    dead rows, a partial last wave, the cross-wave LDS reduction.  (x seed
    11: its first point lies inside the clamp band, so the one-point batch
    has an L1 term and clears G_MIN; seeds 1..10 leave it the eikonal term
    alone, max |g| ~ 1e-5.)"""
    check_train_grads(cuda, "4x32", n, seed=11)


@pytest.mark.gpu
def test_wide_train_grads_empty_batch(cuda):
    from tropical.stanford.sdf_train import SDFTrainer
    net = wide_net("4x32").to(cuda)
    tr = SDFTrainer(net)
    tr.stats.fill_(7.0)
    tr.data_grads(torch.zeros(0, 3, device=cuda), torch.zeros(0, device=cuda))
    assert tr.stats.tolist() == [0.0, 0.0]
    assert not tr.g_table.any() and not tr.g_w.any()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(WIDE))
def test_wide_sdf_autograd_matches_oracle(cuda, name):
    """test_sdf_autograd_matches_oracle's body on the wide shapes."""
    from oracle.train import sdf64
    net = wide_net(name).to(cuda)
    gen = torch.Generator().manual_seed(3)
    n = 513
    x = ((torch.rand(n, 3, generator=gen) * 2 - 1) * 0.9)
    g = torch.rand(n, generator=gen) * 2 - 1
    xg = x.to(cuda).requires_grad_(True)
    y = net.sdf(xg)
    assert y.shape == (n, 1) and y.requires_grad
    (y[:, 0] * g.to(cuda)).sum().backward()
    tab = net.enc.module.params.detach().cpu().double().requires_grad_(True)
    ws = [t.double().requires_grad_(True) for t in _fc(net)]
    xd = x.double().requires_grad_(True)
    yd = sdf64(tab, ws, net.enc.meta, xd)
    assert torch.allclose(y[:, 0].detach().cpu().double(), yd.detach(), atol=1e-5)
    (yd * g.double()).sum().backward()
    got = [xg.grad, net.enc.module.params.grad] + [t.grad for lin in net.fc for t in (lin.weight, lin.bias)]
    want = [xd.grad, tab.grad] + [t.grad for t in ws]
    assert_ref_above_floor(["x"] + _names(net), want)
    for pname, a, b in zip(["x"] + _names(net), got, want):
        assert a is not None, pname
        err = float((a.detach().cpu().double() - b).abs().max())
        assert err <= 2e-4 * float(b.abs().max()) + 1e-7, (pname, err)
    # x only (parameters frozen): the input gradient alone
    for p in net.parameters():
        p.requires_grad_(False)
    x2 = x.to(cuda).requires_grad_(True)
    net.sdf(x2).sum().backward()
    assert x2.grad is not None and torch.isfinite(x2.grad).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(WIDE))
@pytest.mark.parametrize("route", ["normal", "autograd"])
def test_wide_double_backward_matches_oracle(cuda, name, route):
    """test_double_backward_matches_oracle's body on the wide shapes: J, the
    Hessian term in x.grad and every parameter gradient."""
    net = wide_net(name).to(cuda)
    gen = torch.Generator().manual_seed(5)
    n = 401
    x = (torch.rand(n, 3, generator=gen) * 2 - 1) * 0.9
    gJ = torch.rand(n, 3, generator=gen) * 2 - 1
    xg = x.to(cuda).requires_grad_(True)
    if route == "normal":
        J = net.normal(xg, create_graph=True)
    else:
        J = torch.autograd.grad(net.sdf(xg).sum(), xg, create_graph=True)[0]
    assert J.requires_grad
    Jref, want = _double_backward_ref(net, x, gJ)
    assert_ref_above_floor(["x"] + _names(net), want)
    assert float((J.detach().cpu().double() - Jref).abs().max()) <= 2e-4 * float(Jref.abs().max())
    (J * gJ.to(cuda)).sum().backward()
    got = [xg.grad, net.enc.module.params.grad] + [t.grad for lin in net.fc for t in (lin.weight, lin.bias)]
    for pname, a, b in zip(["x"] + _names(net), got, want):
        assert a is not None, pname
        err = float((a.detach().cpu().double() - b).abs().max())
        assert err <= 5e-4 * float(b.abs().max()) + 1e-7, (pname, err, float(b.abs().max()))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(WIDE))
def test_wide_forward_autograd_matches_oracle(cuda, name):
    """test_forward_autograd_matches_oracle's body on the wide shapes:
    upstream on all K = 65 / 97 gathered planes and the 2-wide output."""
    from oracle.train import encode_diff
    net = wide_net(name).to(cuda)
    gen = torch.Generator().manual_seed(7)
    n = 333
    x = (torch.rand(n, 3, generator=gen) * 2 - 1) * 0.9
    xg = x.to(cuda).requires_grad_(True)
    out, inputs = net(xg, gather=True)
    K = net.K
    assert K in (65, 97)
    gpl = torch.rand(n, K, generator=gen) * 2 - 1
    go = torch.rand(n, 2, generator=gen) * 2 - 1
    loss = (out * go.to(cuda)).sum() + (torch.cat(inputs, dim=-1) * gpl.to(cuda)).sum()
    loss.backward()
    tab = net.enc.module.params.detach().cpu().double().requires_grad_(True)
    ws = [t.double().requires_grad_(True) for t in _fc(net)]
    xd = x.double().requires_grad_(True)
    h = encode_diff((xd + 1) / 2, tab, net.enc.meta)
    planes = []
    for i in range(len(ws) // 2):
        h = torch.nn.functional.linear(h, ws[2 * i], ws[2 * i + 1])
        if i < len(ws) // 2 - 1:
            planes.append(h)
            h = torch.relu(h)
    planes.append(h[:, 1:] - h[:, :1])
    ref = (h * go.double()).sum() + (torch.cat(planes, dim=-1) * gpl.double()).sum()
    ref.backward()
    assert torch.allclose(out.detach().cpu().double(), h.detach(), atol=1e-5)
    got = [xg.grad, net.enc.module.params.grad] + [t.grad for lin in net.fc for t in (lin.weight, lin.bias)]
    want = [xd.grad, tab.grad] + [t.grad for t in ws]
    assert_ref_above_floor(["x"] + _names(net), want)
    for pname, a, b in zip(["x"] + _names(net), got, want):
        assert a is not None, pname
        err = float((a.detach().cpu().double() - b).abs().max())
        assert err <= 2e-4 * float(b.abs().max()) + 1e-7, (pname, err)


@pytest.mark.gpu
def test_wide_trainer_reduces_loss(cuda):
    """SDFTrainer on a 3 x 32 net against a sphere's analytic SDF (radius
    0.5, inside positive), points drawn on the fly; the trained net goes
    straight into the extraction.

    The points are drawn as the dataset draws them, around the surface
    (a point of the sphere plus a uniform offset of +-0.2, the clamp band):
    of uniform points in the cube 93 % lie outside the sphere and past the
    clamp, and 150 steps then leave the net without a zero level set.  The
    net is the `train` entry point's with seed 0: the loss clamps the net's
    value to +-0.2, so an initialisation whose constant start value lies
    outside the band (seed 45: tanh(o1 - o0) = -0.28) has no L1 gradient at
    all and stays there."""
    import tropical.subpoly as sp
    from tropical.stanford.model import Net
    from tropical.stanford.sdf_train import SDFTrainer
    from tropical.stanford.train import net_config
    torch.manual_seed(0)
    net = Net(**net_config("small", "sphere", num_layers=3, num_hidden=32)).to(cuda)
    steps = 150
    tr = SDFTrainer(net, lr=3e-3, T_max=steps, batch_size=1000)
    gen = torch.Generator().manual_seed(11)
    losses = []
    for _ in range(steps):
        u = torch.randn(1000, 3, generator=gen)
        x = (0.5 * u / u.norm(dim=1, keepdim=True) + (torch.rand(1000, 3, generator=gen) - 0.5) * 0.4).to(cuda)
        gt = 0.5 - x.norm(dim=1)
        loss, _ = tr.step(x, gt)
        losses.append(loss)
    losses = torch.stack(losses).cpu()
    assert float(losses[-10:].mean()) < float(losses[:10].mean())
    assert all(bool(torch.isfinite(p).all()) for p in net.parameters())
    _, _, faces = sp.subpoly(net, 3, 1.2, force=True)
    assert len(faces) > 0


@pytest.mark.gpu
def test_cli_trains_a_wide_net(cuda, tmp_path, capsys, monkeypatch):
    """`train --mesh sphere.ply --layers 3 --hidden 32`, one epoch: trains,
    saves the state_dict under the shape-suffixed cache name and writes the
    shape-suffixed mesh.  Run without `-c` (which disables the cache, so
    nothing would be saved) and with the cache directory redirected to
    tmp_path.  The sphere is icosphere(4) as in test_train.py: the dataset's
    sampling needs 30 x vertices >= its 50,000 points."""
    import os
    from tropical.stanford import train
    from tropical.utils.mesh import Mesh
    V, F = icosphere(4, r=0.37)
    Mesh(V, F).export(str(tmp_path / "sphere.ply"))
    real_path = train.model_path
    monkeypatch.setattr(train, "model_path", lambda *a: str(tmp_path / "models" / os.path.basename(real_path(*a))))
    rc = train.main(["-d", "bunny", "--mesh", str(tmp_path / "sphere.ply"), "--out", str(tmp_path / "meshes"),
                     "--epochs", "1", "--layers", "3", "--hidden", "32"])
    assert rc == 0
    out = capsys.readouterr().out
    assert "Finished training." in out
    losses = [float(l.split("loss: ")[1].split()[0]) for l in out.splitlines() if "loss: " in l]
    assert len(losses) == 5 and losses[-1] <= losses[0]
    sd = torch.load(tmp_path / "models" / "bunny_sdf_small_45_l3h32.pth", weights_only=True)
    assert sd["fc.0.weight"].shape[0] == 32
    assert os.path.isfile(tmp_path / "meshes" / "bunny" / "our_mesh_small_45_l3h32.ply")
