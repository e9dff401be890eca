"""GPU parity of the homography route through the lane fit: the device grid, the inline fit (``lf_wls_fwd_theta`` /
``lf_wls_bwd_theta``), the explicit grid gradient (``lf_wls_bwd_grid``), the grid generator's backward (``lf_theta_grid_bwd``)
and the module surface on top (``fit_lanes(theta=)``, ``ProjectiveGridGenerator``, ``BEVNet.set_homography``).

Oracle: ``fit_through_theta`` of tests/test_homography_cpu.py (numpy fp64, checked there against the real reference's autograd to
1e-9) and the reference's own fp32 / fp64 runs in tests/golden/homography.npz.  Gates:
  (b) identical inputs -- the oracle reads the device's own fp32 grid: the gates of tests/test_fit_gpu.py:53-56 (beta 2e-7,
      every gradient 2e-6, max-norm relative as there);
  (c) against the reference: every quantity no further (relative L2) from the reference's fp64 run than twice the
      reference's own fp32 run is, plus beta 1e-5 / logits gradient 1e-4 as tests/test_fit_gpu.py holds them.
Measured distances: DESIGN.md 4.5.
"""
import numpy as np
import pytest
import torch

from conftest import relerr
from oracle import erfnet_oracle, fit_oracle, inputs
from test_homography_cpu import BEV, BEV_CASES, BP, case_inputs, fit_through_theta, grid_from_theta, rel_l2, theta_grad_of_grid_grad
from test_homography_cpu import golden  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu


def dev(a, dtype=None):
    t = torch.as_tensor(np.asarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda()


@pytest.fixture(scope="module")
def lf():
    from lanedetection_end2end_amd import fit, geometry, ops
    return type("ns", (), dict(fit=fit, geometry=geometry, ops=ops))


def run_theta(lf, o, theta, gb, zr, order, reg, y_off, normalised, act="square", chol=False):
    """The inline route: (beta, grad_logits, grad_theta fp64, in theta's shape)."""
    ot = dev(o).requires_grad_(True)
    th = dev(theta, torch.float64).requires_grad_(True)           # (fp64 leaf: the kernel's fp64 sums come back unrounded)
    beta, _, status = lf.fit.fit_lanes(ot, None, zr, order, reg, y_off, act, use_cholesky=chol, theta=th, normalised=normalised)
    (beta * dev(gb)).sum().backward()
    assert int(status.abs().sum()) == 0
    return beta.detach().cpu().numpy(), ot.grad.cpu().numpy(), th.grad.cpu().numpy()


def run_grid(lf, o, theta, gb, zr, order, reg, y_off, normalised, act="square", chol=False):
    """The route through a generated grid: (beta, grad_logits, grad_grid, grad_theta, the grid)."""
    N, K, H, W = o.shape
    ot = dev(o).requires_grad_(True)
    th = dev(theta, torch.float64).requires_grad_(True)
    grid = lf.ops.theta_grid(th, H, W, normalised)
    grid.retain_grad()
    beta, _, _ = lf.fit.fit_lanes(ot, grid, zr, order, reg, y_off, act, use_cholesky=chol)
    (beta * dev(gb)).sum().backward()
    return beta.detach().cpu().numpy(), ot.grad.cpu().numpy(), grid.grad.cpu().numpy(), th.grad.cpu().numpy(), grid.detach().cpu().numpy()


def bev_theta(golden, order=2, reg=0.0):
    return golden["bev_o%d_r%g_f64_theta" % (order, reg)]


# ---- (a) the device grid --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flavour", ["bev", "bp"])
def test_device_grid_against_fp64(lf, golden, flavour):
    cfg = BEV if flavour == "bev" else BP
    theta = golden["bev_o2_r0_f64_theta" if flavour == "bev" else "bp_o2_f64_theta"]
    N, H, W = cfg["N"], cfg["H"], cfg["W"]
    live = np.arange(H * W) >= fit_oracle.zero_rows_of(H, 0.3) * W
    gx, gy, _, _, _ = grid_from_theta(theta, H, W, cfg["normalised"])
    ref = np.stack([gx, gy], -1)[:, live]
    got = lf.ops.theta_grid(dev(theta, torch.float32), H, W, cfg["normalised"]).cpu().numpy()
    host = np.stack([lf.geometry.projective_grid(H, W, theta[n], cfg["normalised"]).numpy() for n in range(N)])
    d_dev, d_host, d_between = rel_l2(got[:, live], ref), rel_l2(host[:, live], ref), rel_l2(got[:, live], host[:, live])
    differ = float((got[:, live] != host[:, live]).mean())
    print("%s grid: |device - fp64| %.2e  |host fp32 - fp64| %.2e  |device - host| %.2e  entries that differ %.1f %%"
          % (flavour, d_dev, d_host, d_between, 100 * differ))
    assert got.shape == (N, H * W, 2)
    assert d_dev <= 2 * d_host
    # a (3, 3) theta gives one shared grid, equal to the per-image kernel's
    one = lf.ops.theta_grid(dev(theta[1], torch.float32), H, W, cfg["normalised"]).cpu().numpy()
    assert one.shape == (1, H * W, 2) and np.array_equal(one[0][live], got[1][live])


# ---- (b) identical inputs ---------------------------------------------------------------------------------------------------

def _identical_inputs(lf, o, theta, gb, zr, order, reg, y_off, normalised, tag, act="square", chol=False):
    N, K, H, W = o.shape
    beta, gl, gt = run_theta(lf, o, theta, gb, zr, order, reg, y_off, normalised, act, chol)
    beta2, gl2, gg, gt2, grid = run_grid(lf, o, theta, gb, zr, order, reg, y_off, normalised, act, chol)
    # (the oracle reads what the kernels read: theta rounded to fp32, the device's own fp32 grid)
    t32 = np.asarray(theta, np.float32).astype(np.float64)
    c = fit_through_theta(o, t32, gb, zr, order, reg, y_off, normalised, act, grid=grid)
    per_image = np.asarray(theta).ndim == 3
    ogt = c["grad_theta"] if per_image else c["grad_theta"].sum(0)
    ogg = c["grad_grid"] if per_image else c["grad_grid"].sum(0, keepdims=True)
    e = dict(beta=relerr(beta, c["beta"]), grad_logits=relerr(gl, c["grad_logits"]), grad_grid=relerr(gg, ogg),
             grad_theta=relerr(gt, ogt), grad_theta_via_grid=relerr(gt2, ogt))
    print("identical inputs %s: %s" % (tag, " ".join("%s %.2e" % kv for kv in e.items())))
    assert gt.shape == np.asarray(theta).shape and gg.shape == grid.shape
    assert np.array_equal(beta, beta2) and np.array_equal(gl, gl2)          # (d) the two routes: the same bits
    assert e["beta"] < 2e-7
    assert e["grad_logits"] < 2e-6 and e["grad_grid"] < 2e-6 and e["grad_theta"] < 2e-6 and e["grad_theta_via_grid"] < 2e-6
    assert relerr(gt, gt2) < 2e-6
    return e


@pytest.mark.parametrize("order,reg", BEV_CASES)
def test_identical_inputs_bev(lf, golden, order, reg):
    o, gb, zr = case_inputs(BEV, order)
    _identical_inputs(lf, o, bev_theta(golden, order, reg), gb, zr, order, reg, 1.0, True, "bev o%d r%g" % (order, reg))


@pytest.mark.parametrize("order", [2, 3])
@pytest.mark.parametrize("chol", [False, True])
def test_identical_inputs_bp(lf, golden, order, chol):
    o, gb, zr = case_inputs(BP, order)
    _identical_inputs(lf, o, golden["bp_o%d_f64_theta" % order], gb, zr, order, 0.0, 255.0, False,
                      "bp o%d chol %d" % (order, chol), chol=chol)


@pytest.mark.parametrize("H,W", [(48, 100), (48, 102)])
@pytest.mark.parametrize("order", [0, 1, 2, 3])
def test_identical_inputs_ragged(lf, golden, H, W, order):
    """48 x 100, and 48 x 102 whose rows are no multiple of four pixels (the VEC == 1 kernels)."""
    N, K = 3, 2
    o = inputs.lane_like_logits(N, K, H, W, seed=21)
    gb = np.random.default_rng(22).standard_normal((N, K, order + 1))
    _identical_inputs(lf, o, bev_theta(golden), gb, 15, order, 1e-3, 1.0, True, "ragged %dx%d o%d" % (H, W, order))


@pytest.mark.parametrize("act", ["abs", "relu", "sigmoid", "softplus", "none"])
def test_identical_inputs_activations(lf, golden, act):
    N, K, H, W = 3, 2, 32, 64
    o = inputs.lane_like_logits(N, K, H, W, seed=3) + 0.2
    gb = np.random.default_rng(1).standard_normal((N, K, 3))
    _identical_inputs(lf, o, bev_theta(golden), gb, 10, 2, 0.0, 1.0, True, "act " + act, act=act)


def test_shared_theta_against_per_image(lf, golden):
    """One (3, 3) theta for the batch == the same matrix repeated per image: the same beta bits, and its gradient is the sum of
    the per-image gradients; both against the oracle."""
    o, gb, zr = case_inputs(BEV, 2)
    t = bev_theta(golden)[0]
    _identical_inputs(lf, o, t, gb, zr, 2, 0.0, 1.0, True, "shared (3,3)")
    b1, gl1, gt1 = run_theta(lf, o, t, gb, zr, 2, 0.0, 1.0, True)
    bN, glN, gtN = run_theta(lf, o, np.broadcast_to(t, (3, 3, 3)).copy(), gb, zr, 2, 0.0, 1.0, True)
    assert np.array_equal(b1, bN) and np.array_equal(gl1, glN)
    assert relerr(gt1, gtN.sum(0)) < 1e-12           # fp64 sums of the same terms in another order


# ---- (c) against the reference ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("order,reg", BEV_CASES)
def test_bev_against_reference(lf, golden, order, reg):
    cfg = BEV
    N, H, W = cfg["N"], cfg["H"], cfg["W"]
    o, gb, zr = case_inputs(cfg, order)
    k64, k32 = "bev_o%d_r%g_f64" % (order, reg), "bev_o%d_r%g_f32" % (order, reg)
    theta = golden[k64 + "_theta"]
    beta, gl, gt = run_theta(lf, o, theta, gb, zr, order, reg, 1.0, True)
    _, _, gg, gt2, _ = run_grid(lf, o, theta, gb, zr, order, reg, 1.0, True)
    got = dict(beta=beta, grad_logits=gl[:, :, ::4, ::4], grad_grid=gg.reshape(N, H, W, 2)[:, ::4, ::4], grad_theta=gt)
    for name, mine in got.items():
        d = rel_l2(mine, golden[k64 + "_" + name])
        floor = rel_l2(golden[k32 + "_" + name], golden[k64 + "_" + name])
        print("bev o%d r%g %-11s |hip - ref64| %.2e   |ref32 - ref64| %.2e" % (order, reg, name, d, floor))
        assert d <= 2 * floor, (name, d, floor)
    assert rel_l2(gt2, golden[k64 + "_grad_theta"]) <= 2 * rel_l2(golden[k32 + "_grad_theta"], golden[k64 + "_grad_theta"])
    assert relerr(beta, golden[k64 + "_beta"]) < 1e-5
    assert relerr(got["grad_logits"], golden[k64 + "_grad_logits"]) < 1e-4


# ---- (d) route consistency and surface ------------------------------------------------------------------------------------------

def test_theta_backward_is_deterministic_and_ignores_masked_rows(lf, golden):
    o, gb, zr = case_inputs(BEV, 2)
    theta = bev_theta(golden)
    a = run_theta(lf, o, theta, gb, zr, 2, 0.0, 1.0, True)
    b = run_theta(lf, o, theta, gb, zr, 2, 0.0, 1.0, True)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    bad = o.copy()
    bad[:, :, :zr] = np.nan                                # the masked rows are never read
    c = run_theta(lf, bad, theta, gb, zr, 2, 0.0, 1.0, True)
    assert np.array_equal(a[0], c[0]) and np.array_equal(a[2], c[2]) and np.isfinite(c[1]).all()
    # a homography with a pole inside the masked rows: c = 0 on image row 0
    pole = theta[0].copy()
    pole[2] = [0.0, 1.0, 0.0]
    d = run_theta(lf, o, pole, gb, zr, 2, 1e-3, 1.0, True)
    assert all(np.isfinite(x).all() for x in d)


def test_fit_lanes_takes_grid_or_theta(lf, golden):
    o, gb, zr = case_inputs(BEV, 2)
    grid = lf.ops.theta_grid(dev(bev_theta(golden), torch.float32), 64, 128, True)
    with pytest.raises(ValueError):
        lf.fit.fit_lanes(dev(o), grid, zr, 2, theta=dev(bev_theta(golden)))
    with pytest.raises(ValueError):
        lf.fit.fit_lanes(dev(o), None, zr, 2)
    with pytest.raises(ValueError):
        lf.fit.fit_lanes(dev(o), None, zr, 2, theta=dev(bev_theta(golden))[:2])          # 2 matrices, 3 images
    # theta's dtype comes back on its gradient
    th = dev(bev_theta(golden), torch.float32).requires_grad_(True)
    beta, _, _ = lf.fit.fit_lanes(dev(o), None, zr, 2, theta=th)
    beta.sum().backward()
    assert th.grad.dtype == torch.float32 and th.grad.shape == (3, 3, 3)


@pytest.mark.parametrize("tree", ["bev", "bp"])
def test_grid_generator_honours_its_theta(golden, tree):
    """Per image, changed between calls, with gradient -- and the constant, gradient-free theta keeps the host-made bits."""
    from lanedetection_end2end_amd import geometry
    mod = __import__("lanedetection_end2end_amd.%s.Networks.LSQ_layer" % tree, fromlist=["ProjectiveGridGenerator"])
    N, K, H, W = 3, 2, 64, 128
    size = torch.Size([N, K, H, W])
    normalised = tree == "bev"
    M = (geometry.bev_homography() if normalised else geometry.get_homography(H))[0]
    const = torch.from_numpy(M).unsqueeze(0).expand(N, 3, 3).float().cuda()
    if tree == "bev":
        gen = mod.ProjectiveGridGenerator(size, const, False)
    else:
        gen = lambda th: mod.ProjectiveGridGenerator(size, th, False)
    host = geometry.projective_grid(H, W, M, normalised)
    g0 = gen(const)
    assert g0.shape == (N, H * W, 2) and torch.equal(g0[1].cpu(), host)                   # today's host-made bits
    g1 = gen(const * 1.01)                                                                # another constant theta
    assert not torch.equal(g0, g1) and torch.equal(g1[0].cpu(), geometry.projective_grid(H, W, (const[0] * 1.01).double().cpu().numpy(), normalised))
    rng = np.random.default_rng(4)
    per = (const.double().cpu().numpy() * (1 + 0.02 * rng.standard_normal((N, 3, 3)))).astype(np.float32)
    th = dev(per).requires_grad_(True)
    g2 = gen(th)
    assert g2.shape == (N, H * W, 2) and not torch.equal(g2[0], g2[1]) and not torch.equal(g2, g1)
    gx, gy, _, _, _ = grid_from_theta(per, H, W, normalised)
    live = np.arange(H * W) >= 20 * W
    assert rel_l2(g2.detach().cpu().numpy()[:, live], np.stack([gx, gy], -1)[:, live]) < 1e-6
    up = torch.from_numpy(rng.standard_normal((N, H * W, 2)).astype(np.float32)).cuda()
    up[:, ~torch.from_numpy(live).cuda()] = 0
    (g2 * up).sum().backward()
    want = theta_grad_of_grid_grad(per, up.cpu().numpy(), H, W, normalised)
    assert relerr(th.grad.cpu(), want) < 2e-6
    assert torch.equal(gen(const), g0)                                                    # and back


def test_weighted_least_squares_module_gives_the_grid_gradient(lf, golden):
    """``Weighted_least_squares.forward(W, grid)`` of both trees follows ``WLSFit``: a grid that requires a gradient gets one."""
    from lanedetection_end2end_amd.bev.Networks.LSQ_layer import Weighted_least_squares
    o, gb, zr = case_inputs(BEV, 2)
    N, K, H, W = o.shape
    theta = bev_theta(golden)
    masked = o ** 2
    masked[:, :, :zr] = 0
    grid = lf.ops.theta_grid(dev(theta, torch.float32), H, W, True).requires_grad_(True)
    ls = Weighted_least_squares(torch.Size([N, K, H, W]), K, 2, False, 0, False)
    b0, b1, _, _ = ls(dev(masked), grid)
    (b0[..., 0] * dev(gb[:, 0], torch.float32)).sum().add((b1[..., 0] * dev(gb[:, 1], torch.float32)).sum()).backward()
    # (the module fits the weight maps as they are -- no activation, no masked-row skip: W = o^2 is the weight, s = W^2)
    c = fit_through_theta(masked, np.asarray(theta, np.float32), gb, 0, 2, 0.0, 1.0, True, act="none", grid=grid.detach().cpu().numpy())
    assert relerr(grid.grad.cpu(), c["grad_grid"]) < 2e-6


def _bev_model(N, R, seed=7):
    from argparse import Namespace
    from lanedetection_end2end_amd.bev.Networks.LSQ_layer import Net
    args = Namespace(batch_size=N, nclasses=2, resize=R, end_to_end=True, mod="erfnet", layers=18, channels_in=3, pretrained=False,
                     pool=True, activation_layer="square", no_cuda=False, order=2, reg_ls=0.0, use_cholesky=False,
                     mask_percentage=0.3, clas=False)
    model = Net(args)
    model.net.load_state_dict(erfnet_oracle.make_params(seed=seed, out_channels=2))
    model = model.cuda()
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout2d):
            m.p = 0
    return model


def test_set_homography_none_is_the_constant_grid(golden):
    N, R = 3, 64
    x = torch.from_numpy(inputs.images(N, R, 2 * R, seed=1)).cuda()
    a, b = _bev_model(N, R).eval(), _bev_model(N, R).eval()
    b.set_homography(dev(bev_theta(golden), torch.float32))
    moved = b.detect(x)
    b.set_homography(None)
    with torch.no_grad():
        fa, fb = a(x, True), b(x, True)
    for u, v in zip(fa, fb):
        assert (u is None and v is None) or torch.equal(u, v)
    da, db = a.detect(x), b.detect(x)
    for u, v in zip(da, db):
        assert (u is None and v is None) or torch.equal(u, v)
    assert not torch.equal(moved[0], da[0])                      # detect used the homography while it was set ...
    # ... and agrees with the engine's forward through the same homography (the gate of tests/test_infer_surface_gpu.py:310)
    import lanedetection_end2end_amd as pkg
    b.set_homography(dev(bev_theta(golden), torch.float32))
    pkg.use_inference_engine(b)
    with torch.no_grad():
        fb = b(x, True)
    for k in range(2):
        assert relerr(moved[k].cpu(), fb[k].cpu()) <= 1e-5
    assert fb[5] is b._homography()
    assert "homography" not in dict(b.named_parameters())


def test_bevnet_trains_its_homography(lf, golden):
    """One fp32 training step at 64 x 128 with an ``nn.Parameter`` homography: theta.grad is finite, non-zero, and equals the
    oracle evaluated at the engine's own logits."""
    N, R = 3, 64
    model = _bev_model(N, R).train()
    theta = torch.nn.Parameter(dev(bev_theta(golden), torch.float32))
    model.set_homography(theta)
    assert dict(model.named_parameters())["homography"] is theta
    x = torch.from_numpy(inputs.images(N, R, 2 * R, seed=1)).cuda()
    b0, b1, _, _, masked, M, output, _, _ = model(x, True)
    assert M is theta
    gb = np.random.default_rng(5).standard_normal((N, 2, 3))
    loss = (b0[..., 0] * dev(gb[:, 0], torch.float32)).sum() + (b1[..., 0] * dev(gb[:, 1], torch.float32)).sum()
    loss.backward()
    g = theta.grad
    assert g is not None and g.shape == (N, 3, 3) and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    w = model.net.encoder.layers[3].conv1x3_1.weight.grad
    assert w is not None and bool(torch.isfinite(w).all()) and float(w.abs().max()) > 0
    grid = lf.ops.theta_grid(theta.detach(), R, 2 * R, True).cpu().numpy()
    c = fit_through_theta(output.detach().cpu().numpy(), theta.detach().cpu().numpy(), gb, model.zero_rows, 2, 0.0, 1.0, True,
                          grid=grid)
    e_beta = relerr(torch.stack([b0, b1], 1)[..., 0].detach().cpu(), c["beta"])
    e_theta = relerr(g.cpu(), c["grad_theta"])
    print("BEVNet step: beta %.2e theta.grad %.2e (|theta.grad| max %.3e)" % (e_beta, e_theta, float(g.abs().max())))
    assert e_beta < 2e-6            # (fp32 betas out of the module: one rounding of an fp64 result)
    assert e_theta < 2e-6
