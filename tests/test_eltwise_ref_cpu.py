"""tests/eltwise_ref.py against torch itself, in fp64 on the CPU: the reference the GPU kernel tests (tests/test_eltwise_gpu.py) compare
with must BE the operation of ERFNet.py -- BatchNorm2d(eps=1e-3) in train and eval mode with its running statistics, Dropout2d's
per-image channel mask, the residual ReLU, max_pool2d and its gradient, the stem's cat(conv, pool), the 2x2 transposed-conv head, the
1x1 output convolution -- so that a misread contract cannot hide on both sides of a kernel comparison.  fp64 both ways: 1e-12."""
import pytest
import torch
import torch.nn.functional as F

import eltwise_ref as R

TOL = 1e-12


def close(a, b, tol=TOL):
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


def rows_of(t, bounds, centred):
    """partial rows [C, R] of t [npix, C] over the pixel runs bounds[i] .. bounds[i + 1]: the producers' two row kinds."""
    k0, k1, n = [], [], []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        v = t[lo:hi]
        k0.append(v.sum(0))
        k1.append(((v - v.mean(0)) ** 2).sum(0) if centred else (v * v).sum(0))
        n.append(float(hi - lo))
    return torch.stack(k0, 1), torch.stack(k1, 1), torch.tensor(n, dtype=torch.float64)


def bn_problem(seed, N=3, ppi=35, C=8, offset=0.0):
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(N * ppi, C, generator=g, dtype=torch.float64) * 2 + offset
    res = torch.randn(N * ppi, C, generator=g, dtype=torch.float64)
    dm = (torch.rand(N, C, generator=g) < 0.7).double() / 0.7
    gamma, beta = torch.rand(C, generator=g, dtype=torch.float64) + 0.5, torch.randn(C, generator=g, dtype=torch.float64)
    rmean, rvar = torch.randn(C, generator=g, dtype=torch.float64), torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    gy = torch.randn(N * ppi, C, generator=g, dtype=torch.float64)
    return dict(t=t, res=res, dm=dm, gamma=gamma, beta=beta, rmean=rmean, rvar=rvar, gy=gy, N=N, ppi=ppi, C=C)


def torch_composite(p, training):
    """relu(batch_norm(t) * dm + res) on NCHW views, torch's own operators; -> y, running stats, autograd gradients."""
    N, ppi, C = p["N"], p["ppi"], p["C"]
    t = p["t"].clone().requires_grad_(True)
    gamma, beta = p["gamma"].clone().requires_grad_(True), p["beta"].clone().requires_grad_(True)
    rm, rv = p["rmean"].clone(), p["rvar"].clone()
    tn = t.view(N, ppi, 1, C).permute(0, 3, 1, 2)
    bn = F.batch_norm(tn, rm, rv, gamma, beta, training=training, momentum=0.1, eps=1e-3)
    y = torch.relu(bn * p["dm"].view(N, C, 1, 1) + p["res"].view(N, ppi, 1, C).permute(0, 3, 1, 2))
    yf = y.permute(0, 2, 3, 1).reshape(N * ppi, C)
    (yf * p["gy"]).sum().backward()
    return yf.detach(), rm, rv, t.grad, gamma.grad, beta.grad


@pytest.mark.parametrize("offset", [0.0, 50.0])
@pytest.mark.parametrize("centred", [False, True])
def test_forward_composite_is_batch_norm(centred, offset):
    p = bn_problem(1, offset=offset)
    npix = p["N"] * p["ppi"]
    k0, k1, n = rows_of(p["t"], [0, 7, 40, 41, 90, npix], centred)
    cnt, mean, var = R.batch_stats([dict(kind0=k0, kind1=k1, n=n, centred=centred, ch_off=0)], p["C"])
    assert bool((cnt == npix).all())
    o = R.bn_finalize_fwd(mean, var, npix, p["gamma"], p["beta"], p["rmean"], p["rvar"], True)
    y = R.bn_act(p["t"], o["scale"], o["shift"], p["dm"], p["res"], p["ppi"])
    want, rm, rv, _, _, _ = torch_composite(p, True)
    assert close(y, want, 1e-11) and close(o["rmean"], rm) and close(o["rvar"], rv, 1e-11)
    assert close(o["asc"] * p["gamma"], o["scale"]) and close(p["beta"] + o["ash"] * p["gamma"], o["shift"], 1e-11)


def test_two_sources_and_uncovered_channels():
    p = bn_problem(2, C=12)
    npix, t = p["N"] * p["ppi"], p["t"]
    a = rows_of(t[:, :4], [0, 64, npix], True)
    b = rows_of(t[:, 4:8], [0, 30, 60, npix], False)
    cnt, mean, var = R.batch_stats([dict(kind0=a[0], kind1=a[1], n=a[2], centred=True, ch_off=0),
                                    dict(kind0=b[0], kind1=b[1], n=b[2], centred=False, ch_off=4)], 12)
    assert close(mean[:8], t[:, :8].mean(0)) and close(var[:8], t[:, :8].var(0, unbiased=False), 1e-11)
    assert bool((cnt[8:] == 0).all() and (mean[8:] == 0).all() and (var[8:] == 0).all())


def test_row_pixels_of_segments():
    n = R.row_pixels(8, 256, 2, 256 + 37)                # four phase segments of two rows each, ragged last tile
    assert n.tolist() == [256.0, 37.0] * 4
    assert R.row_pixels(3, 100, 3, 300).tolist() == [100.0] * 3


@pytest.mark.parametrize("training", [True, False])
def test_backward_composite_is_autograd(training):
    p = bn_problem(3)
    npix = p["N"] * p["ppi"]
    mean, var = p["t"].mean(0), p["t"].var(0, unbiased=False)
    o = R.bn_finalize_fwd(mean, var, npix, p["gamma"], p["beta"], p["rmean"], p["rvar"], training)
    y = R.bn_act(p["t"], o["scale"], o["shift"], p["dm"], p["res"], p["ppi"])
    want_y, _, _, gt, ggamma, gbeta = torch_composite(p, training)
    assert close(y, want_y, 1e-11)
    s1, s2 = R.bn_bwd_sums(p["gy"], y, p["t"], p["dm"], p["ppi"])
    f = R.bn_bwd_finalize(s1, s2, o["asc"], o["ash"], npix, training)
    got, gz, S = R.bn_bwd_apply(p["gy"], y, p["t"], o["asc"], o["ash"], p["gamma"], f["c1"], f["c2"], p["dm"], p["ppi"])
    assert close(got, gt, 1e-10) and close(f["ggamma"], ggamma, 1e-10) and close(f["gbeta"], gbeta, 1e-10)
    assert close(gz, p["gy"] * (want_y > 0)) and bool((S >= got.abs() * (1 - 1e-12)).all())
    if not training:
        assert bool((f["c1"] == 0).all() and (f["c2"] == 0).all())


def test_pool_is_max_pool2d_and_its_autograd():
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 6, 10, 8, generator=g, dtype=torch.float64)              # tie-free
    go = torch.randn(2, 3, 5, 8, generator=g, dtype=torch.float64)
    xn = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    want = F.max_pool2d(xn, 2, 2)
    (want * go.permute(0, 3, 1, 2)).sum().backward()
    m, _ = R.pool_argmax(x)
    assert torch.equal(m, want.detach().permute(0, 2, 3, 1))
    assert torch.equal(R.pool_bwd(x, go), xn.grad.permute(0, 2, 3, 1))
    sc, sh = torch.tensor([1.0, -2.0] * 4, dtype=torch.float64), torch.randn(8, generator=g, dtype=torch.float64)
    assert close(R.pool_affine(x, sc, sh), torch.relu(want.detach().permute(0, 2, 3, 1) * sc + sh))


def test_pool_tie_rule_on_a_hand_made_window():
    # windows in scan order (0,0), (0,1), (1,0), (1,1); the FIRST maximum takes the gradient, -0.0 == +0.0 is a tie
    cases = [([1, 1, 1, 1], 0), ([0, 2, 2, 1], 1), ([0, 1, 2, 2], 2), ([-1, -1, -1, 0], 3), ([-0.0, 0.0, -1, -1], 0), ([0.0, -0.0, 0.0, -0.0], 0),
             ([-3, -0.0, 0.0, -0.0], 1)]
    for win, arg in cases:
        x = torch.tensor(win, dtype=torch.float32).view(1, 2, 2, 1)
        m, a = R.pool_argmax(x)
        assert int(a) == arg and float(m) == max(win)
        gx = R.pool_bwd(x, torch.full((1, 1, 1, 1), 7.0))
        want = [0.0] * 4
        want[arg] = 7.0
        assert gx.flatten().tolist() == want
        xn = x.permute(0, 3, 1, 2).clone().requires_grad_(True)                 # ATen's own choice on the same window
        F.max_pool2d(xn, 2, 2).sum().backward()
        assert xn.grad.flatten().tolist() == [float(i == arg) for i in range(4)]


@pytest.mark.parametrize("Cin", [1, 2, 3, 4])
def test_stem_is_cat_conv_pool(Cin):
    g = torch.Generator().manual_seed(5 + Cin)
    img = torch.randn(2, Cin, 6, 10, generator=g, dtype=torch.float64)
    w, b = torch.randn(16 - Cin, Cin, 3, 3, generator=g, dtype=torch.float64), torch.randn(16 - Cin, generator=g, dtype=torch.float64)
    want = torch.cat([F.conv2d(img, w, b, stride=2, padding=1), F.max_pool2d(img, 2, 2)], 1).permute(0, 2, 3, 1)
    assert close(R.stem(img, w, b), want)
    assert bool((R.stem_abs(img, w, b) >= want.abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize("K", [1, 5, 8])
def test_head_is_conv_transpose2d(K):
    g = torch.Generator().manual_seed(20 + K)
    x = torch.randn(2, 3, 5, 16, generator=g, dtype=torch.float64)
    w, b = torch.randn(16, K, 2, 2, generator=g, dtype=torch.float64), torch.randn(K, generator=g, dtype=torch.float64)
    go = torch.randn(2, K, 6, 10, generator=g, dtype=torch.float64)
    xn = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    want = F.conv_transpose2d(xn, w, b, stride=2)
    (want * go).sum().backward()
    assert close(R.head_fwd(x, w, b), want.detach())
    assert close(R.head_bwd_data(go, w), xn.grad.permute(0, 2, 3, 1))


@pytest.mark.parametrize("bias", [True, False])
def test_pointwise_is_conv2d_1x1(bias):
    g = torch.Generator().manual_seed(30)
    C, K = 12, 3
    x = torch.randn(2, 3, 5, C, generator=g, dtype=torch.float64)
    w = torch.randn(K, C, generator=g, dtype=torch.float64).requires_grad_(True)
    b = torch.randn(K, generator=g, dtype=torch.float64).requires_grad_(True) if bias else None
    go = torch.randn(2, K, 3, 5, generator=g, dtype=torch.float64)
    xn = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    want = F.conv2d(xn, w.view(K, C, 1, 1), b)
    (want * go).sum().backward()
    assert close(R.pointwise_fwd(x, w, b), want.detach())
    gx, gw, gb = R.pointwise_bwd(x, go, w)
    assert close(gx, xn.grad.permute(0, 2, 3, 1)) and close(gw, w.grad)
    if bias:
        assert close(gb, b.grad)
