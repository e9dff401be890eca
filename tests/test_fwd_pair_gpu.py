"""tappair_kernel (csrc/lf_conv_pair.hip: a non_bottleneck_1d block's 3x1 -> 1x3 forward pair in one launch, the intermediate tensor
handed over through memory behind a workgroup barrier; BEV/Networks/ERFNet.py:29-60) against the two launches it replaces, ONE PAIR
AT A TIME through the C ABI: the intermediate tensor, the output and the statistics rows bit for bit, with the grid capped so that
one workgroup walks every tile, twice in a row, and the output against torch fp64; NaN pre-fill and guard bands behind every
destination.  Then the whole network with the routing on and off."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

# (N, H, W, dilation) -> what it covers
SHAPES = [(2, 6, 64, 1),      # 3 tiles of 4 rows; the middle tile straddles two images
          (1, 6, 64, 16),     # d >= H: both outer taps of conv_a are padding everywhere; conv_b's d = 16 kills a tap on a quarter of each row
          (3, 3, 128, 2),     # 2-row tiles straddling images; last tile half empty
          (1, 2, 128, 8),     # one tile
          (2, 5, 64, 4),      # 640 pixels: last tile has two live waves
          (2, 7, 48, 1),      # declined (W % 64 != 0): the same call falls back to two launches and still agrees
          (1, 4, 192, 1)]     # declined (256 % W != 0)
# channel counts tappair_kernel is compiled for (lf_conv_pair.hip, g_pair_compiled); a pair at another count runs as two launches
COMPILED = (64, 128)
GUARD = 4096
# tolerances of tests/test_lean_gpu.py: values and sums, M2
TOL_V, TOL_M2 = 2e-6, 5e-6


def taken(shape, C):
    N, H, W, d = shape
    return C in COMPILED and W % 64 == 0 and 256 % W == 0


@pytest.mark.parametrize("pro", [0, 1])
@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("shape", SHAPES)
def test_one_launch_equals_two_bit_for_bit(shape, C, pro):
    import torch.nn.functional as F
    from lanedetection_end2end_amd import _lib
    lib = _lib.load()
    st = _lib.stream()
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    N, H, W, d = shape
    torch.manual_seed(H + W + d + C + pro)
    x = torch.randn(N, H, W, C, device="cuda")
    wa = torch.randn(C, C, 3, device="cuda") * (2.0 / (3 * C)) ** 0.5
    wb = torch.randn(C, C, 3, device="cuda") * (2.0 / (3 * C)) ** 0.5
    ba = torch.randn(C, device="cuda")
    bb = torch.randn(C, device="cuda")
    sc = torch.rand(C, device="cuda") + 0.5
    sh = torch.randn(C, device="cuda") * 0.5 + 0.25     # relu(0 * sc + sh) != 0 on most channels: padding must be zero AFTER the transform
    assert bool((torch.relu(sh) != 0).any())
    scratch = torch.empty(lib.lf_conv1d_scratch_floats(N, H, W, C) + 4096, device="cuda")
    nrows = (N * H * W + 255) // 256
    numel = N * H * W * C

    def guarded(n):        # n NaNs (every stored element must overwrite one) and a guard band of a value no kernel produces
        t = torch.full((n + GUARD,), float("nan"), device="cuda")
        t[n:] = -12345.0
        return t

    def run(mode, cap):
        lib.lf_debug_set_fwd_pair(mode, cap)
        t, y, s = guarded(numel), guarded(numel), guarded(2 * C * nrows)
        rc = lib.lf_debug_conv1d_fwd_pair(P(x), P(wa), P(ba), P(wb), P(bb), P(sc) if pro else None, P(sh) if pro else None, P(t), P(y), P(s),
                                          N, H, W, C, d, P(scratch), st)
        assert rc >= 0, lib.lf_last_error().decode()
        torch.cuda.synchronize()
        return rc, t, y, s

    try:
        ref = run(0, 0)                                   # two launches
        runs = {"every compiled form": run(2, 0), "one workgroup": run(2, 1), "two workgroups": run(2, 2), "again": run(2, 0)}
    finally:
        lib.lf_debug_set_fwd_pair(1, 0)

    assert ref[0] == 0
    _, t0, y0, s0 = ref
    for label, (rc, t1, y1, s1) in runs.items():
        assert rc == (1 if taken(shape, C) else 0), (label, "one launch where the kernel takes the pair, two elsewhere")
        for name, a1, a0, n in (("t", t1, t0, numel), ("y", y1, y0, numel), ("statistics rows", s1, s0, 2 * C * nrows)):
            assert torch.isfinite(a1[:n]).all(), (name, label)
            assert torch.equal(a1[:n], a0[:n]), (name, label)
            assert bool((a1[n:] == -12345.0).all()), (name, label, "guard band behind the destination")

    # against a torch fp64 composition: the two launches first, then the one launch, same assertions
    nchw = lambda v: v.double().permute(0, 3, 1, 2)
    nhwc = lambda v: v.permute(0, 2, 3, 1)
    xin = torch.relu(x.double() * sc.double() + sh.double()) if pro else x.double()
    t64 = torch.relu(F.conv2d(nchw(xin), wa.view(C, C, 3, 1).double(), ba.double(), padding=(d, 0), dilation=(d, 1)))
    y64 = nhwc(F.conv2d(t64, wb.view(C, C, 1, 3).double(), bb.double(), padding=(0, d), dilation=(1, d)))
    flat64 = y64.reshape(-1, C)
    for label, (rc, t, y, s) in [("two launches", ref), ("one launch", runs["every compiled form"])]:
        v = y[:numel].view(N, H, W, C)
        err = float((v.double() - y64).abs().max()) / float(y64.abs().max())
        print("%s: value error %.2e" % (label, err))
        assert err < TOL_V, "%s: %.2e" % (label, err)
        rows_ = s[:2 * C * nrows].view(2, C, nrows)
        e1 = e2 = 0.0
        for r in range(nrows):
            tl = flat64[r * 256: (r + 1) * 256]
            m2 = ((tl - tl.mean(0)) ** 2).sum(0)
            e1 = max(e1, float(((rows_[0, :, r].double() - tl.sum(0)).abs() / tl.abs().sum(0)).max()))
            e2 = max(e2, float(((rows_[1, :, r].double() - m2).abs() / m2).max()))
        print("%s: sums error %.2e, M2 error %.2e" % (label, e1, e2))
        assert e1 < TOL_V and e2 < TOL_M2, "%s: sums %.2e, M2 %.2e" % (label, e1, e2)


def network_step(N, H, W, mode):
    from lanedetection_end2end_amd import _lib
    from lanedetection_end2end_amd.bev.Networks import define_model
    lib = _lib.load()
    torch.manual_seed(11)
    net = define_model('erfnet', layers=18, in_channels=3, out_channels=2, pretrained=False, pool=True).cuda()
    net.train()
    x = torch.randn(N, 3, H, W, device="cuda")
    gy = torch.randn(N, 2, H, W, device="cuda")
    lib.lf_debug_set_fwd_pair(mode, 0)
    try:
        torch.manual_seed(12)                  # the Dropout2d masks
        enc, dec = net(x, True)
        (dec * gy).sum().backward()
        torch.cuda.synchronize()
    finally:
        lib.lf_debug_set_fwd_pair(1, 0)
    out = {"logits": dec.detach().clone(), "encoder output": enc.detach().clone()}
    out.update({"grad " + k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None})
    out.update({"buffer " + k: b.detach().clone() for k, b in net.named_buffers()})
    return out


# batch 1 at 64 x 512: the 64-channel stage is 16 x 128 and the 128-channel stage 8 x 64, so every pair of both stages has the
# geometry the kernel takes (the stages are 1/4 and 1/8 of the image: at 128 x 256 the 128-channel stage is 32 wide and declined);
# batch 2 at 64 x 128: stages of 16 x 32 and 8 x 16, every pair declined
@pytest.mark.parametrize("plan", [(1, 64, 512), (2, 64, 128)])
def test_whole_network_routing_on_against_off(plan):
    """Same seed and Dropout2d masks, fp32, train mode: logits, BatchNorm running statistics and every parameter gradient."""
    on, off = network_step(*plan, 1), network_step(*plan, 0)
    assert on.keys() == off.keys()
    assert any(k.startswith("grad ") for k in on) and any("running_mean" in k for k in on)
    for k in on:
        if on[k].is_floating_point():
            assert bool(torch.isfinite(on[k]).all()), k
        assert torch.equal(on[k], off[k]), k
