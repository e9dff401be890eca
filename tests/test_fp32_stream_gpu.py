"""tapstream_kernel (csrc/lf_conv.hip: the fp32 3-tap C -> C convolutions and data gradients at 64 / 128 channels with the weights
resident in LDS and the pixels streamed past them; BEV/Networks/ERFNet.py:29-60, the non_bottleneck_1d blocks) against tapgemm_kernel
ONE LAUNCH AT A TIME through the C ABI: outputs and statistics rows bit for bit, with the grid capped so that one workgroup walks
every tile, twice in a row, and both against torch fp64; NaN pre-fill and guard bands behind every destination."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

# (N, H, W, axis, dilation): 640 pixels = two full tiles and one with two live waves (both axes); dilation >= H: both outer taps are
# padding everywhere; 3 tiles over 3 images; one row of 192; W % 64 != 0: not the kernel's geometry, falls back and still agrees
SHAPES = [(2, 5, 64, 0, 1), (2, 5, 64, 1, 2), (1, 6, 128, 1, 16), (1, 6, 128, 0, 8), (3, 4, 64, 0, 2), (1, 3, 192, 1, 1), (2, 7, 48, 0, 1)]
GUARD = 4096
# tolerances of tests/test_lean_gpu.py: values and sums, M2
TOL_V, TOL_M2 = 2e-6, 5e-6


@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("shape", SHAPES)
def test_stream_kernel_equals_tapgemm_bit_for_bit(shape, C):
    import torch.nn.functional as F
    from lanedetection_end2end_amd import _lib
    lib = _lib.load()
    st = _lib.stream()
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    N, H, W, axis, d = shape
    torch.manual_seed(H + W + axis + C)
    x = torch.randn(N, H, W, C, device="cuda")
    mask = torch.randn(N, H, W, C, device="cuda")
    add = torch.randn(N, H, W, C, device="cuda")
    aux = torch.randn(N, H, W, C, device="cuda")
    w = torch.randn(C, C, 3, device="cuda") * (2.0 / (3 * C)) ** 0.5
    b = torch.randn(C, device="cuda")
    sc = torch.rand(C, device="cuda") + 0.5
    sh = torch.randn(C, device="cuda") * 0.5           # relu(0 * sc + sh) != 0: padding must be zero AFTER the transform
    scratch = torch.empty(lib.lf_conv1d_scratch_floats(N, H, W, C) + 4096, device="cuda")
    nrows = (N * H * W + 255) // 256
    numel = N * H * W * C

    def guarded(n):        # n NaNs (every stored element must overwrite one) and a guard band of a value no kernel produces
        t = torch.full((n + GUARD,), float("nan"), device="cuda")
        t[n:] = -12345.0
        return t

    # (name, transposed weights, epilogue flags, bias, mask) -- the variants tapstream_kernel is compiled for, forward and transposed
    # (48: mask by a recomputed BatchNorm + BN-backward sums; 38: + residual gradient, * mask, BN-backward sums -- 64 channels only)
    launches = [("fwd + relu", 0, 1, b, None), ("fwd + BN sums", 0, 8, b, None), ("fwd * mask", 0, 2, None, mask),
                ("dgrad + relu", 1, 1, None, None), ("dgrad + BN sums", 1, 8, None, None), ("dgrad * mask", 1, 2, None, mask),
                ("dgrad * recomputed-BN mask + sums", 1, 48, None, None), ("(dgrad + add) * mask + sums", 1, 38, None, mask),
                ("fwd * recomputed-BN mask + sums", 0, 48, None, None), ("bn-relu prologue + relu", 0, -1, b, None)]

    def run(mode, cap):
        lib.lf_debug_set_fp32_stream(mode, cap)
        out = {}
        for name, tr, epi, bias, msk in launches:
            y, s = guarded(numel), guarded(2 * C * nrows)
            if epi < 0:
                _lib.check(lib.lf_debug_conv1d_fwd_pro(P(x), P(w), P(bias), P(sc), P(sh), P(y), N, H, W, C, axis, d, P(scratch), st), name)
            else:
                rc = lib.lf_debug_conv1d_epi(P(x), P(w), P(bias), P(y), tr, epi, P(msk), P(add) if epi & 4 else None, P(aux) if epi & 48 else None,
                                             P(sc) if epi & 16 else None, P(sh) if epi & 16 else None, P(s) if epi & 40 else None,
                                             N, H, W, C, axis, d, P(scratch), st)
                assert rc == (nrows if epi & 40 else 0), (name, lib.lf_last_error().decode())
            out[name] = (y, s)
        torch.cuda.synchronize()
        return out

    try:
        ref = run(0, 0)                                   # tapgemm_kernel
        runs = {"shipped routing": run(1, 0), "shipped routing again": run(1, 0), "one workgroup": run(1, 1), "two workgroups": run(1, 2),
                "every compiled variant": run(2, 0), "every compiled variant, one workgroup": run(2, 1)}
    finally:
        lib.lf_debug_set_fp32_stream(1, 0)

    for name, tr, epi, bias, msk in launches:
        y0, s0 = ref[name]
        for label, got in runs.items():
            y1, s1 = got[name]
            assert torch.isfinite(y1[:numel]).all(), (name, label)
            assert torch.equal(y1[:numel], y0[:numel]), (name, label)
            assert bool((y1[numel:] == -12345.0).all()), (name, label, "guard band behind the destination")
            assert bool((s1[2 * C * nrows:] == -12345.0).all()), (name, label, "guard band behind the statistics rows")
            if epi > 0 and epi & 40:
                assert torch.isfinite(s1[:2 * C * nrows]).all(), (name, label)
                assert torch.equal(s1[:2 * C * nrows], s0[:2 * C * nrows]), (name, label, "statistics rows")

    # against torch fp64: tapgemm_kernel (mode 0) first, then the shipped routing and every compiled variant, same assertions
    w4 = (w.view(C, C, 3, 1) if axis == 0 else w.view(C, C, 1, 3)).double()
    pad, dil = ((d, 0), (d, 1)) if axis == 0 else ((0, d), (1, d))
    nchw = lambda t: t.double().permute(0, 3, 1, 2)
    nhwc = lambda t: t.permute(0, 2, 3, 1)
    conv0 = nhwc(F.conv2d(nchw(x), w4, None, padding=pad, dilation=dil))
    conv = conv0 + b.double()
    convp = nhwc(F.conv2d(nchw(torch.relu(x.double() * sc.double() + sh.double())), w4, b.double(), padding=pad, dilation=dil))
    dg = nhwc(torch.nn.grad.conv2d_input((N, C, H, W), w4, nchw(x), padding=pad, dilation=dil))
    m = mask.double() > 0
    mbn = (aux.double() * sc.double() + sh.double()) > 0
    want = {"dgrad * recomputed-BN mask + sums": dg * mbn, "(dgrad + add) * mask + sums": (dg + add.double()) * m, "fwd * recomputed-BN mask + sums": conv0 * mbn,
            "fwd + relu": torch.relu(conv), "fwd + BN sums": conv, "fwd * mask": conv0 * m, "dgrad + relu": torch.relu(dg),
            "dgrad + BN sums": dg, "dgrad * mask": dg * m, "bn-relu prologue + relu": torch.relu(convp)}
    for label, got in [("tapgemm_kernel", ref), ("shipped routing", runs["shipped routing"]), ("every compiled variant", runs["every compiled variant"])]:
        for name, tr, epi, bias, msk in launches:
            y, s = got[name]
            v = y[:numel].view(N, H, W, C)
            err = float((v.double() - want[name]).abs().max()) / float(want[name].abs().max())
            print("%s / %s: value error %.2e" % (label, name, err))
            assert err < TOL_V, "%s / %s: %.2e" % (label, name, err)
            if epi == 8:
                # rows [0][c][r] = sum v, [1][c][r] = M2 about the row's own mean, over row r's 256-pixel tile of the stored values
                rows_ = s[:2 * C * nrows].view(2, C, nrows)
                flat = v.double().reshape(-1, C)
                e1 = e2 = 0.0
                for r in range(nrows):
                    t = flat[r * 256: (r + 1) * 256]
                    m2 = ((t - t.mean(0)) ** 2).sum(0)
                    e1 = max(e1, float(((rows_[0, :, r].double() - t.sum(0)).abs() / t.abs().sum(0)).max()))
                    e2 = max(e2, float(((rows_[1, :, r].double() - m2).abs() / m2).max()))
                print("%s / %s: sums error %.2e, M2 error %.2e" % (label, name, e1, e2))
                assert e1 < TOL_V and e2 < TOL_M2, "%s / %s: sums %.2e, M2 %.2e" % (label, name, e1, e2)
            if epi > 0 and epi & 32:
                # BN-backward rows: [0] = sum v, [1] = sum v * aux (raw), over the values as stored
                got_ = s[:2 * C * nrows].view(2, C, nrows).double().sum(2)
                vd, va = v.double(), v.double() * aux.double()
                e1 = float(((got_[0] - vd.sum((0, 1, 2))).abs() / vd.abs().sum((0, 1, 2))).max())
                e2 = float(((got_[1] - va.sum((0, 1, 2))).abs() / va.abs().sum((0, 1, 2))).max())
                print("%s / %s: BN-backward sums error %.2e, %.2e" % (label, name, e1, e2))
                assert e1 < TOL_V and e2 < TOL_V, "%s / %s: BN-backward sums %.2e, %.2e" % (label, name, e1, e2)
