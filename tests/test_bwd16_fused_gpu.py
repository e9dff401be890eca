"""The fused backward of the fp32 16 -> 16 channel 3-tap convolutions (tapbwd16_kernel, csrc/lf_bwd16.hip; BEV/Networks/ERFNet.py:29-60 at
the decoder's full-resolution stage): weight gradient and data gradient of one convolution in ONE launch, against the two launches it
replaces -- tapgemm_lean_kernel through lf_debug_conv1d_epi(transposed = 1) and tapwgrad16_f32_kernel through lf_conv1d_bwd_weight /
lf_debug_conv1d_wgrad_pro.  The fused kernel keeps their arithmetic, so gx, gw and gb are compared BIT FOR BIT; the BatchNorm-backward
partial rows are held to tests/test_lean_gpu.py's measure and bound against fp64 sums of the stored values.  Then the whole backward
pass with the fused routing on against off."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

C = 16
# (N, H, W, axis, dilation)
SHAPES = [(1, 4, 64, 0, 1), (1, 4, 64, 1, 1),      # one wave's range, both axes
          (2, 5, 64, 0, 2),                        # 320-pixel images: a 256-pixel range straddles two images, the last range is ragged
          (2, 9, 64, 1, 1),                        # 1152 pixels: more than one 4-wave workgroup, the last one mostly empty
          (1, 3, 64, 0, 4), (1, 2, 128, 1, 16),    # dilation >= extent: whole tap DMAs are padding (zeros, also after the prologue)
          (4, 512, 512, 0, 1)]                     # 2^20 pixels (the flagship step's count): 256-pixel wave ranges, a wave writes its own statistics row
DECLINED = (3, 6, 80, 1, 1)                        # W % 64 != 0
# the four compiled forms: (name, epilogue flags of csrc/lf_conv.h, BN + ReLU prologue on the weight gradient's x)
FORMS = [("mask", 2, False), ("maskbn+sums", 16 | 32, True), ("add+mask+sums", 4 | 2 | 32, False), ("add", 4, False)]
TOL_SUMS = 2e-6                                    # tests/test_lean_gpu.py: partial rows summed in fp64, relative to the absolute sums


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def make_inputs(shape):
    N, H, W, axis, d = shape
    torch.manual_seed(N * 1000 + H * 100 + W + axis + d)
    t = lambda: torch.randn(N, H, W, C, device="cuda")
    x, gy, add, aux = t(), t(), t(), t()
    w = torch.randn(C, C, 3, device="cuda") * (2.0 / (3 * C)) ** 0.5
    sc = torch.rand(C, device="cuda") + 0.5
    sh = torch.rand(C, device="cuda") * 0.5 + 0.25          # relu(0 * sc + sh) > 0: padding must be zero AFTER the prologue
    return x, gy, add, aux, w, sc, sh


def pair_args(form, x, gy, add, aux, w, sc, sh):
    """(add_src, aux, msc, msh, pro_sc, pro_sh) of the fused call for one form"""
    name, epi, pro = form
    return (add if epi & 4 else None, aux if (epi & 32) and not (epi & 16) else None, sc if epi & 16 else None, sh if epi & 16 else None,
            sc if pro else None, sh if pro else None)


@pytest.mark.parametrize("form", FORMS, ids=[f[0] for f in FORMS])
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_fused_pair_equals_the_two_launches(shape, form):
    from lanedetection_end2end_amd import _lib
    lib = _lib.load()
    st = _lib.stream()
    N, H, W, axis, d = shape
    name, epi, pro = form
    x, gy, add, aux, w, sc, sh = make_inputs(shape)
    nrows = (N * H * W + 255) // 256
    need = lib.lf_debug_conv1d_bwd_pair_scratch_floats(N, H, W, C)
    assert need > 0
    GUARD, SENTINEL = 4096, 12345.0
    add_src, aux_own, msc, msh, psc, psh = pair_args(form, x, gy, add, aux, w, sc, sh)

    def fused():
        gx = torch.full_like(x, float("nan"))
        gw = torch.full((C, C, 3), float("nan"), device="cuda")
        gb = torch.full((C,), float("nan"), device="cuda")
        rows = torch.full((2, C, nrows), float("nan"), device="cuda")
        scratch = torch.full((need + GUARD,), SENTINEL, device="cuda")
        rc = lib.lf_debug_conv1d_bwd_pair(P(x), P(gy), P(w), epi, P(add_src), P(aux_own), P(msc), P(msh), P(psc), P(psh), P(gx), P(gw), P(gb),
                                          P(rows), N, H, W, C, axis, d, P(scratch), st)
        assert rc == (nrows if epi & 32 else 0), lib.lf_last_error().decode()
        torch.cuda.synchronize()
        assert bool((scratch[need:] == SENTINEL).all()), "scratch written past its documented extent"
        return gx, gw, gb, rows

    gx, gw, gb, rows = fused()
    # the two launches
    scratch2 = torch.empty(lib.lf_conv1d_scratch_floats(N, H, W, C) + 4096, device="cuda")
    gx_ref = torch.full_like(x, float("nan"))
    rows_ref = torch.full((2, C, nrows), float("nan"), device="cuda")
    second = x if epi & 16 else aux          # the tensor of the second sum
    rc = lib.lf_debug_conv1d_epi(P(gy), P(w), None, P(gx_ref), 1, epi, P(x) if epi & 2 else None, P(add_src), P(second) if epi & (16 | 32) else None,
                                 P(msc), P(msh), P(rows_ref), N, H, W, C, axis, d, P(scratch2), st)
    assert rc == (nrows if epi & 32 else 0), lib.lf_last_error().decode()
    gw_ref = torch.full((C, C, 3), float("nan"), device="cuda")
    gb_ref = torch.full((C,), float("nan"), device="cuda")
    if pro:
        _lib.check(lib.lf_debug_conv1d_wgrad_pro(P(x), P(gy), P(sc), P(sh), P(gw_ref), P(gb_ref), N, H, W, C, axis, d, P(scratch2), st), "wgrad pro")
    else:
        _lib.check(lib.lf_conv1d_bwd_weight(P(x), P(gy), P(gw_ref), P(gb_ref), N, H, W, C, axis, d, P(scratch2), st), "wgrad")
    torch.cuda.synchronize()

    for what, got in (("gx", gx), ("gw", gw), ("gb", gb)):
        assert bool(torch.isfinite(got).all()), "%s: not finite" % what
    assert torch.equal(gx, gx_ref), "gx differs from the data-gradient launch: max %.3e" % float((gx - gx_ref).abs().max())
    assert torch.equal(gw, gw_ref), "gw differs from the weight-gradient launch: max %.3e" % float((gw - gw_ref).abs().max())
    assert torch.equal(gb, gb_ref), "gb differs from the weight-gradient launch: max %.3e" % float((gb - gb_ref).abs().max())
    if epi & 32:
        assert bool(torch.isfinite(rows).all()), "statistics rows not finite"
        got = rows.double().sum(2)
        v, s = gx.double(), second.double()
        s1, s2 = v.sum((0, 1, 2)), (v * s).sum((0, 1, 2))
        a1, a2 = v.abs().sum((0, 1, 2)), (v * s).abs().sum((0, 1, 2))
        e1, e2 = float(((got[0] - s1).abs() / a1).max()), float(((got[1] - s2).abs() / a2).max())
        print("%s %s: BN-backward sums error %.2e, %.2e" % (shape, name, e1, e2))
        assert e1 < TOL_SUMS and e2 < TOL_SUMS, (e1, e2)
    # once more: the same bits
    gx2, gw2, gb2, rows2 = fused()
    assert torch.equal(gx, gx2) and torch.equal(gw, gw2) and torch.equal(gb, gb2)
    if epi & 32:
        assert torch.equal(rows, rows2)


@pytest.mark.parametrize("form", FORMS, ids=[f[0] for f in FORMS])
def test_fused_pair_declines_ragged_rows(form):
    """W % 64 != 0: lf_tapbwd16_ok says no, and the hook reports that instead of running something else."""
    from lanedetection_end2end_amd import _lib
    lib = _lib.load()
    st = _lib.stream()
    N, H, W, axis, d = DECLINED
    name, epi, pro = form
    x, gy, add, aux, w, sc, sh = make_inputs(DECLINED)
    nrows = (N * H * W + 255) // 256
    add_src, aux_own, msc, msh, psc, psh = pair_args(form, x, gy, add, aux, w, sc, sh)
    gx = torch.full_like(x, 7.0)
    gw = torch.full((C, C, 3), 7.0, device="cuda")
    gb = torch.full((C,), 7.0, device="cuda")
    rows = torch.full((2, C, nrows), 7.0, device="cuda")
    scratch = torch.empty(lib.lf_debug_conv1d_bwd_pair_scratch_floats(N, H, W, C) + 4096, device="cuda")
    rc = lib.lf_debug_conv1d_bwd_pair(P(x), P(gy), P(w), epi, P(add_src), P(aux_own), P(msc), P(msh), P(psc), P(psh), P(gx), P(gw), P(gb),
                                      P(rows), N, H, W, C, axis, d, P(scratch), st)
    assert rc == -1
    assert "does not take" in lib.lf_last_error().decode()
    torch.cuda.synchronize()
    assert bool((gx == 7.0).all()) and bool((gw == 7.0).all()) and bool((gb == 7.0).all()) and bool((rows == 7.0).all())      # nothing ran


def backbone_grads(N, H, W, fused):
    from lanedetection_end2end_amd import _lib
    from lanedetection_end2end_amd.bev.Networks import define_model
    lib = _lib.load()
    torch.manual_seed(11)
    net = define_model('erfnet', layers=18, in_channels=3, out_channels=2, pretrained=False, pool=True).cuda()
    for m in net.modules():
        if isinstance(m, torch.nn.Dropout2d):
            m.p = 0
    net.train()
    x = torch.randn(N, 3, H, W, device="cuda")
    gy = torch.randn(N, 2, H, W, device="cuda")
    lib.lf_debug_set_bwd16_fused(fused)
    try:
        enc, dec = net(x, True)
        (dec * gy).sum().backward()
        torch.cuda.synchronize()
    finally:
        lib.lf_debug_set_bwd16_fused(1)
    return {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}


def is_stage16_conv(k):
    # decoder.layers.4 / .5: the two non_bottleneck_1d(16) blocks at half the input resolution
    return (k.startswith("decoder.layers.4.") or k.startswith("decoder.layers.5.")) and ".conv" in k


def test_backward_fused_against_two_launches():
    """lf_erfnet_backward at batch 2, 64 x 128 (the 16-channel stage: 2 x 32 x 64, fused) with the routing on and off."""
    on, off = backbone_grads(2, 64, 128, 1), backbone_grads(2, 64, 128, 0)
    assert on.keys() == off.keys()
    convs = [k for k in on if is_stage16_conv(k)]
    assert len(convs) == 16, convs                 # 2 blocks x 4 convolutions x (weight, bias)
    for k in convs:
        assert torch.equal(on[k], off[k]), k
    # the gradient leaving the stage, as the layers below it see it: the up-sampler in front of the stage and the encoder's first layer
    for k in ("decoder.layers.3.conv.weight", "decoder.layers.3.conv.bias", "encoder.initial_block.conv.weight"):
        assert torch.equal(on[k], off[k]), k
    # BatchNorm parameter gradients: tests/test_backbone_gpu.py's bound on a parameter gradient (2e-5 of its largest element)
    for k in on:
        if ".bn" in k:
            scale = float(off[k].abs().max())
            if scale > 0:
                assert float((on[k] - off[k]).abs().max()) / scale < 2e-5, k


def test_backward_where_the_fused_kernel_declines():
    """48 x 160 images: the 16-channel stage is 80 pixels wide, every pair takes the two launches with the routing on as with it off."""
    on, off = backbone_grads(2, 48, 160, 1), backbone_grads(2, 48, 160, 0)
    assert on.keys() == off.keys()
    for k in on:
        assert bool(torch.isfinite(on[k]).all()), k
        assert torch.equal(on[k], off[k]), k
