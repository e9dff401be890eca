"""tapgemm_thin_kernel (csrc/lf_conv.hip: tapgemm_kernel re-tiled to one 16-pixel tile per wave, for launches whose regular grid
cannot fill the device -- one camera frame) against the kernels the same launch takes without it, ONE LAUNCH AT A TIME through the
debug hooks: outputs bit for bit for every slab count per wave, twice in a row, NaN pre-fill and a guard band behind every
destination, the launch counter exact; and the launches the kernel is not compiled for fall back."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 4096
GUARD_VALUE = -12288.0       # no kernel produces it; exact in bf16 too
# (N, H, W, axis, dilation): 120 pixels = a last workgroup of 56 pixels whose last wave has 8 live ones, ragged rows (both axes);
# whole rows with a tile sequence across the image boundary; large dilation; dilation >= H (both outer taps padding) in exactly
# one workgroup; 24 pixels -- less than one workgroup -- over three images
SHAPES = [(1, 5, 24, 0, 1), (1, 5, 24, 1, 2), (2, 3, 64, 1, 1), (1, 6, 128, 1, 16), (1, 4, 16, 0, 8), (3, 1, 8, 1, 1)]
THIN_RUNS = [(2, 0), (2, 1), (2, 2), (2, 4)]


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def guarded(n, dtype=torch.float32):
    """n NaNs (every stored element must overwrite one) and a guard band of a value no kernel produces"""
    t = torch.full((n + GUARD,), float("nan"), device="cuda", dtype=dtype)
    t[n:] = GUARD_VALUE
    return t


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.fixture
def lib():
    from lanedetection_end2end_amd import _lib
    lib = _lib.load()
    try:
        yield lib
    finally:
        lib.lf_debug_set_thin(0, 0)
        lib.lf_debug_set_ops_precision(0)


@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("shape", SHAPES)
def test_conv1d_thin_equals_regular_bit_for_bit(lib, shape, C):
    from lanedetection_end2end_amd import _lib
    st = _lib.stream()
    N, H, W, axis, d = shape
    torch.manual_seed(H + W + axis + C)
    x = torch.randn(N, H, W, C, device="cuda")
    add = torch.randn(N, H, W, C, device="cuda")
    w = torch.randn(C, C, 3, device="cuda") * (2.0 / (3 * C)) ** 0.5
    b = torch.randn(C, device="cuda")
    scratch = torch.empty(lib.lf_conv1d_scratch_floats(N, H, W, C) + 4096, device="cuda")
    numel = N * H * W * C
    launches = [("bias + relu", 1), ("bias + residual + relu", 5)]

    def run(mode, nt):
        lib.lf_debug_set_thin(mode, nt)
        before = lib.lf_debug_thin_launches()
        out = {}
        for rep in range(2):
            for name, epi in launches:
                y = guarded(numel)
                rc = lib.lf_debug_conv1d_epi(P(x), P(w), P(b), P(y), 0, epi, None, P(add) if epi & 4 else None, None, None, None, None,
                                             N, H, W, C, axis, d, P(scratch), st)
                assert rc == 0, (name, lib.lf_last_error().decode())
                out[name, rep] = y
        torch.cuda.synchronize()
        return out, lib.lf_debug_thin_launches() - before

    ref, n0 = run(0, 0)
    assert n0 == 0
    for mode, nt in THIN_RUNS:
        got, n = run(mode, nt)
        assert n == 2 * len(launches), (mode, nt, n)
        for key, y in got.items():
            assert torch.isfinite(y[:numel]).all(), (key, mode, nt)
            assert torch.equal(y[:numel], ref[key][:numel]), (key, mode, nt)
            assert bool((y[numel:] == GUARD_VALUE).all()), (key, mode, nt, "guard band behind the destination")
    for key, y in ref.items():
        assert torch.isfinite(y[:numel]).all() and bool((y[numel:] == GUARD_VALUE).all()), key
    # ... and the reference is the convolution (fp64, the tolerance of tests/test_fp32_stream_gpu.py)
    import torch.nn.functional as F
    w4 = (w.view(C, C, 3, 1) if axis == 0 else w.view(C, C, 1, 3)).double()
    pad, dil = ((d, 0), (d, 1)) if axis == 0 else ((0, d), (1, d))
    conv = F.conv2d(x.double().permute(0, 3, 1, 2), w4, b.double(), padding=pad, dilation=dil).permute(0, 2, 3, 1)
    for name, want in (("bias + relu", torch.relu(conv)), ("bias + residual + relu", torch.relu(conv + add.double()))):
        err = float((ref[name, 0][:numel].view(N, H, W, C).double() - want).abs().max()) / float(want.abs().max())
        assert err < 2e-6, (name, err)


# kind 0: the down-samplers' 9-tap stride-2 convolution -- (16, 48) has 48 output channels and 9 K-steps, an odd count: the dead step;
# kind 2: the four sub-pixel phases of an up-sampler
@pytest.mark.parametrize("nhw", [(1, 6, 20), (2, 8, 32)])
@pytest.mark.parametrize("kind, cin, cout", [(0, 64, 64), (0, 16, 48), (2, 128, 64)])
def test_stride2_thin_equals_regular_bit_for_bit(lib, nhw, kind, cin, cout):
    from lanedetection_end2end_amd import _lib
    st = _lib.stream()
    N, H, W = nhw
    torch.manual_seed(H + W + cin + kind)
    if kind == 0:
        src = torch.randn(N, H, W, cin, device="cuda")
        w = torch.randn(cout, cin, 3, 3, device="cuda") * (2.0 / (9 * cin)) ** 0.5
        dshape, phases = (N, H // 2, W // 2, cin + cout), [0]
    else:
        src = torch.randn(N, H // 2, W // 2, cin, device="cuda")
        w = torch.randn(cin, cout, 3, 3, device="cuda") * (2.0 / (9 * cin)) ** 0.5
        dshape, phases = (N, H, W, cout), [0, 1, 2, 3]
    b = torch.randn(cout, device="cuda")
    scratch = torch.empty(9 * 128 * 128 + 4096, device="cuda")
    numel = dshape[0] * dshape[1] * dshape[2] * dshape[3]

    def run(mode, nt):
        lib.lf_debug_set_thin(mode, nt)
        before = lib.lf_debug_thin_launches()
        out = {}
        for rep in range(2):
            for ph in phases:
                y = guarded(numel)
                rc = lib.lf_debug_stride2_epi(kind, ph, P(src), P(w), P(b), P(y), 1, None, None, None, None, N, H, W, cin, cout, P(scratch), st)
                assert rc == 0, (ph, lib.lf_last_error().decode())
                out[ph, rep] = y
        torch.cuda.synchronize()
        return out, lib.lf_debug_thin_launches() - before

    ref, n0 = run(0, 0)
    assert n0 == 0
    # the elements one launch writes: the block's first cout channels (kind 0) / the phase's pixels (kind 2)
    written = {}
    for ph in phases:
        m = torch.zeros(dshape, dtype=torch.bool, device="cuda")
        if kind == 0:
            m[..., :cout] = True
        else:
            m[:, (ph >> 1)::2, (ph & 1)::2, :] = True
        written[ph] = m.view(-1)
    for (ph, rep), y in ref.items():
        assert torch.isfinite(y[:numel][written[ph]]).all() and torch.isnan(y[:numel][~written[ph]]).all(), (ph, rep)
    for mode, nt in [(2, 0), (2, 1), (2, 2), (2, 3), (2, 4)]:
        got, n = run(mode, nt)
        assert n == 2 * len(phases), (mode, nt, n)
        for (ph, rep), y in got.items():
            assert same_bits(y[:numel], ref[ph, rep][:numel]), (ph, rep, mode, nt)      # (NaNs left where nothing is written included)
            assert torch.isfinite(y[:numel][written[ph]]).all(), (ph, rep, mode, nt)
            assert bool((y[numel:] == GUARD_VALUE).all()), (ph, rep, mode, nt, "guard band behind the destination")


def test_launches_the_thin_kernel_is_not_compiled_for_fall_back(lib):
    """Under mode 2: the 16-channel launch of the lean kernel, a statistics epilogue, the BN+ReLU operand prologue and bf16 tensors keep
    their kernels -- equal outputs, the counter does not move."""
    from lanedetection_end2end_amd import _lib
    st = _lib.stream()
    N, H, W, C = 1, 5, 24, 64
    torch.manual_seed(3)
    x = torch.randn(N, H, W, C, device="cuda")
    w = torch.randn(C, C, 3, device="cuda") * (2.0 / (3 * C)) ** 0.5
    b = torch.randn(C, device="cuda")
    sc = torch.rand(C, device="cuda") + 0.5
    sh = torch.randn(C, device="cuda") * 0.5
    scratch = torch.empty(max(lib.lf_conv1d_scratch_floats(N, H, W, C), 9 * 128 * 128) + 4096, device="cuda")
    numel, nrows = N * H * W * C, (N * H * W + 255) // 256
    up_src = torch.randn(2, 4, 16, 64, device="cuda")
    up_w = torch.randn(64, 16, 3, 3, device="cuda") * (2.0 / (9 * 64)) ** 0.5
    up_b = torch.randn(16, device="cuda")
    xb = x.bfloat16()

    def run(mode):
        lib.lf_debug_set_thin(mode, 0)
        before = lib.lf_debug_thin_launches()
        out = {}
        y, s = guarded(numel), guarded(2 * C * nrows)
        assert lib.lf_debug_conv1d_epi(P(x), P(w), P(b), P(y), 0, 8, None, None, None, None, None, P(s), N, H, W, C, 1, 1, P(scratch), st) == nrows
        out["statistics"], out["statistics rows"] = y, s
        y = guarded(numel)
        _lib.check(lib.lf_debug_conv1d_fwd_pro(P(x), P(w), P(b), P(sc), P(sh), P(y), N, H, W, C, 1, 1, P(scratch), st), "prologue")
        out["prologue"] = y
        for ph in range(4):         # UpsamplerBlock(64, 16): Cd = 16, the lean kernel's launch
            y = guarded(2 * 8 * 32 * 16)
            assert lib.lf_debug_stride2_epi(2, ph, P(up_src), P(up_w), P(up_b), P(y), 1, None, None, None, None, 2, 8, 32, 64, 16, P(scratch), st) == 0
            out["lean", ph] = y
        lib.lf_debug_set_ops_precision(2)
        try:
            y = guarded(numel, torch.bfloat16)
            assert lib.lf_debug_conv1d_epi(P(xb), P(w), P(b), P(y), 0, 1, None, None, None, None, None, None, N, H, W, C, 1, 1, P(scratch), st) == 0
            out["bf16"] = y
        finally:
            lib.lf_debug_set_ops_precision(0)
        torch.cuda.synchronize()
        return out, lib.lf_debug_thin_launches() - before

    ref, n0 = run(0)
    got, n2 = run(2)
    assert n0 == 0 and n2 == 0
    for key in ref:
        a, g = ref[key], got[key]
        bits = torch.int16 if a.dtype == torch.bfloat16 else torch.int32
        assert torch.equal(a.view(bits), g.view(bits)), key
        assert bool((g[-GUARD:] == GUARD_VALUE).all()), key
