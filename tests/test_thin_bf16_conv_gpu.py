"""tapgemm_bf16_thin_kernel (csrc/lf_conv_bf16.hip: the thin tiling -- one 16-pixel tile per wave -- on bf16 tensors and the bf16 matrix
cores, for launches whose regular grid cannot fill the device) against the kernels the same launch takes without it (wave-private,
whole-line, ring, streaming), ONE LAUNCH AT A TIME through the debug hooks in precision mode 2: outputs bit for bit for every slab
count per wave, twice in a row, NaN pre-fill and a guard band behind every destination, the launch counter exact; the mode-0
reference against torch fp64; the 16-source-channel form with non-finite neighbours; and the launches the kernel is not compiled
for fall back.

The fp64 gate (derived, not measured).  The kernel sees bf16 tensors and bf16-rounded weights, multiplies them exactly (a product
of two bf16 values has 16 significant bits) and adds the K = taps * Cs products, the bias and the residual -- K + 2 terms -- in fp32 in
some order: any order is within (K + 2) * 2^-24 * S of the exact sum to first order, S = sum |w * x| of the element; the factor 2
covers the higher-order terms and the bias / residual magnitudes, which S leaves out.  ReLU does not increase a difference.  The
store rounds to bf16, 8 significant bits: half an ulp is at most 2^-8 * |want|.  So
    |got - want| <= 2^-8 * |want| + 2 * (K + 2) * 2^-24 * S        per element."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 4096
GUARD_VALUE = -12288.0       # no kernel produces it; exact in bf16
BF = torch.bfloat16
# (N, H, W, axis, dilation): 120 pixels = a last workgroup of 56 pixels whose last wave has 8 live ones, ragged rows (both axes);
# whole rows with a tile sequence across the image boundary; large dilation; dilation >= H (both outer taps padding) in exactly
# one workgroup; 24 pixels -- less than one workgroup -- over three images
SHAPES = [(1, 5, 24, 0, 1), (1, 5, 24, 1, 2), (2, 3, 64, 1, 1), (1, 6, 128, 1, 16), (1, 4, 16, 0, 8), (3, 1, 8, 1, 1)]
THIN_RUNS = [(2, 0), (2, 1), (2, 2), (2, 4)]


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def guarded(n, dtype=BF):
    """n NaNs (every stored element must overwrite one) and a guard band of a value no kernel produces"""
    t = torch.full((n + GUARD,), float("nan"), device="cuda", dtype=dtype)
    t[n:] = GUARD_VALUE
    return t


def same_bits(a, b):
    bits = {2: torch.int16, 4: torch.int32}[a.element_size()]
    return a.dtype == b.dtype and torch.equal(a.contiguous().view(bits), b.contiguous().view(bits))


def gate_ok(got, want, S, K):
    """the module docstring's per-element gate; prints the worst ratio before it decides"""
    err = (got.double() - want).abs()
    bound = 2.0 ** -8 * want.abs() + 2.0 * (K + 2) * 2.0 ** -24 * S
    print("worst |got - want| / bound: %.3f" % float((err / bound.clamp_min(1e-300)).max()))
    return bool((err <= bound).all())


@pytest.fixture
def lib():
    from lanedetection_end2end_amd import _lib
    lib = _lib.load()
    lib.lf_debug_set_ops_precision(2)
    try:
        yield lib
    finally:
        lib.lf_debug_set_thin_bf16(0, 0)
        lib.lf_debug_set_thin(0, 0)
        lib.lf_debug_set_ops_precision(0)


@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("shape", SHAPES)
def test_conv1d_thin_equals_regular_bit_for_bit(lib, shape, C):
    import torch.nn.functional as F
    from lanedetection_end2end_amd import _lib
    st = _lib.stream()
    N, H, W, axis, d = shape
    torch.manual_seed(H + W + axis + C)
    x = torch.randn(N, H, W, C, device="cuda").to(BF)
    add = torch.randn(N, H, W, C, device="cuda").to(BF)
    w = torch.randn(C, C, 3, device="cuda") * (2.0 / (3 * C)) ** 0.5
    b = torch.randn(C, device="cuda")
    scratch = torch.empty(lib.lf_conv1d_scratch_floats(N, H, W, C) + 4096, device="cuda")
    numel = N * H * W * C
    launches = [("bias + relu", 1), ("bias + residual + relu", 5)]

    def run(mode, nt):
        lib.lf_debug_set_thin_bf16(mode, nt)
        before, before32 = lib.lf_debug_thin_bf16_launches(), lib.lf_debug_thin_launches()
        out = {}
        for rep in range(2):
            for name, epi in launches:
                y = guarded(numel)
                rc = lib.lf_debug_conv1d_epi(P(x), P(w), P(b), P(y), 0, epi, None, P(add) if epi & 4 else None, None, None, None, None,
                                             N, H, W, C, axis, d, P(scratch), st)
                assert rc == 0, (name, lib.lf_last_error().decode())
                out[name, rep] = y
        torch.cuda.synchronize()
        assert lib.lf_debug_thin_launches() == before32
        return out, lib.lf_debug_thin_bf16_launches() - before

    ref, n0 = run(0, 0)
    assert n0 == 0
    for mode, nt in THIN_RUNS:
        got, n = run(mode, nt)
        assert n == 2 * len(launches), (mode, nt, n)
        for key, y in got.items():
            assert torch.isfinite(y[:numel]).all(), (key, mode, nt)
            assert same_bits(y[:numel], ref[key][:numel]), (key, mode, nt)
            assert bool((y[numel:] == GUARD_VALUE).all()), (key, mode, nt, "guard band behind the destination")
    for key, y in ref.items():
        assert torch.isfinite(y[:numel]).all() and bool((y[numel:] == GUARD_VALUE).all()), key
    # ... and the reference is the convolution: fp64 on the operands the kernel sees (bf16 tensors, bf16-rounded weights)
    wr = w.to(BF).double()
    w4, a4 = (wr.view(C, C, 3, 1), (d, 0)) if axis == 0 else (wr.view(C, C, 1, 3), (0, d))
    dil = (d, 1) if axis == 0 else (1, d)
    xs = x.double().permute(0, 3, 1, 2)
    conv = F.conv2d(xs, w4, b.double(), padding=a4, dilation=dil).permute(0, 2, 3, 1)
    S = F.conv2d(xs.abs(), w4.abs(), None, padding=a4, dilation=dil).permute(0, 2, 3, 1)
    for name, want in (("bias + relu", torch.relu(conv)), ("bias + residual + relu", torch.relu(conv + add.double()))):
        assert gate_ok(ref[name, 0][:numel].view(N, H, W, C), want, S, 3 * C), name


def stride2_problem(kind, cin, cout, nhw):
    N, H, W = nhw
    torch.manual_seed(H + W + cin + kind)
    if kind == 0:
        src = torch.randn(N, H, W, cin, device="cuda").to(BF)
        w = torch.randn(cout, cin, 3, 3, device="cuda") * (2.0 / (9 * cin)) ** 0.5
        dshape, phases = (N, H // 2, W // 2, cin + cout), [0]
    else:
        src = torch.randn(N, H // 2, W // 2, cin, device="cuda").to(BF)
        w = torch.randn(cin, cout, 3, 3, device="cuda") * (2.0 / (9 * cin)) ** 0.5
        dshape, phases = (N, H, W, cout), [0, 1, 2, 3]
    b = torch.randn(cout, device="cuda")
    # the elements one launch writes: the block's first cout channels (kind 0) / the phase's pixels (kind 2)
    written = {}
    for ph in phases:
        m = torch.zeros(dshape, dtype=torch.bool, device="cuda")
        if kind == 0:
            m[..., :cout] = True
        else:
            m[:, (ph >> 1)::2, (ph & 1)::2, :] = True
        written[ph] = m.view(-1)
    return src, w, b, dshape, phases, written


# kind 0: the down-samplers' 9-tap stride-2 convolution -- (16, 48) has 16 source channels (one half-filled step per tap), 48 output
# channels and 9 K-steps, an odd count: the dead step; kind 2: the four sub-pixel phases of an up-sampler (1, 2, 2 and 4 taps)
@pytest.mark.parametrize("nhw", [(1, 6, 20), (2, 8, 32)])
@pytest.mark.parametrize("kind, cin, cout", [(0, 64, 64), (0, 16, 48), (2, 128, 64)])
def test_stride2_thin_equals_regular_bit_for_bit(lib, nhw, kind, cin, cout):
    import torch.nn.functional as F
    from lanedetection_end2end_amd import _lib
    st = _lib.stream()
    N, H, W = nhw
    src, w, b, dshape, phases, written = stride2_problem(kind, cin, cout, nhw)
    scratch = torch.empty(9 * 128 * 128 + 4096, device="cuda")
    numel = dshape[0] * dshape[1] * dshape[2] * dshape[3]

    def run(mode, nt):
        lib.lf_debug_set_thin_bf16(mode, nt)
        before, before32 = lib.lf_debug_thin_bf16_launches(), lib.lf_debug_thin_launches()
        out = {}
        for rep in range(2):
            for ph in phases:
                y = guarded(numel)
                rc = lib.lf_debug_stride2_epi(kind, ph, P(src), P(w), P(b), P(y), 1, None, None, None, None, N, H, W, cin, cout, P(scratch), st)
                assert rc == 0, (ph, lib.lf_last_error().decode())
                out[ph, rep] = y
        torch.cuda.synchronize()
        assert lib.lf_debug_thin_launches() == before32
        return out, lib.lf_debug_thin_bf16_launches() - before

    ref, n0 = run(0, 0)
    assert n0 == 0
    for (ph, rep), y in ref.items():
        assert torch.isfinite(y[:numel][written[ph]]).all() and torch.isnan(y[:numel][~written[ph]]).all(), (ph, rep)
        assert bool((y[numel:] == GUARD_VALUE).all()), (ph, rep)
    for nt in [n for n in (0, 1, 2, 3, 4) if n == 0 or (cout // 16) % n == 0]:
        got, n = run(2, nt)
        assert n == 2 * len(phases), (nt, n)
        for (ph, rep), y in got.items():
            assert same_bits(y[:numel], ref[ph, rep][:numel]), (ph, rep, nt)      # (NaNs left where nothing is written included)
            assert torch.isfinite(y[:numel][written[ph]]).all(), (ph, rep, nt)
            assert bool((y[numel:] == GUARD_VALUE).all()), (ph, rep, nt, "guard band behind the destination")
    # ... and the reference is the layer, in fp64 on the operands the kernel sees
    wr, xs = w.to(BF).double(), src.double().permute(0, 3, 1, 2)
    if kind == 0:
        conv = F.conv2d(xs, wr, b.double(), stride=2, padding=1).permute(0, 2, 3, 1)
        S = F.conv2d(xs.abs(), wr.abs(), None, stride=2, padding=1).permute(0, 2, 3, 1)
        got = ref[0, 0][:numel].view(dshape)[..., :cout]
        assert gate_ok(got, torch.relu(conv), S, 9 * cin)
    else:
        conv = F.conv_transpose2d(xs, wr, b.double(), stride=2, padding=1, output_padding=1).permute(0, 2, 3, 1)
        S = F.conv_transpose2d(xs.abs(), wr.abs(), None, stride=2, padding=1, output_padding=1).permute(0, 2, 3, 1)
        for ph in phases:
            a, c = ph >> 1, ph & 1
            taps = (2 if a else 1) * (2 if c else 1)
            got = ref[ph, 0][:numel].view(dshape)[:, a::2, c::2, :]
            assert gate_ok(got, torch.relu(conv[:, a::2, c::2, :]), S[:, a::2, c::2, :], taps * cin), ph


# where the one non-finite source pixel sits, (image, row, column) of the (2, 8, 32) source.  An unguarded lane kq = 2, 3 of source pixel
# p reads the 32 bytes behind p's own: pixel p + 1 in memory order.  So the pixel that would leak the planted one is its PREDECESSOR,
# and the test sees the leak only if some output window holds the predecessor and not the planted pixel (windows are columns
# 2j - 1 .. 2j + 1, rows 2i - 1 .. 2i + 1):
#   even column 8: the predecessor, column 7, is also in the window of j = 3 (columns 5 .. 7), which does not hold column 8;
#   odd column 7: the predecessor, column 6, lies in the window of j = 3 only, which holds column 7 too -- no clean window can show
#     a leak here; kept for the other parity of the planted pixel's own windows;
#   column 0 of row 4: the predecessor is the LAST column of row 3, read by outputs (i = 1 and 2, j = 15) at the other end of
#     the image row, none of which holds column 0;
#   pixel (1, 0, 0): the predecessor is the last pixel of image 0, read by output (0, 3, 15) of the other image
PLANTS = [(1, 3, 8), (1, 3, 7), (1, 4, 0), (1, 0, 0)]


@pytest.mark.parametrize("plant", PLANTS)
@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan")])
def test_16_source_channels_do_not_read_the_next_pixel(lib, bad, plant):
    """DownsamplerBlock(16, 64)'s 16 -> 48 convolution: a pixel is 32 bytes, the lanes of channels 16..31 of the one half-filled step
    would read the NEXT pixel -- its Inf / NaN against the zero-padded weights is NaN in every output channel.  One non-finite
    source pixel: every output pixel whose 3x3 window does not contain it keeps the clean run's bits."""
    from lanedetection_end2end_amd import _lib
    st = _lib.stream()
    kind, cin, cout, (N, H, W) = 0, 16, 48, (2, 8, 32)
    src, w, b, dshape, phases, written = stride2_problem(kind, cin, cout, (N, H, W))
    scratch = torch.empty(9 * 128 * 128 + 4096, device="cuda")
    numel = dshape[0] * dshape[1] * dshape[2] * dshape[3]
    pn, py, px = plant
    dirty = src.clone()
    dirty[pn, py, px, :] = bad

    def window_holds(n, y, x):
        """the output pixels whose window holds source pixel (n, y, x): rows 2i - 1 .. 2i + 1, columns 2j - 1 .. 2j + 1"""
        m = torch.zeros(dshape[:3], dtype=torch.bool, device="cuda")
        for i in range(H // 2):
            for j in range(W // 2):
                if abs(2 * i - y) <= 1 and abs(2 * j - x) <= 1:
                    m[n, i, j] = True
        return m

    touched = window_holds(pn, py, px)
    assert int(touched.sum()) > 0
    # the plant is one the test can see a leak at (all but the odd column): a clean window holds the predecessor in memory order
    flat = (pn * H + py) * W + px - 1
    pred = window_holds(flat // (H * W), flat // W % H, flat % W)
    assert bool((pred & ~touched).any()) == (plant != (1, 3, 7))

    def run(x, nt):
        lib.lf_debug_set_thin_bf16(2, nt)
        before = lib.lf_debug_thin_bf16_launches()
        y = guarded(numel)
        assert lib.lf_debug_stride2_epi(kind, 0, P(x), P(w), P(b), P(y), 1, None, None, None, None, N, H, W, cin, cout, P(scratch), st) == 0
        torch.cuda.synchronize()
        assert lib.lf_debug_thin_bf16_launches() == before + 1
        return y

    for nt in (0, 1, 3):
        clean, got = run(src, nt), run(dirty, nt)
        c4, g4 = clean[:numel].view(dshape)[..., :cout], got[:numel].view(dshape)[..., :cout]
        assert torch.isfinite(c4).all()
        assert same_bits(g4[~touched], c4[~touched]), nt
        assert not torch.isfinite(g4[touched]).all(), nt          # (the window that holds the pixel does see it)
        assert bool((got[numel:] == GUARD_VALUE).all()), nt


def test_launches_the_thin_kernel_is_not_compiled_for_fall_back(lib):
    """Under mode 2: a statistics epilogue, the BN+ReLU operand prologue, the Cd = 16 up-sampler phase and an fp32 launch keep their
    kernels -- equal outputs, and neither thin counter moves."""
    from lanedetection_end2end_amd import _lib
    st = _lib.stream()
    N, H, W, C = 1, 5, 24, 64
    torch.manual_seed(3)
    x32 = torch.randn(N, H, W, C, device="cuda")
    x = x32.to(BF)
    w = torch.randn(C, C, 3, device="cuda") * (2.0 / (3 * C)) ** 0.5
    b = torch.randn(C, device="cuda")
    sc = torch.rand(C, device="cuda") + 0.5
    sh = torch.randn(C, device="cuda") * 0.5
    scratch = torch.empty(max(lib.lf_conv1d_scratch_floats(N, H, W, C), 9 * 128 * 128) + 4096, device="cuda")
    numel, nrows = N * H * W * C, (N * H * W + 255) // 256
    up_src = torch.randn(2, 4, 16, 64, device="cuda").to(BF)
    up_w = torch.randn(64, 16, 3, 3, device="cuda") * (2.0 / (9 * 64)) ** 0.5
    up_b = torch.randn(16, device="cuda")

    def run(mode):
        lib.lf_debug_set_thin_bf16(mode, 0)
        before, before32 = lib.lf_debug_thin_bf16_launches(), lib.lf_debug_thin_launches()
        out = {}
        y, s = guarded(numel), guarded(2 * C * nrows, torch.float32)
        assert lib.lf_debug_conv1d_epi(P(x), P(w), P(b), P(y), 0, 8, None, None, None, None, None, P(s), N, H, W, C, 1, 1, P(scratch), st) == nrows
        out["statistics"], out["statistics rows"] = y, s
        y = guarded(numel)
        _lib.check(lib.lf_debug_conv1d_fwd_pro(P(x), P(w), P(b), P(sc), P(sh), P(y), N, H, W, C, 1, 1, P(scratch), st), "prologue")
        out["prologue"] = y
        for ph in range(4):         # UpsamplerBlock(64, 16): Cd = 16
            y = guarded(2 * 8 * 32 * 16)
            assert lib.lf_debug_stride2_epi(2, ph, P(up_src), P(up_w), P(up_b), P(y), 1, None, None, None, None, 2, 8, 32, 64, 16, P(scratch), st) == 0
            out["Cd 16", ph] = y
        lib.lf_debug_set_ops_precision(0)
        try:
            y = guarded(numel, torch.float32)
            assert lib.lf_debug_conv1d_epi(P(x32), P(w), P(b), P(y), 0, 1, None, None, None, None, None, None, N, H, W, C, 1, 1, P(scratch), st) == 0
            out["fp32"] = y
        finally:
            lib.lf_debug_set_ops_precision(2)
        torch.cuda.synchronize()
        return out, lib.lf_debug_thin_bf16_launches() - before, lib.lf_debug_thin_launches() - before32

    ref, n0, m0 = run(0)
    got, n2, m2 = run(2)
    assert (n0, m0, n2, m2) == (0, 0, 0, 0)
    for key in ref:
        assert same_bits(ref[key], got[key]), key
        assert bool((got[key][-GUARD:] == GUARD_VALUE).all()), key
