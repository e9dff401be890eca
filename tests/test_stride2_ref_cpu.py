"""The fp64 reference of tests/test_bf16_stride2_kernels_gpu.py against the modules themselves, without a GPU: problem()'s `want` for
all eight cases is what nn.Conv2d(Cin, Cout, 3, stride=2, padding=1) / nn.ConvTranspose2d(Cin, Cout, 3, stride=2, padding=1,
output_padding=1) compute in fp64 -- the forward by calling them, the data gradients (kinds 1 and 3) by torch.autograd.grad of that
forward with respect to its input --, its term count K is the number of in-range taps times Cs plus 2, and window_pixels() is the
support of the same autograd gradient.  The GPU tests hold the kernels to `want` within gates built from K; this file holds `want`,
K and the windows to the layer's definition."""
import pytest
import torch

import test_bf16_stride2_kernels_gpu as T

CASE_NAMES = "ABCDEFGH"
REF_SHAPES = [(2, 4, 6), (3, 6, 10)]


def module_of(case, w=None, bias=None):
    """The layer of the case in fp64; w / bias None: all-ones weights and no bias (a dependency shows as a non-zero value)."""
    c = T.CASES[case]
    if c["kind"] <= 1:
        m = torch.nn.Conv2d(c["Cin"], c["Cout"], 3, stride=2, padding=1, bias=bias is not None)
    else:
        m = torch.nn.ConvTranspose2d(c["Cin"], c["Cout"], 3, stride=2, padding=1, output_padding=1, bias=bias is not None)
    m = m.double()
    with torch.no_grad():
        if w is None:
            m.weight.fill_(1.0)
        else:
            assert m.weight.shape == w.shape, (case, m.weight.shape, w.shape)
            m.weight.copy_(w.double())
        if bias is not None:
            m.bias.copy_(bias.double())
    return m


def launch_of(case, shape, m, src):
    """What the launch of the case computes from its source tensor (N, h, w, s_pix) NHWC, through module m: NHWC over the produced
    channels.  Kinds 0 / 2: m itself; kinds 1 / 3: the gradient of m's forward with respect to its input, src being the gradient of
    its output."""
    c = T.CASES[case]
    N, H, W = shape
    x = src[..., :c["Cs"]].double().permute(0, 3, 1, 2).contiguous()
    if c["kind"] in (0, 2):
        with torch.no_grad():
            y = m(x)
    else:
        inp = torch.zeros((N, c["Cin"], H, W) if c["kind"] == 1 else (N, c["Cin"], H // 2, W // 2), dtype=torch.float64, requires_grad=True)
        out = m(inp)
        assert out.shape == x.shape, (case, out.shape, x.shape)
        y, = torch.autograd.grad(out, inp, grad_outputs=x)
    return y.permute(0, 2, 3, 1).contiguous()


def finite_src(p, case):
    """the operand without the NaN that case G keeps in the channels its launch does not contract"""
    src = p["src"].clone()
    src[..., T.CASES[case]["Cs"]:] = 0
    return src


@pytest.mark.parametrize("shape", REF_SHAPES, ids=T.shape_id)
@pytest.mark.parametrize("case", CASE_NAMES)
def test_want_is_what_the_modules_compute(case, shape):
    c = T.CASES[case]
    p = T.problem(case, shape, 0)
    assert p["dt"] == torch.float32 and p["w"].dtype == torch.float32
    if c.get("nan_tail"):
        assert torch.isnan(p["src"][..., c["Cs"]:]).all() and torch.isfinite(p["src"][..., :c["Cs"]]).all()
    # (the gradients do not depend on the bias; the cases that have one are the forwards)
    assert (p["bias"] is not None) == (c["kind"] in (0, 2))
    ref = launch_of(case, shape, module_of(case, p["w"], p["bias"]), finite_src(p, case))
    assert ref.shape == p["want"].shape == p["oshape"]
    assert torch.isfinite(p["want"]).all() and torch.isfinite(p["S"]).all()
    err = float((p["want"] - ref).abs().max()) / float(ref.abs().max())
    print("case %s %r: max |want - module| / max |module| = %.3e" % (case, shape, err))
    assert err <= 1e-12
    # S: the same operation on the absolute values, bias included
    refS = launch_of(case, shape, module_of(case, p["w"].abs(), None if p["bias"] is None else p["bias"].abs()), finite_src(p, case).abs())
    assert float((p["S"] - refS).abs().max()) <= 1e-12 * float(refS.abs().max())
    assert (p["S"] >= p["want"].abs() * (1 - 1e-12)).all()


def all_taps_in_range_pixels(case):
    """(phase, (Y, X)) destination pixels all of whose taps lie inside the source, at both REF_SHAPES: the 9-tap windows of small pixel
    (1, 1) cover large rows and columns 1..3; phase (a, b) of large pixel (a, 2 + b) reads small rows 0..a and columns 1..1 + b"""
    if T.CASES[case]["nph"] == 1:
        return [(0, (1, 1))]
    return [(2 * a + b, (a, 2 + b)) for a in range(2) for b in range(2)]


@pytest.mark.parametrize("shape", REF_SHAPES, ids=T.shape_id)
@pytest.mark.parametrize("case", CASE_NAMES)
def test_term_count_is_the_in_range_taps_times_the_source_channels(case, shape):
    """K at a pixel with every tap in range, per phase: the source PIXELS that destination pixel depends on -- counted through the
    all-ones module -- times Cs, + 2."""
    c = T.CASES[case]
    p = T.problem(case, shape, 0)
    N, H, W = shape
    sshape, dshape = T.sizes(case, shape)
    m = module_of(case)
    K = p["K"].expand(1, dshape[1], dshape[2], 1)
    seen = set()
    for ph, (Y, X) in all_taps_in_range_pixels(case):
        # the launch is linear: probe it with one-hot sources, pixel by pixel
        deps = 0
        for y in range(sshape[1]):
            for x in range(sshape[2]):
                src = torch.zeros(sshape, dtype=torch.float64)
                src[0, y, x, 0] = 1.0
                deps += int(launch_of(case, shape, m, src)[0, Y, X, 0] != 0)
        want_taps = 9 if c["nph"] == 1 else (1 + (ph >> 1)) * (1 + (ph & 1))
        assert deps == want_taps, (case, ph, deps)
        assert float(K[0, Y, X, 0]) == deps * c["Cs"] + 2, (case, ph, float(K[0, Y, X, 0]), deps)
        seen.add(deps)
    assert seen == ({9} if c["nph"] == 1 else {1, 2, 4})
    # and nowhere does a pixel have MORE terms than K allows it (edges have fewer: K is an upper bound there)
    ones = torch.zeros(sshape, dtype=torch.float64)
    ones[..., :c["Cs"]] = 1.0
    terms = launch_of(case, shape, m, ones)[..., :1]
    assert (terms + 2 <= K).all() and float((K - terms).min()) == 2.0


@pytest.mark.parametrize("case", CASE_NAMES)
def test_window_pixels_is_the_support_of_the_autograd_gradient(case):
    """One planted source element per position of planted_positions(): the destination pixels the all-ones module carries it to are
    exactly window_pixels() -- for case G's position d, in the channels the launch does not contract, none."""
    shape = (3, 6, 10)
    sshape, dshape = T.sizes(case, shape)
    m = module_of(case)
    names = []
    for name, pos in T.planted_positions(case, sshape):
        src = torch.zeros(sshape, dtype=torch.float64)
        src[pos] = 1.0
        support = (launch_of(case, shape, m, src) != 0).any(-1).numpy()
        want = T.window_pixels(case, shape, pos)
        assert want.shape == support.shape == dshape[:3]
        assert (support == want).all(), (case, name, support.sum(), want.sum())
        assert name == "d" or want.any()
        names.append(name)
    assert names == (["a", "b", "c", "d"] if case in "CG" else ["a", "b", "c"])
