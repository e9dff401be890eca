"""The weight gradients outside the 3-tap C -> C geometry ONE LAYER AT A TIME, as the plan issues them: the stride-2 convolution
and the four sub-pixel phases of the transposed convolution through lf_debug_stride2_wgrad (tapwgrad_kernel over the plan's own
geometries, csrc/lf_plan.h, then the immediate or the batched reduction with its chained bias rows), the stem and the head through
lf_debug_stem_wgrad / lf_debug_head_wgrad (stem_wgrad_kernel / head_wgrad_kernel and their row sums) -- against torch on the CPU in
fp64, fed the operands as the kernel sees them (bf16-rounded activations and gradients in mode 2; partial rows and gradients fp32).

Two data sets per case:

  integers   every element from {-2, -1, 1, 2} (no zeros: a padding tap that reads a neighbour shows).  Every product and every
             partial sum is an integer far below 2^24 (|sum| <= 4 * pixels: about 8e3 at the largest stride-2 shape, 4 * 147,712 at
             the capped stem / head shape), so fp32 is exact in ANY summation order and the result must EQUAL the fp64 reference:
             one dropped, doubled or misplaced pixel, tap or bias row fails.
  Gaussian   randn (x: randn + 0.25), which integers cannot replace for reduced-precision accumulation.  Two gates, neither fitted to
             the kernels: per element |got - want| <= K * 2^-23 * S with S the same gradient of |x| and |g| and K = logical
             pixels + 2 (any fp32 summation order of n terms is within n * 2^-24 * S of the exact sum: the per-element gate of
             tests/test_bf16_stride2_kernels_gpu.py), and max |got - want| / max |want| < 3e-6 (what
             test_fp32_kernel_parity_every_addressing_path holds the 3-tap weight gradient to).  Both measured values are printed.

Stride-2 layers: Down(16 -> 48 of 64), Down(64 -> 64 of 128), Up(128 -> 64), Up(64 -> 16).  Shapes (N, H, W) of the LARGER tensor,
the smallest that reach each path of wgrad_cfg (csrc/lf_wgrad.hip) as it stands (logical pixels = N * H/2 * W/2; a wave walks its pixels in
groups of 4 * U; rows = workgroup rows = partial rows per launch):

  shape        pixels  U  rows       reaches
  (3, 6, 16)       72  1  1          one workgroup, waves of 20/20/20/12 pixels, image boundaries inside a wave
  (2, 10, 32)     160  4  1          16-pixel groups, a last wave of 16 of 48
  (2, 20, 40)     400  1  2          two workgroup rows with a ragged tail; phase grids 4 / 8 / 16: with and without the
                                     (gridDim.x & 7) == 0 workgroup remap
  (1, 32, 48)     384  1  2          width 24, reachable in the network
  (2, 64, 64)    2048  4  8          every launch takes the remap; the BFM form in mode 2
  (3, 16, 96)    1152  4  4 or 5     the four phases write DIFFERENT numbers of rows (4/4/4/5 at 128 -> 64, 5/4/4/4 at 64 -> 16):
                                     chained bias rows and n_bias_rows

Stem (Cin 1, 3, 4: 1, 2, 3 column tiles, the ones-column that carries the bias in a different tile each time) and head (K 1, 2, 3,
5), shapes (N, Ho, Wo) of the half-resolution grid (16-pixel groups, workgroups = partial rows):

  (1, 1, 16)         1 group      1 workgroup   one wave works, three are idle
  (3, 3, 16)         9 groups     2             workgroups of 5 and 4 groups, image boundaries inside a workgroup
  (2, 9, 32)        36 groups     5             the last workgroup has 4 groups
  (2, 577, 128)   9232 groups     1024 (cap)    10 groups each: about 100 trailing workgroups own nothing and must write zero rows
                                                (Cin 3 / K 2, integers only)

The test does not compute any of this: the hooks return the rows written, which must be > 1 where the table says so (a changed
wgrad_cfg cannot quietly turn these into single-workgroup cases), differ between the phases at (3, 16, 96), and be 1024 at the cap.

Memory, every case: x and g lie inside NaN-filled allocations (the pooled channels of Down's / the stem's concat gradient hold NaN
too); the partial-row scratch is NaN up to lf_debug_*_scratch_floats with a canary band directly behind it, so a finite result means
every row a reduction read was written and no operand was read out of bounds; gw is pre-filled with a canary pattern which no element
may keep (the four phases cover the nine 3x3 elements), gb with NaN (the first phase must store, the later ones accumulate); both sit
between canary guard bands.  Two consecutive runs agree bit for bit; gb = null leaves a bias buffer untouched and gw unchanged.
Each reduce route is compared with the reference, never with the other route.
"""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 4096                       # elements either side of every tensor (a multiple of 64: the carved tensor stays 256-byte aligned)
CANARY = {torch.bfloat16: (torch.int16, 0x5A5B), torch.float32: (torch.int32, 0x5A5B5C5D)}
NAN = float("nan")

LAYERS = {"down16_48": dict(kind=0, Cin=16, Cout=48), "down64_64": dict(kind=0, Cin=64, Cout=64),
          "up128_64": dict(kind=2, Cin=128, Cout=64), "up64_16": dict(kind=2, Cin=64, Cout=16)}
SHAPES = [(3, 6, 16), (2, 10, 32), (2, 20, 40), (1, 32, 48), (2, 64, 64), (3, 16, 96)]
MULTI_ROW = {(2, 20, 40), (1, 32, 48), (2, 64, 64), (3, 16, 96)}       # more than one partial row per launch
UNEQUAL_PHASES = (3, 16, 96)                                          # Up: the phases write different numbers of rows

END_SHAPES = [(1, 1, 16), (3, 3, 16), (2, 9, 32)]
END_MULTI_ROW = {(3, 3, 16), (2, 9, 32)}
CAPPED = (2, 577, 128)


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def carve(shape, dtype, fill=None):
    """(whole allocation, the tensor in its middle).  fill None: the canary bit pattern everywhere."""
    n = 1
    for s in shape:
        n *= s
    if fill is None:
        idt, pat = CANARY[dtype]
        whole = torch.full((n + 2 * GUARD,), pat, dtype=idt, device="cuda").view(dtype)
    else:
        whole = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    return whole, whole[GUARD:GUARD + n].view(shape)


def is_canary(t):
    idt, pat = CANARY[t.dtype]
    return t.contiguous().view(idt) == pat


def guards_intact(whole):
    return bool(is_canary(whole[:GUARD]).all() and is_canary(whole[-GUARD:]).all())


def guarded_scratch(nfloats):
    """NaN up to nfloats, the canary band directly behind."""
    whole = torch.full((nfloats + GUARD,), CANARY[torch.float32][1], dtype=torch.int32, device="cuda").view(torch.float32)
    whole[:nfloats] = NAN
    return whole


def draw(gen, data, shape, shift=0.0):
    if data == "int":
        return torch.tensor([-2.0, -1.0, 1.0, 2.0])[torch.randint(0, 4, shape, generator=gen)]
    return torch.randn(*shape, generator=gen) + shift


def nchw(t):
    return t.double().permute(0, 3, 1, 2).contiguous()


# ---- the stride-2 layers ----------------------------------------------------------------------------------------------------------

def stride2_grads(kind, Cin, Cout, xn, gn):
    """fp64 (gw, gb) of the layer from NCHW operands."""
    import torch.nn.functional as F
    if kind == 0:
        gw = torch.nn.grad.conv2d_weight(xn, (Cout, Cin, 3, 3), gn, stride=2, padding=1)
    else:
        w = torch.zeros(Cin, Cout, 3, 3, dtype=torch.float64, requires_grad=True)
        (F.conv_transpose2d(xn, w, None, stride=2, padding=1, output_padding=1) * gn).sum().backward()
        gw = w.grad
    return gw, gn.sum((0, 2, 3))


@functools.lru_cache(maxsize=None)
def stride2_problem(layer, shape, mode, data):
    """Operands as the kernel sees them (NHWC; g: the produced channels only) and the fp64 reference, once per case."""
    c = LAYERS[layer]
    N, H, W = shape
    dt = torch.bfloat16 if mode == 2 else torch.float32
    gen = torch.Generator().manual_seed(7919 * list(LAYERS).index(layer) + 31 * H * W + 3 * mode + (data == "int"))
    small, large = (N, H // 2, W // 2), (N, H, W)
    xs, gs = (large, small) if c["kind"] == 0 else (small, large)
    x = draw(gen, data, xs + (c["Cin"],), 0.25).to(dt)
    g = draw(gen, data, gs + (c["Cout"],)).to(dt)
    xn, gn = nchw(x), nchw(g)
    gw, gb = stride2_grads(c["kind"], c["Cin"], c["Cout"], xn, gn)
    p = dict(x=x, g=g, gw=gw, gb=gb, dt=dt, K=N * (H // 2) * (W // 2) + 2)
    if data == "gauss":
        p["Sw"], p["Sb"] = stride2_grads(c["kind"], c["Cin"], c["Cout"], xn.abs(), gn.abs())
    return p


def check_result(tag, p, data, gw, gb):
    """gw / gb (device, fp32) against the problem's reference: equal on integers, inside both gates on Gaussian data."""
    assert torch.isfinite(gw).all(), tag + ": gw not finite (an unwritten partial row or an operand read out of bounds)"
    assert not is_canary(gw).any(), tag + ": %d elements of gw never written" % int(is_canary(gw).sum())
    pairs = [("gw", gw.double().cpu(), p["gw"], p.get("Sw"))]
    if gb is not None:
        assert torch.isfinite(gb).all(), tag + ": gb not finite (the first launch must store, not accumulate)"
        pairs.append(("gb", gb.double().cpu(), p["gb"], p.get("Sb")))
    for name, got, want, S in pairs:
        assert got.shape == want.shape
        if data == "int":
            bad = got != want
            assert not bad.any(), "%s: %s differs from the exact result in %d of %d elements, first at %s: got %s, want %s" % (
                tag, name, int(bad.sum()), bad.numel(), bad.nonzero()[0].tolist(), float(got[bad][0]), float(want[bad][0]))
        else:
            err = (got - want).abs()
            gate = p["K"] * 2.0 ** -23 * S
            frac = float((err / gate).max())
            rel = float(err.max() / want.abs().max())
            print("%s %s: max err / element gate = %.2e, max-norm relative error = %.2e (%.3f of 3e-6)" % (tag, name, frac, rel, rel / 3e-6))
            assert (err <= gate).all(), (tag, name, frac, int((err > gate).sum()))
            assert rel < 3e-6, (tag, name, rel)


class Stride2:
    """Device copies of a problem's operands inside NaN-filled allocations, and one whole weight gradient per call."""

    def __init__(self, layer, shape, mode, data):
        from lanedetection_end2end_amd import _lib
        self.lib, self.st = _lib.load(), _lib.stream()
        self.c, self.shape = LAYERS[layer], shape
        p = self.p = stride2_problem(layer, shape, mode, data)
        c = self.c
        self.x_whole, self.x = carve(tuple(p["x"].shape), p["dt"], NAN)
        self.x.copy_(p["x"])
        gshape = tuple(p["g"].shape[:3]) + ((c["Cin"] + c["Cout"],) if c["kind"] == 0 else (c["Cout"],))
        self.g_whole, self.g = carve(gshape, p["dt"], NAN)      # Down: the pooled channels [Cout, Cin + Cout) keep their NaN
        self.g[..., :c["Cout"]] = p["g"].cuda()
        self.wshape = (c["Cout"], c["Cin"], 3, 3) if c["kind"] == 0 else (c["Cin"], c["Cout"], 3, 3)

    def __call__(self, reduce, bias=True):
        """(gw, gb or None, rows); asserts what every call must keep."""
        c, lib = self.c, self.lib
        N, H, W = self.shape
        nfl = lib.lf_debug_stride2_wgrad_scratch_floats(c["kind"], reduce, N, H, W, c["Cin"], c["Cout"])
        assert nfl > 0, lib.lf_last_error().decode()
        scratch = guarded_scratch(nfl)
        gw_whole, gw = carve(self.wshape, torch.float32)
        gb_whole, gb = carve((c["Cout"],), torch.float32, NAN if bias else None)
        rows = lib.lf_debug_stride2_wgrad(c["kind"], reduce, P(self.x), P(self.g), P(gw), P(gb) if bias else None, N, H, W, c["Cin"],
                                          c["Cout"], P(scratch), self.st)
        assert rows >= 1, (rows, lib.lf_last_error().decode())
        torch.cuda.synchronize()
        assert is_canary(scratch[nfl:]).all(), "floats behind the partial-row scratch written"
        assert guards_intact(gw_whole), "guard band of gw written"
        if bias:
            assert torch.isnan(gb_whole[:GUARD]).all() and torch.isnan(gb_whole[-GUARD:]).all(), "guard band of gb written"
        else:
            assert is_canary(gb_whole).all(), "gb = null: the bias buffer was written"
        # rows: every one of them holds at least one tap's Cin x Cout block and one bias row of the batched route's regions
        nph = 1 if c["kind"] == 0 else 4
        per_row = (9 if nph == 1 else 1) * c["Cin"] * c["Cout"] + c["Cout"]
        bound = lib.lf_debug_stride2_wgrad_scratch_floats(c["kind"], 1, N, H, W, c["Cin"], c["Cout"]) // per_row
        assert nph <= rows <= bound, (rows, bound)
        if self.shape in MULTI_ROW:
            assert rows >= 2 * nph, "%r is meant to give every launch more than one partial row: %d rows in %d launches" % (self.shape, rows, nph)
        if self.shape == UNEQUAL_PHASES and nph == 4:
            assert rows % 4 != 0, "%r is meant to give the four phases different numbers of rows: %d in all" % (self.shape, rows)
        return gw, (gb if bias else None), rows


@pytest.mark.parametrize("mode", [0, 2], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("layer", list(LAYERS))
def test_stride2_weight_gradient_against_fp64(layer, shape, mode):
    """Both data sets through both reduce routes, each against the fp64 reference; run-to-run bit identity; gb = null."""
    from lanedetection_end2end_amd import _lib
    lib = _lib.load()
    try:
        lib.lf_debug_set_ops_precision(mode)
        for data in ("int", "gauss"):
            L = Stride2(layer, shape, mode, data)
            for reduce in (0, 1):
                tag = "%s %r mode %d %s reduce %d" % (layer, shape, mode, data, reduce)
                gw, gb, rows = L(reduce)
                check_result(tag, L.p, data, gw, gb)
                gw2, gb2, rows2 = L(reduce)
                assert rows2 == rows and torch.equal(gw.view(torch.int32), gw2.view(torch.int32)) and \
                    torch.equal(gb.view(torch.int32), gb2.view(torch.int32)), tag + ": two runs differ"
                gw3, _, rows3 = L(reduce, bias=False)
                assert rows3 == rows and torch.equal(gw.view(torch.int32), gw3.view(torch.int32)), tag + ": gw changes with gb = null"
    finally:
        lib.lf_debug_set_ops_precision(0)


def test_stride2_weight_gradient_hook_refuses_other_modes():
    """Precision modes other than 0 and 2, the data-gradient kinds of lf_debug_stride2_epi and odd sizes are errors, not launches."""
    from lanedetection_end2end_amd import _lib
    lib = _lib.load()
    t = torch.zeros(64, device="cuda")
    try:
        lib.lf_debug_set_ops_precision(9)
        assert lib.lf_debug_stride2_wgrad_scratch_floats(0, 0, 1, 8, 16, 16, 48) == -1
        assert lib.lf_debug_stride2_wgrad(0, 0, P(t), P(t), P(t), None, 1, 8, 16, 16, 48, P(t), _lib.stream()) == -1
        lib.lf_debug_set_ops_precision(0)
        for kind, reduce, H in ((1, 0, 8), (3, 0, 8), (0, 2, 8), (0, 0, 7)):
            assert lib.lf_debug_stride2_wgrad_scratch_floats(kind, reduce, 1, H, 16, 16, 48) == -1
            assert lib.lf_debug_stride2_wgrad(kind, reduce, P(t), P(t), P(t), None, 1, H, 16, 16, 48, P(t), _lib.stream()) == -1
    finally:
        lib.lf_debug_set_ops_precision(0)
        torch.cuda.synchronize()


# ---- the stem and the head --------------------------------------------------------------------------------------------------------

def stem_grads(Cin, img, gn):
    Cc = 16 - Cin
    return torch.nn.grad.conv2d_weight(img, (Cc, Cin, 3, 3), gn[:, :Cc].contiguous(), stride=2, padding=1), gn[:, :Cc].sum((0, 2, 3))


def head_grads(K, x, gout):
    """x (N,h,w,16), gout (N,K,2h,2w): dW[ci][k][a][b] = sum x[n,i,j,ci] * gout[n,k,2i+a,2j+b], db[k] = sum gout."""
    N, h, w, _ = x.shape
    return torch.einsum("nijc,nkiajb->ckab", x, gout.view(N, K, h, 2, w, 2)), gout.sum((0, 2, 3))


@functools.lru_cache(maxsize=None)
def end_problem(which, ch, shape, mode, data):
    """which "stem": ch = Cin, operands img (N,Cin,2Ho,2Wo) fp32 and gcat (N,Ho,Wo,16) (channels [16 - Cin, 16): not read);
    "head": ch = K, operands x (N,Ho,Wo,16) and gout (N,K,2Ho,2Wo) fp32.  gcat / x hold bf16 in mode 2."""
    N, Ho, Wo = shape
    dt = torch.bfloat16 if mode == 2 else torch.float32
    gen = torch.Generator().manual_seed(104729 * (which == "head") + 613 * ch + 31 * Ho * Wo + 3 * mode + (data == "int"))
    p = dict(dt=dt, K=N * Ho * Wo + 2)
    if which == "stem":
        img = draw(gen, data, (N, ch, 2 * Ho, 2 * Wo), 0.25)
        g = draw(gen, data, (N, Ho, Wo, 16)).to(dt)
        p.update(a=img, b=g)
        p["gw"], p["gb"] = stem_grads(ch, img.double(), nchw(g))
        if data == "gauss":
            p["Sw"], p["Sb"] = stem_grads(ch, img.double().abs(), nchw(g).abs())
    else:
        x = draw(gen, data, (N, Ho, Wo, 16), 0.25).to(dt)
        gout = draw(gen, data, (N, ch, 2 * Ho, 2 * Wo))
        p.update(a=x, b=gout)
        p["gw"], p["gb"] = head_grads(ch, x.double(), gout.double())
        if data == "gauss":
            p["Sw"], p["Sb"] = head_grads(ch, x.double().abs(), gout.double().abs())
    return p


class End:
    """The stem's or the head's weight gradient on device copies of a problem's operands inside NaN-filled allocations."""

    def __init__(self, which, ch, shape, mode, data):
        from lanedetection_end2end_amd import _lib
        self.lib, self.st = _lib.load(), _lib.stream()
        self.which, self.ch, self.shape = which, ch, shape
        p = self.p = end_problem(which, ch, shape, mode, data)
        self.a_whole, self.a = carve(tuple(p["a"].shape), p["a"].dtype, NAN)
        self.a.copy_(p["a"])
        self.b_whole, self.b = carve(tuple(p["b"].shape), p["b"].dtype, NAN)
        if which == "stem":
            self.b[..., :16 - ch] = p["b"][..., :16 - ch].cuda()        # the pooled channels [16 - Cin, 16) keep their NaN
            self.wshape, self.nb = (16 - ch, ch, 3, 3), 16 - ch
        else:
            self.b.copy_(p["b"])
            self.wshape, self.nb = (16, ch, 2, 2), ch

    def __call__(self, reduce, bias=True):
        lib = self.lib
        N, Ho, Wo = self.shape
        stem = self.which == "stem"
        dims = (N, self.ch, 2 * Ho, 2 * Wo) if stem else (N, Ho, Wo, self.ch)
        nfl = (lib.lf_debug_stem_wgrad_scratch_floats if stem else lib.lf_debug_head_wgrad_scratch_floats)(*dims)
        assert nfl > 0
        scratch = guarded_scratch(nfl)
        gw_whole, gw = carve(self.wshape, torch.float32)
        gb_whole, gb = carve((self.nb,), torch.float32, NAN if bias else None)
        fn = lib.lf_debug_stem_wgrad if stem else lib.lf_debug_head_wgrad
        rows = fn(reduce, P(self.a), P(self.b), P(gw), P(gb) if bias else None, *dims, P(scratch), self.st)
        assert rows >= 1, (rows, lib.lf_last_error().decode())
        torch.cuda.synchronize()
        assert is_canary(scratch[nfl:]).all(), "floats behind the partial-row scratch written"
        assert guards_intact(gw_whole), "guard band of gw written"
        if bias:
            assert torch.isnan(gb_whole[:GUARD]).all() and torch.isnan(gb_whole[-GUARD:]).all(), "guard band of gb written"
        else:
            assert is_canary(gb_whole).all(), "gb = null: the bias buffer was written"
        nw = 1
        for s in self.wshape:
            nw *= s
        assert rows * (nw + self.nb) == nfl, (rows, nfl)          # the scratch is exactly the rows written
        if self.shape in END_MULTI_ROW:
            assert rows > 1, "%r is meant to take more than one workgroup" % (self.shape,)
        if self.shape == CAPPED:
            assert rows == 1024, "%r is meant to reach the 1024-workgroup cap: %d rows" % (self.shape, rows)
        return gw, (gb if bias else None), rows


def run_end_case(which, ch, shape, mode, datasets):
    from lanedetection_end2end_amd import _lib
    lib = _lib.load()
    try:
        lib.lf_debug_set_ops_precision(mode)
        for data in datasets:
            L = End(which, ch, shape, mode, data)
            for reduce in (0, 1):
                tag = "%s %d %r mode %d %s reduce %d" % (which, ch, shape, mode, data, reduce)
                gw, gb, rows = L(reduce)
                check_result(tag, L.p, data, gw, gb)
                gw2, gb2, rows2 = L(reduce)
                assert rows2 == rows and torch.equal(gw.view(torch.int32), gw2.view(torch.int32)) and \
                    torch.equal(gb.view(torch.int32), gb2.view(torch.int32)), tag + ": two runs differ"
                gw3, _, rows3 = L(reduce, bias=False)
                assert rows3 == rows and torch.equal(gw.view(torch.int32), gw3.view(torch.int32)), tag + ": gw changes with gb = null"
    finally:
        lib.lf_debug_set_ops_precision(0)


@pytest.mark.parametrize("mode", [0, 2], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", END_SHAPES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("Cin", [1, 3, 4])
def test_stem_weight_gradient_against_fp64(Cin, shape, mode):
    run_end_case("stem", Cin, shape, mode, ("int", "gauss"))


@pytest.mark.parametrize("mode", [0, 2], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", END_SHAPES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("K", [1, 2, 3, 5])
def test_head_weight_gradient_against_fp64(K, shape, mode):
    run_end_case("head", K, shape, mode, ("int", "gauss"))


@pytest.mark.parametrize("mode", [0, 2], ids=["fp32", "bf16"])
@pytest.mark.parametrize("which,ch", [("stem", 3), ("head", 2)], ids=["stem3", "head2"])
def test_workgroup_cap_trailing_workgroups_write_zero_rows(which, ch, mode):
    """9232 pixel groups on 1024 workgroups of 10: the last ~100 workgroups own no group, and the row sums read their rows all the
    same.  Integers only: the result must still be exact."""
    run_end_case(which, ch, CAPPED, mode, ("int",))
