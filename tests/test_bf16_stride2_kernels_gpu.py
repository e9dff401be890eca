"""The stride-2 launches of the network ONE AT A TIME through lf_debug_stride2_epi, with the geometries and the weight gather the
plan itself builds (csrc/lf_plan.h): the 9-tap stride-2 convolution of DownsamplerBlock(16, 64) and the four sub-pixel phases of its
data gradient, the four phases of UpsamplerBlock(64, 16)'s transposed convolution and its 9-tap data gradient -- in the bf16
precision mode (the compiled-in whole-step forms of tapgemm_bf16_kernel at 16 and 48 source channels, which no other kernel-level
test reaches) and on the fp32 kernels, against torch fp64 convolutions of the operands the kernel sees.

  case  launch                        channels                         forms in the bf16 mode
  A     down forward                  Cin 16 -> Cc 48 of Ccat 64       <3, 0, EPI, FAST>: 9 steps (odd: one dead step)
  B     up data gradient              Co 16 -> Cin 64                  <4, 0, EPI, FAST>: 9 steps
  C     down data gradient, 4 phases  Cs 48 at pixel stride 64 -> 16   <1, 0, EPI, FAST>: two 32-channel steps per tap
  D     up forward, 4 phases          64 -> 16                         <1, 0, EPI, FAST>: whole steps

and the same four launches of the 64 <-> 128 pair, DownsamplerBlock(64, 128) and UpsamplerBlock(128, 64), which select other kernels:
on fp32 tensors tapgemm_kernel<4, 0, E> in its rectangular forms (two 64-channel output slabs, a 128-channel source, 64 channels read
at pixel stride 128; both row-arithmetic variants), on bf16 tensors the persistent LDS-DMA ring (tapgemm_bf16_ring_kernel) where
Wl % 16 == 0 and tapgemm_bf16_kernel<4, 0, E, true> at ragged widths:

  E     down forward                  Cin 64 -> Cc 64 of Ccat 128      9 taps x 2 steps
  F     up data gradient              Co 64 -> Cin 128                 9 taps x 2 steps, two output slabs
  G     down data gradient, 4 phases  Cs 64 at pixel stride 128 -> 64  channels [64, 128) of every source pixel hold NaN
  H     up forward, 4 phases          128 -> 64                        1 / 2 / 2 / 4 taps x 4 steps

lf_debug_bf16_ring_launches pins which bf16 kernel ran; lf_debug_set_bf16_max_workgroups caps the ring's grid so that ONE workgroup walks
every item of a small launch, across tiles and output slabs (the product launches cap the grid at the resident workgroups only, which
no small shape exceeds).

Every tensor is carved out of the middle of a larger allocation: sources lie between NaN guard bands, destinations are pre-filled with
a canary bit pattern which the guard bands, the pooled channels [48, 64) of case A ([64, 128) of case E) and the other phases' pixels
of cases C, D, G and H must still hold afterwards.

Per-element gate (derived, not measured): with K = taps * Cs + 2 terms and S the same convolution of |x| with |w| plus |bias| and
|add|, any fp32 accumulation order is within K * 2^-24 * S of the exact sum, and a bf16 store adds half a bf16 ulp:
|got - want| <= 2^-8 * |want| + K * 2^-23 * S on bf16 tensors, K * 2^-23 * S on fp32 tensors.

Statistics rows ([2][Cd][rows], row r = the r-th 256-pixel tile of the launch's logical pixels), as LF_TAPGEMM_EPILOGUE writes them and
lf_eltwise.hip's stat_channel_sums combines them:
  STATS_SQ    [0] = sum v (raw), [1] = M2 = sum (v - mean_tile)^2, CENTRED on the tile's own mean (accumulated about a pivot, merged
              with Chan's formula); the finalise forms sum v^2 = sum_r (M2_r + (sum v)_r^2 / n_r) in fp64, n_r the tile's pixel count
  STATS_XHAT  [0] = sum v, [1] = sum v * aux, both RAW; the finalise adds the rows up
-- v the values as stored.  Compared, combined that way, against fp64 sums at 2e-5 * the sum of absolute values.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

RELU, MASK, ADD, STATS_SQ, STATS_XHAT = 1, 2, 4, 8, 32
GUARD = 4096                       # elements either side of every tensor (a multiple of 64: the carved tensor stays 256-byte aligned)
CANARY = {torch.bfloat16: (torch.int16, 0x5A5B), torch.float32: (torch.int32, 0x5A5B5C5D)}

# (N, H, W) of the LARGER tensor: one partial workgroup with three images (3x5 per image); 16-pixel groups straddling rows and the
# image boundary, two workgroups with a ragged tail (10x22); width 24, reachable in the network (16x24); gridDim.x == 8, the
# smallest launch that takes the (gridDim.x & 7) == 0 workgroup remap (32x32)
SHAPES = [(3, 6, 10), (2, 20, 44), (1, 32, 48), (2, 64, 64)]
# ... of cases E-H, Wl = W / 2: Wl 5, 45 pixels, one partial workgroup on the streaming kernels; Wl 16, 192 pixels: the ring, one partial
# item with the image boundary inside it; Wl 48, 720 pixels = three tiles, the last partial, tiles straddling images (240 pixels each);
# Wl 128, two full tiles: the fp32 wave-uniform row variant ((Wl & 63) == 0); Wl 32, eight tiles: the (gridDim.x & 7) == 0 remap
WIDE_SHAPES = [(3, 6, 10), (2, 12, 32), (3, 10, 96), (1, 8, 256), (2, 64, 64)]

#        kind, phases, Cin, Cout, source channels (pixel stride), contracted, destination channels (pixel stride), produced, bias
CASES = {"A": dict(kind=0, nph=1, Cin=16, Cout=48, s_pix=16, Cs=16, d_pix=64, Cd=48, bias=True, src_large=True),
         "B": dict(kind=3, nph=1, Cin=64, Cout=16, s_pix=16, Cs=16, d_pix=64, Cd=64, bias=False, src_large=True),
         "C": dict(kind=1, nph=4, Cin=16, Cout=48, s_pix=64, Cs=48, d_pix=16, Cd=16, bias=False, src_large=False),
         "D": dict(kind=2, nph=4, Cin=64, Cout=16, s_pix=64, Cs=64, d_pix=16, Cd=16, bias=True, src_large=False),
         "E": dict(kind=0, nph=1, Cin=64, Cout=64, s_pix=64, Cs=64, d_pix=128, Cd=64, bias=True, src_large=True),
         "F": dict(kind=3, nph=1, Cin=128, Cout=64, s_pix=64, Cs=64, d_pix=128, Cd=128, bias=False, src_large=True),
         "G": dict(kind=1, nph=4, Cin=64, Cout=64, s_pix=128, Cs=64, d_pix=64, Cd=64, bias=False, src_large=False, nan_tail=True),
         "H": dict(kind=2, nph=4, Cin=128, Cout=64, s_pix=128, Cs=128, d_pix=64, Cd=64, bias=True, src_large=False)}
EPIS = {"A": (0, RELU, STATS_SQ), "B": (0, MASK | STATS_XHAT), "C": (0, ADD), "D": (0, STATS_SQ, RELU),
        "E": (0, RELU, STATS_SQ), "F": (0, MASK | STATS_XHAT), "G": (0, ADD), "H": (0, STATS_SQ, RELU)}
WIDE = "EFGH"
CASE_SHAPES = [(case, shape) for case in "ABCD" for shape in SHAPES] + [(case, shape) for case in WIDE for shape in WIDE_SHAPES]
shape_id = lambda s: "%dx%dx%d" % s


def scratch_floats(case):
    """9 * roundup(Kc, 32) * Nc floats (csrc/lf_debug.h; 73728 for case F), no less than the 9 * 64 * 64 cases A-D ran with, plus slack"""
    c = CASES[case]
    return max(9 * 64 * 64, 9 * ((c["Cs"] + 31) // 32 * 32) * c["Cd"]) + 4096


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def carve(shape, dtype, fill=None):
    """(whole allocation, the tensor in its middle).  fill None: the canary bit pattern everywhere (a destination)."""
    n = int(np.prod(shape))
    if fill is None:
        idt, pat = CANARY[dtype]
        whole = torch.full((n + 2 * GUARD,), pat, dtype=idt, device="cuda").view(dtype)
    else:
        whole = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    return whole, whole[GUARD:GUARD + n].view(shape)


def bits(t):
    return t.contiguous().view(CANARY[t.dtype][0])


def is_canary(t):
    idt, pat = CANARY[t.dtype]
    return bits(t) == pat


def sizes(case, shape):
    N, H, W = shape
    c = CASES[case]
    small, large = (N, H // 2, W // 2), (N, H, W)
    s, d = (large, small) if c["src_large"] else (small, large)
    return s + (c["s_pix"],), d + (c["d_pix"],)


@functools.lru_cache(maxsize=None)
def problem(case, shape, mode):
    """Operands (as the kernel sees them: bf16-rounded tensors and weights in mode 2, fp32 bias) and the fp64 reference, once per
    (case, shape, mode): want / S before the epilogue, NHWC over the produced channels; K per destination pixel."""
    import torch.nn.functional as F
    c = CASES[case]
    N, H, W = shape
    dt = torch.bfloat16 if mode == 2 else torch.float32
    gen = torch.Generator().manual_seed(1000 * "ABCDEFGH".index(case) + H * W + mode)
    sshape, dshape = sizes(case, shape)
    rnd = lambda *s: torch.randn(*s, generator=gen).to(dt)
    src = rnd(*sshape)
    taps = 9 if c["nph"] == 1 else 4
    # Conv2d(Cin, Cout) / ConvTranspose2d(Cin, Cout) layouts
    wshape = (c["Cout"], c["Cin"], 3, 3) if c["kind"] <= 1 else (c["Cin"], c["Cout"], 3, 3)
    w = torch.randn(*wshape, generator=gen) * (2.0 / (taps * c["Cs"])) ** 0.5
    bias = torch.randn(c["Cd"], generator=gen) if c["bias"] else None
    oshape = dshape[:3] + (c["Cd"],)
    mask, add, aux = rnd(*oshape), rnd(*oshape), rnd(*oshape)
    wk = (w.to(dt) if mode == 2 else w).double()
    nchw = lambda t: t.double().permute(0, 3, 1, 2).contiguous()
    xs = nchw(src[..., :c["Cs"]])

    def op(x, wt, b):
        if c["kind"] == 0:
            return F.conv2d(x, wt, b, stride=2, padding=1)
        if c["kind"] == 3:          # the adjoint of conv_transpose2d(., w) is conv2d(., w)
            return F.conv2d(x, wt, None, stride=2, padding=1)
        if c["kind"] == 1:
            return torch.nn.grad.conv2d_input((N, c["Cin"], H, W), wt, x, stride=2, padding=1)
        return F.conv_transpose2d(x, wt, b, stride=2, padding=1, output_padding=1)
    bd = bias.double() if bias is not None else None
    want = op(xs, wk, bd).permute(0, 2, 3, 1).contiguous()
    S = op(xs.abs(), wk.abs(), bd.abs() if bd is not None else None).permute(0, 2, 3, 1).contiguous()
    assert want.shape == oshape
    if c.get("nan_tail"):           # the other slice of the concat gradient: the launch must not read it (xs above is taken without it)
        src[..., c["Cs"]:] = float("nan")
    # terms per destination pixel: 9 taps, or the phase's 1, 2, 2, 4
    K = torch.full(oshape[1:3], 9.0 * c["Cs"] + 2, dtype=torch.float64)
    if c["nph"] == 4:
        for a in range(2):
            for b in range(2):
                K[a::2, b::2] = (1 + a) * (1 + b) * c["Cs"] + 2
    return dict(src=src, w=w, bias=bias, mask=mask, add=add, aux=aux, want=want, S=S, K=K[None, :, :, None], dt=dt, oshape=oshape)


class Launcher:
    """Device copies of a problem's operands inside guarded allocations, and one launch (all phases) per call."""

    def __init__(self, case, shape, mode):
        from lanedetection_end2end_amd import _lib
        self.lib, self.st = _lib.load(), _lib.stream()
        self.case, self.shape, self.mode, self.c = case, shape, mode, CASES[case]
        p = self.p = problem(case, shape, mode)
        sshape, self.dshape = sizes(case, shape)
        self.src_whole, self.src = carve(sshape, p["dt"], float("nan"))
        self.src.copy_(p["src"])
        dev = lambda t: None if t is None else t.cuda()
        self.w, self.bias = dev(p["w"]), dev(p["bias"])
        # epilogue tensors in the DESTINATION's layout (case A: Ccat-wide pixels, the produced channels first)
        self.epi_t = {}
        for k in ("mask", "add", "aux"):
            _, t = carve(self.dshape, p["dt"], float("nan"))
            t[..., :self.c["Cd"]] = p[k].cuda()
            self.epi_t[k] = t
        self.scratch = torch.empty(scratch_floats(case), device="cuda")
        N, H, W = shape
        self.npix = N * (H // 2) * (W // 2)          # logical pixels of every launch here
        self.rows = (self.npix + 255) // 256

    def __call__(self, epi):
        """dst (whole allocation, tensor), [per phase: statistics rows [2][Cd][rows] or None]; asserts what every launch must keep."""
        c, lib = self.c, self.lib
        N, H, W = self.shape
        whole, dst = carve(self.dshape, self.p["dt"])
        stats = []
        for ph in range(c["nph"]):
            wph, dph = (whole, dst) if c["nph"] == 1 else carve(self.dshape, self.p["dt"])
            sbuf = torch.full((2 * c["Cd"] * self.rows + 64,), float("nan"), device="cuda") if epi & (STATS_SQ | STATS_XHAT) else None
            rc = lib.lf_debug_stride2_epi(c["kind"], ph, P(self.src), P(self.w), P(self.bias), P(dph), epi,
                                          P(self.epi_t["mask"]) if epi & MASK else None, P(self.epi_t["add"]) if epi & ADD else None,
                                          P(self.epi_t["aux"]) if epi & STATS_XHAT else None, P(sbuf), N, H, W, c["Cin"], c["Cout"],
                                          P(self.scratch), self.st)
            assert rc == (self.rows if sbuf is not None else 0), (rc, lib.lf_last_error().decode())
            torch.cuda.synchronize()
            assert is_canary(wph[:GUARD]).all() and is_canary(wph[-GUARD:]).all(), "guard band written"
            if c["nph"] == 4:       # a phase writes its own pixels and no others
                a, b = ph >> 1, ph & 1
                own = torch.zeros(self.dshape[:3], dtype=torch.bool, device="cuda")
                own[:, a::2, b::2] = True
                assert is_canary(dph)[~own].all(), "phase %d wrote another phase's pixels" % ph
                assert not is_canary(dph)[own].any(), "phase %d left pixels of its own unwritten" % ph
                dst[:, a::2, b::2] = dph[:, a::2, b::2]
            if sbuf is not None:
                assert torch.isnan(sbuf[2 * c["Cd"] * self.rows:]).all(), "floats behind the last statistics row written"
                stats.append(sbuf[:2 * c["Cd"] * self.rows].view(2, c["Cd"], self.rows).clone())
            else:
                stats.append(None)
        if c["d_pix"] > c["Cd"]:
            assert is_canary(dst[..., c["Cd"]:]).all(), "the concat buffer's pooled channels written"
        return whole, dst, stats


def set_mode(lib, mode, no_partial_fast=0):
    lib.lf_debug_set_ops_precision(mode)
    lib.lf_debug_set_bf16_no_partial_fast(no_partial_fast)


def reset(lib):
    lib.lf_debug_set_ops_precision(0)
    lib.lf_debug_set_bf16_no_partial_fast(0)
    lib.lf_debug_set_bf16_lds(4)
    lib.lf_debug_set_bf16_max_workgroups(0)


def check_stats(L, epi, dst, stats, tag):
    """The rows, combined as stat_channel_sums combines them, against fp64 sums of the stored values."""
    c = L.c
    aux = L.p["aux"].double()
    for ph, rows in enumerate(stats):
        assert torch.isfinite(rows).all(), tag
        a, b = ph >> 1, ph & 1
        v = dst[..., :c["Cd"]].double().cpu()
        x = aux
        if c["nph"] == 4:
            v, x = v[:, a::2, b::2], x[:, a::2, b::2]
        v, x = v.reshape(-1, c["Cd"]), x.reshape(-1, c["Cd"])
        r = rows.double().cpu()
        if epi & STATS_SQ:
            n_r = torch.tensor([min(256, L.npix - 256 * i) for i in range(L.rows)], dtype=torch.float64)
            got = (r[0].sum(1), (r[1] + r[0] ** 2 / n_r).sum(1))
            ref = (v.sum(0), (v * v).sum(0))
            mag = (v.abs().sum(0), (v * v).sum(0))
        else:
            got = (r[0].sum(1), r[1].sum(1))
            ref = (v.sum(0), (v * x).sum(0))
            mag = (v.abs().sum(0), (v * x).abs().sum(0))
        for k in range(2):
            err = (got[k] - ref[k]).abs() / mag[k]
            print("%s phase %d sums kind %d: max err / sum|.| = %.3e (gate 2e-5)" % (tag, ph, k, float(err.max())))
            assert float(err.max()) < 2e-5, (tag, ph, k, float(err.max()))


@pytest.mark.parametrize("mode", [2, 0], ids=["bf16", "fp32"])
@pytest.mark.parametrize("case,shape", CASE_SHAPES, ids=["%s-%s" % (c, shape_id(s)) for c, s in CASE_SHAPES])
def test_stride2_launch_against_fp64(case, shape, mode):
    """Every element of every launch inside its derived gate, the statistics rows against fp64 sums, guards and canaries intact.
    (fp32: lf_tapgemm_launch takes every epilogue set for these geometries -- tapgemm_kernel<3> and tapgemm_lean_kernel<1> in their
    run-time-flag or compiled-in forms, tapgemm_kernel<4> compiled-in -- so the bf16 mode's sets are used there too.)  Cases E-H
    run at WIDE_SHAPES; in the bf16 mode the ring kernel takes their launches wherever Wl % 16 == 0 (the shipped routing), which
    lf_debug_bf16_ring_launches pins."""
    L = Launcher(case, shape, mode)
    p, c = L.p, L.c
    ring = L.lib.lf_debug_bf16_ring_launches
    on_ring = c["nph"] if case in WIDE and mode == 2 and (shape[2] // 2) % 16 == 0 else 0
    try:
        set_mode(L.lib, mode)
        for epi in EPIS[case]:
            tag = "case %s %r mode %d epi %d" % (case, shape, mode, epi)
            n0 = ring()
            _, dst, stats = L(epi)
            if case in WIDE:
                assert ring() - n0 == on_ring, "%s: %d launches on the ring kernel, expected %d" % (tag, ring() - n0, on_ring)
            want, S = p["want"], p["S"]
            if epi & ADD:
                want, S = want + p["add"].double(), S + p["add"].double().abs()
            if epi & MASK:
                want = want * (p["mask"].double() > 0)
            if epi & RELU:
                want = torch.relu(want)
            got = dst[..., :c["Cd"]].double().cpu()
            assert torch.isfinite(got).all(), tag
            gate = p["K"] * 2.0 ** -23 * S + (2.0 ** -8 * want.abs() if mode == 2 else 0.0)
            err = (got - want).abs()
            print("%s: max err / gate = %.3f" % (tag, float((err / gate).max())))
            assert (err <= gate).all(), (tag, float((err / gate).max()), int((err > gate).sum()))
            if epi & (STATS_SQ | STATS_XHAT):
                check_stats(L, epi, dst, stats, tag)
    finally:
        reset(L.lib)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("case", "ABC")
def test_compiled_in_forms_equal_the_run_time_flag_form_bit_for_bit(case, shape):
    """16 / 48 source channels on bf16 tensors: the compiled-in whole-step forms against the run-time-flag form (which clamps a
    partial step's channel offsets inside the pixel) -- the lanes beyond Cs multiply zero weights in both, the accumulators see the
    same sequence: stored values AND statistics rows equal in bits.  lf_debug_partial_fast_launches pins which form ran: with the
    switch off every launch here (one per phase) takes a compiled-in form, with it on none does."""
    L = Launcher(case, shape, 2)
    count = L.lib.lf_debug_partial_fast_launches
    try:
        for epi in EPIS[case]:
            set_mode(L.lib, 2, 0)
            n0 = count()
            _, d0, s0 = L(epi)
            n1 = count()
            set_mode(L.lib, 2, 1)
            _, d1, s1 = L(epi)
            assert (n1 - n0, count() - n1) == (L.c["nph"], 0), "case %s %r epi %d: launches on the compiled-in forms with the " \
                "switch off / on: %d / %d, expected %d / 0" % (case, shape, epi, n1 - n0, count() - n1, L.c["nph"])
            assert torch.isfinite(d0[..., :L.c["Cd"]].float()).all()
            assert torch.equal(bits(d0), bits(d1)), "case %s %r epi %d: values differ" % (case, shape, epi)
            for a, b in zip(s0, s1):
                assert (a is None and b is None) or torch.equal(a, b), "case %s %r epi %d: statistics rows differ" % (case, shape, epi)
    finally:
        reset(L.lib)


@pytest.mark.parametrize("shape", WIDE_SHAPES, ids=shape_id)
@pytest.mark.parametrize("case", WIDE)
def test_ring_kernel_equals_the_streaming_kernel_bit_for_bit(case, shape):
    """Cases E-H on bf16 tensors, every epilogue set of the case, five runs per launch: lf_debug_set_bf16_lds(4) (the shipped routing:
    the ring wherever Wl % 16 == 0), the same again (ONE determinism comparison, not a retry), (4) with the grid capped to 1 and to 2
    workgroups (lf_debug_set_bf16_max_workgroups: one workgroup then walks every item of the launch -- with case F 2 * ntiles of
    them, changing the output slab at every other one -- with its load cursor running ahead across the item boundaries), and
    lf_debug_set_bf16_lds(0), the streaming kernel.  lf_debug_bf16_ring_launches rises by the launches of the case (1, or 4 phases) in
    each of the first four runs and by 0 in the last; at (3, 6, 10), Wl = 5, it does not rise at all.  Stored values AND statistics
    rows are equal in bits across all five runs ("K order = tapgemm_bf16_kernel's: results bit-identical", lf_conv_bf16.hip; both
    kernels end in LF_TAPGEMM_EPILOGUE on the same accumulator layout, so the rows are summed in the same order too)."""
    L = Launcher(case, shape, 2)
    lib, c = L.lib, L.c
    ring = lib.lf_debug_bf16_ring_launches
    on_ring = c["nph"] if (shape[2] // 2) % 16 == 0 else 0
    runs = (("ring", 4, 0), ("ring again", 4, 0), ("ring, 1 workgroup", 4, 1), ("ring, 2 workgroups", 4, 2), ("streaming", 0, 0))
    try:
        set_mode(lib, 2)
        for epi in EPIS[case]:
            tag = "case %s %r epi %d" % (case, shape, epi)
            first, counts = None, []
            for name, lds, cap in runs:
                lib.lf_debug_set_bf16_lds(lds)
                lib.lf_debug_set_bf16_max_workgroups(cap)
                n0 = ring()
                _, dst, stats = L(epi)
                counts.append(ring() - n0)
                assert torch.isfinite(dst[..., :c["Cd"]].float()).all(), (tag, name)
                if first is None:
                    first = (dst, stats)
                    continue
                diff = (bits(dst) != bits(first[0])).reshape(-1, c["d_pix"]).any(1)
                assert not diff.any(), "%s, %s: %d pixels differ from the first run (first at %d)" % (tag, name, int(diff.sum()),
                                                                                                   int(diff.nonzero()[0]))
                for ph, (x, y) in enumerate(zip(stats, first[1])):
                    assert (x is None and y is None) or torch.equal(x, y), "%s, %s: statistics rows of phase %d differ" % (tag, name, ph)
            print("%s: ring launches per run %r" % (tag, counts))
            assert counts == [on_ring] * 4 + [0], "%s: ring launches per run %r, expected %r" % (tag, counts, [on_ring] * 4 + [0])
    finally:
        reset(lib)


def planted_positions(case, sshape):
    """(name, (n, y, x, channel)) in the source tensor: (a) an interior pixel at an even column, (b) column 0 of a row -- the pixel in
    front of it in memory is the previous row's last --, (c) pixel (0, 0) of image 1 -- ... image 0's last --, and for case C (d) one
    of the channels 48..63 of a source pixel, which the Cs = 48 launch must not read as data (case G: one of [64, 128))."""
    N, Hs, Ws, _ = sshape
    pos = [("a", (0, Hs // 2, 2 * (Ws // 4), 5)), ("b", (0, Hs // 2 + 1, 0, 9)), ("c", (1, 0, 0, 3))]
    if case == "C":
        pos.append(("d", (0, Hs // 2, 2 * (Ws // 4), 53)))
    if case == "G":
        pos.append(("d", (0, Hs // 2, 2 * (Ws // 4), 117)))
    return pos


def window_pixels(case, shape, pos):
    """Destination pixels (bool (N, Hd, Wd)) whose tap window contains source pixel pos, from the layer's definition: the 3x3
    stride-2 pad-1 window of small pixel (i, j) covers large rows 2i-1..2i+1 and columns 2j-1..2j+1 -- cases A, B gather along
    it (large -> small), case C scatters back along it (small -> large).  E, F: as A, B; G and H: as C -- large pixel (Y, X) of the
    transposed convolution H receives small pixel (i, j) exactly where |Y - 2i| <= 1 and |X - 2j| <= 1 too.  A channel the launch does
    not contract (>= Cs) has an empty window.  (tests/test_stride2_ref_cpu.py: equal to the support of the modules' autograd gradient.)"""
    N, H, W = shape
    n, y, x, ch = pos
    c = CASES[case]
    if ch >= c["Cs"]:
        return np.zeros((N, H, W) if not c["src_large"] else (N, H // 2, W // 2), dtype=bool)
    if c["src_large"]:
        out = np.zeros((N, H // 2, W // 2), dtype=bool)
        for i in range(H // 2):
            for j in range(W // 2):
                out[n, i, j] = abs(y - 2 * i) <= 1 and abs(x - 2 * j) <= 1
    else:
        out = np.zeros((N, H, W), dtype=bool)
        for Y in range(H):
            for X in range(W):
                out[n, Y, X] = abs(Y - 2 * y) <= 1 and abs(X - 2 * x) <= 1
    return out


# position c needs two images.  E-H: the streaming shape, then the ring at one partial item, at tiles straddling images, at eight tiles
CONTAINMENT = [(case, epi, shape) for case, epis in (("A", (0, RELU)), ("B", (0, RELU)), ("C", (0,))) for epi in epis
               for shape in SHAPES[:2] + SHAPES[3:]] + \
              [(case, epi, shape) for case, epis in (("E", (0, RELU)), ("F", (0,)), ("G", (0,)), ("H", (0, RELU))) for epi in epis
               for shape in (WIDE_SHAPES[1], WIDE_SHAPES[2], WIDE_SHAPES[4], WIDE_SHAPES[0])]


@pytest.mark.parametrize("value", [float("inf"), float("-inf"), float("nan")], ids=["+inf", "-inf", "nan"])
@pytest.mark.parametrize("case,epi,shape", CONTAINMENT, ids=["%s-epi%d-%s" % (c, e, shape_id(s)) for c, e, s in CONTAINMENT])
def test_a_non_finite_value_stays_inside_its_tap_windows(case, epi, shape, value):
    """One +Inf, -Inf or NaN in the source (no STATS flag: through the sums it legitimately reaches the whole channel): the
    non-finite output pixels are EXACTLY those whose tap window contains the planted pixel, every other element keeps the clean
    run's bits, and the run-time-flag form gives the same set.  Which form ran is pinned by lf_debug_partial_fast_launches: every
    launch with the switch off takes a compiled-in form, except case B with ReLU, which the network does not launch and which runs
    on the run-time-flag form either way.

    Before the lanes beyond Cs of a partial 32-channel step read buffer zeros (tapgemm_bf16_kernel, FAST) this failed with every
    value: 0 * Inf and 0 * NaN against the zero-padded weights are NaN, so at 16 source channels (cases A, B, epilogue 0) the pixel
    BEHIND a window pixel in memory poisoned all output channels -- positions a, b, c: 1-2 extra non-finite pixels each, the output
    pixel(s) whose window ends one column (b: one row, c: one image) in front of the planted pixel -- and at 48 (case C) channels
    48..63 of the window's own pixels did (position d).

    The ReLU cases ([A-epi1, B-epi1] x the first two shapes x all three values) failed a second way while the epilogue's ReLU was a
    signed-integer maximum of the bit patterns (max0, lf_conv_dev.h): the matrix cores return a NaN with its sign bit set, which that
    maximum stores as 0 where torch.relu keeps the NaN -- 0 non-finite pixels where 1-2 are expected, with a planted NaN at every
    position and with +-Inf at position b (channel 9) on the run-time-flag form, whose clamped lanes re-read channels 8..15 of the
    SAME pixel against zero weights (0 * Inf = NaN in every channel of the window pixels).  The bf16 kernels' epilogues now take
    relu_keep_nan (v <= 0 ? 0 : v), which differs from max0 on a sign-set NaN only.

    Cases E-H have Cs % 32 == 0 and no partial step: their two forms are the shipped routing (lf_debug_set_bf16_lds(4): the ring
    kernel wherever Wl % 16 == 0, pinned by lf_debug_bf16_ring_launches; its padding is the DMA's out-of-range offset) and the
    streaming kernel alone (lf_debug_set_bf16_lds(0)).  E, F gather like A, B; G, H scatter like C, and G's position d lies in the
    channels [64, 128) the launch does not contract -- which hold NaN in the clean run already."""
    L = Launcher(case, shape, 2)
    c = L.c
    sshape, _ = sizes(case, shape)
    bad = []
    wide = case in WIDE
    count = L.lib.lf_debug_bf16_ring_launches if wide else L.lib.lf_debug_partial_fast_launches
    if wide:
        compiled_in = c["nph"] if (shape[2] // 2) % 16 == 0 else 0       # launches on the ring kernel under the shipped routing
        forms = ("shipped routing", "streaming")
    else:
        compiled_in = 0 if (case, epi) == ("B", RELU) else c["nph"]
        forms = ("compiled-in", "run-time-flag")
    try:
        set_mode(L.lib, 2, 0)
        _, clean, _ = L(epi)
        clean = clean[..., :c["Cd"]].clone()
        assert torch.isfinite(clean.float()).all()
        for name, pos in planted_positions(case, sshape):
            want_set = window_pixels(case, shape, pos)
            assert name == "d" or want_set.any()
            src = L.p["src"].clone()
            src[pos] = value
            L.src.copy_(src)
            for flagform in (0, 1):
                set_mode(L.lib, 2, 0 if wide else flagform)
                if wide:
                    L.lib.lf_debug_set_bf16_lds(0 if flagform else 4)
                n0 = count()
                _, got, _ = L(epi)
                assert count() - n0 == (0 if flagform else compiled_in), (name, flagform, count() - n0)
                got = got[..., :c["Cd"]]
                got_set = (~torch.isfinite(got.float())).any(-1).cpu().numpy()
                rest = torch.from_numpy(~(got_set | want_set)).cuda()
                same = torch.equal(bits(got[rest]), bits(clean[rest]))
                if not (got_set == want_set).all() or not same:
                    extra = np.argwhere(got_set & ~want_set)
                    bad.append("position %s, %s form: %d non-finite pixels, %d expected, %d outside the windows (first %s)%s"
                               % (name, forms[flagform], got_set.sum(), want_set.sum(), len(extra),
                                  extra[0].tolist() if len(extra) else None, "" if same else "; finite elements changed"))
        assert not bad, "case %s epi %d %r value %s:\n" % (case, epi, shape, value) + "\n".join(bad)
    finally:
        reset(L.lib)
