"""The bandwidth-bound half of the backbone ONE LAUNCH AT A TIME, against tests/eltwise_ref.py in fp64 (itself checked against torch's
own operators by tests/test_eltwise_ref_cpu.py): the BatchNorm statistics finalise / apply / backward reduce / backward finalise /
backward apply, the max-pool branch (training, inference, backward), the stem forward (training, inference), the head forward and
data gradient -- through the lf_debug_* hooks of csrc/lf_debug.h -- and the 1x1 lf_pointwise_* entry points.

Memory, every launch: every tensor -- inputs too -- lies in the middle of a NaN-filled allocation (GUARD elements either side), and
so does every region a launch must NOT write (row floats in [nrows, ld), rows past the returned count, concat channels outside
[choff, choff + Cin), g_z / gw / gb when not requested).  After the launch the allocation must be bit for bit what it was outside the
region the contract names, and FINITE inside it: an element the kernel skipped is still NaN, an operand read out of bounds makes a
NaN result.  No element is excluded from a comparison: ReLU masks come from a y the test supplies, pool arg-maxima from an x it
supplies, and where a ReLU follows arithmetic (bn_act, the inference forms) the bound is absolute, so a flipped sign near zero is
inside it.

Tolerances are derived, none is measured.  u = 2^-24; an fp32 output is held to B = k * u * S per element, S = the sum of the absolute
values of the terms that form it (the reference evaluated on absolute operands), k = the roundings of the longest chain + 2:

  bn_act                 4 u (|x sc dm| + |sh dm| + |res|)                  mul, add, mul, add
  bn_bwd_apply           8 u |gamma rstd| (|gm| + |c1| + (|t rstd| + |ash|) |c2|)
  g_z                    bitwise
  finalise outputs       2 u S (fp64 arithmetic, one rounding), e.g. S = |beta| + |mean scale| for the shift
  partial rows           (n + 8) u sum |term|, n = the most pixels one row covers: min(npix, roundup(ceil(npix / rows), 256)) for the
                         reduce / pool rows (csrc/lf_debug.h), 256 for the stem; the written rows are summed in fp64 and compared
                         with the column sums, as tests/test_lean_gpu.py does
  pool affine form       4 u (|m sc| + |sh|)                                mul, add
  stem convolution       (9 Cin + 2) u (sum |w x| + |b|)
  stem inference form    that bound times |sc|, plus 3 u (|v sc| + |sh|)
  head forward           18 u (sum |x w| + |b|);  head data gradient  (4 K + 1) u sum |g w|
  pointwise forward      (C + 1) u (sum |x w| + |b|);  data gradient  (K + 1) u sum |g w|;  gw, gb  (256 + rows + 8) u sum |g x|
  bf16 output            2^-8 (|ref| + B) + B
  pool values and pool gradients: exact (gradients bit for bit, -0.0 / +0.0 included)

The stem's statistics rows are sums of the values BEFORE rounding to the storage type (csrc/lf_debug.h): with fp32 storage they are
compared with the stored concat values; with bf16 storage with the fp64 reference, the bound widened by the kernel's own error of
each term (sum B_conv, 2 sum |v| B_conv) -- the stored bf16 values are 2^-9 away from what was summed.

Every test prints its worst error / bound; a ratio above 1 fails.  Measured on an MI355X (worst over each group's cases):
  finalize_fwd raw row counts                                        0.487
  finalize_fwd centred rows                                          0.490
  finalize_fwd two sources / uncovered / eval / count 1 / constant   0.484
  finalize_bwd                                                       0.427
  bn_act fp32                                                        0.478
  bn_act bf16                                                        0.989
  bn_act (grid / row cap)                                            0.636
  bn_bwd_reduce fp32                                                 0.161
  bn_bwd_reduce bf16                                                 0.176
  bn_bwd_reduce (grid / row cap)                                     0.000
  bn_bwd_apply fp32                                                  0.430
  bn_bwd_apply bf16                                                  0.993
  bn_bwd_apply (grid / row cap)                                      0.510
  five launches chained                                              0.191
  pool_concat_fwd fp32                                               0.088
  pool_concat_fwd bf16                                               0.066
  pool_concat_fwd (grid / row cap)                                   0.000
  pool_affine_fwd fp32                                               0.226
  pool_affine_fwd bf16                                               0.961
  stem_fwd training fp32                                             0.264
  stem_fwd rows fp32                                                 0.110
  stem_fwd inference fp32                                            0.328
  stem_fwd training bf16                                             0.994
  stem_fwd rows bf16                                                 0.074
  stem_fwd inference bf16                                            0.993
  head fp32                                                          0.448
  head bf16                                                          0.993
  head (grid / row cap)                                              0.656
  pointwise fp32                                                     0.600
  pointwise bf16                                                     0.996
(bf16: round-to-nearest-even is half an ulp, 2^-8 of the binade's lower end, so values just above a power of two come close to 1 by
construction and cannot pass it; the 0.000 of the capped rows: 65606 pixels' rounding errors against a bound that adds them all up
-- those two cases lean on the exact integer-data check.)  The pool gradients: 62 - 81 % of the windows tie, exact in every case.
"""
import ctypes
import math

import pytest
import torch

import eltwise_ref as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
GUARD = 256                        # elements either side (a multiple of 64: the carved tensor stays 256-byte aligned)
NAN = float("nan")
BITS = {torch.float32: torch.int32, torch.bfloat16: torch.int16}
M32 = float(torch.tensor(0.1, dtype=torch.float32))          # momentum and eps as the float arguments carry them
E32 = float(torch.tensor(1e-3, dtype=torch.float32))


def lib():
    from lanedetection_end2end_amd import _lib
    return _lib.load()


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def dt(s16):
    return torch.bfloat16 if s16 else torch.float32


def roundup(a, b):
    return (a + b - 1) // b * b


class Buf:
    """A tensor in the middle of a NaN-filled allocation; check() after the launch."""

    def __init__(self, shape, dtype=torch.float32, init=None):
        shape = tuple(shape)
        n = math.prod(shape)
        self.whole = torch.full((n + 2 * GUARD,), NAN, dtype=dtype, device="cuda")
        self.t = self.whole[GUARD:GUARD + n].view(shape)
        if init is not None:
            self.t.copy_(init)
        self.before = self.whole.clone()

    def check(self, written=None):
        """written: None = nothing may have changed; True = the whole tensor; else a mask broadcastable to the tensor's shape.
        Outside it: bit for bit as before the launch.  Inside it: finite."""
        n = self.t.numel()
        w = torch.zeros(self.whole.numel(), dtype=torch.bool, device="cuda")
        if written is True:
            w[GUARD:GUARD + n] = True
        elif written is not None:
            w[GUARD:GUARD + n] = written.to("cuda").expand(self.t.shape).reshape(-1)
        bits = BITS[self.whole.dtype]
        same = self.whole.view(bits) == self.before.view(bits)
        assert bool(same[~w].all()), "the launch wrote outside its output region"
        assert bool(torch.isfinite(self.whole[w]).all()), "an output element was not written, or is not finite"


def P(b):
    return None if b is None else ctypes.c_void_p(b.t.data_ptr())


def worst(got, ref, bound):
    err = (got.double() - ref).abs()
    r = torch.where(bound > 0, err / bound, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, math.inf)))
    return float(r.max())


def out_bound(ref, B, s16):
    return 2.0 ** -8 * (ref.abs() + B) + B if s16 else B


def report(name, ratio):
    print("%s: worst error / bound = %.3f" % (name, ratio))
    assert ratio <= 1.0, name


def cuda_gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def randn(gen, *shape):
    return torch.randn(*shape, device="cuda", generator=gen)


def rand(gen, *shape):
    return torch.rand(*shape, device="cuda", generator=gen)


def signed(gen, *shape):
    """magnitudes in [0.5, 1.5), signs alternating along the last axis from a random start: both signs wherever there are two elements"""
    flip = int(torch.randint(0, 2, (1,), device="cuda", generator=gen))
    return (0.5 + rand(gen, *shape)) * (1.0 - 2.0 * ((torch.arange(shape[-1], device="cuda") + flip) % 2))


# ---- finalise kernels ---------------------------------------------------------------------------------------------------------

ROW_COUNTS = [1, 3, 4, 5, 1023, 1024, 1025, 2047, 2048, 2049, 3200, 4097]


def raw_pixels(nrows):
    n = torch.full((nrows,), 64.0, dtype=torch.float64)
    n[-1] = 37.0
    return n


def synth_source(gen, C, n, ld, ch_off=0, ratio=0.0, tile_pix=0, seg_rows=0, seg_pix=0):
    """Partial rows as a producer would leave them, rounded to fp32: raw (sum, sum of squares >= sum^2 / n) or centred (sum, M2 >= 0),
    channel mean = ratio * its standard deviation; the floats in [nrows, ld) are NaN."""
    nrows, centred = n.numel(), tile_pix > 0
    sd = 0.5 + 1.5 * torch.rand(C, 1, generator=gen, dtype=torch.float64)
    mu = sd * (ratio + torch.randn(C, 1, generator=gen, dtype=torch.float64))
    k0 = n * (mu + sd * torch.randn(C, nrows, generator=gen, dtype=torch.float64) / n.sqrt())
    m2 = sd * sd * n * (0.5 + torch.rand(C, nrows, generator=gen, dtype=torch.float64))
    k1 = m2 if centred else m2 + k0 * k0 / n
    return make_source(k0.float(), k1.float(), n, ld, ch_off, tile_pix, seg_rows, seg_pix)


def make_source(k0, k1, n, ld, ch_off=0, tile_pix=0, seg_rows=0, seg_pix=0):
    C, nrows = k0.shape
    buf = Buf((2, C, ld))
    buf.t[:, :, :nrows] = torch.stack([k0, k1]).cuda()
    buf.before = buf.whole.clone()
    return dict(kind0=k0, kind1=k1, n=n, centred=tile_pix > 0, ch_off=ch_off, buf=buf,
                geom=[nrows, ld, C, ch_off, tile_pix, seg_rows, seg_pix])


def source_args(srcs):
    a = []
    for i in range(2):
        a += [P(srcs[i]["buf"])] + srcs[i]["geom"] if i < len(srcs) else [None, 0, 0, 0, 0, 0, 0, 0]
    return a


def bn_params(gen, C):
    gamma = (0.5 + torch.rand(C, generator=gen)) * torch.where(torch.rand(C, generator=gen) < 0.25, -1.0, 1.0)
    return gamma, torch.randn(C, generator=gen), torch.randn(C, generator=gen), 0.5 + torch.rand(C, generator=gen)


def finalize_fwd(name, srcs, C, count, gen, training=1):
    gamma, beta, rmean, rvar = bn_params(gen, C)
    ins = [Buf((C,), init=v) for v in (gamma, beta)]
    run = [Buf((C,), init=v) for v in (rmean, rvar)]
    outs = [Buf((C,)) for _ in range(4)]
    rc = lib().lf_debug_bn_finalize_fwd(*source_args(srcs), C, float(count), P(ins[0]), P(ins[1]), P(run[0]), P(run[1]), M32, E32, training,
                                        *[P(o) for o in outs], stream())
    torch.cuda.synchronize()
    assert rc == 0, lib().lf_last_error()
    for s in srcs:
        s["buf"].check()
    for b in ins:
        b.check()
    for b in run:
        b.check(True if training else None)
    for b in outs:
        b.check(True)
    cnt, mean, var = R.batch_stats(srcs, C)
    if training:
        assert bool(((cnt == count) | (cnt == 0)).all())
    ref = R.bn_finalize_fwd(mean, var, count, gamma, beta, rmean, rvar, training, momentum=M32, eps=E32)
    got = dict(zip(("scale", "shift", "asc", "ash"), [o.t.cpu() for o in outs]))
    keys = ["scale", "shift", "asc", "ash"]
    if training:
        got["rmean"], got["rvar"] = run[0].t.cpu(), run[1].t.cpu()
        keys += ["rmean", "rvar"]
    ratio = max(worst(got[k], ref[k], 2 * U * ref["S_" + k]) for k in keys)
    report(name, ratio)
    return ref, got


@pytest.mark.parametrize("nrows", ROW_COUNTS)
def test_finalize_fwd_row_counts(nrows):
    """Raw rows of 64 pixels (the last: 37), C = 16, ld = roundup4(nrows) and + 8, NaN between nrows and ld: one and two row groups per
    thread, one and two trips.  Every output is fp64 arithmetic on the fp64 column sums and ONE rounding: 2 u S."""
    for extra in (0, 8):
        gen = torch.Generator().manual_seed(100 + nrows + extra)
        n = raw_pixels(nrows)
        src = synth_source(gen, 16, n, roundup(nrows, 4) + extra, ratio=2.0)
        finalize_fwd("finalize_fwd rows=%d ld+%d" % (nrows, extra), [src], 16, float(n.sum()), gen)


CENTRED = [(5, 1280, 256, 1), (5, 256 * 4 + 37, 256, 1), (3, 256 * 2 + 37, 256, 4), (4, 313, 100, 4)]      # seg_rows, seg_pix, tile_pix, segments


@pytest.mark.parametrize("ratio", [0.0, 50.0])
@pytest.mark.parametrize("seg_rows,seg_pix,tile_pix,nseg", CENTRED)
def test_finalize_fwd_centred_rows(seg_rows, seg_pix, tile_pix, nseg, ratio):
    """Centred rows (sum v, M2) of one launch and of four phase launches laid end to end, whole and ragged last tiles, a tile of 100
    pixels; channel mean / std 0 and 50.  The reference merges (n_r, mean_r, M2_r) pairwise; 2 u S."""
    nrows = seg_rows * nseg
    for extra in (0, 8):
        gen = torch.Generator().manual_seed(200 + seg_pix + nseg + extra + int(ratio))
        n = R.row_pixels(nrows, tile_pix, seg_rows, seg_pix)
        src = synth_source(gen, 16, n, roundup(nrows, 4) + extra, ratio=ratio, tile_pix=tile_pix, seg_rows=seg_rows, seg_pix=seg_pix)
        finalize_fwd("finalize_fwd centred %dx%d of %d/%d" % (nseg, seg_rows, seg_pix, tile_pix), [src], 16, float(n.sum()), gen)


@pytest.mark.parametrize("Ca,Cb", [(48, 16), (64, 64)])
def test_finalize_fwd_two_sources(Ca, Cb):
    """The DownsamplerBlock case: centred convolution rows for channels [0, Ca) and raw pool rows for [Ca, Ca + Cb), different row
    counts and leading dimensions, the same 549 pixels.  2 u S."""
    gen = torch.Generator().manual_seed(300 + Ca)
    na, nb = R.row_pixels(3, 256, 3, 549), raw_pixels(9)
    assert float(na.sum()) == float(nb.sum()) == 549.0
    a = synth_source(gen, Ca, na, 4, ratio=3.0, tile_pix=256, seg_rows=3, seg_pix=549)
    b = synth_source(gen, Cb, nb, 20, ch_off=Ca, ratio=-3.0)
    finalize_fwd("finalize_fwd two sources %d+%d" % (Ca, Cb), [a, b], Ca + Cb, 549.0, gen)


def test_finalize_fwd_uncovered_channels_have_mean_zero():
    """A channel no source covers: the documented result is mean 0, variance 0 -- scale = gamma / sqrt(eps), shift = beta."""
    gen = torch.Generator().manual_seed(310)
    n = raw_pixels(5)
    ref, got = finalize_fwd("finalize_fwd uncovered", [synth_source(gen, 8, n, 8)], 16, float(n.sum()), gen)
    assert bool((got["ash"][8:] == 0).all()) and bool(((ref["asc"][8:] - E32 ** -0.5).abs() < 1e-12).all())


def test_finalize_fwd_eval_mode_uses_running_statistics():
    """training = 0, zero sources: the outputs come from the running statistics, which stay bit for bit (finalize_fwd checks)."""
    finalize_fwd("finalize_fwd eval", [], 16, 4096.0, torch.Generator().manual_seed(320), training=0)


def test_finalize_fwd_count_one():
    """One pixel: the unbiased-variance factor count / (count - 1) is skipped (csrc/lf_debug.h), not a division by zero."""
    gen = torch.Generator().manual_seed(330)
    v = torch.randn(16, 1, generator=gen).double()
    src = make_source(v.float(), (v * v).float(), torch.ones(1, dtype=torch.float64), 4)
    ref, got = finalize_fwd("finalize_fwd count 1", [src], 16, 1.0, gen)
    assert bool(torch.isfinite(got["rvar"]).all())


def test_finalize_fwd_constant_channel_clamps_negative_variance():
    """A constant channel v: rows (64 v, fl32(64 v^2)) with v chosen so that the rounding goes DOWN -- E[v^2] - mean^2 < 0 exactly.
    The clamp makes rstd = 1 / sqrt(eps); without it the variance would be negative by 2^-24 v^2.  2 u S."""
    vs = []
    x = 1.1
    while len(vs) < 16:
        v = float(torch.tensor(x, dtype=torch.float32))
        if float(torch.tensor(64 * v * v, dtype=torch.float32)) < 64 * v * v:         # v * v is exact in fp64 (two 24-bit factors)
            vs.append(v)
        x += 0.37
    v = torch.tensor(vs, dtype=torch.float64).view(16, 1).expand(16, 4)
    k0, k1 = (64 * v).float(), (64 * v * v).float()
    assert bool((k1.double().sum(1) / 256 - (k0.double().sum(1) / 256) ** 2 < 0).all())
    src = make_source(k0, k1, torch.full((4,), 64.0, dtype=torch.float64), 4)
    ref, got = finalize_fwd("finalize_fwd constant channel", [src], 16, 256.0, torch.Generator().manual_seed(340))
    assert bool((got["asc"] == torch.tensor(E32 ** -0.5).float()).all())


@pytest.mark.parametrize("training", [1, 0])
@pytest.mark.parametrize("nrows", ROW_COUNTS)
def test_finalize_bwd_row_counts(nrows, training):
    """Raw backward rows (sum g, sum g t) of mixed sign, the forward test's row counts and leading dimensions.  gbeta = S1, ggamma =
    asc S2 + ash S1, c1 / c2 = those / count (0 in eval mode): fp64 and one rounding, 2 u S with S from the absolute rows."""
    C, count = 16, 64.0 * nrows
    for extra in (0, 8):
        gen = torch.Generator().manual_seed(400 + nrows + extra)
        k0, k1 = torch.randn(C, nrows, generator=gen), 3 * torch.randn(C, nrows, generator=gen)
        src = make_source(k0, k1, torch.full((nrows,), 64.0, dtype=torch.float64), roundup(nrows, 4) + extra)
        asc, ash = 0.5 + torch.rand(C, generator=gen), torch.randn(C, generator=gen)
        ins = [Buf((C,), init=asc), Buf((C,), init=ash)]
        outs = [Buf((C,)) for _ in range(4)]
        rc = lib().lf_debug_bn_bwd_finalize(*source_args([src]), C, count, P(ins[0]), P(ins[1]), *[P(o) for o in outs], training, stream())
        torch.cuda.synchronize()
        assert rc == 0, lib().lf_last_error()
        src["buf"].check()
        for b in ins:
            b.check()
        for b in outs:
            b.check(True)
        ref = R.bn_bwd_finalize(k0.double().sum(1), k1.double().sum(1), asc, ash, count, training)
        S = R.bn_bwd_finalize(k0.double().abs().sum(1), k1.double().abs().sum(1), asc, ash.abs(), count, training)
        ratio = max(worst(o.t.cpu(), ref[k], 2 * U * S[k]) for o, k in zip(outs, ("c1", "c2", "ggamma", "gbeta")))
        if not training:
            assert bool((outs[0].t == 0).all() and (outs[1].t == 0).all())
        report("finalize_bwd rows=%d ld+%d training=%d" % (nrows, extra, training), ratio)


# ---- streaming kernels ----------------------------------------------------------------------------------------------------------

STREAM_C = [4, 8, 16, 64, 128]
LAYOUTS = [(3, 35), (1, 1)]            # (images, pixels per image): workgroups straddle images, 105 pixels; one pixel


def drop_mask(gen, N, C):
    return torch.where(rand(gen, N, C) < 0.7, 1.0 / 0.7, 0.0).float()


def act_case(gen, C, s16, N, ppi, use_dm, use_res):
    npix = N * ppi
    x, sc, sh = randn(gen, npix, C).to(dt(s16)), signed(gen, C), randn(gen, C)
    dm = drop_mask(gen, N, C) if use_dm else None
    res = randn(gen, npix, C).to(dt(s16)) if use_res else None
    bx, bsc, bsh = Buf(x.shape, dt(s16), x), Buf((C,), init=sc), Buf((C,), init=sh)
    bdm = Buf(dm.shape, init=dm) if use_dm else None
    bres = Buf(res.shape, dt(s16), res) if use_res else None
    by = Buf(x.shape, dt(s16))
    rc = lib().lf_debug_bn_act(P(bx), P(bsc), P(bsh), P(bdm), P(bres), P(by), npix, C, ppi, s16, stream())
    torch.cuda.synchronize()
    assert rc == 0, lib().lf_last_error()
    for b in (bx, bsc, bsh, bdm, bres):
        if b is not None:
            b.check()
    by.check(True)
    ref = R.bn_act(x, sc, sh, dm, res, ppi)
    S = R.bn_act(x.abs(), sc.abs(), sh.abs(), dm, None if res is None else res.abs(), ppi)
    return worst(by.t, ref, out_bound(ref, 4 * U * S, s16))


@pytest.mark.parametrize("s16", [0, 1])
@pytest.mark.parametrize("C", STREAM_C)
def test_bn_act(C, s16):
    """y = relu((x sc + sh) dm + res): mul, add, mul, add -> 4 u (|x sc dm| + |sh dm| + |res|); with and without dm (values 0 and
    1 / 0.7) and res; 3 images of 35 pixels and a single pixel.  bf16, C = 4: the one-quad form, else 8 channels per thread."""
    gen = cuda_gen(500 + C + s16)
    ratio = max(act_case(gen, C, s16, N, ppi, use_dm, use_res) for N, ppi in LAYOUTS for use_dm in (1, 0) for use_res in (1, 0))
    report("bn_act C=%d s16=%d" % (C, s16), ratio)


def test_bn_act_grid_cap():
    """C = 128, 131072 + 33 pixels, fp32: 4,195,360 units against 16384 workgroups of 256 -- the second trip of the grid-stride loop,
    one image boundary inside."""
    report("bn_act grid cap", act_case(cuda_gen(510), 128, 0, 5, 26221, 1, 1))


def small_ints(gen, *shape):
    """from {-2, -1, 1, 2}: products and sums of fewer than 2^22 of them are exact in fp32 in any order"""
    return torch.tensor([-2.0, -1.0, 1.0, 2.0], device="cuda")[torch.randint(0, 4, shape, device="cuda", generator=gen)]


def bwd_operands(gen, C, s16, N, ppi, use_dm, use_y, ints=False):
    npix = N * ppi
    g, t = randn(gen, npix, C).to(dt(s16)), (2 * randn(gen, npix, C) + 1).to(dt(s16))
    if ints:
        g, t = small_ints(gen, npix, C).to(dt(s16)), small_ints(gen, npix, C).to(dt(s16))
    y = torch.relu(randn(gen, npix, C)).to(dt(s16)) if use_y else None
    dm = drop_mask(gen, N, C) if use_dm else None
    return g, y, t, dm


def reduce_case(gen, C, s16, N, ppi, use_dm, use_y, ints=False):
    """ints: g and t from {-2, -1, 1, 2}, no dropout mask -- every partial sum is an exact integer, the rows must add up to the column
    sums EXACTLY: one dropped or doubled pixel fails at any pixel count."""
    npix = N * ppi
    g, y, t, dm = bwd_operands(gen, C, s16, N, ppi, use_dm and not ints, use_y, ints)
    asc, ash = 0.5 + rand(gen, C), randn(gen, C)
    nrows = min((npix + 63) // 64, 1024)
    ld = roundup(nrows, 4) + 4
    bg, bt, basc, bash = Buf(g.shape, dt(s16), g), Buf(t.shape, dt(s16), t), Buf((C,), init=asc), Buf((C,), init=ash)
    by = Buf(y.shape, dt(s16), y) if use_y else None
    bdm = Buf(dm.shape, init=dm) if use_dm else None
    rows = Buf((2, C, ld))
    rc = lib().lf_debug_bn_bwd_reduce(P(bg), P(by), P(bt), P(basc), P(bash), P(bdm), P(rows), ld, npix, C, ppi, s16, stream())
    torch.cuda.synchronize()
    assert rc == nrows, (rc, nrows, lib().lf_last_error())
    for b in (bg, by, bt, basc, bash, bdm):
        if b is not None:
            b.check()
    rows.check((torch.arange(ld) < nrows).view(1, 1, ld))
    got = rows.t[:, :, :nrows].double().sum(-1)
    s1, s2 = R.bn_bwd_sums(g, y, t, dm, ppi)
    if ints:
        assert torch.equal(got[0], s1) and torch.equal(got[1], s2), "integer data: the rows add up exactly"
    a1, a2 = R.bn_bwd_sums(g.abs(), y, t.abs(), dm, ppi)
    n = min(npix, roundup(-(-npix // nrows), 256))
    return max(worst(got[0], s1, (n + 8) * U * a1), worst(got[1], s2, (n + 8) * U * a2))


@pytest.mark.parametrize("s16", [0, 1])
@pytest.mark.parametrize("C", STREAM_C)
def test_bn_bwd_reduce(C, s16):
    """Partial rows of (sum gm, sum gm t), gm = g [y > 0] dm: the written rows summed in fp64 against the column sums, (n + 8) u
    sum |term|, and EXACTLY on integer data; the row count is min(ceil(npix / 64), 1024), the rest of the row buffer stays NaN."""
    gen = cuda_gen(600 + C + s16)
    ratio = max(reduce_case(gen, C, s16, N, ppi, use_dm, use_y) for N, ppi in LAYOUTS for use_dm in (1, 0) for use_y in (1, 0))
    reduce_case(gen, C, s16, 3, 35, 0, 1, ints=True)
    report("bn_bwd_reduce C=%d s16=%d" % (C, s16), ratio)


def test_bn_bwd_reduce_row_cap():
    """C = 16, 65536 + 70 pixels: 1026 rows of 64 pixels are capped at 1024, a row covers more than 64 pixels."""
    gen = cuda_gen(610)
    reduce_case(gen, 16, 0, 2, 32803, 0, 1, ints=True)
    report("bn_bwd_reduce row cap", reduce_case(gen, 16, 0, 2, 32803, 1, 1))


def apply_case(gen, C, s16, N, ppi, use_dm, use_y, use_gz):
    npix = N * ppi
    g, y, t, dm = bwd_operands(gen, C, s16, N, ppi, use_dm, use_y)
    vecs = [0.5 + rand(gen, C), randn(gen, C), signed(gen, C), 0.1 * randn(gen, C), 0.1 * randn(gen, C)]      # asc ash gamma c1 c2
    bg, bt = Buf(g.shape, dt(s16), g), Buf(t.shape, dt(s16), t)
    by = Buf(y.shape, dt(s16), y) if use_y else None
    bdm = Buf(dm.shape, init=dm) if use_dm else None
    bv = [Buf((C,), init=v) for v in vecs]
    bgt, bgz = Buf(g.shape, dt(s16)), Buf(g.shape, dt(s16))
    rc = lib().lf_debug_bn_bwd_apply(P(bg), P(by), P(bt), *[P(b) for b in bv], P(bdm), P(bgt), P(bgz) if use_gz else None, npix, C, ppi, s16,
                                     stream())
    torch.cuda.synchronize()
    assert rc == 0, lib().lf_last_error()
    for b in [bg, by, bt, bdm] + bv:
        if b is not None:
            b.check()
    bgt.check(True)
    bgz.check(True if use_gz else None)
    gt, gz, S = R.bn_bwd_apply(g, y, t, vecs[0], vecs[1], vecs[2], vecs[3], vecs[4], dm, ppi)
    if use_gz:
        want = g if y is None else torch.where(y > 0, g, torch.zeros_like(g))
        assert torch.equal(bgz.t.view(BITS[dt(s16)]), want.view(BITS[dt(s16)])), "g_z is g [y > 0] bit for bit"
    return worst(bgt.t, gt, out_bound(gt, 8 * U * S, s16))


@pytest.mark.parametrize("s16", [0, 1])
@pytest.mark.parametrize("C", STREAM_C)
def test_bn_bwd_apply(C, s16):
    """g_t = gamma rstd (gm - c1 - xhat c2): xhat 2 roundings, the dropout product, two subtractions with a product, gamma rstd and
    the last product -> 8 u |gamma rstd| (|gm| + |c1| + (|t rstd| + |ash|) |c2|); g_z bit for bit, and untouched when not asked for."""
    gen = cuda_gen(700 + C + s16)
    ratio = max(apply_case(gen, C, s16, N, ppi, use_dm, use_y, use_gz) for N, ppi in LAYOUTS for use_dm, use_y, use_gz in
                ((1, 1, 1), (0, 1, 0), (1, 0, 1), (0, 0, 0), (1, 1, 0)))
    report("bn_bwd_apply C=%d s16=%d" % (C, s16), ratio)


def test_bn_bwd_apply_grid_cap():
    """C = 128, 131072 + 33 pixels, fp32: the second trip of the grid-stride loop."""
    report("bn_bwd_apply grid cap", apply_case(cuda_gen(710), 128, 0, 5, 26221, 1, 1, 1))


def test_bn_five_launches_chained():
    """N = 3, 5 x 7, C = 16, fp32: finalise-forward, act, reduce, finalise-backward, apply back to back on the device, against torch
    fp64 AUTOGRAD of relu(batch_norm(t) dm + res).  The forward rows are the centred rows of t (64-pixel tiles) rounded to fp32; res
    is chosen so that every pre-activation is at least 1 from zero: no ReLU mask can differ.  Bounds, with d = relative error 8 u of
    every per-channel vector (rows u, finalise 2 u, the variance and the products of two such factors):
      y       4 u S_act + 8 u (|t scale| + |mean scale| + |beta|) dm
      sums    rows of up to npix pixels: e1 = (npix + 8) u sum |gm|, e2 = (npix + 8) u sum |gm t|
      gbeta   e1;  ggamma  rstd e2 + |ash| e1 + 16 u (rstd sum |gm t| + |ash| sum |gm|)
      g_t     8 u S_apply + |gamma rstd| (d_c1 + |xhat| d_c2) + 24 u S_apply,  d_c1 = e_gbeta / count, d_c2 = e_ggamma / count"""
    import torch.nn.functional as F
    N, ppi, C = 3, 35, 16
    npix = N * ppi
    gen = cuda_gen(800)
    t = 2 * randn(gen, npix, C) + 1
    gamma, beta, dm, gy = signed(gen, C), randn(gen, C), drop_mask(gen, N, C), randn(gen, npix, C)
    rmean, rvar = randn(gen, C), 0.5 + rand(gen, C)
    td = t.double()
    bnd = (td - td.mean(0)) / torch.sqrt(td.var(0, unbiased=False) + E32) * gamma.double() + beta.double()
    pre = bnd * dm.double()[R.image_of_pixel(npix, ppi, "cuda")]
    res = (torch.where(rand(gen, npix, C) < 0.5, -1.0, 1.0) * (1.5 + rand(gen, npix, C)) - pre).float()
    assert float((pre + res.double()).abs().min()) > 1.0
    # torch's own composite and its autograd
    tt, gg, bb = td.clone().requires_grad_(True), gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    rm, rv = rmean.double(), rvar.double()
    bn = F.batch_norm(tt.view(N, ppi, 1, C).permute(0, 3, 1, 2), rm, rv, gg, bb, training=True, momentum=M32, eps=E32)
    yref = torch.relu(bn.permute(0, 2, 3, 1).reshape(npix, C) * dm.double()[R.image_of_pixel(npix, ppi, "cuda")] + res.double())
    (yref * gy.double()).sum().backward()
    # the five launches
    k0 = torch.stack([td[:64].sum(0), td[64:].sum(0)], 1)
    k1 = torch.stack([((td[:64] - td[:64].mean(0)) ** 2).sum(0), ((td[64:] - td[64:].mean(0)) ** 2).sum(0)], 1)
    src = make_source(k0.float().cpu(), k1.float().cpu(), R.row_pixels(2, 64, 2, npix), 4, tile_pix=64, seg_rows=2, seg_pix=npix)
    b = {k: Buf((C,), init=v) for k, v in (("gamma", gamma), ("beta", beta), ("rmean", rmean), ("rvar", rvar))}
    for k in ("scale", "shift", "asc", "ash", "c1", "c2", "ggamma", "gbeta"):
        b[k] = Buf((C,))
    bt, bres, bdm, bgy = Buf(t.shape, init=t), Buf(t.shape, init=res), Buf(dm.shape, init=dm), Buf(t.shape, init=gy)
    by, bgt, bgz, rows = Buf(t.shape), Buf(t.shape), Buf(t.shape), Buf((2, C, 4))
    L, st = lib(), stream()
    rcs = [L.lf_debug_bn_finalize_fwd(*source_args([src]), C, float(npix), P(b["gamma"]), P(b["beta"]), P(b["rmean"]), P(b["rvar"]), M32, E32, 1,
                                      P(b["scale"]), P(b["shift"]), P(b["asc"]), P(b["ash"]), st),
           L.lf_debug_bn_act(P(bt), P(b["scale"]), P(b["shift"]), P(bdm), P(bres), P(by), npix, C, ppi, 0, st),
           L.lf_debug_bn_bwd_reduce(P(bgy), P(by), P(bt), P(b["asc"]), P(b["ash"]), P(bdm), P(rows), 4, npix, C, ppi, 0, st)]
    rows_src = dict(buf=rows, geom=[2, 4, C, 0, 0, 0, 0])
    rcs += [L.lf_debug_bn_bwd_finalize(*source_args([rows_src]), C, float(npix), P(b["asc"]), P(b["ash"]), P(b["c1"]), P(b["c2"]), P(b["ggamma"]),
                                       P(b["gbeta"]), 1, st),
            L.lf_debug_bn_bwd_apply(P(bgy), P(by), P(bt), P(b["asc"]), P(b["ash"]), P(b["gamma"]), P(b["c1"]), P(b["c2"]), P(bdm), P(bgt), P(bgz),
                                    npix, C, ppi, 0, st)]
    torch.cuda.synchronize()
    assert rcs == [0, 0, 2, 0, 0], (rcs, L.lf_last_error())
    for k in ("scale", "shift", "asc", "ash", "c1", "c2", "ggamma", "gbeta", "rmean", "rvar"):
        b[k].check(True)
    for x in (by, bgt, bgz):
        x.check(True)
    rows.check((torch.arange(4) < 2).view(1, 1, 4))
    for x in (bt, bres, bdm, bgy, b["gamma"], b["beta"]):
        x.check()
    dmx = dm.double()[R.image_of_pixel(npix, ppi, "cuda")]
    mean, rstd = td.mean(0), 1 / torch.sqrt(td.var(0, unbiased=False) + E32)
    scale = (gamma.double() * rstd).abs()
    S_act = ((td.abs() + mean.abs()) * scale + beta.double().abs()) * dmx + res.double().abs()
    r_y = worst(by.t, yref.detach(), 4 * U * S_act + 8 * U * ((td.abs() + mean.abs()) * scale + beta.double().abs()) * dmx)
    gm = gy.double() * (yref.detach() > 0) * dmx
    a1, a2 = gm.abs().sum(0), (gm * td).abs().sum(0)
    e1, e2 = (npix + 8) * U * a1, (npix + 8) * U * a2
    ash = (mean * rstd).abs()
    e_gbeta, e_ggamma = e1, rstd * e2 + ash * e1 + 16 * U * (rstd * a2 + ash * a1)
    r_p = max(worst(b["gbeta"].t, bb.grad, e_gbeta), worst(b["ggamma"].t, gg.grad, e_ggamma),
              worst(b["rmean"].t, rm, 8 * U * (rmean.double().abs() + mean.abs())),
              worst(b["rvar"].t, rv, 8 * U * (rvar.double().abs() + td.var(0))))
    xhat = ((td - mean) * rstd).abs()
    S_apply = scale * (gm.abs() + a1 / npix + (td.abs() * rstd + ash) * (rstd * a2 + ash * a1) / npix)
    r_g = worst(bgt.t, tt.grad, 32 * U * S_apply + scale * (e_gbeta + xhat * e_ggamma) / npix)
    assert torch.equal(bgz.t, torch.where(by.t > 0, gy, torch.zeros_like(gy)))
    report("five launches chained (y, parameter gradients and running statistics, g_t)", max(r_y, r_p, r_g))


# ---- pool branch ------------------------------------------------------------------------------------------------------------------

POOL_SHAPES = [(3, 6, 10, 16, 64, 48), (2, 4, 6, 64, 128, 64), (1, 2, 2, 16, 16, 0), (2, 6, 10, 4, 12, 4)]      # N, H, W, Cin, cat_pix, choff


def channel_mask(cat_pix, choff, Cin):
    c = torch.arange(cat_pix)
    return ((c >= choff) & (c < choff + Cin)).view(1, 1, 1, cat_pix)


def tied_input(gen, shape, s16):
    """five distinct values, the largest drawn half of the time, zero with either sign: most 2x2 windows tie, some between -0.0
    and +0.0"""
    vals = torch.tensor([-1.5, -0.5, 0.0, 0.5, 1.0], device="cuda")
    x = vals[torch.bucketize(rand(gen, *shape), torch.tensor([0.1, 0.2, 0.35, 0.5], device="cuda"))]
    x = torch.where((x == 0) & (rand(gen, *shape) < 0.5), -x, x)
    return x.to(dt(s16))


def pool_fwd_case(gen, shape, s16, x=None, with_rows=True):
    """x given: tied_input -- multiples of 1/2, so every sum of values and of squares is exact in fp32 and the rows must add up EXACTLY."""
    N, H, W, Cin, cat_pix, choff = shape
    exact = x is not None
    Ho, Wo = H // 2, W // 2
    npo = N * Ho * Wo
    if x is None:
        x = randn(gen, N, H, W, Cin).to(dt(s16))
    nrows = min((npo + 63) // 64, 1024)
    ld = roundup(nrows, 4) + 4
    bx, cat, rows = Buf(x.shape, dt(s16), x), Buf((N, Ho, Wo, cat_pix), dt(s16)), Buf((2, Cin, ld))
    rc = lib().lf_debug_pool_concat_fwd(P(bx), N, H, W, Cin, P(cat), cat_pix, choff, P(rows) if with_rows else None, ld, s16, stream())
    torch.cuda.synchronize()
    assert rc == nrows, (rc, nrows, lib().lf_last_error())
    bx.check()
    cat.check(channel_mask(cat_pix, choff, Cin))
    rows.check((torch.arange(ld) < nrows).view(1, 1, ld) if with_rows else None)
    stored = cat.t[..., choff:choff + Cin]
    want, _ = R.pool_argmax(x)
    assert torch.equal(stored, want), "pooled values are exact"            # (by value: -0.0 == +0.0)
    if not with_rows:
        return 0.0
    v = stored.double().reshape(npo, Cin)
    got = rows.t[:, :, :nrows].double().sum(-1)
    if exact:
        assert torch.equal(got[0], v.sum(0)) and torch.equal(got[1], (v * v).sum(0)), "multiples of 1/2: the rows add up exactly"
    n = min(npo, roundup(-(-npo // nrows), 256))
    return max(worst(got[0], v.sum(0), (n + 8) * U * v.abs().sum(0)), worst(got[1], (v * v).sum(0), (n + 8) * U * (v * v).sum(0)))


@pytest.mark.parametrize("s16", [0, 1])
@pytest.mark.parametrize("shape", POOL_SHAPES)
def test_pool_concat_fwd(shape, s16):
    """Values exact, the other channels of the concat buffer untouched; raw rows (sum v, sum v^2) against the STORED values, (n + 8) u
    sum |term|; random and heavily tied input; rows = NULL leaves the row buffer alone and still returns the count."""
    gen = cuda_gen(900 + shape[1] * shape[2] + s16)
    ratio = max(pool_fwd_case(gen, shape, s16), pool_fwd_case(gen, shape, s16, x=tied_input(gen, shape[:4], s16)),
                pool_fwd_case(gen, shape, s16, with_rows=False))
    report("pool_concat_fwd %s s16=%d" % (shape, s16), ratio)


def test_pool_concat_fwd_row_cap():
    """65536 + 70 output pixels, Cin = 16: 1026 rows capped at 1024."""
    gen, shape = cuda_gen(910), (1, 4, 2 * 32803, 16, 16, 0)
    pool_fwd_case(gen, shape, 0, x=tied_input(gen, shape[:4], 0))
    report("pool_concat_fwd row cap", pool_fwd_case(gen, shape, 0))


@pytest.mark.parametrize("s16", [0, 1])
@pytest.mark.parametrize("shape", POOL_SHAPES)
def test_pool_affine_fwd(shape, s16):
    """Inference form relu(max sc + sh) with scales of both signs -- the affine map after the max: mul, add -> 4 u (|m sc| + |sh|)."""
    N, H, W, Cin, cat_pix, choff = shape
    gen = cuda_gen(920 + H * W + s16)
    x, sc, sh = randn(gen, N, H, W, Cin).to(dt(s16)), signed(gen, Cin), randn(gen, Cin)
    assert bool((sc < 0).any() and (sc > 0).any())
    bx, bsc, bsh, cat = Buf(x.shape, dt(s16), x), Buf((Cin,), init=sc), Buf((Cin,), init=sh), Buf((N, H // 2, W // 2, cat_pix), dt(s16))
    rc = lib().lf_debug_pool_affine_fwd(P(bx), N, H, W, Cin, P(cat), cat_pix, choff, P(bsc), P(bsh), s16, stream())
    torch.cuda.synchronize()
    assert rc == 0, lib().lf_last_error()
    for b in (bx, bsc, bsh):
        b.check()
    cat.check(channel_mask(cat_pix, choff, Cin))
    ref = R.pool_affine(x, sc, sh)
    S = R.pool_argmax(x.double())[0].abs() * sc.double().abs() + sh.double().abs()
    report("pool_affine_fwd %s s16=%d" % (shape, s16), worst(cat.t[..., choff:choff + Cin], ref, out_bound(ref, 4 * U * S, s16)))


def pool_bwd_case(gen, shape, s16):
    N, H, W, Cin, cat_pix, choff = shape
    x = tied_input(gen, (N, H, W, Cin), s16)
    # hand-made first window of channels 0..2, scan order: zeros of both signs tie for the maximum -> arg-max 0, 0, 1
    x[0, :2, :2, :3] = torch.tensor([[[-0.0, 0.0, -1.5], [0.0, -0.0, -0.0]], [[-0.5, -0.0, 0.0], [-1.5, 0.0, -0.5]]], device="cuda").to(dt(s16))
    win = R.pool_windows(x.float())
    tied = (win == win.max(-1, keepdim=True)[0]).sum(-1) > 1
    zero_mix = tied & (win.max(-1)[0] == 0) & (torch.signbit(win) & (win == 0)).any(-1) & (~torch.signbit(win) & (win == 0)).any(-1)
    gcat = randn(gen, N, H // 2, W // 2, cat_pix).to(dt(s16))
    bx, bg, gx = Buf(x.shape, dt(s16), x), Buf(gcat.shape, dt(s16), gcat), Buf(x.shape, dt(s16))
    rc = lib().lf_debug_pool_bwd(P(bx), P(bg), N, H, W, Cin, cat_pix, choff, P(gx), s16, stream())
    torch.cuda.synchronize()
    assert rc == 0, lib().lf_last_error()
    bx.check()
    bg.check()
    gx.check(True)
    want = R.pool_bwd(x, gcat[..., choff:choff + Cin].contiguous())
    assert torch.equal(gx.t.view(BITS[dt(s16)]), want.view(BITS[dt(s16)])), "the pooled gradient goes to the first maximum, bit for bit"
    return float(tied.double().mean()), int(zero_mix.sum())


@pytest.mark.parametrize("s16", [0, 1])
@pytest.mark.parametrize("shape", POOL_SHAPES)
def test_pool_bwd_ties(shape, s16):
    """Input from five distinct values with zeros of either sign: most windows tie.  Every element of gx is written: the gradient at
    the FIRST maximum in scan order, +0 elsewhere, bit for bit in both storage types."""
    tied, zero_mix = pool_bwd_case(cuda_gen(930 + shape[1] * shape[2] + s16), shape, s16)
    print("pool_bwd %s s16=%d: %.0f%% of the windows tie, %d between -0.0 and +0.0; exact" % (shape, s16, 100 * tied, zero_mix))
    assert zero_mix >= 3 and tied > (0.5 if shape[0] * shape[1] * shape[2] * shape[3] >= 400 else 0.25)


def test_pool_bwd_grid_cap():
    """N = 1, 516 x 512, Cin = 64, fp32: 1,056,768 units against 4096 workgroups of 256 -- the second trip."""
    tied, zero_mix = pool_bwd_case(cuda_gen(940), (1, 516, 512, 64, 64, 0), 0)
    assert tied > 0.5 and zero_mix >= 3


# ---- stem forward -------------------------------------------------------------------------------------------------------------------

STEM_SHAPES = [(2, 6, 10), (3, 18, 34), (1, 2, 2)]             # (N, H/2, W/2): 30 pixels; 459 = two tiles; one pixel


def stem_image(gen, N, Cin, H, W):
    """column 0 and the last column hold values unlike the interior: a tap that crosses the left padding into the previous row's last
    pixel changes the result by ~10 w"""
    img = randn(gen, N, Cin, H, W)
    img[..., 0] = 10 + randn(gen, N, Cin, H)
    img[..., W - 1] = -10 + randn(gen, N, Cin, H)
    return img


@pytest.mark.parametrize("s16", [0, 1])
@pytest.mark.parametrize("shape", STEM_SHAPES)
@pytest.mark.parametrize("Cin", [1, 2, 3, 4])
def test_stem_fwd(Cin, shape, s16):
    """cat = [conv 3x3 stride 2 pad 1 | maxpool] of the NCHW image: (9 Cin + 2) u (sum |w x| + |b|) on the convolution channels, the
    pooled channels exact (bf16: rounded once); raw statistics rows, one per 256 pixels (module docstring); then the inference form
    with scales of both signs: the convolution bound times |sc| plus 3 u (|v sc| + |sh|)."""
    N, Ho, Wo = shape
    H, W, Cc, npo = 2 * Ho, 2 * Wo, 16 - Cin, N * Ho * Wo
    gen = cuda_gen(1000 + 16 * Cin + Ho + s16)
    img, w, b = stem_image(gen, N, Cin, H, W), 0.3 * randn(gen, Cc, Cin, 3, 3), randn(gen, Cc)
    sc, sh = signed(gen, 16), randn(gen, 16)
    nrows = (npo + 255) // 256
    ld = roundup(nrows, 4) + 4
    ins = [Buf(v.shape, init=v) for v in (img, w, b, sc, sh)]
    cat, rows, cat2 = Buf((N, Ho, Wo, 16), dt(s16)), Buf((2, 16, ld)), Buf((N, Ho, Wo, 16), dt(s16))
    rc = lib().lf_debug_stem_fwd(P(ins[0]), N, Cin, H, W, P(ins[1]), P(ins[2]), None, None, P(cat), P(rows), ld, s16, stream())
    rc2 = lib().lf_debug_stem_fwd(P(ins[0]), N, Cin, H, W, P(ins[1]), P(ins[2]), P(ins[3]), P(ins[4]), P(cat2), None, 0, s16, stream())
    torch.cuda.synchronize()
    assert (rc, rc2) == (nrows, 0), (rc, rc2, lib().lf_last_error())
    for x in ins:
        x.check()
    cat.check(True)
    cat2.check(True)
    rows.check((torch.arange(ld) < nrows).view(1, 1, ld))
    ref, S = R.stem(img, w, b), R.stem_abs(img, w, b)
    B = (9 * Cin + 2) * U * S
    B[..., Cc:] = 0
    r_train = worst(cat.t, ref, out_bound(ref, B, s16))
    if not s16:
        assert torch.equal(cat.t[..., Cc:], ref[..., Cc:].float()), "pooled channels are exact"
    # statistics rows: fp32 storage -- the stored values are what was summed; bf16 -- the reference, with the kernel's own error per term
    v = (ref if s16 else cat.t.double()).reshape(npo, 16)
    e = B.reshape(npo, 16) if s16 else torch.zeros_like(v)
    got = rows.t[:, :, :nrows].double().sum(-1)
    n = min(npo, 256)
    r_rows = max(worst(got[0], v.sum(0), (n + 8) * U * v.abs().sum(0) + e.sum(0)),
                 worst(got[1], (v * v).sum(0), (n + 8) * U * (v * v).sum(0) + (2 * v.abs() * e + e * e).sum(0)))
    ref2 = torch.relu(ref * sc.double() + sh.double())
    B2 = B * sc.double().abs() + 3 * U * ((ref * sc.double()).abs() + sh.double().abs())
    r_inf = worst(cat2.t, ref2, out_bound(ref2, B2, s16))
    print("stem_fwd Cin=%d %s s16=%d: training %.3f, rows %.3f, inference %.3f" % (Cin, shape, s16, r_train, r_rows, r_inf))
    report("stem_fwd Cin=%d %s s16=%d" % (Cin, shape, s16), max(r_train, r_rows, r_inf))


# ---- head ---------------------------------------------------------------------------------------------------------------------------

def head_case(gen, K, N, h, wd, s16):
    x, w, b = randn(gen, N, h, wd, 16).to(dt(s16)), 0.3 * randn(gen, 16, K, 2, 2), randn(gen, K)
    gout = randn(gen, N, K, 2 * h, 2 * wd)
    bx, bw, bb, bg = Buf(x.shape, dt(s16), x), Buf(w.shape, init=w), Buf((K,), init=b), Buf(gout.shape, init=gout)
    out, gx = Buf(gout.shape), Buf(x.shape, dt(s16))
    rc = lib().lf_debug_head_fwd(P(bx), P(bw), P(bb), P(out), N, h, wd, K, s16, stream())
    rc2 = lib().lf_debug_head_bwd_data(P(bg), P(bw), P(gx), N, h, wd, K, s16, stream())
    torch.cuda.synchronize()
    assert (rc, rc2) == (0, 0), lib().lf_last_error()
    for v in (bx, bw, bb, bg):
        v.check()
    out.check(True)
    gx.check(True)
    r_f = worst(out.t, R.head_fwd(x, w, b), 18 * U * R.head_fwd(x.abs(), w.abs(), b.abs()))
    ref = R.head_bwd_data(gout, w)
    r_b = worst(gx.t, ref, out_bound(ref, (4 * K + 1) * U * R.head_bwd_data(gout.abs(), w.abs()), s16))
    return max(r_f, r_b)


@pytest.mark.parametrize("s16", [0, 1])
@pytest.mark.parametrize("shape", [(2, 3, 5), (1, 1, 1), (3, 7, 16)])
@pytest.mark.parametrize("K", [1, 2, 5, 8])
def test_head_fwd_and_bwd_data(K, shape, s16):
    """ConvTranspose2d(16, K, 2, stride 2): 16 fused multiply-adds on the bias -> 18 u (sum |x w| + |b|); its data gradient 4 K
    fused multiply-adds -> (4 K + 1) u sum |g w| (bf16 gx: the bf16 rule)."""
    report("head K=%d %s s16=%d" % (K, shape, s16), head_case(cuda_gen(1100 + 8 * K + shape[1] + s16), K, *shape, s16))


def test_head_grid_cap():
    """K = 1, 4096 * 256 + 19 pixels, fp32: the second trip of both kernels' grid-stride loops."""
    report("head grid cap", head_case(cuda_gen(1110), 1, 1, 1, 4096 * 256 + 19, 0))


# ---- pointwise (encoder.output_conv) ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(3, 5, 7), (1, 1, 1), (2, 16, 17)])
@pytest.mark.parametrize("C,K,s16", [(4, 1, 0), (128, 2, 0), (256, 8, 0), (128, 2, 1), (256, 8, 1)])
def test_pointwise(C, K, s16, shape):
    """Conv2d(C, K, 1), NHWC in, NCHW out: forward (C + 1) u (sum |x w| + |b|), with and without a bias; data gradient (K + 1) u
    sum |g w|; gw, gb from rows of 256 pixels and their sum: (256 + rows + 8) u sum |g x|.  gx = NULL, gw only and gb only leave the
    others' buffers untouched.  (The bf16 entry points take C % 8 == 0: no (4, 1) case there.)"""
    N, h, wd = shape
    npix = N * h * wd
    gen = cuda_gen(1200 + C + h + s16)
    x, w, b, gy = randn(gen, N, h, wd, C).to(dt(s16)), 0.3 * randn(gen, K, C), randn(gen, K), randn(gen, N, K, h, wd)
    L = lib()
    fwd, bwd = (L.lf_pointwise_bf16_fwd, L.lf_pointwise_bf16_bwd) if s16 else (L.lf_pointwise_fwd, L.lf_pointwise_bwd)
    bx, bw, bb, bg = Buf(x.shape, dt(s16), x), Buf(w.shape, init=w), Buf((K,), init=b), Buf(gy.shape, init=gy)
    nscr = L.lf_pointwise_scratch_floats(N, h, wd, C, K)
    rows = (npix + 255) // 256
    assert nscr == rows * (K * C + K)
    ratios = []
    for bias in (1, 0):
        y = Buf(gy.shape)
        assert fwd(P(bx), P(bw), P(bb) if bias else None, P(y), N, h, wd, C, K, stream()) == 0, L.lf_last_error()
        torch.cuda.synchronize()
        y.check(True)
        zero = torch.zeros_like(b)
        ratios.append(worst(y.t, R.pointwise_fwd(x, w, b if bias else None), (C + 1) * U * R.pointwise_fwd(x.abs(), w.abs(), b.abs() if bias else zero)))
    rgx, rgw, rgb = R.pointwise_bwd(x, gy, w)
    agx, agw, agb = R.pointwise_bwd(x.abs(), gy.abs(), w.abs())
    for want_gx, want_gw, want_gb in ((1, 1, 1), (0, 1, 1), (0, 1, 0), (0, 0, 1)):
        gx, gw, gb, scr = Buf(x.shape, dt(s16)), Buf(w.shape), Buf((K,)), Buf((nscr,))
        rc = bwd(P(bx), P(bg), P(bw), P(gx) if want_gx else None, P(gw) if want_gw else None, P(gb) if want_gb else None, N, h, wd, C, K,
                 P(scr), stream())
        torch.cuda.synchronize()
        assert rc == 0, L.lf_last_error()
        gx.check(True if want_gx else None)
        gw.check(True if want_gw else None)
        gb.check(True if want_gb else None)
        scr.check(True)
        if want_gx:
            ratios.append(worst(gx.t, rgx, out_bound(rgx, (K + 1) * U * agx, s16)))
        if want_gw:
            ratios.append(worst(gw.t, rgw, (256 + rows + 8) * U * agw))
        if want_gb:
            ratios.append(worst(gb.t, rgb, (256 + rows + 8) * U * agb))
    for v in (bx, bw, bb, bg):
        v.check()
    report("pointwise C=%d K=%d %s s16=%d" % (C, K, shape, s16), max(ratios))


# ---- host refusals ------------------------------------------------------------------------------------------------------------------

def test_host_refusals_do_not_launch():
    """Arguments outside a launcher's geometry return -1 with a message and launch nothing: every output stays NaN."""
    L, C = lib(), 16
    gen = torch.Generator().manual_seed(1300)
    src = synth_source(gen, C, raw_pixels(6), 8)
    vec = [Buf((C,), init=torch.ones(C)) for _ in range(4)]
    outs = [Buf((C,)) for _ in range(4)]

    def fin(geom, rows_ptr=None):
        a = [rows_ptr if rows_ptr is not None else P(src["buf"])] + geom + [None, 0, 0, 0, 0, 0, 0, 0]
        return L.lf_debug_bn_finalize_fwd(*a, C, 357.0, *[P(v) for v in vec], M32, E32, 1, *[P(o) for o in outs], stream())

    def fin_bwd(geom):
        a = [P(src["buf"])] + geom + [None, 0, 0, 0, 0, 0, 0, 0]
        return L.lf_debug_bn_bwd_finalize(*a, C, 357.0, P(vec[0]), P(vec[1]), *[P(o) for o in outs], 1, stream())

    bad = {"ld < nrows": [9, 8, C, 0, 0, 0, 0], "ld % 4 != 0": [6, 7, C, 0, 0, 0, 0],
           "centred rows, nrows % seg_rows != 0": [6, 8, C, 0, 256, 4, 1000]}
    for what, geom in bad.items():
        assert fin(geom) == -1 and L.lf_last_error(), what
        assert fin_bwd(geom) == -1, what
    assert fin([6, 8, C, 0, 0, 0, 0], ctypes.c_void_p(src["buf"].t.data_ptr() + 4)) == -1, "misaligned rows pointer"
    x, w, b = Buf((1, 2, 2, 16)), Buf((16, 9, 2, 2)), Buf((9,))
    out = Buf((1, 9, 4, 4))
    assert L.lf_debug_head_fwd(P(x), P(w), P(b), P(out), 1, 2, 2, 9, 0, stream()) == -1, "K = 9"
    assert L.lf_debug_head_bwd_data(P(out), P(w), P(x), 1, 2, 2, 9, 0, stream()) == -1, "K = 9"
    px, cat, gx = Buf((1, 3, 4, 16)), Buf((1, 1, 2, 16)), Buf((1, 3, 4, 16))
    assert L.lf_debug_pool_bwd(P(px), P(cat), 1, 3, 4, 16, 16, 0, P(gx), 0, stream()) == -1, "odd H"
    assert L.lf_debug_pool_concat_fwd(P(px), 1, 3, 4, 16, P(cat), 16, 0, None, 0, 0, stream()) == -1, "odd H"
    img, sw, sb = Buf((1, 3, 3, 4)), Buf((13, 3, 3, 3)), Buf((13,))
    assert L.lf_debug_stem_fwd(P(img), 1, 3, 3, 4, P(sw), P(sb), None, None, P(cat), None, 0, 0, stream()) == -1, "odd H"
    torch.cuda.synchronize()
    for v in outs + [out, x, cat, gx]:
        v.check()
    assert fin([6, 8, C, 0, 0, 0, 0]) == 0                                   # the same call with a good geometry runs
    torch.cuda.synchronize()
    for o in outs:
        o.check(True)
