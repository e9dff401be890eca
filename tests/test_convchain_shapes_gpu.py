"""The --clas conv chain (csrc/lf_convchain.hip, lf_convchain_* of include/lanefit.h) off its one product shape, through the C ABI:
the 9-tap, stride-1, 3x3 form of the tap-GEMM family and its 1x1 form at ragged widths, partial tiles, waves that straddle images,
H = 1 and H = 2, the reduced-width kernels (16 / 48 channels) and every weight-gradient tile the launcher has; lf_poolflat_* off 32x64.

Reference: tests/convchain_ref.py in fp64 (checked by tests/test_convchain_ref_cpu.py).  Every block is compared TEACHER-FORCED: block
i's reference reads relu(z * sc + sh) of the engine's own stored z_{i-1} and fp32 vectors, the backward is the straight-through one
at the engine's state, so no ReLU decision is compared across precisions and no element is excluded.

Memory: the workspaces are filled with NaN bit patterns before every call, every output is NaN-filled and followed by a guard band of
GUARD elements of -12345; after the call the outputs are finite and the guard bands intact.

Gates.  fp32 tensors (mode 0): the project's metric e = max|got - ref| / max|ref| per tensor, bound max(2e-6, 4 * e32), e32 = the same
metric of torch's fp32 CPU operators on the same operands (convchain_ref with dtype = float32) -- computed here, never taken from the
engine.  bf16 tensors (mode 2): relative L2 < 2^-7 forward, infer and eval-mode backward; 2^-5 train-mode backward, the last BatchNorm's
gamma / beta 2^-7 (tests/test_clas_bf16_gpu.py).  y against relu(z * sc + sh) of the stored values: tests/test_eltwise_gpu.py's
bn_act bound, 4 u (|z sc| + |sh|) per element (bf16: 2^-8 (|ref| + B) + B).
BatchNorm vectors and running statistics, per element: test_eltwise_gpu's finalise gate 2 u S (fp64 arithmetic, one rounding) plus what
the statistics ROWS may carry into it, propagated through the formulas: a row sums at most 256 pixels in fp32, (256 + 8) u sum|term|
(test_eltwise_gpu's bound for partial rows, terms on absolute operands), so d mean = 264 u E|z| and d var = 264 u (E(|z| + |mean|)^2
+ 2 E(|z| + |mean|) |z|) <= 3 * 264 u E(|z| + |mean|)^2 (the centred M2 terms, and the rows' means entering the between-rows term); in
mode 2 the sums are of the fp32 values BEFORE the bf16 store (include/lanefit.h), 2^-9 relative away from the stored z they are
compared with: d mean += 2^-9 E|z|, d var += 2^-8 E(|z| + |mean|) |z|.  rstd moves by at most rstd(var - d var) - rstd(var) (clamped
at var = 0, as the kernel clamps).  A channel whose variance over 32 pixels is tiny gets a wide bound by this propagation and a tight one
otherwise: no case is widened by hand.  In eval mode the vectors come from the running statistics alone: 2 u S.
A conv bias in front of a train-mode BatchNorm has gradient zero: |gb| < 1e-5 ||gw|| in mode 0 (tests/test_clas_gpu.py); in mode 2 the
masked gradient and d loss / d z are each stored as bf16, 2^-9 relative, all of one sign at worst, and |gamma rstd gm| is within a
factor of two of |gz| summed over a channel: |gb_c| <= 2^-7 sum_pixels |gz_ref| + 1e-5 ||gw||.

Operands come from torch.Generator().manual_seed(SEED + case index) on the CPU, SEED = 4100: the first seed tried; the fp64-versus-fp32-CPU
baseline e32 is printed for every tensor and stayed between 2.2e-8 and 1.7e-6 in every case, (2, 1, 16) in train mode included: no
quantity came out ill-conditioned.

Measured on an MI355X, the tensor closest to its bound per chain (mode 0: kernel error / e32 / bound; mode 2: relative L2 / bound):
  A  1x2x64 train block 2 bn.weight gradient    4.99e-07 / 1.83e-07 / 2.00e-06     2x1x16 eval block 0 conv.bias gradient  5.07e-03 / 7.81e-03
  B  2x1x16 train block 0 bn.weight gradient    4.19e-07 / 2.28e-07 / 2.00e-06     2x1x16 eval block 0 conv.bias gradient  5.12e-03 / 7.81e-03
  C  1x2x64 train block 1 conv.weight gradient  5.52e-07 / 3.50e-07 / 2.00e-06     2x5x80 eval block 0 conv.bias gradient  5.49e-03 / 7.81e-03
  D  2x5x80 train block 1 bn.weight gradient    4.56e-07 / 1.26e-07 / 2.00e-06     2x5x80 eval block 0 conv.bias gradient  4.34e-03 / 7.81e-03
  E  3x6x20 train z0                            1.71e-07 / 5.91e-07 / 2.36e-06     3x6x20 infer                            2.10e-03 / 7.81e-03
Worst error / bound of the per-element gates over all chains: BatchNorm vectors and running statistics 0.49 (eval mode; train mode
0.08 in mode 0, where the bound carries the rows' worst case), y from the stored values 0.25 (mode 0) and 0.995 (mode 2: half an ulp of
bf16 just above a power of two, as in test_eltwise_gpu), |gb| / limit 0.004 (mode 0) and 0.20 (mode 2).

Found by this file and fixed with it (the failing case stays: chain A, (2, 5, 80), mode 2): the LDS-ring and lean bf16 kernels walked
the 16-pixel groups past the last pixel of a partial tile on through the tensor's end, and the shared epilogue multiplied the zeroed
gradient of such a group with whatever the BN-backward operand load found there -- 0 * NaN from the workspace behind z made every
gamma gradient, and all gradients below, NaN (lf_conv_bf16.hip, groups_at).
"""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

import convchain_ref as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
B7, B5 = 2.0 ** -7, 2.0 ** -5
GUARD, FILL = 4096, -12345.0
NAN = float("nan")
M32 = float(torch.tensor(R.MOMENTUM, dtype=torch.float32))          # momentum and eps as the float arguments carry them
E32 = float(torch.tensor(R.EPS, dtype=torch.float32))
SEED = 4100

CHAINS = {
    "A": ((128, 128, 128, 64, 64), (1, 3, 3, 3)),       # the product trunk
    "B": ((16, 16, 16), (3, 3)),                        # the lean kernel's general 9-tap path; weight-gradient tiles 1x1
    "C": ((16, 48, 64, 16), (3, 3, 3)),                 # NT = 3; weight-gradient tiles 1x3, 3x4, 4x1; data gradients 48->16, 64->48, 16->64
    "D": ((64, 48, 16), (3, 1)),                        # weight-gradient tiles 4x3, 3x1
    "E": ((32, 32), (3,)),                              # forward / infer only: no weight-gradient instantiation
}
SHAPES = [(3, 6, 20), (2, 5, 80), (1, 2, 64), (2, 1, 16)]
CASES = [(c, s) for c in "ABCD" for s in SHAPES] + [("A", (1, 32, 64))]
LIMIT_CASES = [("E", (3, 6, 20)), ("B", (1, 3, 6)), ("C", (1, 3, 6))]
BITS = {torch.float32: torch.int32, torch.bfloat16: torch.int16}


def case_ids(cases):
    return ["%s-%s" % (c, "x".join(map(str, s))) for c, s in cases]


def lib():
    from lanedetection_end2end_amd import _lib
    return _lib.load()


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def ptr_array(ts):
    arr = (ctypes.c_void_p * len(ts))()
    for i, t in enumerate(ts):
        arr[i] = t.data_ptr()
    return arr


def nchw(t):
    return t.permute(0, 3, 1, 2)


def bf16(t):
    return t.to(torch.bfloat16).to(t.dtype)


def bits(t):
    return t.contiguous().view(BITS[t.dtype])


class Out:
    """An output: NaN-filled, followed by a guard band."""

    def __init__(self, shape, dtype=torch.float32):
        self.n = math.prod(shape)
        self.whole = torch.full((self.n + GUARD,), FILL, dtype=dtype, device="cuda")
        self.whole[:self.n] = NAN
        self.t = self.whole[:self.n].view(tuple(shape))
        self.band = self.whole[self.n:].clone()

    def check(self, name):
        assert bool(torch.isfinite(self.t).all()), "%s: an element was not written, or is not finite" % name
        assert torch.equal(bits(self.whole[self.n:]), bits(self.band)), "%s: the guard band was written" % name


def make_operands(chain, shape, mode, seed):
    channels, ksize = CHAINS[chain]
    N, H, W = shape
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=gen)
    ru = lambda *s: 0.5 + torch.rand(*s, generator=gen)
    x, gy = rn(N, H, W, channels[0]), rn(N, H, W, channels[-1])
    params, running = [], []
    for ci, co, k in zip(channels[:-1], channels[1:], ksize):
        params += [rn(co, ci, k, k) / math.sqrt(ci * k * k), 0.3 * rn(co), ru(co), 0.5 * rn(co)]
        running += [0.5 * rn(co), ru(co)]
    if mode == 2:      # what the bf16 matrix cores multiply, as test_trunk_bf16_against_fp64 rounds
        x, gy = bf16(x), bf16(gy)
        params = [bf16(p) if p.dim() == 4 else p for p in params]
    return dict(chain=chain, shape=shape, mode=mode, channels=channels, ksize=ksize, x=x, gy=gy, params=params, running=running)


class Engine:
    def __init__(self, case):
        L = lib()
        self.case, self.mode = case, case["mode"]
        self.channels, self.ksize, (self.N, self.H, self.W) = case["channels"], case["ksize"], case["shape"]
        self.nl = len(self.ksize)
        ch = (ctypes.c_int * len(self.channels))(*self.channels)
        ks = (ctypes.c_int * self.nl)(*self.ksize)
        self.plan = L.lf_convchain_plan_create(self.N, self.H, self.W, self.nl, ch, ks)
        assert self.plan, L.lf_last_error()
        assert L.lf_convchain_set_precision(self.plan, self.mode) == 0
        self.dt = torch.bfloat16 if self.mode == 2 else torch.float32
        self.x = case["x"].to(self.dt).cuda()
        self.gy = case["gy"].to(self.dt).cuda()
        self.params = [p.cuda() for p in case["params"]]
        self.running = [r.cuda() for r in case["running"]]
        self.ph, self.rh = ptr_array(self.params), ptr_array(self.running)
        self.pd = torch.tensor([p.data_ptr() for p in self.params], dtype=torch.int64, device="cuda")
        self.ws_bytes = L.lf_convchain_workspace_bytes(self.plan)
        assert self.ws_bytes == L.lf_convchain_workspace_bytes_for(self.plan, self.mode) and self.ws_bytes % 4 == 0
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device="cuda")
        self.iws_bytes = L.lf_convchain_infer_workspace_bytes(self.plan, self.mode)
        self.iws = torch.empty(self.iws_bytes, dtype=torch.uint8, device="cuda")

    def close(self):
        lib().lf_convchain_plan_destroy(self.plan)

    def forward(self, training):
        for r, r0 in zip(self.running, self.case["running"]):
            r.copy_(r0)
        self.ws.fill_(0xFF)            # NaN as fp32 and as bf16
        y = Out((self.N, self.H, self.W, self.channels[-1]), self.dt)
        rc = lib().lf_convchain_forward(self.plan, P(self.x), self.ph, P(self.pd), self.rh, int(training), M32, E32, P(y.t), P(self.ws),
                                        self.ws_bytes, stream())
        torch.cuda.synchronize()
        return rc, y

    def z_raw(self, i):
        """block i's stored pre-BN tensor (N,H,W,C) in its storage type, a view of the workspace"""
        off, n = lib().lf_debug_convchain_offset(self.plan, i, 0), self.N * self.H * self.W * self.channels[i + 1]
        assert off >= 0
        flat = self.ws.view(self.dt)
        k = 2 if self.mode == 2 else 1
        return flat[k * off: k * off + n].view(self.N, self.H, self.W, self.channels[i + 1])

    def vec(self, i, which):
        off = lib().lf_debug_convchain_offset(self.plan, i, which)
        assert off >= 0
        return self.ws.view(torch.float32)[off: off + self.channels[i + 1]]

    def state(self):
        """per block: dict of z (NCHW, CPU, storage type), sc, sh, asc, ash (fp32, CPU)"""
        out = []
        for i in range(self.nl):
            d = {"z": nchw(self.z_raw(i)).cpu()}
            for which, k in enumerate(("sc", "sh", "asc", "ash"), 1):
                d[k] = self.vec(i, which).cpu().clone()
            out.append(d)
        return out

    def backward(self, y, training, want_gx=True):
        grads = [Out(p.shape) for p in self.params]
        gx = Out(self.x.shape, self.dt) if want_gx else None
        rc = lib().lf_convchain_backward(self.plan, P(self.x), P(y.t), P(self.gy), self.ph, ptr_array([g.t for g in grads]),
                                         P(gx.t) if want_gx else None, int(training), P(self.ws), self.ws_bytes, stream())
        torch.cuda.synchronize()
        return rc, gx, grads

    def infer(self):
        self.iws.fill_(0xFF)
        y = Out((self.N, self.H, self.W, self.channels[-1]), self.dt)
        rc = lib().lf_convchain_infer(self.plan, P(self.x), self.ph, P(self.pd), self.rh, E32, P(y.t), P(self.iws), self.iws_bytes, stream())
        torch.cuda.synchronize()
        return rc, y


def tag(case):
    return "chain %s %s mode %d" % (case["chain"], "x".join(map(str, case["shape"])), case["mode"])


def gate(case, name, got, ref64, ref32=None, bound16=B7):
    """mode 0: max-norm metric against max(2e-6, 4 e32); mode 2: relative L2 against bound16."""
    if case["mode"] == 0:
        e, e32 = R.relmax(got, ref64), R.relmax(ref32, ref64)
        bound = max(2e-6, 4 * e32)
        print("%s %s: error %.2e, fp32 CPU baseline e32 %.2e, bound %.2e" % (tag(case), name, e, e32, bound))
    else:
        e, bound = R.rell2(got, ref64), bound16
        print("%s %s: relative L2 %.2e, bound %.2e" % (tag(case), name, e, bound))
    assert e <= bound, (tag(case), name, e, bound)


def ratio_gate(case, name, got, ref, bound):
    err = (got.double() - ref).abs()
    r = float(torch.where(bound > 0, err / bound, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, math.inf))).max())
    print("%s %s: worst error / bound = %.3f" % (tag(case), name, r))
    assert r <= 1.0, (tag(case), name, r)


def bn_bounds(z, v, gamma, beta, rmean, rvar, training, mode):
    """Per-element bounds of the BatchNorm vectors and the running statistics (module docstring); z: the stored tensor in fp64."""
    g, b, mean, rstd = gamma.double().abs(), beta.double().abs(), v["mean"], v["asc"]
    zero = torch.zeros_like(mean)
    dmean, dvar, unb = zero, zero, 1.0
    if training:
        count = z.numel() // z.shape[1]
        az, am = z.abs(), R._c(mean.abs())
        dmean = 264 * U * az.mean((0, 2, 3))
        dvar = 3 * 264 * U * ((az + am) ** 2).mean((0, 2, 3))
        if mode == 2:
            dmean = dmean + 2.0 ** -9 * az.mean((0, 2, 3))
            dvar = dvar + 2.0 ** -8 * ((az + am) * az).mean((0, 2, 3))
        unb = count / (count - 1.0) if count > 1 else 1.0
    drstd = 1.0 / torch.sqrt((v["var"] - dvar).clamp(min=0) + E32) - rstd
    dash = rstd * dmean + (mean.abs() + dmean) * drstd
    B = {"asc": 2 * U * rstd + drstd, "ash": 2 * U * (mean * rstd).abs() + dash, "sc": 2 * U * g * rstd + g * drstd,
         "sh": 2 * U * (b + (mean * rstd).abs() * g) + g * dash}
    if training:
        rm, rv = rmean.double().abs(), rvar.double().abs()
        B["rmean"] = 2 * U * ((1 - M32) * rm + M32 * mean.abs()) + M32 * dmean
        B["rvar"] = 2 * U * ((1 - M32) * rv + M32 * unb * v["var"]) + M32 * unb * dvar
    return B


def check_forward(eng, training, rc, y):
    """Finite outputs, z_i teacher-forced, BatchNorm vectors and running statistics from the stored z_i, y from the stored values.
    -> the state as convchain_ref takes it."""
    case, mode = eng.case, eng.mode
    assert rc == 0, lib().lf_last_error()
    name = "train" if training else "eval"
    y.check("y")
    st = eng.state()
    for i, d in enumerate(st):
        assert all(bool(torch.isfinite(t).all()) for t in d.values()), (tag(case), name, "block %d state" % i)
    state = [(d["z"], d["sc"], d["sh"]) for d in st]
    x = nchw(case["x"])
    z64 = R.forward_teacher(x, case["params"], state)
    z32 = R.forward_teacher(x, case["params"], state, torch.float32) if mode == 0 else [None] * eng.nl
    for i, d in enumerate(st):
        gate(case, "%s z%d" % (name, i), d["z"], z64[i], z32[i])
        gamma, beta = case["params"][4 * i + 2], case["params"][4 * i + 3]
        rmean, rvar = case["running"][2 * i], case["running"][2 * i + 1]
        v = R.bn_vectors(d["z"], gamma, beta, rmean, rvar, training, M32, E32)
        B = bn_bounds(d["z"].double(), v, gamma, beta, rmean, rvar, training, mode)
        got = dict(d, rmean=eng.running[2 * i].cpu(), rvar=eng.running[2 * i + 1].cpu())
        for k in B:
            ratio_gate(case, "%s block %d %s" % (name, i, k), got[k], v[k], B[k])
        if not training:
            assert torch.equal(got["rmean"], rmean) and torch.equal(got["rvar"], rvar), "eval mode wrote the running statistics"
    zl, sc, sh = (t.double() for t in state[-1])
    Bx = 4 * U * ((zl * R._c(sc)).abs() + R._c(sh).abs())
    ref = R.output(state)
    ratio_gate(case, "%s y from the stored z, sc, sh" % name, nchw(y.t).cpu(), ref, 2.0 ** -8 * (ref.abs() + Bx) + Bx if mode == 2 else Bx)
    return state


def check_backward(eng, training, state, y):
    case, mode = eng.case, eng.mode
    name = "train" if training else "eval"
    rc, gx, grads = eng.backward(y, training)
    assert rc == 0, lib().lf_last_error()
    gx.check("gx")
    for i, g in enumerate(grads):
        g.check("gradient %d" % i)
    x, gy = nchw(case["x"]), nchw(case["gy"])
    gx64, g64, gz64 = R.backward_straight_through(x, gy, case["params"], case["running"], state, training, E32)
    if mode == 0:
        gx32, g32, _ = R.backward_straight_through(x, gy, case["params"], case["running"], state, training, E32, torch.float32)
    else:
        gx32, g32 = None, [None] * len(g64)
    b16 = B5 if training else B7
    gate(case, "%s gx" % name, nchw(gx.t).cpu(), gx64, gx32, b16)
    kinds = ("conv.weight", "conv.bias", "bn.weight", "bn.bias")
    for i, g in enumerate(grads):
        blk, kind = divmod(i, 4)
        nm = "%s block %d %s gradient" % (name, blk, kinds[kind])
        if training and kind == 1:
            limit = 1e-5 * float(g64[i - 1].norm())
            if mode == 2:
                limit = limit + 2.0 ** -7 * gz64[blk].abs().sum((0, 2, 3))
            r = float((g.t.cpu().double().abs() / limit).max())
            print("%s %s: worst |gb| / limit = %.3f" % (tag(case), nm, r))
            assert r < 1.0, (tag(case), nm, r)
        else:
            gate(case, nm, g.t.cpu(), g64[i], g32[i], B7 if (blk == eng.nl - 1 and kind >= 2) else b16)
    # determinism, and gx = NULL leaves every other gradient bit for bit
    rc2, gx2, grads2 = eng.backward(y, training)
    rc3, _, grads3 = eng.backward(y, training, want_gx=False)
    assert rc2 == 0 and rc3 == 0, lib().lf_last_error()
    assert torch.equal(bits(gx.t), bits(gx2.t)), "gx differs between two runs"
    for i, (a, b, c) in enumerate(zip(grads, grads2, grads3)):
        c.check("gradient %d (gx = NULL)" % i)
        assert torch.equal(bits(a.t), bits(b.t)), "gradient %d differs between two runs" % i
        assert torch.equal(bits(a.t), bits(c.t)), "gradient %d differs with gx = NULL" % i


def check_infer(eng, y_eval=None):
    case, mode = eng.case, eng.mode
    rc, yi = eng.infer()
    assert rc == 0, lib().lf_last_error()
    yi.check("infer y")
    x = nchw(case["x"])
    f64 = R.folded(x, case["params"], case["running"], E32)
    f32 = R.folded(x, case["params"], case["running"], E32, torch.float32) if mode == 0 else None
    got = nchw(yi.t).cpu()
    gate(case, "infer", got, f64, f32)
    if mode == 0 and y_eval is not None:       # against forward(training = 0) of the same plan, at the same gate
        e, bound = R.relmax(got, nchw(y_eval.t).cpu()), max(2e-6, 4 * R.relmax(f32, f64))
        print("%s infer against forward(training = 0): %.2e, bound %.2e" % (tag(case), e, bound))
        assert e <= bound
    rc, yi2 = eng.infer()
    assert rc == 0 and torch.equal(bits(yi.t), bits(yi2.t)), "infer differs between two runs"
    for r, r0 in zip(eng.running, case["running"]):
        assert torch.equal(r.cpu(), r0), "infer wrote the running statistics"


def forward_twice(eng, training):
    rc, y = eng.forward(training)
    state = check_forward(eng, training, rc, y)
    zb = [bits(eng.z_raw(i)).clone() for i in range(eng.nl)]
    vb = [eng.vec(i, w).clone() for i in range(eng.nl) for w in (1, 2, 3, 4)] + [r.clone() for r in eng.running]
    rc2, y2 = eng.forward(training)
    assert rc2 == 0 and torch.equal(bits(y.t), bits(y2.t)), "y differs between two runs"
    assert all(torch.equal(a, bits(eng.z_raw(i))) for i, a in enumerate(zb)), "a stored z differs between two runs"
    vb2 = [eng.vec(i, w) for i in range(eng.nl) for w in (1, 2, 3, 4)] + eng.running
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(vb, vb2)), "a BatchNorm vector differs between two runs"
    return state, y2


@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("chain,shape", CASES, ids=case_ids(CASES))
def test_chain(chain, shape, mode):
    case = make_operands(chain, shape, mode, SEED + CASES.index((chain, shape)))
    eng = Engine(case)
    try:
        y_eval = None
        for training in (1, 0):
            state, y = forward_twice(eng, training)
            check_backward(eng, training, state, y)
            y_eval = y
        check_infer(eng, y_eval)
    finally:
        eng.close()


def test_debug_offset_refuses_out_of_range():
    case = make_operands("B", (2, 1, 16), 0, SEED)
    eng = Engine(case)
    try:
        L = lib()
        assert [L.lf_debug_convchain_offset(eng.plan, b, w) for b, w in ((-1, 0), (2, 0), (0, -1), (0, 5))] == [-1] * 4
        assert L.lf_debug_convchain_offset(None, 0, 0) == -1
        offs = [L.lf_debug_convchain_offset(eng.plan, b, w) for b in range(2) for w in range(5)]
        assert all(o >= 0 and o % 64 == 0 for o in offs) and len(set(offs)) == 10 and offs == sorted(offs)
    finally:
        eng.close()


NAN_CASES =[(c, s) for c in "AB" for s in ((3, 6, 20), (1, 2, 64))]


@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("chain,shape", NAN_CASES, ids=case_ids(NAN_CASES))
def test_nan_stays_inside_its_receptive_window(chain, shape, mode):
    """One NaN in x (eval mode: the BatchNorm vectors do not depend on the batch): every stored z_i outside the pixel's receptive window
    -- 1x1, 3x3, 5x5, 7x7 for chain A, 3x3, 5x5 for chain B, clipped to the image -- keeps the clean run's bits; in particular the next
    row's first column and the neighbouring images.  z is read, not y: a ReLU can swallow a NaN."""
    case = make_operands(chain, shape, mode, SEED + 50)
    eng = Engine(case)
    N, H, W = shape
    try:
        rc, _ = eng.forward(0)
        assert rc == 0, lib().lf_last_error()
        clean = [bits(eng.z_raw(i)).clone() for i in range(eng.nl)]
        x0 = eng.x.clone()
        for n, h, w in ((min(1, N - 1), H - 1, W - 1), (0, 0, 0)):
            eng.x.copy_(x0)
            eng.x[n, h, w, 5] = NAN
            rc, _ = eng.forward(0)
            assert rc == 0, lib().lf_last_error()
            rad = 0
            for i in range(eng.nl):
                rad += eng.ksize[i] // 2
                inside = torch.zeros(N, H, W, dtype=torch.bool, device="cuda")
                inside[n, max(h - rad, 0): h + rad + 1, max(w - rad, 0): w + rad + 1] = True
                z = eng.z_raw(i)
                same = (bits(z) == clean[i]).all(-1)
                bad = torch.nonzero(~same & ~inside)
                assert bad.numel() == 0, "%s: NaN at %s changed z%d at (n, h, w) = %s" % (tag(case), (n, h, w), i, bad[:8].tolist())
                if i == 0:
                    assert bool(torch.isnan(z[n, h, w]).all()), "the poisoned pixel itself is not NaN in z0"
        eng.x.copy_(x0)
    finally:
        eng.close()


@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("chain,shape", LIMIT_CASES, ids=case_ids(LIMIT_CASES))
def test_backward_limits_are_refused_and_the_plan_stays_usable(chain, shape, mode):
    """Channel pairs the weight gradient is not compiled for ((32, 32)) and widths that are no multiple of 4 (W = 6): forward and infer
    run and pass the forward checks, lf_convchain_backward returns < 0 with a message, and the next forward on the plan succeeds."""
    case = make_operands(chain, shape, mode, SEED + 60 + LIMIT_CASES.index((chain, shape)))
    eng = Engine(case)
    try:
        for training in (1, 0):
            state, y = forward_twice(eng, training)
            yb = bits(y.t).clone()
            rc, gx, grads = eng.backward(y, training)
            msg = lib().lf_last_error()
            assert rc < 0 and msg, (rc, msg)
            print("%s: lf_convchain_backward refused: %s" % (tag(case), msg.decode()))
            assert torch.equal(bits(gx.whole[gx.n:]), bits(gx.band)) and all(torch.equal(bits(g.whole[g.n:]), bits(g.band)) for g in grads)
            rc, y2 = eng.forward(training)
            check_forward(eng, training, rc, y2)
            assert torch.equal(bits(y2.t), yb)
        check_infer(eng, y2)
    finally:
        eng.close()


# ---- lf_poolflat_* off 32x64 --------------------------------------------------------------------------------------------------------

POOL_SHAPES = [(3, 6, 10, 16), (2, 4, 6, 48)]


def tied_input(gen, shape, dtype):
    """(N,H,W,C): every 2x2 window holds its maximum twice, at two different positions of the scan order."""
    N, H, W, C = shape
    v = torch.randn(N, H // 2, W // 2, C, 4, generator=gen).to(dtype).float()
    arg = v.argmax(-1, keepdim=True)
    other = (arg + 1 + torch.randint(0, 3, arg.shape, generator=gen)) % 4
    v.scatter_(-1, other, v.gather(-1, arg))
    v = v.view(N, H // 2, W // 2, C, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(N, H, W, C)
    return v.to(dtype)


@pytest.mark.parametrize("s16", [0, 1])
@pytest.mark.parametrize("pmode", [0, 1])
@pytest.mark.parametrize("shape", POOL_SHAPES)
def test_poolflat(shape, pmode, s16):
    L = lib()
    N, H, W, C = shape
    dt = torch.bfloat16 if s16 else torch.float32
    gen = torch.Generator().manual_seed(SEED + 70 + 2 * pmode + s16)
    y = tied_input(gen, shape, dt)
    yd = nchw(y).double().requires_grad_(True)
    ref = (F.max_pool2d(yd, 2) if pmode == 0 else F.avg_pool2d(yd, (1, W))).reshape(N, -1)
    g = torch.randn(ref.shape, generator=gen)
    (ref * g.double()).sum().backward()
    if pmode == 0:
        win = nchw(y).float().unfold(2, 2, 2).unfold(3, 2, 2).reshape(N, C, H // 2, W // 2, 4)
        assert bool(((win == win.amax(-1, keepdim=True)).sum(-1) >= 2).all()), "a window without a tie"
    yc, gc = y.cuda(), g.cuda()
    fwd, bwd = (L.lf_poolflat_bf16_fwd, L.lf_poolflat_bf16_bwd) if s16 else (L.lf_poolflat_fwd, L.lf_poolflat_bwd)
    out, gy = Out(ref.shape), Out(shape, dt)
    assert fwd(P(yc), N, H, W, C, pmode, P(out.t), stream()) == 0, L.lf_last_error()
    assert bwd(P(yc), P(gc), N, H, W, C, pmode, P(gy.t), stream()) == 0, L.lf_last_error()
    torch.cuda.synchronize()
    out.check("features")
    gy.check("gy")
    got, ggot, gref = out.t.cpu(), nchw(gy.t).cpu(), yd.grad
    if pmode == 0:          # values and gradients exact: the first maximum in scan order takes the gradient (bf16: rounded once)
        assert torch.equal(got.double(), ref.detach())
        assert torch.equal(ggot.double(), gref.float().to(dt).double())
        assert int((ggot != 0).sum()) == ref.numel()
    else:                   # W sequential fp32 additions and one division; g * (1 / W): two roundings
        Bf = (W + 2) * U * F.avg_pool2d(nchw(y).double().abs(), (1, W)).reshape(N, -1)
        r = float(((got.double() - ref.detach()).abs() / Bf).max())
        Bg = 3 * U * gref.abs()
        rg = float(((ggot.double() - gref).abs() / (2.0 ** -8 * (gref.abs() + Bg) + Bg if s16 else Bg)).max())
        print("poolflat avg %s s16=%d: worst error / bound forward %.3f, backward %.3f" % (shape, s16, r, rg))
        assert r <= 1.0 and rg <= 1.0
