"""``lf_clas_tail`` -- pooling, the fully connected layers of both --clas heads, the line-type flags, the horizon row and the lane
decoding of one frame in three launches -- against the composition of the existing pieces: ``lf_poolflat_*`` (``clas._PoolFlatFn``),
``ops.linear``, ``clas.horizon_row``, ``clas.line_flags`` and ``Projections.decode_lanes`` (``lf_lane_decode`` with test_model's gates).
Logits, flags, rows and lanes are compared bit for bit.

The fused tail sums the horizon's sigmoids in fp64, torch in fp32: a fp32 sum of <= 256 sigmoids is off by at most about 4e-3 in p,
1e-3 in t = (p * 2.5 + 80) / 10, and the flags are round(sigmoid(z)).  So every case ASSERTS, on the composed path's own logits, that
every line logit has |z| >= 1e-4 and every t has |frac(t) - 0.5| >= 0.01; the seeds below were chosen with the CPU model of this
file (``inputs`` + ``cpu_logits``: the same operands through torch's CPU operators) so that both hold with room -- the smallest
values it gave over all random cases: |z| 0.035, |frac(t) - 0.5| 0.063.
"""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle.gen_golden_clas import decode_inputs

S = 56
Z_MARGIN, T_MARGIN = 1e-4, 0.01
# (N, H, W, C, O1, R, L, order)
SHAPES = {
    "one_pooled_pixel": (1, 2, 2, 16, 8, 5, 2, 0),
    "scalar_gemv": (3, 2, 6, 5, 7, 9, 4, 3),               # K = 15 and 10: not multiples of 4
    "nine_rows": (9, 4, 4, 16, 8, 12, 4, 2),               # crosses the 8-rows-per-workgroup edge
    "product": (1, 32, 64, 64, 128, 256, 4, 3),
}
SEEDS = {"one_pooled_pixel": 1, "scalar_gemv": 2, "nine_rows": 19, "product": 2}


def inputs(shape, seed, bf16=False):
    """CPU operands of one case: post-ReLU trunk outputs, the three Linear layers, plausible BP-space lane polynomials."""
    N, H, W, C, O1, R, L, order = shape
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    K1, K2 = C * (H // 2) * (W // 2), C * H
    d = dict(y_line=torch.relu(rn(N, H, W, C)), y_hor=torch.relu(rn(N, H, W, C)),
             w1=rn(O1, K1) / K1 ** 0.5, b1=0.1 * rn(O1), wl=3 * rn(4, O1) / O1 ** 0.5, bl=0.5 * rn(4),
             wh=3 * rn(R, K2) / K2 ** 0.5, bh=rn(R))
    if bf16:
        d["y_line"], d["y_hor"] = d["y_line"].to(torch.bfloat16), d["y_hor"].to(torch.bfloat16)
    rng = np.random.default_rng(seed)
    beta = np.zeros((N, L, order + 1))
    beta[..., -1] = rng.uniform(60, 450, (N, L))
    if order >= 1:
        beta[..., -2] = rng.uniform(-0.6, 0.6, (N, L))
    if order >= 2:
        beta[..., -3] = rng.uniform(-2e-3, 2e-3, (N, L))
    if order >= 3:
        beta[..., -4] = rng.uniform(-4e-6, 4e-6, (N, L))
    d["beta"] = torch.from_numpy(beta)
    return d


def planted(line, rows, R, order_beta):
    """Operands that make the heads say exactly ``line`` (N, 4) flags and ``rows`` (N) horizon rows (multiples of 10 from 80 up):
    image n's trunk outputs are one-hot in channel n, fully_connected1 passes the one-hot on, the line layer reads +-5 from it, the
    horizon layer +30 for the first (row - 80) / 2.5 votes of image n and -30 for the rest."""
    N = len(rows)
    H = W = 2
    C, O1 = 16, 8
    assert N <= O1
    y = torch.zeros(N, H, W, C)
    for n in range(N):
        y[n, :, :, n] = 1
    w1 = torch.zeros(O1, C)
    w1[torch.arange(O1), torch.arange(O1)] = 1
    wl = torch.zeros(4, O1)
    wl[:, :N] = torch.from_numpy(np.asarray(line, np.float32)).t() * 10 - 5
    wh = torch.zeros(R, C * H)
    for n, row in enumerate(rows):
        votes = (int(row) - 80) * 2 // 5
        assert 0 <= votes <= R and (int(row) - 80) * 2 % 5 == 0
        wh[:votes, n * H] = 60                      # feature (channel n, row 0): the average over W = 2 of (1, 1) is 1
    return dict(y_line=y, y_hor=y.clone(), w1=w1, b1=torch.zeros(O1), wl=wl, bl=torch.zeros(4), wh=wh, bh=torch.full((R,), -30.0),
                beta=torch.from_numpy(np.asarray(order_beta, np.float64)))


def cpu_logits(d):
    """The two heads' logits through torch's CPU operators (fp32): the model the seeds were chosen with."""
    yl, yh = d["y_line"].float().permute(0, 3, 1, 2), d["y_hor"].float().permute(0, 3, 1, 2)
    fl = torch.nn.functional.max_pool2d(yl, 2, 2).flatten(1)
    fh = yh.mean(3).flatten(1)
    f1 = torch.relu(fl @ d["w1"].t() + d["b1"])
    return f1 @ d["wl"].t() + d["bl"], fh @ d["wh"].t() + d["bh"]


def margins(line, horizon):
    """(min |z| over the line logits, min |frac(t) - 0.5| over the images), from logits on any device"""
    p = torch.sigmoid(horizon.double()).sum(1)
    t = (p * 2.5 + 80) / 10
    return float(line.abs().min()), float(((t - torch.floor(t)) - 0.5).abs().min())


def test_seeds_keep_the_margins_on_the_cpu_model():
    for name, shape in SHAPES.items():
        for bf16 in ((False, True) if name == "product" else (False,)):
            for k in range(3 if name == "nine_rows" else 1):          # (the three consecutive calls use seeds s, s + 10, s + 20)
                z, t = margins(*cpu_logits(inputs(shape, SEEDS[name] + 10 * k, bf16)))
                print("%s bf16=%s seed+%d: min|z| %.3g, min|frac(t) - 0.5| %.3g" % (name, bf16, 10 * k, z, t))
                assert z >= 100 * Z_MARGIN and t >= T_MARGIN + 5e-3


# ---- the GPU side -------------------------------------------------------------------------------------------------------------
def lib():
    from lanedetection_end2end_amd import _lib
    return _lib.load()


def projections(order):
    from lanedetection_end2end_amd.clas import Projections
    return Projections(SimpleNamespace(resize=256, order=order))


def composed(d, order):
    """The existing pieces, one after the other, as Classification.forward and test_model issue them."""
    from lanedetection_end2end_amd import clas, ops
    f = clas._PoolFlatFn.apply(d["y_line"], 0)
    f = ops.linear(f, d["w1"], d["b1"], relu=True)
    line = ops.linear(f, d["wl"], d["bl"])
    horizon = ops.linear(clas._PoolFlatFn.apply(d["y_hor"], 1), d["wh"], d["bh"])
    flags, row = clas.line_flags(line), clas.horizon_row(horizon)
    L = d["beta"].shape[1]
    betas = [d["beta"][:, l, :, None] for l in range(L)]
    _, lanes = projections(order).decode_lanes(betas, flags, row)
    return line, horizon, flags, row, lanes


class Tail:
    """One workspace, reused by every call of a test."""

    def __init__(self, shape):
        N, H, W, C, O1, R, L, order = shape
        self.shape = shape
        self.nbytes = lib().lf_clas_tail_workspace_bytes(N, H, W, C, O1)
        assert self.nbytes > 0
        self.ws = torch.full((self.nbytes,), 0xFF, dtype=torch.uint8, device="cuda")
        self.proj = projections(order)
        self.y_eval, self.y_prime = self.proj._device_consts(torch.device("cuda", torch.cuda.current_device()))

    def __call__(self, d, out=None):
        N, H, W, C, O1, R, L, order = self.shape
        line = torch.full((N, 4), float("nan"), device="cuda")
        horizon = torch.full((N, R), float("nan"), device="cuda")
        flags = torch.full((N, 4), float("nan"), device="cuda")
        row = torch.full((N,), -1, dtype=torch.int32, device="cuda")
        lanes = torch.full((N, L, S), -1, dtype=torch.int32, device="cuda") if out is None else out
        assert lanes.is_contiguous() and tuple(lanes.shape) == (N, L, S)
        P = lambda t: ctypes.c_void_p(t.data_ptr())
        for k in ("y_line", "y_hor", "w1", "b1", "wl", "bl", "wh", "bh", "beta"):
            assert d[k].is_cuda and d[k].is_contiguous(), k
        rc = lib().lf_clas_tail(P(d["y_line"]), P(d["y_hor"]), int(d["y_line"].dtype == torch.bfloat16), N, H, W, C, P(d["w1"]), P(d["b1"]),
                                O1, P(d["wl"]), P(d["bl"]), P(d["wh"]), P(d["bh"]), R, P(d["beta"]), L, order, P(self.y_eval),
                                P(self.y_prime), S, self.proj._minv, 2.5, 0.0, 1279.0, -2.0, P(line), P(horizon), P(flags), P(row),
                                P(lanes), P(self.ws), self.nbytes, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, lib().lf_last_error().decode()
        return line, horizon, flags, row, lanes


def on_gpu(d):
    return {k: v.cuda().contiguous() for k, v in d.items()}


def compare(got, want, what=""):
    names = ("line", "horizon", "line_flags", "horizon_row", "lanes")
    z, t = margins(want[0], want[1])
    print("%s: composed path min|z| %.3g, min|frac(t) - 0.5| %.3g" % (what, z, t))
    assert z >= Z_MARGIN and t >= T_MARGIN, "the case sits on a rounding edge of the flags / the horizon row: choose another seed"
    for name, g, w in zip(names, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        if g.dtype == torch.float32:
            assert torch.equal(g.view(torch.int32), w.view(torch.int32)), "%s %s" % (what, name)
        else:
            assert torch.equal(g, w), "%s %s" % (what, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SHAPES))
def test_tail_equals_composed(name):
    shape = SHAPES[name]
    d = on_gpu(inputs(shape, SEEDS[name]))
    compare(Tail(shape)(d), composed(d, shape[7]), name)


@pytest.mark.gpu
def test_product_shape_bf16_trunk_outputs():
    shape = SHAPES["product"]
    d = on_gpu(inputs(shape, SEEDS["product"], bf16=True))
    assert d["y_line"].dtype == torch.bfloat16
    compare(Tail(shape)(d), composed(d, shape[7]), "product bf16")


@pytest.mark.gpu
def test_three_calls_on_one_workspace():
    """nothing in the workspace carries over from one call to the next"""
    shape = SHAPES["nine_rows"]
    tail = Tail(shape)
    for k in range(3):
        d = on_gpu(inputs(shape, SEEDS["nine_rows"] + 10 * k))
        compare(tail(d), composed(d, shape[7]), "call %d" % k)


@pytest.fixture(scope="module")
def golden_clas():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clas.npz"))


@pytest.mark.gpu
@pytest.mark.parametrize("order", [1, 2, 3])
def test_planted_heads_give_the_golden_lanes(golden_clas, order):
    """decode_inputs' betas, with its flags and horizon rows planted in the heads' weights -> the reference's rounded lanes"""
    beta, line, horizon = decode_inputs(order)
    N, L, _ = beta.shape
    R = 128
    d = on_gpu(planted(line, horizon, R, beta))
    shape = (N, 2, 2, 16, 8, R, L, order)
    got = Tail(shape)(d)
    compare(got, composed(d, order), "planted order %d" % order)
    assert torch.equal(got[2].cpu(), torch.from_numpy(line)) and torch.equal(got[3].cpu(), torch.from_numpy(horizon))
    assert (got[4].cpu().numpy() == golden_clas["decode_int_o%d" % order]).all()


@pytest.mark.gpu
def test_gates_and_out_slice():
    """a lane with flag 0; a horizon bound >= 56 (everything above the horizon); a row below 160 (a negative bound: python's slice
    [:bound] counts from the end); and the lanes written into a slice of a larger buffer whose neighbours stay untouched"""
    order, R = 2, 256
    beta, _, _ = decode_inputs(order, N=4, L=4)
    line = np.ones((4, 4), np.float32)
    line[0, 0] = 0                                       # flag 0 of the dataset's order gates lane 2 (lane l reads flag [1, 2, 0, 3][l])
    rows = np.array([200, 720, 150, 80], np.int32)       # bounds 4, 56, trunc(-1) = -1 -> the first 55, trunc(-8) = -8 -> the first 48
    d = on_gpu(planted(line, rows, R, beta))
    shape = (4, 2, 2, 16, 8, R, 4, order)
    buf = torch.full((6, 4, S), 777, dtype=torch.int32, device="cuda")
    got = Tail(shape)(d, out=buf[1:5])
    want = composed(d, order)
    compare(got, want, "gates")
    assert got[4].data_ptr() == buf[1].data_ptr()
    assert bool((buf[0] == 777).all()) and bool((buf[5] == 777).all())
    lanes = buf[1:5].cpu()
    assert torch.equal(got[3].cpu(), torch.from_numpy(rows))
    assert bool((lanes[0, 2] == -2).all()) and bool((lanes[0, 0, :4] == -2).all()) and bool((lanes[0, 0, 4:] != -2).any())
    assert bool((lanes[1] == -2).all())
    assert bool((lanes[2, :, :55] == -2).all()) and bool((lanes[3, :, :48] == -2).all())
    free = projections(order).decode_lanes([d["beta"][:, l, :, None] for l in range(4)])[1].cpu()      # no gate but the frame's
    assert torch.equal(lanes[2, :, 55], free[2, :, 55]) and torch.equal(lanes[3, :, 48:], free[3, :, 48:])


@pytest.mark.gpu
def test_argument_checks():
    shape = SHAPES["one_pooled_pixel"]
    d = on_gpu(inputs(shape, 1))
    tail = Tail(shape)
    tail.nbytes -= 1
    with pytest.raises(AssertionError, match="too small"):
        tail(d)
    assert lib().lf_clas_tail_workspace_bytes(1, 3, 1, 16, 8) == 0
