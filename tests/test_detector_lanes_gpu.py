"""The frozen detector with ``--clas`` heads (lsq.LaneDetector): ``det(frame)`` equals ``model.detect(frame)`` bit for bit and folds
nothing per call -- the heads' conv trunks are frozen too (lf_convchain_infer_fold / _folded) --, and ``det.lanes(frame)`` (the backbone
call, the two trunks, lf_clas_tail) equals the composed path: ``det(frame)``, then ``clas.horizon_row`` / ``clas.line_flags`` /
``Projections.decode_lanes`` as ``bp/test.py::test_model`` issues them.  Same logits bits, flags, rows and int32 lanes.

The fused tail sums the horizon's sigmoids in fp64 (tests/test_clas_tail_gpu.py): every comparison ASSERTS on the composed path's
logits that every line logit has |z| >= 1e-4 and every t = (p * 2.5 + 80) / 10 has |frac(t) - 0.5| >= 0.01.
"""
from types import SimpleNamespace

import pytest
import torch

from test_clas_tail_gpu import T_MARGIN, Z_MARGIN, margins
from test_detector_gpu import frames, make, same

pytestmark = pytest.mark.gpu

R = 256
CASES = [("fp32", 1), ("fp32", 2), ("bf16", 1), ("bf16", 2), ("fp32x9", 1)]
_models = {}


def model_for(precision, N):
    """one model per (precision, batch) for the whole file; tests that change it change it back"""
    if (precision, N) not in _models:
        _models[(precision, N)] = make("bp", N, R=R, precision=precision, clas=True)
    return _models[(precision, N)]


def composed(model, six):
    """the tail of test_model on det(frame)'s / detect(frame)'s 6-tuple"""
    from lanedetection_end2end_amd import clas
    betas, line, horizon = six[:4], six[4], six[5]
    z, t = margins(line, horizon)
    print("composed path: min|z| %.3g, min|frac(t) - 0.5| %.3g" % (z, t))
    assert z >= Z_MARGIN and t >= T_MARGIN, "the frame sits on a rounding edge of the flags / the horizon row: choose another seed"
    flags, row = clas.line_flags(line), clas.horizon_row(horizon)
    proj = clas.Projections(SimpleNamespace(resize=model.resize, order=model.order))
    _, lanes = proj.decode_lanes(betas, flags, row)
    return flags, row, lanes


def check_lanes(model, det, x):
    want = model.detect(x)
    wst = model.last_status.clone()
    flags, row, lanes = composed(model, want)
    model.last_status = None
    got = det.lanes(x)
    assert got._fields == ("lanes", "betas", "line", "horizon", "line_flags", "horizon_row")
    same(tuple(got.betas) + (got.line, got.horizon), want)
    assert torch.equal(model.last_status, wst) and torch.equal(det.last_status, wst)
    N, L = x.shape[0], model.nclasses
    assert got.lanes.dtype == torch.int32 and got.lanes.shape == (N, L, 56) and torch.equal(got.lanes, lanes)
    assert got.line_flags.dtype == torch.float32 and torch.equal(got.line_flags, flags)
    assert got.horizon_row.dtype == torch.int32 and torch.equal(got.horizon_row, row)
    return got


@pytest.mark.parametrize("precision,N", CASES)
def test_call_equals_detect_and_folds_nothing(precision, N):
    from lanedetection_end2end_amd import _lib
    lib = _lib.load()
    model = model_for(precision, N)
    x = frames(N, R, seed=71)
    f0 = lib.lf_debug_fold_pack_launches()
    det = model.detector(batch=N, thin=True)
    assert lib.lf_debug_fold_pack_launches() == f0 + 3          # the backbone and the two heads, once each
    want = model.detect(x)
    wst = model.last_status.clone()
    f1 = lib.lf_debug_fold_pack_launches()
    for _ in range(10):
        got = det(x)
    assert lib.lf_debug_fold_pack_launches() == f1              # (the code before the heads were frozen folded twice per call)
    same(got, want)
    assert torch.equal(det.last_status, wst)
    assert got[4].shape == (N, 4) and got[5].shape == (N, R)
    det.frozen_heads = False                                    # the un-frozen heads: the same bits, two folds per call
    same(det(x), want)
    assert lib.lf_debug_fold_pack_launches() == f1 + 2


def test_heads_take_the_thin_route():
    from lanedetection_end2end_amd import _lib
    lib = _lib.load()
    x = frames(1, R, seed=71)
    for precision, counter in (("fp32", lib.lf_debug_thin_launches), ("bf16", lib.lf_debug_thin_bf16_launches)):
        model = model_for(precision, 1)
        on, off = model.detector(thin=True), model.detector(thin=False)
        on.frozen_heads = False
        c0 = counter()
        on(x)
        backbone_only = counter() - c0
        on.frozen_heads = True
        c0 = counter()
        on(x)
        assert counter() - c0 > backbone_only
        c0 = counter()
        off(x)
        assert counter() == c0
        same(on(x), off(x))
        # "auto": the heads by their own constants (one frame is within both), the same bits
        auto = model.detector(thin="auto")
        c0 = counter()
        got = auto(x)
        assert counter() - c0 > backbone_only
        same(got, off(x))


def make_bev_clas():
    """test_detector_gpu.make("bev", 1, R=256, clas=True), with the BEV tree's own line head (four 3-way classifiers) in the
    state it loads"""
    from argparse import Namespace

    from lanedetection_end2end_amd.bev.Networks.LSQ_layer import Net
    from oracle import clas_oracle, erfnet_oracle
    from test_detector_gpu import nontrivial_bn
    args = Namespace(batch_size=1, nclasses=2, resize=R, end_to_end=True, mod="erfnet", layers=18, channels_in=3, pretrained=False,
                     pool=True, activation_layer="square", no_cuda=False, order=2, reg_ls=0.0, use_cholesky=False, mask_percentage=0.3,
                     clas=True, no_mapping=False, loss_policy="backproject", weight_seg=30, weight_funct="none", precision="fp32")
    model = Net(args)
    model.net.load_state_dict(erfnet_oracle.make_params(seed=5, out_channels=2))
    model.line_classification.load_state_dict(clas_oracle.make_clas_params("line", seed=11, tree="bev"))
    model.horizon_estimation.load_state_dict(clas_oracle.make_clas_params("horizon", seed=12))
    nontrivial_bn(model.net, 31)
    model = model.cuda().eval()
    model.check_singular = False
    return model


def test_bev_clas_call_equals_detect():
    model = make_bev_clas()
    x = frames(1, R, seed=71)
    det = model.detector(thin=True)
    want = model.detect(x)
    got = det(x)
    same(got, want)
    assert got[4].shape == (1, 3, 4)
    with pytest.raises(RuntimeError, match="BP tree"):
        det.lanes(x)


@pytest.mark.parametrize("precision,N", CASES)
def test_lanes_equal_composed(precision, N):
    model = model_for(precision, N)
    x = frames(N, R, seed=71)
    det = model.detector(batch=N, thin=True)
    got = check_lanes(model, det, x)
    again = det.lanes(x)
    assert torch.equal(again.lanes, got.lanes) and again.lanes.data_ptr() != got.lanes.data_ptr()
    # in place, into a slice of a larger buffer
    buf = torch.full((N + 2, model.nclasses, 56), 777, dtype=torch.int32, device="cuda")
    res = det.lanes(x, out=buf[1:N + 1])
    assert res.lanes.data_ptr() == buf[1].data_ptr() and torch.equal(buf[1:N + 1], got.lanes)
    assert bool((buf[0] == 777).all()) and bool((buf[N + 1] == 777).all())
    with pytest.raises(ValueError, match="out"):
        det.lanes(x, out=buf)
    same(det(x), model.detect(x))                                # the 6-tuple call and lanes() share the heads' workspaces


def test_refresh():
    model = model_for("fp32", 1)
    x = frames(1, R, seed=71)
    det = model.detector(thin=True)
    before = check_lanes(model, det, x)
    line, hor = model.line_classification, model.horizon_estimation
    saved = [t.detach().clone() for t in (hor.conv2.weight, line.conv3_bn.running_mean, line.fully_connected1.bias)]
    try:
        with torch.no_grad():
            hor.conv2.weight[:, :, 1, 1] *= 1.5
            line.conv3_bn.running_mean += 0.25
            line.fully_connected1.bias += 0.5
        det.refresh()
        after = check_lanes(model, det, x)
        assert not torch.equal(after.line, before.line) and not torch.equal(after.horizon, before.horizon)
    finally:
        with torch.no_grad():
            for t, s in zip((hor.conv2.weight, line.conv3_bn.running_mean, line.fully_connected1.bias), saved):
                t.copy_(s)


def test_two_detectors_interleaved():
    model = model_for("fp32", 2)
    xa, xb = frames(1, R, seed=71), frames(1, R, seed=72)
    x2 = torch.cat([xa, xb])
    one, two = model.detector(batch=1, thin=True), model.detector(batch=2, thin=False)
    a = one.lanes(xa)
    pair = two.lanes(x2)
    b = one.lanes(xb)
    assert not torch.equal(a.line, b.line)
    for u, v in ((one.lanes(xa), a), (two.lanes(x2), pair), (one.lanes(xb), b)):
        same(tuple(u.betas) + tuple(u[2:]) + (u.lanes,), tuple(v.betas) + tuple(v[2:]) + (v.lanes,))
    same((pair.line, pair.horizon), model.detect(x2)[4:])


def test_lanes_refuses_other_models():
    x = frames(1, 64)
    with pytest.raises(RuntimeError, match="--clas"):
        make("bp", 1).detector().lanes(x)
    with pytest.raises(RuntimeError, match="segmentation-mode"):
        make("bp", 1, end_to_end=False).detector().lanes(x)
    # (a BEV --clas model: test_bev_clas_call_equals_detect)
