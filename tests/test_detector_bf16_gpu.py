"""``model.detector()`` in precision mode ``bf16`` with the thin bf16 tap-GEMM route (tapgemm_bf16_thin_kernel, csrc/lf_conv_bf16.hip)
against ``model.detect`` / ``model.segment``: every element of the results bit for bit for ``thin`` True, False and "auto", both
trees, the ``--clas`` heads and segmentation-mode models; the two thin launch counters (the bf16 one moves under ``thin=True`` only,
the fp32 one never, ``fp32x9`` moves neither); ``refresh()``.  Models, frames and comparisons are tests/test_detector_gpu.py's."""
import pytest
import torch

from test_detector_gpu import check, frames, make, same

pytestmark = pytest.mark.gpu

THIN = (True, False, "auto")


def counters():
    from lanedetection_end2end_amd import _lib
    lib = _lib.load()
    return lib.lf_debug_thin_bf16_launches(), lib.lf_debug_thin_launches()


@pytest.mark.parametrize("N", [1, 2, 3])
@pytest.mark.parametrize("tree", ["bev", "bp"])
def test_equals_detect(tree, N):
    model = make(tree, N, precision="bf16")
    x = frames(N, 64)
    _, f0 = counters()
    for thin in THIN:
        det = model.detector(batch=N, thin=thin)
        assert det.precision == "bf16"
        h0, _ = counters()
        got = check(model, det, x)
        h1, f1 = counters()
        assert all(torch.isfinite(t).all() for t in got[:2])
        if thin is True:
            assert h1 > h0
        if thin is False:
            assert h1 == h0
        assert f1 == f0


def test_clas_heads_at_256x512():
    """--clas: ``line`` and ``horizon`` come from the encoder output inside the detector's workspace, behind thin launches"""
    model = make("bp", 1, R=256, precision="bf16", clas=True)
    x = frames(1, 256, seed=71)
    for thin in THIN:
        got = check(model, model.detector(thin=thin), x)
        assert got[4].shape == (1, 4) and got[5].shape == (1, 256)


@pytest.mark.parametrize("tree, N", [("bev", 2), ("bp", 1)])
def test_segmentation_mode_equals_detect_and_segment(tree, N):
    model = make(tree, N, precision="bf16", end_to_end=False)
    x = frames(N, 64)
    want = model.segment(x)
    wst = model.last_status.clone()
    for thin in THIN:
        det = model.detector(batch=N, thin=thin)
        h0, f0 = counters()
        check(model, det, x)
        got = det.segment(x)
        assert got.dtype == torch.uint8 and got.shape == (N, 64, 128) and torch.equal(got, want)
        assert torch.equal(det.last_status, wst) and torch.equal(model.last_status, wst)
        h1, f1 = counters()
        assert (h1 > h0 if thin is True else h1 == h0 if thin is False else True) and f1 == f0


def test_counters():
    model = make("bev", 1, precision="bf16")
    x = frames(1, 64)
    on, off = model.detector(thin=True), model.detector(thin=False)
    h0, f0 = counters()
    first = on(x)
    h1, _ = counters()
    assert h1 > h0
    same(on(x), first)
    h2, _ = counters()
    assert h2 - h1 == h1 - h0           # the same launches every call
    off(x)
    model.detect(x)
    assert counters() == (h2, f0)
    split = make("bev", 1, precision="fp32x9").detector(thin=True)
    split(x)
    assert counters() == (h2, f0)
    # ... and an fp32 detector moves its own counter only
    make("bev", 1).detector(thin=True)(x)
    h3, f3 = counters()
    assert h3 == h2 and f3 > f0


def test_refresh():
    model = make("bev", 1, precision="bf16")
    x = frames(1, 64)
    det = model.detector(thin=True)
    before = check(model, det, x)
    with torch.no_grad():
        block = model.net.encoder.layers[3]
        block.conv1x3_1.weight[3, 5, 0, 1] += 0.25
        block.bn1.running_mean[7] += 0.5
        block.bn2.running_var[2] *= 1.5
    det.refresh()
    h0, _ = counters()
    after = check(model, det, x)
    assert counters()[0] > h0
    assert not torch.equal(after[0], before[0])
