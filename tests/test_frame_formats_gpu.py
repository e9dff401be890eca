"""BGR, NV12 and YUYV frames through the input pipeline and the camera detector.  ONE requirement everywhere: the result on frames in
format F is BIT-EQUAL to the same entry point on an ``rgb`` plan, fed the RGB frames tests/frame_formats_ref.py makes from them (the
Q16 definition of include/lanefit.h; chroma replicated).  No tolerance.

Kernel level (lf_pipeline_image, lf_debug_frame_stem, lf_pipeline_image_indexed), geometries (Hin, Win, crop_top, crop_h -> out):
  (180, 320, 20, 160 -> 64 x 128)   the compiled 7 / 7 taps
  (100, 130, 20,  80 -> 64 x 128)   5 / 5 taps
  ( 30,  50,  6,  24 -> 32 x  64)   up-scaling, the generic taps; the crop ends at the frame's last row (NV12: the last chroma dword
                                    of the buffer is the byte-wise tail)
  ( 98, 334, 33,  64 -> 36 x  68)   odd crop_top (the first crop row shares its chroma row with a row above the crop), ragged tiles,
                                    windows that start at odd columns: inside a chroma pair
  ( 40,  60, 10,  30 -> 12 x  20)   smaller than a tile
  (  8,   8,  0,   8 ->  2 x   2)   one stem pixel
Frames are seeded uniform bytes -- most YCbCr triples are out of gamut, so all three clamps fire at both ends (asserted) -- with
the rows above the crop AND the chroma rows that belong only to them at 255.  Frames sit in guarded allocations (nothing written),
outputs in NaN-guarded ones (everything written, nothing outside).

Detector level: ``det.camera(..., pixel_format=F, yuv=P)`` against ``det.camera(...)`` on the RGB frames, every element and
``last_status``; ``lanes`` on the BP --clas model, ``segment`` on a segmentation-mode model, ``InputPipeline(pixel_format=F)``; the
refusals."""
import ctypes

import numpy as np
import pytest
import torch

import frame_formats_ref as F
import test_eltwise_gpu as E
from test_detector_gpu import make, same
from test_frame_stem_gpu import Plan, U8Buf, fused, operands

pytestmark = pytest.mark.gpu

GEOMS = [(180, 320, 20, 160, 64, 128), (100, 130, 20, 80, 64, 128), (30, 50, 6, 24, 32, 64), (98, 334, 33, 64, 36, 68),
         (40, 60, 10, 30, 12, 20), (8, 8, 0, 8, 2, 2)]
FORMATS = ["bgr", "nv12", "yuyv"]
PRESETS = ["jfif", "bt709"]
FRAME_HW, CROP = (180, 320), 160


class FPlan(Plan):
    """test_frame_stem_gpu.Plan with a frame format"""

    def __init__(self, geom, fmt="rgb", yuv="jfif"):
        super().__init__(geom)
        if fmt != "rgb":
            coef = (ctypes.c_int * 6)(*F.PRESETS[yuv])
            assert E.lib().lf_pipeline_plan_set_format(self.h, F.FORMATS[fmt], coef) == 0, E.lib().lf_last_error()
        assert E.lib().lf_pipeline_frame_bytes(self.h) == F.frame_bytes(fmt, geom[0], geom[1])


def make_frames(seed, fmt, N, H, W, top):
    """seeded uniform bytes in format fmt (numpy); the rows above the crop, and the chroma rows only they use, at 255"""
    f = np.random.default_rng(seed).integers(0, 256, F.frames_shape(fmt, N, H, W), dtype=np.uint8)
    f[:, :top] = 255
    if fmt == "nv12":
        f[:, H:H + top // 2] = 255
    return f


def image(plan, frames, N):
    oh, ow = plan.geom[4:]
    out = E.Buf((N, 3, oh, ow))
    rc = E.lib().lf_pipeline_image(plan.h, ctypes.c_void_p(frames.t.data_ptr()), N, plan.T(), None, E.P(out), E.stream())
    assert rc == 0, E.lib().lf_last_error()
    return out


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "%dx%d+%d+%d-%dx%d" % g)
def test_kernels_equal_the_rgb_plan_on_the_converted_frames(geom, fmt, N):
    H, W, top = geom[:3]
    raw = make_frames(9000 + H + N, fmt, N, H, W, top)
    frames = U8Buf(torch.from_numpy(raw).cuda())
    gen = E.cuda_gen(9100 + H)
    ins = [E.Buf(v.shape, init=v) for v in operands(gen)]
    rgb_plan = FPlan(geom)
    for yuv in PRESETS:
        host_rgb = F.to_rgb(raw, fmt, H, W, F.PRESETS[yuv])
        if fmt != "bgr" and H * W >= 1000:
            for c in range(3):
                assert (host_rgb[..., c] == 0).any() and (host_rgb[..., c] == 255).any(), "a clamp does not fire"
        rgb = U8Buf(torch.from_numpy(host_rgb).cuda())
        plan = FPlan(geom, fmt, yuv)
        assert plan.ok == rgb_plan.ok == 1
        got, want = image(plan, frames, N), image(rgb_plan, rgb, N)
        torch.cuda.synchronize()
        got.check(True)
        want.check(True)
        assert torch.equal(got.t.view(torch.int32), want.t.view(torch.int32)), "lf_pipeline_image (%s, %s)" % (fmt, yuv)
        for s16 in (0, 1):
            rc, got = fused(plan, frames, ins, N, s16)
            rc2, want = fused(rgb_plan, rgb, ins, N, s16)
            torch.cuda.synchronize()
            assert (rc, rc2) == (0, 0), E.lib().lf_last_error()
            got.check(True)
            want.check(True)
            bits = E.BITS[E.dt(s16)]
            assert torch.equal(got.t.view(bits), want.t.view(bits)), "lf_debug_frame_stem (%s, %s, s16=%d)" % (fmt, yuv, s16)
        rgb.check()
    frames.check()
    for x in ins:
        x.check()


@pytest.mark.parametrize("fmt", FORMATS)
def test_indexed_pool_counts_and_does_not_read_an_index_outside(fmt):
    geom = GEOMS[3]
    H, W, top = geom[:3]
    oh, ow = geom[4:]
    pool_n = 5
    raw = make_frames(9200, fmt, pool_n, H, W, top)
    host_rgb = F.to_rgb(raw, fmt, H, W, F.PRESETS["bt709"])
    pool, rgb = U8Buf(torch.from_numpy(raw).cuda()), U8Buf(torch.from_numpy(host_rgb).cuda())
    sel = torch.tensor([3, 0, 7, 4, 1, -1], dtype=torch.int64, device="cuda")         # 7 and -1: outside the pool, read entry 0
    flip = torch.tensor([0, 1, 0, 0, 1, 1], dtype=torch.uint8, device="cuda")
    outs = []
    for plan, buf in ((FPlan(geom, fmt, "bt709"), pool), (FPlan(geom), rgb)):
        out = E.Buf((sel.numel(), 3, oh, ow))
        bad = torch.zeros(1, dtype=torch.int32, device="cuda")
        rc = E.lib().lf_pipeline_image_indexed(plan.h, ctypes.c_void_p(buf.t.data_ptr()), pool_n, ctypes.c_void_p(sel.data_ptr()), sel.numel(),
                                               plan.T(), ctypes.c_void_p(flip.data_ptr()), E.P(out), ctypes.c_void_p(bad.data_ptr()), E.stream())
        torch.cuda.synchronize()
        assert rc == 0, E.lib().lf_last_error()
        assert int(bad) == 2
        out.check(True)
        buf.check()
        outs.append(out.t)
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    assert torch.equal(outs[0][2], outs[0][1].flip(-1)) and not torch.equal(outs[0][0], outs[0][3])


def format_frames(fmt, yuv, N, hw=FRAME_HW, crop=CROP, seed=4):
    """(frames in fmt, the RGB frames they are) on the device"""
    raw = make_frames(seed, fmt, N, hw[0], hw[1], hw[0] - crop)
    return torch.from_numpy(raw).cuda(), torch.from_numpy(F.to_rgb(raw, fmt, hw[0], hw[1], F.PRESETS[yuv])).cuda()


@pytest.mark.parametrize("N", [1, 2])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("tree", ["bev", "bp"])
def test_camera_equals_the_rgb_camera(tree, precision, N):
    model = make(tree, N, precision=precision)
    det = model.detector(batch=N)
    ref = det.camera(frame_hw=FRAME_HW, crop=CROP)
    for fmt in FORMATS:
        for yuv in PRESETS:
            cam = det.camera(frame_hw=FRAME_HW, crop=CROP, pixel_format=fmt, yuv=yuv)
            assert cam.fits and cam.fused == "auto" and cam.pixel_format == fmt
            assert cam.frame_shape == F.frames_shape(fmt, N, *FRAME_HW)
            f, rgb = format_frames(fmt, yuv, N)
            for fused_ in (True, False, "auto"):
                ref.fused = cam.fused = fused_
                want = ref(rgb)
                wst = ref.last_status.clone()
                model.last_status = cam.last_status = None
                got = cam(f)
                assert len(got) == 6
                same(got, want)
                assert torch.equal(cam.last_status, wst) and torch.equal(model.last_status, wst)


def test_camera_takes_six_ints_and_refreshes():
    model = make("bev", 1)
    det = model.detector()
    custom = (65536, 0, 90000, 22000, 46000, 116000)
    cam = det.camera(frame_hw=FRAME_HW, crop=CROP, pixel_format="nv12", yuv=custom, fused=True)
    ref = det.camera(frame_hw=FRAME_HW, crop=CROP, fused=True)
    raw = make_frames(5, "nv12", 1, FRAME_HW[0], FRAME_HW[1], FRAME_HW[0] - CROP)
    f, rgb = torch.from_numpy(raw).cuda(), torch.from_numpy(F.to_rgb(raw, "nv12", FRAME_HW[0], FRAME_HW[1], custom)).cuda()
    before = cam(f)
    same(before, ref(rgb))
    assert not torch.equal(before[0], det.camera(frame_hw=FRAME_HW, crop=CROP, pixel_format="nv12")(f)[0])
    with torch.no_grad():
        model.net.encoder.initial_block.conv.weight[2, 1, 0, 1] += 0.25
    det.refresh()
    after = cam(f)
    assert not torch.equal(after[0], before[0])
    same(after, ref(rgb))


@pytest.mark.parametrize("fmt,precision", [("bgr", "fp32"), ("nv12", "fp32"), ("yuyv", "fp32"), ("nv12", "bf16")])
def test_lanes_on_720x1280_frames(fmt, precision):
    from oracle import pipeline_oracle as po
    model = make("bp", 1, R=256, precision=precision, clas=True)
    det = model.detector(thin=True)
    # a frame with structure, re-read as format fmt: the planes of the synthetic RGB frame stand in for B G R / Y Cb Cr
    src = po.synthetic_frame(3)[0]
    if fmt == "bgr":
        raw = src[None].copy()
    elif fmt == "nv12":
        raw = np.concatenate([src[..., 1], src[::2, ::2, [2, 0]].reshape(360, 1280)])[None]
    else:
        raw = np.stack([src[..., 1], np.where(np.arange(1280) % 2 == 0, src[..., 2], src[..., 0])], axis=-1)[None]
    raw = np.ascontiguousarray(raw)
    rgb = torch.from_numpy(F.to_rgb(raw, fmt, 720, 1280, F.PRESETS["bt709"])).cuda()
    f = torch.from_numpy(raw).cuda()
    cam, ref = det.camera(pixel_format=fmt, yuv="bt709"), det.camera()
    assert cam.fits and cam.frame_shape == F.frames_shape(fmt, 1, 720, 1280)
    for fused_ in (True, False):
        ref.fused = cam.fused = fused_
        want = ref.lanes(rgb)
        wst = ref.last_status.clone()
        got = cam.lanes(f)
        assert got._fields == want._fields
        same(tuple(got.betas) + tuple(got[2:]) + (got.lanes,), tuple(want.betas) + tuple(want[2:]) + (want.lanes,))
        assert torch.equal(cam.last_status, wst)
        same(cam(f), ref(rgb))


def test_segmentation_mode():
    N = 2
    model = make("bp", N, end_to_end=False)
    det = model.detector(batch=N, thin=True)
    ref = det.camera(frame_hw=FRAME_HW, crop=CROP)
    for fmt in FORMATS:
        cam = det.camera(frame_hw=FRAME_HW, crop=CROP, pixel_format=fmt, yuv="bt709")
        f, rgb = format_frames(fmt, "bt709", N)
        for fused_ in (True, False):
            ref.fused = cam.fused = fused_
            want = ref.segment(rgb)
            wst = ref.last_status.clone()
            got = cam.segment(f)
            assert got.dtype == torch.uint8 and got.shape == (N, 64, 128) and torch.equal(got, want)
            assert torch.equal(cam.last_status, wst)
            same(cam(f), ref(rgb))


@pytest.mark.parametrize("fmt", FORMATS)
def test_input_pipeline_image(fmt):
    from lanedetection_end2end_amd.pipeline import InputPipeline
    N = 3
    for yuv in PRESETS:
        pipe = InputPipeline(64, "bp", frame_hw=FRAME_HW, crop=CROP, pixel_format=fmt, yuv=yuv)
        ref = InputPipeline(64, "bp", frame_hw=FRAME_HW, crop=CROP)
        f, rgb = format_frames(fmt, yuv, N, seed=6)
        labels = torch.randint(0, 5, (N,) + FRAME_HW, dtype=torch.uint8, device="cuda")
        flip = torch.tensor([True, False, True])
        got, want = pipe(f, labels, flip), ref(rgb, labels, flip)
        assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32)) and torch.equal(got[1], want[1])
        assert torch.equal(pipe(f)[0].view(torch.int32), ref(rgb)[0].view(torch.int32))
        index = torch.tensor([2, 0, 0, 1], device="cuda")
        got, want = pipe(f, flip=flip[[0, 1, 1, 0]], index=index), ref(rgb, flip=flip[[0, 1, 1, 0]], index=index)
        pipe.flush()
        ref.flush()
        assert got[0].shape == (4, 3, 64, 128) and torch.equal(got[0].view(torch.int32), want[0].view(torch.int32))
        pipe(f, index=torch.tensor([0, 3], device="cuda"))
        with pytest.raises(IndexError):
            pipe.flush()


def test_refusals_launch_nothing():
    from lanedetection_end2end_amd import _lib
    from lanedetection_end2end_amd.pipeline import InputPipeline
    model = make("bev", 1)
    det = model.detector()
    for kw, match in (({"pixel_format": "i420"}, "pixel_format"), ({"pixel_format": "nv12", "yuv": "bt601"}, "yuv"),
                      ({"pixel_format": "yuyv", "yuv": (1, 2, 3, 4, 5)}, "yuv"), ({"yuv": (1, 2, 3, 4, 5, 6, 7)}, "yuv"),
                      ({"pixel_format": "nv12", "yuv": (1 << 24, 0, 1, 1, 1, 1)}, "int32")):
        with pytest.raises(ValueError, match=match):
            det.camera(frame_hw=FRAME_HW, crop=CROP, **kw)
    for hw, fmt in (((181, 320), "nv12"), ((180, 321), "nv12"), ((180, 321), "yuyv")):
        with pytest.raises(ValueError, match="even"):
            det.camera(frame_hw=hw, crop=CROP, pixel_format=fmt)
        with pytest.raises(ValueError, match="even"):
            InputPipeline(64, "bev", frame_hw=hw, crop=CROP, pixel_format=fmt)
    model.last_status = None
    for fmt in FORMATS:
        cam = det.camera(frame_hw=FRAME_HW, crop=CROP, pixel_format=fmt)
        pipe = InputPipeline(64, "bev", frame_hw=FRAME_HW, crop=CROP, pixel_format=fmt)
        f, rgb = format_frames(fmt, "jfif", 1)
        wrong = [format_frames(other, "jfif", 1)[0] for other in ("rgb", "nv12", "yuyv") if F.frames_shape(other, 1, *FRAME_HW) != tuple(f.shape)]
        wrong += [torch.cat([f, f]), f[:, :-2]]
        for w in wrong:
            with pytest.raises(ValueError, match="shape"):
                cam(w)
        for w in wrong[:-2] + [f[:, :-2]]:
            with pytest.raises(ValueError, match="shape"):
                pipe(w)
        with pytest.raises(ValueError, match="uint8"):
            cam(f.float())
        with pytest.raises(ValueError, match="uint8"):
            pipe(f.float())
        with pytest.raises(ValueError, match="contiguous"):
            cam(torch.cat([f, f], 2)[:, :, :f.shape[2]])
        with pytest.raises(_lib.LaneFitLibraryError, match="no CPU path"):
            cam(f.cpu())
        with pytest.raises(_lib.LaneFitLibraryError, match="CPU path"):
            pipe(f.cpu())
        assert cam.last_status is None and model.last_status is None, "a refused call ran the backbone"
