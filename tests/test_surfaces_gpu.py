"""Decoder surfaces through the input pipeline and the camera detector: pitched rows, planes at offsets, a frame stride, plane
pointers, and the formats I420, RGBX, BGRX.  ONE requirement everywhere, the frame formats' own: every result is BIT-EQUAL to the same
entry point on a tight plan -- for rgb, bgr, nv12 and yuyv the tight plan of the SAME format on the frames extracted from the surface
(the code path every plan ran before there were layouts), for i420, rgbx and bgrx the tight ``rgb`` plan on
``surface_ref.to_rgb(...)``.  No tolerance.  Every byte of a surface that is not a pixel is seeded-random: a padding byte that reaches
a result breaks the equality.

Kernel level (lf_pipeline_image, lf_debug_frame_stem; fp32 and bf16 storage; N in {1, 3}; all seven formats; both YUV presets for the
YCbCr ones), geometries (Hin, Win, crop_top, crop_h -> out):
  ( 98, 334, 33,  64 -> 36 x  68)   odd crop top, ragged tiles, windows that start inside a chroma pair
  ( 30,  50,  6,  24 -> 32 x  64)   the crop ends at the surface's last row: the allocation ends exactly at the span
  (  8,   8,  0,   8 ->  2 x   2)   one stem pixel
  (180, 320, 20, 160 -> 64 x 128)   the compiled 7 / 7 taps
each under the four layouts of surface_ref.kernel_layout: 1 padded pitches, odd where legal (rgb / bgr + 5; i420 Y + 3, chroma + 1;
nv12 Y + 6, CbCr + 10; yuyv / rgbx / bgrx + 12); 2 = 1 + a gap of three padded rows before each later plane; 3 = 2 + a frame stride
with a gap; 4 = plane pointers, every plane in a guarded allocation of exactly span(p) bytes, the table rows in shuffled frame order.
Surfaces sit in guarded uint8 allocations (nothing written), outputs in NaN-guarded ones (everything written, nothing outside).

Detector level: ``det.camera(layout=L)`` against ``det.camera()`` on the RGB frames, every returned tensor and ``last_status``, for
pitched nv12, i420 and rgbx, fused and two launches, contiguous and through ``bind``; ``segment``; ``InputPipeline(layout=)`` with
flips; 720 x 1280 NV12 at pitch 1536 with the chroma plane at row 736 against the tight nv12 camera; the refusals."""
import ctypes

import numpy as np
import pytest
import torch

import frame_formats_ref as F
import surface_ref as S
import test_eltwise_gpu as E
from test_detector_gpu import make, same
from test_frame_formats_gpu import FPlan
from test_frame_stem_gpu import Plan, U8Buf, fused, operands

pytestmark = pytest.mark.gpu

GEOMS = [(98, 334, 33, 64, 36, 68), (30, 50, 6, 24, 32, 64), (8, 8, 0, 8, 2, 2), (180, 320, 20, 160, 64, 128)]
FORMATS = ["rgb", "bgr", "nv12", "yuyv", "i420", "rgbx", "bgrx"]
FRAME_HW, CROP = (180, 320), 160


def c_layout(L):
    from lanedetection_end2end_amd.pipeline import _CLayout
    pad3 = lambda v: tuple(v) + (0,) * (3 - len(v))
    return _CLayout(S.FORMATS[L.fmt], int(L.pointers), (ctypes.c_long * 3)(*pad3(L.given[0])), (ctypes.c_long * 3)(*pad3(L.given[1])),
                    L.given[2])


class SPlan(Plan):
    """test_frame_stem_gpu.Plan with a frame layout (surface_ref.Layout)"""

    def __init__(self, geom, L, yuv="jfif"):
        super().__init__(geom)
        lib = E.lib()
        coef = (ctypes.c_int * 6)(*F.PRESETS[yuv])
        assert lib.lf_pipeline_plan_set_layout(self.h, ctypes.byref(c_layout(L)), coef) == 0, lib.lf_last_error()
        assert lib.lf_pipeline_frame_bytes(self.h) == L.stride and lib.lf_pipeline_surface_span(self.h, -1) == L.frame_span
        assert [lib.lf_pipeline_surface_span(self.h, p) for p in range(len(L.dims))] == L.span


def tight_frames(seed, fmt, N, H, W, top):
    """seeded uniform bytes, the rows above the crop (and the chroma rows only they use) at 255"""
    x = np.random.default_rng(seed).integers(0, 256, S.tight_shape(fmt, N, H, W), dtype=np.uint8)
    planes = S.planes_of(x, fmt, H, W)
    planes[0][:, :top] = 255
    for c in planes[1:]:
        c[:, :top // 2] = 255
    return np.concatenate([p.reshape(N, -1) for p in planes], axis=1).reshape(x.shape)


class Surface:
    """A batch under layout L on the device: the guarded batch allocation (contiguous) or one guarded allocation of exactly span(p)
    bytes per plane and the pointer table, its rows in the order ``perm`` (pointer mode)."""

    def __init__(self, tight, L, seed, perm=None):
        N = tight.shape[0]
        batch, planes = S.embed(tight, L, seed)
        self.L, self.N, self.bufs = L, N, []
        if L.pointers:
            perm = list(range(N)) if perm is None else perm
            rows = []
            for n in perm:
                bs = [U8Buf(torch.from_numpy(planes[n][p]).cuda()) for p in range(len(L.dims))]
                assert all(b.t.numel() == L.span[p] and b.t.data_ptr() % 4 == 0 for p, b in enumerate(bs))
                self.bufs += bs
                rows.append([b.t.data_ptr() for b in bs])
            self.table = torch.tensor(rows, dtype=torch.int64).cuda()
            self.ptr = ctypes.c_void_p(self.table.data_ptr())
        else:
            b = U8Buf(torch.from_numpy(batch).cuda())
            assert b.t.numel() == L.batch_bytes(N) and b.t.data_ptr() % 4 == 0
            self.bufs.append(b)
            self.ptr = ctypes.c_void_p(b.t.data_ptr())
        # fused() / image() of the other test files take an object with .t
        self.t = self

    def data_ptr(self):
        return self.ptr.value

    def check(self):
        for b in self.bufs:
            b.check()


def image(plan, frames, N):
    oh, ow = plan.geom[4:]
    out = E.Buf((N, 3, oh, ow))
    rc = E.lib().lf_pipeline_image(plan.h, ctypes.c_void_p(frames.t.data_ptr()), N, plan.T(), None, E.P(out), E.stream())
    assert rc == 0, E.lib().lf_last_error()
    return out


def oracle_for(geom, fmt, yuv, tight):
    """(plan, frames) of the tight oracle: the same format for the four existing ones, rgb on to_rgb for the new ones"""
    H, W = geom[:2]
    if fmt in F.FORMATS:
        return FPlan(geom, fmt, yuv), U8Buf(torch.from_numpy(tight).cuda())
    return FPlan(geom), U8Buf(torch.from_numpy(S.to_rgb(tight, fmt, H, W, F.PRESETS[yuv])).cuda())


def results(plan, frames, ins, N):
    """[image bits, fused fp32 bits, fused bf16 bits], every output checked for its guard"""
    outs = [image(plan, frames, N)]
    for s16 in (0, 1):
        rc, got = fused(plan, frames, ins, N, s16)
        assert rc == 0, E.lib().lf_last_error()
        outs.append(got)
    torch.cuda.synchronize()
    bits = [torch.int32, torch.int32, torch.int16]
    for o in outs:
        o.check(True)
    return [o.t.view(b).clone() for o, b in zip(outs, bits)]


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "%dx%d+%d+%d-%dx%d" % g)
def test_kernels_equal_the_tight_plan(geom, fmt, N):
    H, W, top = geom[:3]
    tight = tight_frames(9300 + H + N, fmt, N, H, W, top)
    gen = E.cuda_gen(9400 + H)
    ins = [E.Buf(v.shape, init=v) for v in operands(gen)]
    perm = [2, 0, 1][:N] if N == 3 else [0]
    for yuv in (("jfif", "bt709") if fmt in S.YCC else ("jfif",)):
        oplan, oframes = oracle_for(geom, fmt, yuv, tight)
        assert oplan.ok == 1
        want = results(oplan, oframes, ins, N)
        oframes.check()
        for kind in (1, 2, 3, 4):
            L = S.kernel_layout(fmt, H, W, kind)
            surf = Surface(tight, L, 70 + kind, perm if kind == 4 else None)
            if kind != 4:
                assert np.array_equal(S.extract(surf.bufs[0].t.cpu().numpy(), L, N), tight)
            plan = SPlan(geom, L, yuv)
            assert plan.ok == 1
            got = results(plan, surf, ins, N)
            surf.check()
            order = torch.tensor(perm if kind == 4 else list(range(N)), device="cuda")
            for what, g, w in zip(("lf_pipeline_image", "lf_debug_frame_stem fp32", "lf_debug_frame_stem bf16"), got, want):
                assert torch.equal(g, w[order]), "%s (%s, %s, layout %d)" % (what, fmt, yuv, kind)
    for x in ins:
        x.check()


def test_yv12_is_i420_with_the_chroma_pointers_exchanged():
    geom = GEOMS[0]
    H, W, top = geom[:3]
    N = 2
    tight = tight_frames(9500, "i420", N, H, W, top)
    gen = E.cuda_gen(9501)
    ins = [E.Buf(v.shape, init=v) for v in operands(gen)]
    L = S.kernel_layout("i420", H, W, 4)
    surf = Surface(tight, L, 3)
    surf.table = surf.table[:, [0, 2, 1]].contiguous()
    surf.ptr = ctypes.c_void_p(surf.table.data_ptr())
    got = results(SPlan(geom, L, "bt709"), surf, ins, N)
    surf.check()
    oplan, oframes = oracle_for(geom, "i420", "bt709", S.swap_chroma(tight, H, W))
    want = results(oplan, oframes, ins, N)
    same_order = results(oplan, U8Buf(torch.from_numpy(S.to_rgb(tight, "i420", H, W, F.PRESETS["bt709"])).cuda()), ins, N)
    for g, w, s in zip(got, want, same_order):
        assert torch.equal(g, w) and not torch.equal(g, s)
    # ... and through the offsets of a contiguous frame: planes 1 and 2 exchanged
    c = S.Layout("i420", H, W)
    yv = S.Layout("i420", H, W, offsets=(0, c.offsets[2], c.offsets[1]))
    buf = U8Buf(torch.from_numpy(np.ascontiguousarray(tight)).cuda())
    got = results(SPlan(geom, yv, "bt709"), buf, ins, N)
    buf.check()
    for g, w in zip(got, want):
        assert torch.equal(g, w)


def test_nv12_chroma_pointer_aligned_to_two_bytes_only():
    """The contract lets the NV12 CbCr pointer be 2-byte aligned: the staging then loads the aligned dword 2 bytes in front of the plane
    (csrc/lf_pipeline_dev.h, Bounds).  Every chroma plane sits at + 2 of a guarded allocation whose first two bytes are seeded-random:
    the same bits as the tight plan, nothing written."""
    geom = GEOMS[0]
    H, W, top = geom[:3]
    N = 3
    tight = tight_frames(9550, "nv12", N, H, W, top)
    gen = E.cuda_gen(9551)
    ins = [E.Buf(v.shape, init=v) for v in operands(gen)]
    L = S.kernel_layout("nv12", H, W, 4)
    _, planes = S.embed(tight, L, 8)
    front = np.random.default_rng(9).integers(0, 256, 2, dtype=np.uint8)
    bufs, rows = [], []
    for n in range(N):
        y = U8Buf(torch.from_numpy(planes[n][0]).cuda())
        c = U8Buf(torch.from_numpy(np.concatenate([front, planes[n][1]])).cuda())
        bufs += [y, c]
        rows.append([y.t.data_ptr(), c.t.data_ptr() + 2])
        assert rows[-1][1] % 4 == 2
    surf = Surface(tight, L, 8)
    surf.bufs, surf.table = bufs, torch.tensor(rows, dtype=torch.int64).cuda()
    surf.ptr = ctypes.c_void_p(surf.table.data_ptr())
    for yuv in ("jfif", "bt709"):
        oplan, oframes = oracle_for(geom, "nv12", yuv, tight)
        want = results(oplan, oframes, ins, N)
        got = results(SPlan(geom, L, yuv), surf, ins, N)
        surf.check()
        for g, w in zip(got, want):
            assert torch.equal(g, w)


def test_indexed_pool_on_a_strided_nv12_pool():
    geom = GEOMS[0]
    H, W, top = geom[:3]
    oh, ow = geom[4:]
    pool_n = 5
    tight = tight_frames(9600, "nv12", pool_n, H, W, top)
    L = S.kernel_layout("nv12", H, W, 3)
    surf = Surface(tight, L, 9)
    ref = U8Buf(torch.from_numpy(tight).cuda())
    sel = torch.tensor([3, 0, 7, 4, 1, -1], dtype=torch.int64, device="cuda")         # 7 and -1: outside the pool, read entry 0
    flip = torch.tensor([0, 1, 0, 0, 1, 1], dtype=torch.uint8, device="cuda")
    outs = []
    for plan, buf in ((SPlan(geom, L, "bt709"), surf), (FPlan(geom, "nv12", "bt709"), ref)):
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


def test_indexed_call_on_a_pointer_plan_is_refused():
    geom = GEOMS[0]
    H, W, top = geom[:3]
    L = S.kernel_layout("nv12", H, W, 4)
    surf = Surface(tight_frames(9700, "nv12", 2, H, W, top), L, 1)
    plan = SPlan(geom, L)
    sel = torch.tensor([1, 0], dtype=torch.int64, device="cuda")
    out = E.Buf((2, 3) + geom[4:])
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    rc = E.lib().lf_pipeline_image_indexed(plan.h, surf.ptr, 2, ctypes.c_void_p(sel.data_ptr()), 2, plan.T(), None, E.P(out),
                                           ctypes.c_void_p(bad.data_ptr()), E.stream())
    torch.cuda.synchronize()
    assert rc != 0 and b"contiguous pools only" in E.lib().lf_last_error()
    out.check()
    surf.check()
    assert int(bad) == 0


# ---- detector level -------------------------------------------------------------------------------------------------------------
def frame_layouts(plane_pointers=False):
    from lanedetection_end2end_amd.pipeline import FrameLayout
    H, W = FRAME_HW
    return [FrameLayout("nv12", FRAME_HW, pitch=(384, 384), plane_offsets=None if plane_pointers else (0, 184 * 384), plane_pointers=plane_pointers),
            FrameLayout("i420", FRAME_HW, pitch=(W + 3, W // 2 + 1, W // 2 + 3), plane_pointers=plane_pointers),
            FrameLayout("rgbx", FRAME_HW, pitch=4 * W + 64, frame_stride=0 if plane_pointers else (4 * W + 64) * (H + 2), plane_pointers=plane_pointers)]


def ref_layout(lay):
    return S.Layout(lay.pixel_format, lay.frame_hw[0], lay.frame_hw[1], lay._given[0], lay._given[1], lay._given[2], lay.plane_pointers)


def surface_and_rgb(lay, yuv, N, seed=4):
    """(contiguous surface tensor, per-frame plane tensors, the RGB frames they are), on the device"""
    H, W = lay.frame_hw
    tight = tight_frames(seed, lay.pixel_format, N, H, W, H - CROP if (H, W) == FRAME_HW else 80)
    batch, planes = S.embed(tight, ref_layout(lay), seed + 1)
    rgb = torch.from_numpy(S.to_rgb(tight, lay.pixel_format, H, W, F.PRESETS[yuv])).cuda()
    return torch.from_numpy(batch).cuda(), [tuple(torch.from_numpy(p).cuda() for p in fr) for fr in planes], rgb


@pytest.mark.parametrize("N", [1, 2])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("tree", ["bev", "bp"])
def test_camera_equals_the_rgb_camera(tree, precision, N):
    model = make(tree, N, precision=precision)
    det = model.detector(batch=N)
    ref = det.camera(frame_hw=FRAME_HW, crop=CROP)
    for pointers in (False, True):
        for lay in frame_layouts(pointers):
            cam = det.camera(frame_hw=FRAME_HW, crop=CROP, layout=lay, yuv="bt709")
            assert cam.fits and cam.fused == "auto" and cam.pixel_format == lay.pixel_format and cam.frame_shape is None
            batch, planes, rgb = surface_and_rgb(lay, "bt709", N)
            arg = cam.bind(planes) if pointers else batch
            if pointers:
                assert arg.pointers.shape == (N, lay.planes) and arg.pointers.dtype == torch.int64 and arg.pointers.is_cuda
            for fused_ in (True, False):
                ref.fused = cam.fused = fused_
                want = ref(rgb)
                wst = ref.last_status.clone()
                model.last_status = cam.last_status = None
                got = cam(arg)
                assert len(got) == 6
                same(got, want)
                assert torch.equal(cam.last_status, wst) and torch.equal(model.last_status, wst)
            if not pointers:                                   # a decoder's buffer may be larger, and of any shape
                bigger = torch.cat([batch, torch.full((4096 - batch.numel() % 4096,), 9, dtype=torch.uint8, device="cuda")]).view(-1, 4096)
                same(cam(bigger), want)


def test_segmentation_mode():
    N = 2
    model = make("bp", N, end_to_end=False)
    det = model.detector(batch=N, thin=True)
    ref = det.camera(frame_hw=FRAME_HW, crop=CROP)
    for pointers in (False, True):
        for lay in frame_layouts(pointers):
            cam = det.camera(frame_hw=FRAME_HW, crop=CROP, layout=lay, yuv="bt709")
            batch, planes, rgb = surface_and_rgb(lay, "bt709", N)
            arg = cam.bind(planes) if pointers else batch
            for fused_ in (True, False):
                ref.fused = cam.fused = fused_
                want = ref.segment(rgb)
                wst = ref.last_status.clone()
                got = cam.segment(arg)
                assert got.dtype == torch.uint8 and got.shape == (N, 64, 128) and torch.equal(got, want)
                assert torch.equal(cam.last_status, wst)
                same(cam(arg), ref(rgb))


def test_input_pipeline_with_a_layout_and_flips():
    from lanedetection_end2end_amd.pipeline import InputPipeline
    N = 3
    ref = InputPipeline(64, "bp", frame_hw=FRAME_HW, crop=CROP)
    labels = torch.randint(0, 5, (N,) + FRAME_HW, dtype=torch.uint8, device="cuda")
    flip = torch.tensor([True, False, True])
    for pointers in (False, True):
        for lay in frame_layouts(pointers):
            pipe = InputPipeline(64, "bp", frame_hw=FRAME_HW, crop=CROP, layout=lay, yuv="bt709")
            batch, planes, rgb = surface_and_rgb(lay, "bt709", N, seed=6)
            arg = pipe.bind(planes) if pointers else batch
            got, want = pipe(arg, labels, flip), ref(rgb, labels, flip)
            assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32)) and torch.equal(got[1], want[1])
            index = torch.tensor([2, 0, 0, 1], device="cuda")
            if pointers:
                assert torch.equal(pipe(arg)[0].view(torch.int32), ref(rgb)[0].view(torch.int32))      # the table knows its count
                with pytest.raises(ValueError, match="index"):
                    pipe(arg, index=index)
                continue
            assert torch.equal(pipe(arg, n=N)[0].view(torch.int32), ref(rgb)[0].view(torch.int32))
            # the count is never guessed from a buffer with room for more than one frame (a decoder's buffer may be larger) ...
            with pytest.raises(ValueError, match="n="):
                pipe(arg)
            with pytest.raises(ValueError, match="n="):
                pipe(arg, flip=flip[[0, 1, 1, 0]], index=index)
            # ... a buffer with room for one frame only is one frame, slack or not
            one = arg[:lay.batch_bytes(1) + lay.frame_stride - 1]
            assert one.numel() < lay.batch_bytes(2)
            assert torch.equal(pipe(one)[0].view(torch.int32), ref(rgb[:1])[0].view(torch.int32))
            got, want = pipe(arg, flip=flip[[0, 1, 1, 0]], index=index, n=N), ref(rgb, flip=flip[[0, 1, 1, 0]], index=index)
            pipe.flush()
            ref.flush()
            assert got[0].shape == (4, 3, 64, 128) and torch.equal(got[0].view(torch.int32), want[0].view(torch.int32))
            pipe(arg, index=torch.tensor([0, 3], device="cuda"), n=N)
            with pytest.raises(IndexError):
                pipe.flush()


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_lanes_on_a_720x1280_decoder_surface(precision):
    from lanedetection_end2end_amd.pipeline import FrameLayout
    from oracle import pipeline_oracle as po
    model = make("bp", 1, R=256, precision=precision, clas=True)
    det = model.detector(thin=True)
    src = po.synthetic_frame(3)[0]                     # a frame with structure: its planes stand in for Y Cb Cr
    tight = np.ascontiguousarray(np.concatenate([src[..., 1], src[::2, ::2, [2, 0]].reshape(360, 1280)])[None])
    lay = FrameLayout("nv12", (720, 1280), pitch=(1536, 1536), plane_offsets=(0, 736 * 1536))
    assert lay.frame_span == 736 * 1536 + 359 * 1536 + 1280
    surface, _ = S.embed(tight, ref_layout(lay), 12)
    surface = torch.from_numpy(surface).cuda()
    f = torch.from_numpy(tight).cuda()
    cam, ref = det.camera(layout=lay, yuv="bt709"), det.camera(pixel_format="nv12", yuv="bt709")
    assert cam.fits and cam.frame_shape is None
    for fused_ in (True, False):
        ref.fused = cam.fused = fused_
        want = ref.lanes(f)
        wst = ref.last_status.clone()
        got = cam.lanes(surface)
        assert got._fields == want._fields
        same(tuple(got.betas) + tuple(got[2:]) + (got.lanes,), tuple(want.betas) + tuple(want[2:]) + (want.lanes,))
        assert torch.equal(cam.last_status, wst)


def test_python_side_refusals_launch_nothing():
    from lanedetection_end2end_amd import _lib
    from lanedetection_end2end_amd.pipeline import FrameLayout, InputPipeline
    model = make("bev", 1)
    det = model.detector()
    nv12, _, _ = frame_layouts(False)
    with pytest.raises(ValueError, match="pixel_format"):
        det.camera(frame_hw=FRAME_HW, crop=CROP, layout=nv12, pixel_format="nv12")
    with pytest.raises(ValueError, match="frame_hw"):
        det.camera(frame_hw=(182, 320), crop=CROP, layout=nv12)
    with pytest.raises(ValueError, match="yuv"):
        det.camera(frame_hw=FRAME_HW, crop=CROP, layout=nv12, yuv="bt601")
    model.last_status = None
    cam = det.camera(frame_hw=FRAME_HW, crop=CROP, layout=nv12)
    pipe = InputPipeline(64, "bev", frame_hw=FRAME_HW, crop=CROP, layout=nv12)
    batch, planes, _ = surface_and_rgb(nv12, "jfif", 1)
    for call in (cam, pipe):
        with pytest.raises(ValueError, match="bytes"):
            call(batch[:-1])                                              # a short buffer
        with pytest.raises(ValueError, match="uint8"):
            call(batch.float())
        with pytest.raises(ValueError, match="contiguous"):
            call(torch.cat([batch, batch]).view(-1, 2)[:, 0])
        with pytest.raises(ValueError, match="aligned"):
            call(torch.cat([batch, batch])[1:])                           # a misaligned base
        with pytest.raises(_lib.LaneFitLibraryError, match="CPU path"):
            call(batch.cpu())
    with pytest.raises(ValueError, match="plane_pointers"):
        cam.bind(planes)
    ptr_lay = frame_layouts(True)[0]
    pcam = det.camera(frame_hw=FRAME_HW, crop=CROP, layout=ptr_lay)
    ppipe = InputPipeline(64, "bev", frame_hw=FRAME_HW, crop=CROP, layout=frame_layouts(True)[0])
    _, planes, _ = surface_and_rgb(ptr_lay, "jfif", 1)
    y, c = planes[0]
    table = pcam.bind(planes)
    with pytest.raises(ValueError, match="bind"):
        pcam(batch)                                                       # a pointer layout takes the table
    with pytest.raises(ValueError, match="index"):
        ppipe(ppipe.bind(planes), index=torch.tensor([0], device="cuda"))          # a table passed with index=
    with pytest.raises(ValueError, match="another layout"):
        ppipe(table)
    with pytest.raises(ValueError, match="batch of 1"):
        pcam.bind(planes + planes)
    with pytest.raises(ValueError, match="plane"):
        pcam.bind([(y,)])
    with pytest.raises(ValueError, match="pitch"):
        pcam.bind([(torch.zeros(180, 400, dtype=torch.uint8, device="cuda")[:, :320], c)])      # a wrong pitch
    with pytest.raises(ValueError, match="aligned"):
        pcam.bind([(torch.cat([y, y])[1:], c)])                                                # a misaligned base
    with pytest.raises(ValueError, match="aligned"):
        pcam.bind([(y, torch.cat([c, c])[1:])])                                                # the CbCr plane: 2 bytes
    pcam.bind([(y, torch.cat([c, c])[2:])])
    with pytest.raises(ValueError, match="span"):
        pcam.bind([(y[:-1], c)])
    with pytest.raises(ValueError, match="uint8"):
        pcam.bind([(y.float(), c)])
    with pytest.raises(_lib.LaneFitLibraryError, match="CPU path"):
        pcam.bind([(y.cpu(), c)])
    ok2d = torch.zeros(180, 384, dtype=torch.uint8, device="cuda")[:, :320]
    pcam.bind([(ok2d, c)])
    assert cam.last_status is None and pcam.last_status is None and model.last_status is None, "a refused call ran the backbone"
    same(pcam(table), det.camera(frame_hw=FRAME_HW, crop=CROP, pixel_format="nv12")(
        torch.from_numpy(S.extract([[p.cpu().numpy() for p in planes[0]]], ref_layout(ptr_lay), 1)).cuda()))
