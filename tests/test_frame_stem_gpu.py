"""frame_stem_kernel alone (csrc/lf_frame_stem.hip, through lf_debug_frame_stem): decoded uint8 frames -> the stem's NHWC 16-channel
buffer in one launch, BIT FOR BIT what lf_pipeline_image followed by the inference form of lf_debug_stem_fwd gives, fp32 and bf16
storage, and -- for the 2.5x and the ragged geometry -- inside the derived bound of test_eltwise_gpu.test_stem_fwd's inference form
against fp64 on the Pillow oracle's pixels (no tolerance of its own: B = (9 * 3 + 2) u sum |w x| on the convolution channels, the
pooled ones exact; B2 = B |sc| + 3 u (|v sc| + |sh|); out_bound for bf16).

Geometries (Hin, Win, crop_top, crop_h -> out_h x out_w), the smallest that reach every path of the kernel:
  (180, 320, 20, 160 -> 64 x 128)   2.5x, the compiled 7 / 7 taps, two workgroups per row of tiles
  (100, 130, 20,  80 -> 64 x 128)   5 / 5 taps
  ( 30,  50,  6,  24 -> 32 x  64)   up-scaling, 3 taps, the generic path
  ( 97, 333, 33,  64 -> 36 x  68)   ragged tiles (stem 18 x 34), odd source width, mixed tap counts
  ( 40,  60, 10,  30 -> 12 x  20)   stem 6 x 10: smaller than a tile
  (  8,   8,  0,   8 ->  2 x   2)   one stem pixel
Frames are random bytes with the rows above the crop at 255, the first / last row of the crop at 0 / 255 and the first / last column
at 255 / 0: a read above the crop, or a tap that crosses the padding into a neighbouring row, changes the result visibly.  Outputs sit
in NaN-guarded allocations (test_eltwise_gpu.Buf): every element written, nothing outside.
"""
import ctypes

import numpy as np
import pytest
import torch

import eltwise_ref as R
import test_eltwise_gpu as E
from oracle import pipeline_oracle as po

pytestmark = pytest.mark.gpu

GEOMS = [(180, 320, 20, 160, 64, 128), (100, 130, 20, 80, 64, 128), (30, 50, 6, 24, 32, 64), (97, 333, 33, 64, 36, 68),
         (40, 60, 10, 30, 12, 20), (8, 8, 0, 8, 2, 2)]
FP64_GEOMS = [GEOMS[0], GEOMS[3]]


class U8Buf:
    """uint8 frames in the middle of a guarded allocation (test_eltwise_gpu.Buf is for floating types); nothing may change.  The
    frames END 256 bytes before the allocation's end: the staging's last dword stays inside the buffer it was given."""

    def __init__(self, init):
        n = init.numel()
        self.whole = torch.full((n + 2 * E.GUARD,), 77, dtype=torch.uint8, device="cuda")
        self.t = self.whole[E.GUARD:E.GUARD + n].view(init.shape)
        self.t.copy_(init)
        self.before = self.whole.clone()

    def check(self):
        assert torch.equal(self.whole, self.before), "the launch wrote into the frames"


class Plan:
    def __init__(self, geom):
        lib = E.lib()
        self.geom = geom
        self.h = ctypes.c_void_p(lib.lf_pipeline_plan_create(*geom))
        assert self.h, lib.lf_last_error()
        self.tables = torch.empty(lib.lf_pipeline_table_bytes(self.h), dtype=torch.uint8, device="cuda")
        assert lib.lf_pipeline_upload(self.h, ctypes.c_void_p(self.tables.data_ptr()), E.stream()) == 0
        self.ok = lib.lf_pipeline_frame_stem_ok(self.h)

    def T(self):
        return ctypes.c_void_p(self.tables.data_ptr())

    def __del__(self):
        try:
            E.lib().lf_pipeline_plan_destroy(self.h)
        except Exception:
            pass


def make_frames(gen, N, geom):
    Hin, Win, top, ch = geom[:4]
    f = torch.randint(0, 256, (N, Hin, Win, 3), device="cuda", generator=gen, dtype=torch.int32).to(torch.uint8)
    f[:, :top] = 255
    f[:, top] = 0
    f[:, top + ch - 1] = 255
    f[:, :, 0] = 255
    f[:, :, Win - 1] = 0
    return f


def operands(gen):
    return 0.3 * E.randn(gen, 13, 3, 3, 3), E.randn(gen, 13), E.signed(gen, 16), E.randn(gen, 16)


def two_launches(plan, frames, ins, N, s16):
    """lf_pipeline_image -> lf_debug_stem_fwd(sc, sh): (image, cat)"""
    lib = E.lib()
    oh, ow = plan.geom[4:]
    img = torch.empty(N, 3, oh, ow, device="cuda")
    cat = E.Buf((N, oh // 2, ow // 2, 16), E.dt(s16))
    rc = lib.lf_pipeline_image(plan.h, ctypes.c_void_p(frames.t.data_ptr()), N, plan.T(), None, ctypes.c_void_p(img.data_ptr()), E.stream())
    rc2 = lib.lf_debug_stem_fwd(ctypes.c_void_p(img.data_ptr()), N, 3, oh, ow, E.P(ins[0]), E.P(ins[1]), E.P(ins[2]), E.P(ins[3]), E.P(cat),
                                None, 0, s16, E.stream())
    assert (rc, rc2) == (0, 0), (rc, rc2, lib.lf_last_error())
    return img, cat


def fused(plan, frames, ins, N, s16):
    oh, ow = plan.geom[4:]
    cat = E.Buf((N, oh // 2, ow // 2, 16), E.dt(s16))
    rc = E.lib().lf_debug_frame_stem(plan.h, ctypes.c_void_p(frames.t.data_ptr()), N, plan.T(), E.P(ins[0]), E.P(ins[1]), E.P(ins[2]),
                                     E.P(ins[3]), E.P(cat), s16, E.stream())
    return rc, cat


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("s16", [0, 1])
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "%dx%d+%d+%d-%dx%d" % g)
def test_bits_of_the_two_launches(geom, s16, N):
    plan = Plan(geom)
    gen = E.cuda_gen(7000 + geom[0] + 2 * s16 + N)
    frames = U8Buf(make_frames(gen, N, geom))
    ins = [E.Buf(v.shape, init=v) for v in operands(gen)]
    assert bool((ins[2].t > 0).any()) and bool((ins[2].t < 0).any()), "scales of both signs"
    rc, got = fused(plan, frames, ins, N, s16)
    torch.cuda.synchronize()
    if not plan.ok:
        assert rc == -1 and E.lib().lf_last_error()
        got.check()
        return
    assert rc == 0, E.lib().lf_last_error()
    _, want = two_launches(plan, frames, ins, N, s16)
    torch.cuda.synchronize()
    frames.check()
    for x in ins:
        x.check()
    got.check(True)
    want.check(True)
    bits = E.BITS[E.dt(s16)]
    assert torch.equal(got.t.view(bits), want.t.view(bits)), "frame_stem_kernel differs from lf_pipeline_image -> stem"


@pytest.mark.parametrize("s16", [0, 1])
@pytest.mark.parametrize("geom", FP64_GEOMS, ids=lambda g: "%dx%d+%d+%d-%dx%d" % g)
def test_against_fp64_on_the_oracle_pixels(geom, s16):
    N = 2
    plan = Plan(geom)
    assert plan.ok
    Hin, Win, top, ch, oh, ow = geom
    gen = E.cuda_gen(7100 + geom[0] + s16)
    frames = U8Buf(make_frames(gen, N, geom))
    w, b, sc, sh = operands(gen)
    ins = [E.Buf(v.shape, init=v) for v in (w, b, sc, sh)]
    rc, got = fused(plan, frames, ins, N, s16)
    torch.cuda.synchronize()
    assert rc == 0, E.lib().lf_last_error()
    got.check(True)
    host = frames.t.cpu().numpy()
    pix = np.stack([po.resize_bilinear_u8(host[n, top:top + ch], oh, ow) for n in range(N)])            # (N, oh, ow, 3) uint8
    img = torch.from_numpy((pix.astype(np.float32) / np.float32(255)).transpose(0, 3, 1, 2).copy()).cuda()
    ref, S = R.stem(img, w, b), R.stem_abs(img, w, b)
    B = (9 * 3 + 2) * E.U * S
    B[..., 13:] = 0
    ref2 = torch.relu(ref * sc.double() + sh.double())
    B2 = B * sc.double().abs() + 3 * E.U * ((ref * sc.double()).abs() + sh.double().abs())
    ratio = E.worst(got.t, ref2, E.out_bound(ref2, B2, s16))
    E.report("frame_stem %s s16=%d against fp64" % (geom, s16), ratio)


def test_refusals_launch_nothing():
    lib = E.lib()
    gen = E.cuda_gen(7200)
    ins = [E.Buf(v.shape, init=v) for v in operands(gen)]

    def refused(plan, geom, null=None):
        frames = U8Buf(make_frames(gen, 1, geom))
        cat = E.Buf((1, max(geom[4] // 2, 1), max(geom[5] // 2, 1), 16))
        args = [plan.h, ctypes.c_void_p(frames.t.data_ptr()), 1, plan.T(), E.P(ins[0]), E.P(ins[1]), E.P(ins[2]), E.P(ins[3]), E.P(cat)]
        if null is not None:
            args[null] = None
        rc = lib.lf_debug_frame_stem(*args, 0, E.stream())
        torch.cuda.synchronize()
        assert rc == -1 and lib.lf_last_error(), (geom, null)
        cat.check()
        frames.check()

    for geom in [(8, 8, 0, 8, 3, 2), (8, 8, 0, 8, 2, 3)]:                      # odd out_h, odd out_w
        plan = Plan(geom)
        assert plan.ok == 0
        refused(plan, geom)
    big = (640, 1280, 0, 640, 64, 128)                                         # 21 taps per axis: no tile fits the LDS budget
    plan = Plan(big)
    assert plan.ok == 0
    refused(plan, big)
    small = GEOMS[4]
    plan = Plan(small)
    assert plan.ok == 1
    for null in (0, 1, 3, 4, 5, 6, 7, 8):
        refused(plan, small, null)
