"""Decoder surfaces restated in numpy (include/lanefit.h, "additions since 5 -- surfaces"): where the pixels of a frame lie in a
surface with pitched rows, planes at offsets and a frame stride, and what RGB frames the three formats that exist only with a layout
are.  No device, no package code: the layout is a plain description (``Layout``), computed here a second time.

  tight frames (what embed takes and extract returns), uint8:
    rgb, bgr  (N, H, W, 3)      nv12  (N, H * 3 // 2, W)      yuyv  (N, H, W, 2)
    i420      (N, H * W * 3 // 2): the Y plane, the Cb plane (H / 2 x W / 2), the Cr plane
    rgbx, bgrx (N, H, W, 4)
"""
import numpy as np

import frame_formats_ref as F

FORMATS = {"rgb": 0, "bgr": 1, "nv12": 2, "yuyv": 3, "i420": 4, "rgbx": 5, "bgrx": 6}
YCC = ("nv12", "yuyv", "i420")


def plane_dims(fmt, H, W):
    """[(rows, row bytes)] per plane"""
    if fmt in ("rgb", "bgr"):
        return [(H, 3 * W)]
    if fmt in ("rgbx", "bgrx"):
        return [(H, 4 * W)]
    if fmt == "yuyv":
        return [(H, 2 * W)]
    if fmt == "nv12":
        return [(H, W), (H // 2, W)]
    return [(H, W), (H // 2, W // 2), (H // 2, W // 2)]


def tight_shape(fmt, N, H, W):
    if fmt == "i420":
        return (N, H * W * 3 // 2)
    if fmt in ("rgbx", "bgrx"):
        return (N, H, W, 4)
    return F.frames_shape(fmt, N, H, W)


class Layout:
    """pitch / offsets: per plane, 0 = default; stride 0 = default.  The resolved numbers, by the header's rules."""

    def __init__(self, fmt, H, W, pitch=(), offsets=(), stride=0, pointers=False):
        self.fmt, self.H, self.W, self.pointers = fmt, H, W, pointers
        self.dims = plane_dims(fmt, H, W)
        P = len(self.dims)
        pitch, offsets = tuple(pitch) + (0,) * (P - len(pitch)), tuple(offsets) + (0,) * (P - len(offsets))
        self.given = (pitch, offsets, stride)
        self.pitch = [pitch[p] or self.dims[p][1] for p in range(P)]
        self.offsets = [0]
        for p in range(1, P):
            self.offsets.append(offsets[p] or self.offsets[p - 1] + self.dims[p - 1][0] * self.pitch[p - 1])
        self.span = [(self.dims[p][0] - 1) * self.pitch[p] + self.dims[p][1] for p in range(P)]
        self.frame_span = max(o + s for o, s in zip(self.offsets, self.span))
        self.stride = stride or max(self.offsets[p] + self.dims[p][0] * self.pitch[p] for p in range(P))

    def batch_bytes(self, n):
        return (n - 1) * self.stride + self.frame_span


def planes_of(tight, fmt, H, W):
    """tight frames (N, ...) -> [plane p as (N, rows, row bytes)]"""
    N = tight.shape[0]
    flat = np.ascontiguousarray(tight).reshape(N, -1)
    out, at = [], 0
    for rows, rb in plane_dims(fmt, H, W):
        out.append(flat[:, at:at + rows * rb].reshape(N, rows, rb))
        at += rows * rb
    assert at == flat.shape[1], (fmt, tight.shape)
    return out


def embed(tight, L, seed):
    """The surface bytes of tight frames under layout L: (batch (batch_bytes,) uint8, [[plane arrays of frame n]]), every byte that is
    not a pixel seeded-random.  The plane arrays (pointer mode: exactly span(p) bytes each) carry the same pixels AND the same padding."""
    tight = np.asarray(tight)
    N = tight.shape[0]
    assert tight.dtype == np.uint8 and tight.shape == tight_shape(L.fmt, N, L.H, L.W), (tight.shape, L.fmt)
    rng = np.random.default_rng(seed)
    batch = rng.integers(0, 256, L.batch_bytes(N), dtype=np.uint8)
    planes = [[rng.integers(0, 256, L.span[p], dtype=np.uint8) for p in range(len(L.dims))] for _ in range(N)]
    for p, src in enumerate(planes_of(tight, L.fmt, L.H, L.W)):
        rows, rb = L.dims[p]
        for n in range(N):
            for y in range(rows):
                a = n * L.stride + L.offsets[p] + y * L.pitch[p]
                batch[a:a + rb] = src[n, y]
                planes[n][p][y * L.pitch[p]:y * L.pitch[p] + rb] = src[n, y]
    return batch, planes


def extract(surface, L, N):
    """The inverse of embed: ``surface`` is the batch array, or the [[plane arrays]] of pointer mode -> the tight frames."""
    out = []
    for p, (rows, rb) in enumerate(L.dims):
        pl = np.empty((N, rows, rb), dtype=np.uint8)
        for n in range(N):
            for y in range(rows):
                if isinstance(surface, np.ndarray):
                    a = n * L.stride + L.offsets[p] + y * L.pitch[p]
                    pl[n, y] = surface[a:a + rb]
                else:
                    pl[n, y] = surface[n][p][y * L.pitch[p]:y * L.pitch[p] + rb]
        out.append(pl.reshape(N, -1))
    return np.concatenate(out, axis=1).reshape(tight_shape(L.fmt, N, L.H, L.W))


def i420_to_nv12(tight, H, W):
    """(N, H W 3 / 2) planar -> (N, H 3 / 2, W) with the chroma samples interleaved"""
    N = tight.shape[0]
    Y, Cb, Cr = planes_of(tight, "i420", H, W)
    C = np.stack([Cb, Cr], axis=-1).reshape(N, H // 2, W)
    return np.concatenate([Y, C], axis=1)


def swap_chroma(tight, H, W):
    """an i420 frame with its Cb and Cr planes exchanged (what YV12 holds)"""
    N = tight.shape[0]
    Y, Cb, Cr = planes_of(tight, "i420", H, W)
    return np.concatenate([Y.reshape(N, -1), Cr.reshape(N, -1), Cb.reshape(N, -1)], axis=1)


def to_rgb(tight, fmt, H, W, coef=F.PRESETS["jfif"]):
    """tight frames in any of the seven formats -> (N, H, W, 3) uint8 RGB"""
    tight = np.asarray(tight)
    if fmt == "i420":
        return F.to_rgb(i420_to_nv12(tight, H, W), "nv12", H, W, coef)
    if fmt == "rgbx":
        return np.ascontiguousarray(tight[..., :3])
    if fmt == "bgrx":
        return np.ascontiguousarray(tight[..., 2::-1])
    return F.to_rgb(tight, fmt, H, W, coef)


# the four layouts of the kernel-level tests: padded pitches (odd where legal), + a gap of three padded rows before each later plane,
# + a frame stride with a gap, plane pointers
PAD = {"rgb": (5,), "bgr": (5,), "i420": (3, 1, 1), "nv12": (6, 10), "yuyv": (12,), "rgbx": (12,), "bgrx": (12,)}


def kernel_layout(fmt, H, W, kind):
    dims = plane_dims(fmt, H, W)
    pitch = tuple(rb + pad for (_, rb), pad in zip(dims, PAD[fmt]))
    if kind in (1, 4):
        return Layout(fmt, H, W, pitch, pointers=kind == 4)
    offsets = [0]
    for p in range(1, len(dims)):
        o = offsets[p - 1] + (dims[p - 1][0] + 3) * pitch[p - 1]
        offsets.append(o + (o & 1 if fmt == "nv12" else 0))
    if kind == 2:
        return Layout(fmt, H, W, pitch, offsets)
    tight = Layout(fmt, H, W, pitch, offsets)
    return Layout(fmt, H, W, pitch, offsets, tight.stride + 3 * pitch[0] + 8)
