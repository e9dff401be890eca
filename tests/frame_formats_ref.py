"""The frame formats of the input pipeline and the camera detector, restated in numpy (include/lanefit.h, "additions since 5 --
frame formats"): what RGB frames a BGR, NV12 or YUYV frame IS.  Everything behind the staging of a source window runs on these uint8
RGB values, so every test of a format compares against the same call on an ``rgb`` plan fed ``to_rgb(...)``.

  rgb, bgr  (N, H, W, 3)       packed
  nv12      (N, H * 3 // 2, W) H rows of Y, then H / 2 rows of interleaved Cb Cr pairs; H, W even
  yuyv      (N, H, W, 2)       Y0 Cb Y1 Cr per pixel pair; W even
Chroma of pixel (y, x): nv12 -- the pair at chroma row y >> 1, column x >> 1; yuyv -- the pair of pixel pair x >> 1 in row y.
Replicated, no interpolation.  YCbCr -> RGB, int32, arithmetic shift (floor):
  y' = Y - y_off;  u = Cb - 128;  v = Cr - 128
  R = clamp8((c_y y' + c_rv v + 32768) >> 16);  G = clamp8((c_y y' - c_gu u - c_gv v + 32768) >> 16);  B = clamp8((c_y y' + c_bu u + 32768) >> 16)
"""
import numpy as np

FORMATS = {"rgb": 0, "bgr": 1, "nv12": 2, "yuyv": 3}
#          c_y    y_off  c_rv    c_gu   c_gv   c_bu
PRESETS = {"jfif": (65536, 0, 91881, 22554, 46802, 116130), "bt709": (76309, 16, 117489, 13975, 34925, 138438)}


def ycc_to_rgb(Y, Cb, Cr, coef, intermediates=False):
    """uint8 arrays of one shape -> (..., 3) uint8 RGB.  int64 arithmetic: ``intermediates=True`` also returns the largest magnitude any
    sum reached (the claim that int32 is enough is checked, not assumed)."""
    c_y, y_off, c_rv, c_gu, c_gv, c_bu = (int(c) for c in coef)
    y = c_y * (Y.astype(np.int64) - y_off)
    u, v = Cb.astype(np.int64) - 128, Cr.astype(np.int64) - 128
    sums = (y + c_rv * v + 32768, y - c_gu * u - c_gv * v + 32768, y + c_bu * u + 32768)
    rgb = np.stack([np.clip(s >> 16, 0, 255) for s in sums], axis=-1).astype(np.uint8)
    if intermediates:
        parts = (y, c_rv * v, c_gu * u, c_gv * v, c_bu * u, y - c_gu * u) + sums
        return rgb, max(int(np.abs(p).max()) for p in parts)
    return rgb


def frames_shape(fmt, N, H, W):
    return {"rgb": (N, H, W, 3), "bgr": (N, H, W, 3), "nv12": (N, H * 3 // 2, W), "yuyv": (N, H, W, 2)}[fmt]


def frame_bytes(fmt, H, W):
    return int(np.prod(frames_shape(fmt, 1, H, W)))


def to_rgb(frames, fmt, H, W, coef=PRESETS["jfif"]):
    """frames (N, ...) uint8 in format ``fmt`` of H x W pixels -> (N, H, W, 3) uint8 RGB by the definition above."""
    frames = np.asarray(frames)
    N = frames.shape[0]
    assert frames.dtype == np.uint8 and frames.shape == frames_shape(fmt, N, H, W), (frames.shape, fmt, H, W)
    if fmt == "rgb":
        return frames.copy()
    if fmt == "bgr":
        return frames[..., ::-1].copy()
    yy, xx = np.arange(H)[:, None], np.arange(W)[None, :]
    if fmt == "nv12":
        assert H % 2 == 0 and W % 2 == 0
        Y = frames[:, :H]
        C = frames[:, H:].reshape(N, H // 2, W // 2, 2)
        Cb, Cr = C[:, yy >> 1, xx >> 1, 0], C[:, yy >> 1, xx >> 1, 1]
    else:
        assert W % 2 == 0
        Y = frames[..., 0]
        G = frames.reshape(N, H, W // 2, 4)
        Cb, Cr = G[:, yy, xx >> 1, 1], G[:, yy, xx >> 1, 3]
    return ycc_to_rgb(Y, Cb, Cr, coef)


def float_ycc_to_rgb(Y, Cb, Cr, c_y, y_off, c_rv, c_gu, c_gv, c_bu):
    """the matrix in floating point: floor(v + 0.5), clamped"""
    y = c_y * (Y.astype(np.float64) - y_off)
    u, v = Cb.astype(np.float64) - 128, Cr.astype(np.float64) - 128
    ch = (y + c_rv * v, y - c_gu * u - c_gv * v, y + c_bu * u)
    return np.stack([np.clip(np.floor(c + 0.5), 0, 255) for c in ch], axis=-1).astype(np.uint8)
