"""On-device input pipeline: decoded uint8 frames + label maps already in HBM -> the
``(image, gt[, horizon])`` tensors ``LaneDataset.__getitem__`` produces (BEV/Dataloader/Load_Data_new.py:62-117,
BP/Dataloader/Load_Data_new.py:110-197), batched, bit-identical to the PIL/torchvision result.

Only the pixel work lives here (crop, BILINEAR / NEAREST resize, class remap, flip, ToTensor).  The label half (polynomial
parameters, lane x-coordinates, valid points, the BP horizon, line-type lists) of a RESIDENT dataset is one launch in
``loader.ResidentDataset`` (``lf_label_batch_bp`` / ``lf_label_batch_bev``), which hands its effective flips to this pipeline; for a
loader of one's own that keeps it host-side numpy as the reference does, ``flip_params_bev`` / ``flip_lanes_bp`` / ``mirror_list``
below mirror the flip statements.
"""
import ctypes

import numpy as np
import torch

from . import _lib


# Frame formats (include/lanefit.h, "additions since 5 -- frame formats"): LF_FRAME_* codes, and the YCbCr -> RGB presets
# (c_y, y_off, c_rv, c_gu, c_gv, c_bu) of the Q16 form  R = clamp8((c_y (Y - y_off) + c_rv (Cr - 128) + 32768) >> 16), ...
#   "jfif":  full-range BT.601 -- the integers of libjpeg's decoder, bit for bit what Image.open(jpeg).convert("RGB") holds;
#   "bt709": limited-range BT.709, what video decoders usually emit: round(65536 x) of 1.164384, 1.792741, 0.213249, 0.532909, 2.112402.
PIXEL_FORMATS = {"rgb": 0, "bgr": 1, "nv12": 2, "yuyv": 3}
YUV_PRESETS = {"jfif": (65536, 0, 91881, 22554, 46802, 116130), "bt709": (76309, 16, 117489, 13975, 34925, 138438)}


def yuv_coefficients(yuv):
    """The six ints of a ``yuv=`` argument: a preset name or a 6-tuple of ints (``ValueError`` otherwise)."""
    if isinstance(yuv, str):
        if yuv not in YUV_PRESETS:
            raise ValueError("yuv=%r: the presets are %s (or give six ints c_y, y_off, c_rv, c_gu, c_gv, c_bu)" % (yuv, sorted(YUV_PRESETS)))
        return YUV_PRESETS[yuv]
    try:
        coef = tuple(yuv)
    except TypeError:
        raise ValueError("yuv=%r: a preset name or six ints (c_y, y_off, c_rv, c_gu, c_gv, c_bu)" % (yuv,))
    if len(coef) != 6 or not all(isinstance(c, (int, np.integer)) and not isinstance(c, bool) for c in coef):
        raise ValueError("yuv=%r: a preset name or six ints (c_y, y_off, c_rv, c_gu, c_gv, c_bu)" % (yuv,))
    return tuple(int(c) for c in coef)


def frames_shape(pixel_format, n, frame_hw):
    """Shape of ``n`` frames of ``frame_hw`` in ``pixel_format``; ``ValueError`` for an unknown format or a size it cannot hold."""
    if pixel_format not in PIXEL_FORMATS:
        raise ValueError("pixel_format=%r: one of %s" % (pixel_format, sorted(PIXEL_FORMATS)))
    H, W = int(frame_hw[0]), int(frame_hw[1])
    if pixel_format == "nv12":
        if H % 2 or W % 2:
            raise ValueError("nv12 frames have an even height and width, got %d x %d" % (H, W))
        return (n, H * 3 // 2, W)
    if pixel_format == "yuyv":
        if W % 2:
            raise ValueError("yuyv frames have an even width, got %d" % W)
        return (n, H, W, 2)
    return (n, H, W, 3)


def set_plan_format(handle, pixel_format, yuv):
    """``lf_pipeline_plan_set_format`` on a plan handle, from the Python names.  Validates both before touching the plan."""
    code = PIXEL_FORMATS.get(pixel_format)
    if code is None:
        raise ValueError("pixel_format=%r: one of %s" % (pixel_format, sorted(PIXEL_FORMATS)))
    coef = yuv_coefficients(yuv)
    if code == 0:
        return                                   # a plan that never gets the call is an RGB plan
    lib = _lib.load()
    if lib.lf_pipeline_plan_set_format(handle, code, (ctypes.c_int * 6)(*coef)) != 0:
        raise ValueError("lf_pipeline_plan_set_format failed: %s" % lib.lf_last_error().decode())


class InputPipeline:
    """``InputPipeline(resize, tree='bev'|'bp', nclasses=2, frame_hw=(720, 1280), crop=640, pixel_format='rgb', yuv='jfif')``;
    ``__call__(frames_u8, labels_u8=None, flip=None) -> (image, gt, horizon)``.

    frames_u8 (N, H, W, 3) uint8 and labels_u8 (N, H, W) uint8 on the GPU; flip (N,) bool (the reference draws
    ``np.random.uniform() > 0.5 and flip_on`` per training sample).  image (N,3,R,2R) fp32, gt (N,1,R,2R) int64,
    horizon (N,R) fp32 for tree='bev' (the BP tree derives its horizon from the lane coordinates on the host).

    ``pixel_format``: what the frames hold -- ``'rgb'`` / ``'bgr'`` (N, H, W, 3), ``'nv12'`` (N, H * 3 // 2, W: the Y plane, then the
    interleaved CbCr rows; H, W even) or ``'yuyv'`` (N, H, W, 2; W even), contiguous.  The image is bit for bit the ``'rgb'`` image of
    the frames the Q16 definition above makes from them (chroma replicated; ``yuv``: ``'jfif'``, ``'bt709'`` or six ints; ignored for
    ``'rgb'`` / ``'bgr'``).  Labels know no format."""

    def __init__(self, resize, tree="bev", nclasses=2, frame_hw=(720, 1280), crop=640, pixel_format="rgb", yuv="jfif"):
        assert tree in ("bev", "bp")
        H, W = frame_hw
        self.frames_shape = frames_shape(pixel_format, -1, (H, W))[1:]
        yuv_coefficients(yuv)
        lib = _lib.load()
        self.resize, self.tree, self.nclasses, self.frame_hw = resize, tree, nclasses, (H, W)
        self.pixel_format = pixel_format
        self.handle = lib.lf_pipeline_plan_create(H, W, H - crop, crop, resize, 2 * resize)
        if not self.handle:
            raise _lib.LaneFitLibraryError("lf_pipeline_plan_create failed: %s" % lib.lf_last_error().decode())
        set_plan_format(self.handle, pixel_format, yuv)
        self.mode = (1 if (tree == "bev" or nclasses < 3) else 0) | (2 if tree == "bp" else 0)
        self._tables = None
        self._lut = None
        # Out-of-pool indices (``index`` form): the kernels count them on the device and read pool entry 0 instead; the count of
        # call k is copied to pinned memory right behind its kernels (``_lib.DeferredRead``) and inspected at the START of call
        # k + 1 or by flush() -- IndexError like the reference's tensor indexing, one call late, without a host sync per step.
        self._bad = None
        self._pending = None

    def flush(self):
        """Raise now if the previous indexed call saw an index outside the pool."""
        pend, self._pending = self._pending, None
        if pend is not None:
            n = int(pend[0].get()[0])
            if n:
                self._bad.zero_()
                raise IndexError("InputPipeline: %d index value(s) outside the pool of %d frames" % (n, pend[1]))

    def __del__(self):
        try:
            _lib.load().lf_pipeline_plan_destroy(self.handle)
        except Exception:
            pass

    def host_tables(self):
        """(bounds_x, weights_x, bounds_y, weights_y, nearest_x, nearest_y) as numpy int32 (tests)."""
        lib = _lib.load()
        ksx, ksy = ctypes.c_int(), ctypes.c_int()
        lib.lf_pipeline_tables_host(self.handle, ctypes.byref(ksx), ctypes.byref(ksy), None, None, None, None, None, None)
        R = self.resize
        arrs = [np.zeros(n, dtype=np.int32) for n in (4 * R, 2 * R * ksx.value, 2 * R, R * ksy.value, 2 * R, R)]
        ptrs = [a.ctypes.data_as(ctypes.c_void_p) for a in arrs]
        lib.lf_pipeline_tables_host(self.handle, None, None, *ptrs)
        bx, kx, by, ky, ntx, nty = arrs
        return bx.reshape(-1, 2), kx.reshape(2 * R, -1), by.reshape(-1, 2), ky.reshape(R, -1), ntx, nty

    def _device_state(self, device):
        lib = _lib.load()
        if self._tables is None or self._tables.device != device:
            self._tables = torch.empty(lib.lf_pipeline_table_bytes(self.handle), dtype=torch.uint8, device=device)
            _lib.check(lib.lf_pipeline_upload(self.handle, _lib.ptr(self._tables), _lib.stream()), "lf_pipeline_upload")
            # (ToTensor()(gt) * 255).long() per palette index, evaluated with the reference's fp32 ops
            v = torch.arange(256, dtype=torch.uint8).to(torch.float32).div(255)
            self._lut = (v * 255).long().to(device)
        return self._tables, self._lut

    def __call__(self, frames_u8, labels_u8=None, flip=None, index=None):
        """``index`` (N,) int64 on the device: ``frames_u8`` / ``labels_u8`` are a resident POOL and batch element n is pool entry
        ``index[n]`` -- gathered inside the kernels (``lf_pipeline_image_indexed``), no copy of the N selected frames first."""
        lib = _lib.load()
        if not frames_u8.is_cuda:
            raise _lib.LaneFitLibraryError("InputPipeline needs the decoded frames on the MI355X; there is no CPU path")
        if tuple(frames_u8.shape[1:]) != self.frames_shape or frames_u8.dtype != torch.uint8:
            raise ValueError("this pipeline takes %s frames of shape (N,) + %s, uint8; got %s, %s"
                             % (self.pixel_format, self.frames_shape, tuple(frames_u8.shape), frames_u8.dtype))
        pool, (H, W) = frames_u8.shape[0], self.frame_hw
        dev = frames_u8.device
        tables, lut = self._device_state(dev)
        R = self.resize
        sel = None
        N = pool
        if index is not None:
            self.flush()
            sel = index.to(device=dev, dtype=torch.int64).contiguous()
            N = sel.numel()
            if self._bad is None or self._bad.device != dev:
                self._bad = torch.zeros(1, dtype=torch.int32, device=dev)
        fl = None if flip is None else flip.to(device=dev, dtype=torch.uint8).contiguous()
        frames_u8 = frames_u8.contiguous()
        image = torch.empty(N, 3, R, 2 * R, dtype=torch.float32, device=dev)
        if sel is None:
            _lib.check(lib.lf_pipeline_image(self.handle, _lib.ptr(frames_u8), N, _lib.ptr(tables), _lib.ptr(fl),
                                             _lib.ptr(image), _lib.stream()), "lf_pipeline_image")
        else:
            _lib.check(lib.lf_pipeline_image_indexed(self.handle, _lib.ptr(frames_u8), pool, _lib.ptr(sel), N, _lib.ptr(tables),
                                                     _lib.ptr(fl), _lib.ptr(image), _lib.ptr(self._bad), _lib.stream()),
                       "lf_pipeline_image_indexed")
        gt = horizon = None
        if labels_u8 is not None:
            assert labels_u8.shape == (pool, H, W) and labels_u8.dtype == torch.uint8
            labels_u8 = labels_u8.contiguous()
            gt = torch.empty(N, 1, R, 2 * R, dtype=torch.int64, device=dev)
            if self.tree == "bev":
                horizon = torch.empty(N, R, dtype=torch.float32, device=dev)
            if sel is None:
                _lib.check(lib.lf_pipeline_label(self.handle, _lib.ptr(labels_u8), N, _lib.ptr(tables), _lib.ptr(fl),
                                                 self.mode, _lib.ptr(lut), _lib.ptr(gt), _lib.ptr(horizon), _lib.stream()),
                           "lf_pipeline_label")
            else:
                _lib.check(lib.lf_pipeline_label_indexed(self.handle, _lib.ptr(labels_u8), pool, _lib.ptr(sel), N, _lib.ptr(tables),
                                                         _lib.ptr(fl), self.mode, _lib.ptr(lut), _lib.ptr(gt), _lib.ptr(horizon),
                                                         None, _lib.stream()), "lf_pipeline_label_indexed")
        if sel is not None:
            self._pending = (_lib.DeferredRead(self._bad), pool)      # (the image kernel counted: the label kernel sees the same indices)
        return image, gt, horizon


def mirror_list(lst):
    """Load_Data_new.py ``mirror_list``: mirror the line-type list for a flipped sample."""
    middle = len(lst) // 2
    return list(reversed(lst[middle:])) + list(reversed(lst[:middle]))


def flip_params_bev(params):
    """BEV/Dataloader/Load_Data_new.py:93-96 -- params (4, 3) of a flipped sample."""
    p = -np.asarray(params, dtype=np.float64)[[1, 0, 3, 2]]
    p[:, -1] = 1 + p[:, -1]
    return p


def flip_lanes_bp(lanes, resize):
    """BP/Dataloader/Load_Data_new.py:166-168 -- lanes (4, 56) in resized pixels, -2 = absent."""
    lanes = np.asarray(lanes, dtype=np.float64)
    track = lanes < 0
    out = (2 * resize - 1) - lanes
    out[track] = -2
    return out[[1, 0, 3, 2]]
