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


# Surfaces (include/lanefit.h, "additions since 5 -- surfaces"): the formats a FrameLayout takes -- the four above and the three that
# exist only with a layout.  A table of its own: PIXEL_FORMATS, frames_shape and pixel_format= keep their four names.
SURFACE_FORMATS = {"rgb": 0, "bgr": 1, "nv12": 2, "yuyv": 3, "i420": 4, "rgbx": 5, "bgrx": 6}


class _CLayout(ctypes.Structure):
    """``lf_frame_layout``"""
    _fields_ = [("format", ctypes.c_int), ("plane_pointers", ctypes.c_int), ("pitch", ctypes.c_long * 3),
                ("plane_offset", ctypes.c_long * 3), ("frame_stride", ctypes.c_long)]


class FrameLayout:
    """``FrameLayout(pixel_format, frame_hw, pitch=None, plane_offsets=None, frame_stride=None, plane_pointers=False)``: where the
    pixels of a decoder surface lie (``lf_frame_layout``).  ``pixel_format``: one of ``SURFACE_FORMATS``.  ``pitch``: bytes between
    rows, one int (plane 0) or one per plane, ``None`` / 0 = the row's own bytes; ``plane_offsets``: bytes from a frame's base to each
    plane (``[0]`` is 0; ``None`` / 0 for a later plane = directly behind the one before, its rows x its pitch); ``frame_stride``:
    bytes between the frames of a contiguous batch (``None`` / 0 = the end of the furthest plane at full pitch);
    ``plane_pointers=True``: the planes are separate tensors, bound once with ``bind`` (``SurfaceTable``); ``plane_offsets`` and
    ``frame_stride`` are then not read and not looked at.  YV12 is ``"i420"`` with
    the offsets (or the bound tensors) of planes 1 and 2 exchanged.

    Resolved attributes: ``planes``, ``plane_rows``, ``plane_row_bytes``, ``pitch``, ``plane_offsets``, ``frame_stride`` (tuples /
    int, no zero left), ``span`` (per plane: ``(rows - 1) pitch + row bytes``), ``frame_span`` (the furthest byte of one frame),
    ``batch_bytes(n)`` = ``(n - 1) frame_stride + frame_span``.  Raises ``ValueError`` for what ``lf_pipeline_plan_set_layout``
    refuses (the same rules, restated here: no device, no library call): an unknown format, an odd size where the format needs an
    even one, a negative value, a pitch below the row's bytes, ``plane_offsets[0] != 0``, pitch / offset / stride that are not
    multiples of 4 for ``yuyv`` / ``rgbx`` / ``bgrx``, an odd chroma pitch / chroma offset / frame stride for ``nv12``."""

    def __init__(self, pixel_format, frame_hw, pitch=None, plane_offsets=None, frame_stride=None, plane_pointers=False):
        if pixel_format not in SURFACE_FORMATS:
            raise ValueError("FrameLayout: pixel_format=%r: one of %s" % (pixel_format, sorted(SURFACE_FORMATS)))
        H, W = int(frame_hw[0]), int(frame_hw[1])
        fmt = pixel_format
        if fmt in ("nv12", "i420") and (H % 2 or W % 2):
            raise ValueError("%s frames have an even height and width, got %d x %d" % (fmt, H, W))
        if fmt == "yuyv" and W % 2:
            raise ValueError("yuyv frames have an even width, got %d" % W)
        self.pixel_format, self.frame_hw, self.plane_pointers = fmt, (H, W), bool(plane_pointers)
        self.planes = 3 if fmt == "i420" else (2 if fmt == "nv12" else 1)
        row0 = {"rgb": 3 * W, "bgr": 3 * W, "yuyv": 2 * W, "rgbx": 4 * W, "bgrx": 4 * W}.get(fmt, W)
        self.plane_rows = (H, H // 2, H // 2)[:self.planes]
        self.plane_row_bytes = (row0, W if fmt == "nv12" else W // 2, W // 2)[:self.planes]

        def per_plane(v, what):
            if v is None:
                return (0,) * self.planes
            try:
                v = (v,) if isinstance(v, (int, float, np.number)) else tuple(v)
            except TypeError:
                raise ValueError("FrameLayout: %s takes an int or up to %d ints, got %r" % (what, self.planes, v))
            if len(v) > self.planes or not all(isinstance(x, (int, np.integer)) and not isinstance(x, bool) for x in v):
                raise ValueError("FrameLayout: %s takes up to %d ints for %s, got %r" % (what, self.planes, fmt, v))
            return tuple(int(x) for x in v) + (0,) * (self.planes - len(v))

        if self.plane_pointers:      # plane pointers: offsets and stride are not read, and not looked at (as the C call)
            plane_offsets = frame_stride = None
        self._given = (per_plane(pitch, "pitch"), per_plane(plane_offsets, "plane_offsets"), int(frame_stride or 0))
        gp, go, gs = self._given
        if min(gp + go + (gs,)) < 0:
            raise ValueError("FrameLayout: negative pitch, plane offset or frame stride")
        if go[0] != 0:
            raise ValueError("FrameLayout: plane_offsets[0] must be 0")
        dword = fmt in ("yuyv", "rgbx", "bgrx")
        res_p, res_o, span = [], [], []
        for p in range(self.planes):
            rows, rb = self.plane_rows[p], self.plane_row_bytes[p]
            if gp[p] and gp[p] < rb:
                raise ValueError("FrameLayout: pitch %d of plane %d is below the %d bytes of a row" % (gp[p], p, rb))
            if gp[p] > 0x7fffffff:
                raise ValueError("FrameLayout: pitch of 2^31 bytes or more")
            res_p.append(gp[p] or rb)
            res_o.append(0 if p == 0 else (go[p] or res_o[p - 1] + self.plane_rows[p - 1] * res_p[p - 1]))
            span.append((rows - 1) * res_p[p] + rb)
            if dword and (res_p[p] % 4 or (res_o[p] % 4 and not self.plane_pointers)):
                raise ValueError("FrameLayout: %s surfaces need pitch and plane offset in multiples of 4" % fmt)
            if fmt == "nv12" and p == 1 and (res_p[p] % 2 or (res_o[p] % 2 and not self.plane_pointers)):
                raise ValueError("FrameLayout: the nv12 chroma plane needs an even pitch and offset")
        self.pitch, self.plane_offsets, self.span = tuple(res_p), tuple(res_o), tuple(span)
        self.frame_span = max(o + s for o, s in zip(res_o, span))
        self.frame_stride = gs or max(o + r * q for o, r, q in zip(res_o, self.plane_rows, res_p))
        if dword and self.frame_stride % 4 and not self.plane_pointers:
            raise ValueError("FrameLayout: %s surfaces need a frame stride in multiples of 4" % fmt)
        if fmt == "nv12" and self.frame_stride % 2 and not self.plane_pointers:
            raise ValueError("FrameLayout: nv12 surfaces need an even frame stride")

    def batch_bytes(self, n):
        """Bytes a contiguous batch of ``n`` frames must grant behind its base."""
        return (int(n) - 1) * self.frame_stride + self.frame_span

    def plane_alignment(self, p):
        """Bytes a plane's base pointer must be aligned to (4; 2 for the nv12 CbCr plane)."""
        return 2 if (self.pixel_format == "nv12" and p == 1) else 4

    def _c(self):
        gp, go, gs = self._given
        pad = (0,) * (3 - self.planes)
        return _CLayout(SURFACE_FORMATS[self.pixel_format], int(self.plane_pointers), (ctypes.c_long * 3)(*(gp + pad)),
                        (ctypes.c_long * 3)(*(go + pad)), gs)

    def apply(self, handle, yuv):
        """``lf_pipeline_plan_set_layout`` on a plan handle (and a cross-check of the two restatements of the arithmetic)."""
        coef = yuv_coefficients(yuv)
        lib = _lib.load()
        c = self._c()
        if lib.lf_pipeline_plan_set_layout(handle, ctypes.byref(c), (ctypes.c_int * 6)(*coef)) != 0:
            raise ValueError("lf_pipeline_plan_set_layout failed: %s" % lib.lf_last_error().decode())
        got = tuple(lib.lf_pipeline_surface_span(handle, p) for p in range(self.planes))
        assert got == self.span and lib.lf_pipeline_surface_span(handle, -1) == self.frame_span \
            and lib.lf_pipeline_frame_bytes(handle) == self.frame_stride, "internal: FrameLayout and lf_surface_resolve disagree"

    def check_batch(self, frames, what):
        """A contiguous batch: a contiguous uint8 device tensor of any shape with at least ``batch_bytes(N)`` elements, 4-byte
        aligned; N is not known from the shape, so the caller gives it.  Returns nothing; raises ``ValueError``."""
        if self.plane_pointers:
            raise ValueError("%s: this layout has plane_pointers=True: bind() the surfaces once and pass the SurfaceTable" % what)
        if not torch.is_tensor(frames):
            raise ValueError("%s takes a uint8 tensor, got %s" % (what, type(frames).__name__))
        if not frames.is_cuda:
            raise _lib.LaneFitLibraryError("%s needs its frames on the MI355X; there is no CPU path" % what)
        if frames.dtype != torch.uint8 or not frames.is_contiguous():
            raise ValueError("%s takes a contiguous uint8 tensor, got %s%s" % (what, frames.dtype, "" if frames.is_contiguous() else ", not contiguous"))
        if frames.data_ptr() % 4:
            raise ValueError("%s: the surface's base must be 4-byte aligned" % what)

    def bind(self, surfaces, n=None):
        """N items, each a plane tensor or a tuple of plane tensors -> ``SurfaceTable``.  Each plane: uint8, on the device, at least
        1-D, unit stride inside a row, row stride equal to the layout's pitch (a 1-D tensor is a flat buffer at that pitch), at least
        the plane's span reachable from its first element, base aligned to ``plane_alignment(p)``.  ``n``: the batch it must hold."""
        if not self.plane_pointers:
            raise ValueError("bind() is for a layout with plane_pointers=True; a contiguous layout takes the batch tensor itself")
        items = [tuple(s) if isinstance(s, (tuple, list)) else (s,) for s in surfaces]
        if n is not None and len(items) != n:
            raise ValueError("bind(): %d surface(s) for a batch of %d" % (len(items), n))
        if not items:
            raise ValueError("bind(): no surfaces")
        ptrs, dev = [], None
        for i, planes in enumerate(items):
            if len(planes) != self.planes:
                raise ValueError("bind(): surface %d has %d plane(s), %s has %d" % (i, len(planes), self.pixel_format, self.planes))
            for p, t in enumerate(planes):
                where = "bind(): surface %d plane %d" % (i, p)
                if not torch.is_tensor(t) or t.dtype != torch.uint8 or t.dim() < 1:
                    raise ValueError("%s is not a uint8 tensor" % where)
                if not t.is_cuda:
                    raise _lib.LaneFitLibraryError("%s is not on the MI355X; there is no CPU path" % where)
                dev = dev or t.device
                if t.device != dev:
                    raise ValueError("%s is on another device" % where)
                if t.stride(-1) != 1 and t.shape[-1] > 1:
                    raise ValueError("%s: the bytes of a row are not adjacent (stride %d)" % (where, t.stride(-1)))
                if t.dim() >= 2:
                    lead = t.shape[:-2]
                    if any(s != 1 for s in lead) or (t.shape[-2] > 1 and t.stride(-2) != self.pitch[p]):
                        raise ValueError("%s: row stride %d is not the layout's pitch %d" % (where, t.stride(-2), self.pitch[p]))
                    reach = (t.shape[-2] - 1) * self.pitch[p] + t.shape[-1]
                else:
                    reach = t.shape[0]
                # what the tensor's storage holds behind the first element bounds the reach too
                reach = min(reach, t.untyped_storage().nbytes() - t.storage_offset())
                if reach < self.span[p]:
                    raise ValueError("%s reaches %d bytes, the plane's span is %d" % (where, reach, self.span[p]))
                if t.data_ptr() % self.plane_alignment(p):
                    raise ValueError("%s: base %#x is not %d-byte aligned" % (where, t.data_ptr(), self.plane_alignment(p)))
                ptrs.append(t.data_ptr())
        return SurfaceTable(self, items, torch.tensor(ptrs, dtype=torch.int64).view(len(items), self.planes).to(dev))


class SurfaceTable:
    """What ``bind`` returns: the (N, planes) int64 device tensor of plane base pointers (one small upload, made once -- surface
    pools recycle) and the plane tensors it points into, kept alive.  Pass it where a frames tensor goes."""

    def __init__(self, layout, surfaces, pointers):
        self.layout, self.surfaces, self.pointers = layout, surfaces, pointers
        self.n, self.device, self.is_cuda = len(surfaces), pointers.device, True

    def __len__(self):
        return self.n

    def data_ptr(self):
        return self.pointers.data_ptr()


def _as_layout(layout, frame_hw, pixel_format):
    """Validates the layout= argument of InputPipeline / camera() against their frame_hw and pixel_format."""
    if not isinstance(layout, FrameLayout):
        raise ValueError("layout= takes a pipeline.FrameLayout, got %s" % type(layout).__name__)
    if pixel_format != "rgb":
        raise ValueError("layout= carries the format (%s): leave pixel_format at its default, got pixel_format=%r"
                         % (layout.pixel_format, pixel_format))
    if layout.frame_hw != (int(frame_hw[0]), int(frame_hw[1])):
        raise ValueError("layout= is for frames of %s, frame_hw is %s" % (layout.frame_hw, tuple(frame_hw)))
    return layout


class InputPipeline:
    """``InputPipeline(resize, tree='bev'|'bp', nclasses=2, frame_hw=(720, 1280), crop=640, pixel_format='rgb', yuv='jfif')``;
    ``__call__(frames_u8, labels_u8=None, flip=None) -> (image, gt, horizon)``.

    frames_u8 (N, H, W, 3) uint8 and labels_u8 (N, H, W) uint8 on the GPU; flip (N,) bool (the reference draws
    ``np.random.uniform() > 0.5 and flip_on`` per training sample).  image (N,3,R,2R) fp32, gt (N,1,R,2R) int64,
    horizon (N,R) fp32 for tree='bev' (the BP tree derives its horizon from the lane coordinates on the host).

    ``pixel_format``: what the frames hold -- ``'rgb'`` / ``'bgr'`` (N, H, W, 3), ``'nv12'`` (N, H * 3 // 2, W: the Y plane, then the
    interleaved CbCr rows; H, W even) or ``'yuyv'`` (N, H, W, 2; W even), contiguous.  The image is bit for bit the ``'rgb'`` image of
    the frames the Q16 definition above makes from them (chroma replicated; ``yuv``: ``'jfif'``, ``'bt709'`` or six ints; ignored for
    ``'rgb'`` / ``'bgr'``).  Labels know no format.

    ``layout``: a ``FrameLayout`` -- the frames are decoder surfaces (pitched rows, planes at offsets, a frame stride, ``i420`` /
    ``rgbx`` / ``bgrx``), read where they lie.  The layout carries the format (``pixel_format`` stays at its default; ``yuv`` works
    as above) and ``frames_shape`` is ``None``.  Contiguous layouts take a contiguous uint8 device tensor of ANY shape with at least
    ``layout.batch_bytes(N)`` elements (a decoder's buffer may be larger); N -- with ``index=`` the pool's size -- is ``n=`` of the
    call, else the labels' count, else (without ``index=``) the flips'; with none of them a buffer that has room for one frame only
    is one frame, and a larger one is a ``ValueError``: slack is never taken for frames.  ``plane_pointers`` layouts take the ``SurfaceTable`` of ``pipe.bind(surfaces)``
    (built once; ``index=`` is refused with it).  Same bits as the ``'rgb'`` pipeline on the pixels' RGB frames."""

    def __init__(self, resize, tree="bev", nclasses=2, frame_hw=(720, 1280), crop=640, pixel_format="rgb", yuv="jfif", layout=None):
        assert tree in ("bev", "bp")
        H, W = frame_hw
        self.layout = None if layout is None else _as_layout(layout, (H, W), pixel_format)
        self.frames_shape = frames_shape(pixel_format, -1, (H, W))[1:] if layout is None else None
        yuv_coefficients(yuv)
        lib = _lib.load()
        self.resize, self.tree, self.nclasses, self.frame_hw = resize, tree, nclasses, (H, W)
        self.pixel_format = pixel_format if layout is None else layout.pixel_format
        self.handle = lib.lf_pipeline_plan_create(H, W, H - crop, crop, resize, 2 * resize)
        if not self.handle:
            raise _lib.LaneFitLibraryError("lf_pipeline_plan_create failed: %s" % lib.lf_last_error().decode())
        if layout is None:
            set_plan_format(self.handle, pixel_format, yuv)
        else:
            layout.apply(self.handle, yuv)
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

    def bind(self, surfaces):
        """``layout.bind(surfaces)``: the ``SurfaceTable`` of a ``plane_pointers`` layout, built once."""
        if self.layout is None:
            raise ValueError("bind() is for a pipeline built with layout=FrameLayout(..., plane_pointers=True)")
        return self.layout.bind(surfaces)

    def _surface_pool(self, frames_u8, labels_u8, flip, index, n):
        """The checks of a layout pipeline's frames argument -> the number of frames behind it."""
        lay = self.layout
        if isinstance(frames_u8, SurfaceTable):
            if frames_u8.layout is not lay:
                raise ValueError("this SurfaceTable was bound for another layout")
            if index is not None:
                raise ValueError("index= gathers from a contiguous pool; a SurfaceTable is refused (bind the surfaces in the order wanted)")
            if n is not None and n != frames_u8.n:
                raise ValueError("n=%d, the SurfaceTable holds %d surface(s)" % (n, frames_u8.n))
            return frames_u8.n
        lay.check_batch(frames_u8, "InputPipeline(layout=)")
        if n is None:
            n = labels_u8.shape[0] if labels_u8 is not None else (flip.numel() if flip is not None and index is None else None)
        if n is None:
            # only ONE whole frame fits: no doubt.  A larger buffer may be frames or a decoder's slack -- the caller says which
            if frames_u8.numel() >= lay.batch_bytes(2):
                raise ValueError("InputPipeline(layout=): the tensor holds %d bytes, room for more than one frame (a frame stride is %d): "
                                 "give n= (or labels), a decoder's buffer may be larger than its frames" % (frames_u8.numel(), lay.frame_stride))
            n = 1
        if n < 1 or frames_u8.numel() < lay.batch_bytes(n):
            raise ValueError("InputPipeline(layout=): %d frame(s) need %d bytes, the tensor holds %d" % (max(n, 1), lay.batch_bytes(max(n, 1)), frames_u8.numel()))
        return n

    def __call__(self, frames_u8, labels_u8=None, flip=None, index=None, n=None):
        """``index`` (N,) int64 on the device: ``frames_u8`` / ``labels_u8`` are a resident POOL and batch element n is pool entry
        ``index[n]`` -- gathered inside the kernels (``lf_pipeline_image_indexed``), no copy of the N selected frames first.
        ``n``: layout pipelines only, the frames behind a contiguous surface buffer (see the class)."""
        lib = _lib.load()
        if self.layout is not None:
            pool = self._surface_pool(frames_u8, labels_u8, flip, index, n)
        else:
            if n is not None:
                raise ValueError("n= is for a pipeline with a layout: the frames' shape gives the count")
            if not frames_u8.is_cuda:
                raise _lib.LaneFitLibraryError("InputPipeline needs the decoded frames on the MI355X; there is no CPU path")
            if tuple(frames_u8.shape[1:]) != self.frames_shape or frames_u8.dtype != torch.uint8:
                raise ValueError("this pipeline takes %s frames of shape (N,) + %s, uint8; got %s, %s"
                                 % (self.pixel_format, self.frames_shape, tuple(frames_u8.shape), frames_u8.dtype))
            pool = frames_u8.shape[0]
        (H, W) = self.frame_hw
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
        if self.layout is None:
            frames_u8 = frames_u8.contiguous()
            frames_ptr = _lib.ptr(frames_u8)
        else:
            frames_ptr = ctypes.c_void_p(frames_u8.data_ptr())
        image = torch.empty(N, 3, R, 2 * R, dtype=torch.float32, device=dev)
        if sel is None:
            _lib.check(lib.lf_pipeline_image(self.handle, frames_ptr, N, _lib.ptr(tables), _lib.ptr(fl),
                                             _lib.ptr(image), _lib.stream()), "lf_pipeline_image")
        else:
            _lib.check(lib.lf_pipeline_image_indexed(self.handle, frames_ptr, pool, _lib.ptr(sel), N, _lib.ptr(tables),
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
