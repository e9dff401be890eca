"""The reference's ``LSQ_layer.Net`` wrappers (backbone -> activation -> row mask -> grid -> WLS),
BEV flavour (normalised coordinates, fp32 betas) and BP flavour (pixel coordinates, fp64 betas).

Reference: BEV/Networks/LSQ_layer.py:231-326, BP/Networks/LSQ_layer.py:210-315.
"""
import ctypes
import weakref
from collections import namedtuple
from math import ceil
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn as nn

from . import erfnet, fit, geometry, ops, pipeline
from .clas import Classification, ClassificationBEV, Projections


def activation_layer(activation='square', no_cuda=False):
    """Returns a callable like the reference's (LSQ_layer.py:43-63); inside ``Net`` the activation is
    fused into the WLS kernel, this exists for API compatibility."""
    table = {'sigmoid': torch.sigmoid, 'relu': torch.relu, 'softplus': nn.functional.softplus,
             'square': lambda x: x ** 2, 'abs': torch.abs, 'none': lambda x: x}
    if activation not in table:
        raise NotImplementedError('Activation type: {} is not implemented'.format(activation))
    return table[activation]


class _LaneFitNet(nn.Module):
    normalised = True
    y_offset = 1.0
    beta_dtype = torch.float32
    max_order = 2
    cholesky_drops_reg = False       # BP only: its --use_cholesky branch is GELS, which has no regulariser
    classification_cls = Classification      # the tree's own --clas head class (the BEV tree's line head differs)
    # detect() of an end_to_end=False model: True = one call (lf_lane_infer_seg) wherever it is not the slower way -- a batch of
    # ONE image keeps the three-step path (engine forward, lf_seg_maps, fit): its fused launch has 16 workgroups per lane, the
    # whole head on that many CUs, and measures 0.7 % behind (profiles/seg_detect_time.json); "always" = the one call at every
    # batch; False = the three-step path.  All give the same bits; tests and timing alternate them in one process.
    fused_seg_detect = True

    def _common_init(self, args, M, backbone_cls):
        self.nclasses = args.nclasses
        self.order = args.order
        if self.order < 0 or self.order > self.max_order:
            raise NotImplementedError(
                'Requested order {} for polynomial fit is not implemented'.format(self.order))
        if getattr(args, "no_cuda", False):
            raise RuntimeError("lanefit: no_cuda=True requested but this implementation has no CPU path")
        out_channels = args.nclasses + int(not args.end_to_end)
        self.net = backbone_cls(layers=args.layers, in_channels=args.channels_in, out_channels=out_channels,
                                pretrained=args.pretrained, pool=args.pool)
        self.activation_name = args.activation_layer
        self.activation = activation_layer(args.activation_layer)
        resize = args.resize
        self.resize = resize
        self.zero_rows = ceil(resize * args.mask_percentage)          # LSQ_layer.py:257
        self.reg_ls = float(args.reg_ls)
        self.use_cholesky = bool(args.use_cholesky)
        self.end_to_end = args.end_to_end
        self.pretrained = args.pretrained
        self.classification_branch = bool(getattr(args, "clas", False))
        if self.classification_branch:
            # LSQ_layer.py:247-254 (BP) / :270-277 (BEV): both heads read the (32, 64) encoder output
            cls = self.classification_cls
            self.line_classification = cls('line', size=(32, 64), channels_in=128, resize=resize).cuda()
            self.horizon_estimation = cls('horizon', size=(32, 64), channels_in=128, resize=resize).cuda()
        self.net.export_encoder_output = self.classification_branch
        # precision mode of the backbone (erfnet.Net.precision): "fp32" unless args.precision says otherwise
        # (in "bf16" the --clas heads run on the bf16 encoder output in place; their line / horizon outputs stay fp32)
        self.net.precision = getattr(args, "precision", "fp32")
        self.check_singular = True      # False: skip the per-step D2H status read; inspect self.last_status
        self.return_masked = True
        self.last_status = None
        # True: an end_to_end=False forward leaves the lane maps and their fit to losses.SegStepCriterion (coefficients and masked
        # come back as None)
        self.defer_seg_fit = False
        # constant (H*W,2) grid, computed once on the host with the reference's fp32 ops
        self._grid_cpu = geometry.projective_grid(resize, 2 * resize, M, self.normalised)
        self._grid = None
        self._theta = None              # BEVNet.set_homography: fit through this homography instead of the constant grid

    def grid_on(self, device):
        if self._grid is None or self._grid.device != device:
            self._grid = self._grid_cpu.to(device)
        return self._grid

    def _heads(self, shared_encoder, end_to_end):
        if end_to_end and self.classification_branch:
            return self.line_classification(shared_encoder), self.horizon_estimation(shared_encoder)
        return None, None

    def _seg_maps(self, output, gt_line=None):
        """Non-end-to-end path: arg-max of the segmentation logits -> per-lane maps valued k at class k (LSQ_layer.py:302-308;
        BP :279-293), the masked rows zeroed (``index_fill``) and, in the BP tree, "Prevent singular matrix" (BP :308-311): lanes
        flagged in ``gt_line`` borrow map [0, 0].  One launch (``lf_seg_maps``), detached, no host read of ``gt_line.sum()``."""
        lanes = 2 if self.nclasses < 3 else 4
        return ops.seg_maps(output, gt_line, self.zero_rows, lanes)

    def _homography(self):
        """What ``BEVNet.set_homography`` was given: the registered Parameter (followed through ``.cuda()`` / ``.to()``), a plain
        tensor, or None."""
        return self._parameters.get("homography", self._theta)

    def _geometry(self, device):
        """The fit's source of coordinates: the constant grid, or the homography of ``set_homography`` for the inline route."""
        theta = self._homography()
        if theta is None:
            return dict(grid=self.grid_on(device))
        return dict(theta=theta if theta.device == device else theta.to(device), normalised=self.normalised)

    def _fit(self, output, end_to_end, gt_line=None):
        if self.defer_seg_fit and not end_to_end:
            return (None, None, None, None), None
        geo = self._geometry(output.device)
        reg = 0.0 if (self.use_cholesky and self.cholesky_drops_reg) else self.reg_ls
        if end_to_end:
            beta, masked, status = fit.fit_lanes(output, geo.pop("grid", None), self.zero_rows, self.order, reg, self.y_offset,
                                                 self.activation_name, self.use_cholesky, self.return_masked,
                                                 self.check_singular, **geo)
        else:
            maps = self._seg_maps(output, gt_line)
            # (the masked rows are zeros already; handing zero_rows to the fit keeps its kernels from reading them at all --
            # at 320 x 640 the BP grid has a pole on a masked row, and 0 * inf is NaN)
            beta, _, status = fit.fit_lanes(maps, geo.pop("grid", None), self.zero_rows, self.order, reg, self.y_offset, "none",
                                            self.use_cholesky, False, self.check_singular, **geo)
            masked = maps
        self.last_status = status
        return fit.split_lanes(beta, self.nclasses, self.beta_dtype), masked


    @torch.no_grad()
    def detect(self, input, gt_line=None):
        """Image -> ``(beta0, beta1, beta2, beta3, line, horizon)``: the fields of ``forward`` that test time consumes
        (``validate()``, BP/test.py:35-88), with ``forward``'s dtypes, shapes and ``None``s, on the inference engine whatever the
        ``inference_engine`` switches say and whatever the caller's grad state.  Eval mode only (the wrapper, its backbone and its heads).

        Either kind of model runs ONE C call from the image to the lane coefficients.  End-to-end models: ``lf_lane_infer`` (the
        backbone's inference schedule, then head + activation + row mask + moments fused -- neither the logits nor the weight maps
        are written) and the ``--clas`` heads with their BatchNorms folded in, on the encoder output inside that call's workspace.
        Segmentation-mode models (``end_to_end=False``): ``lf_lane_infer_seg`` (the same schedule, then head + arg-max + moments
        fused -- neither the class logits nor the lane maps are written), bit for bit the coefficients and statuses of the
        engine-on ``forward``.  ``fused_seg_detect = False`` restores the three-step path (inference-engine forward,
        ``lf_seg_maps``, the fit); a batch of one image keeps it too unless ``fused_seg_detect = "always"`` (the same bits, and
        there the three steps measure 0.7 % faster), and so does a ``pretrained`` model, whose segmentation head is the decoder's
        second one.  ``gt_line`` is what BP's ``forward`` takes for its "prevent singular matrix" borrow (lanes flagged in it fit map
        [0, 0]): pass the same tensor to get ``forward``'s coefficients for such lanes; the default ``None`` borrows nothing, as
        test time has no labels.  ``last_status`` is set; a singular system raises ``RuntimeError`` under ``check_singular`` as in
        ``forward``."""
        self._require_eval_on_device(input, "detect")
        reg = 0.0 if (self.use_cholesky and self.cholesky_drops_reg) else self.reg_ls
        if not self.end_to_end and not self.pretrained and (
                self.fused_seg_detect == "always" or (self.fused_seg_detect and input.shape[0] > 1)):
            beta, _ = self._seg_infer(input, gt_line, False)
            return fit.split_lanes(beta, self.nclasses, self.beta_dtype) + (None, None)
        if not self.end_to_end:
            was = self.net.inference_engine
            self.net.inference_engine = True
            try:
                output = self.net(input, False)[1]       # forward's flag: end_to_end * pretrained = 0 (the segmentation head)
            finally:
                self.net.inference_engine = was
            maps = self._seg_maps(output, gt_line)
            geo = self._geometry(output.device)
            beta, _, status = fit.fit_lanes(maps, geo.pop("grid", None), self.zero_rows, self.order, reg, self.y_offset,
                                            "none", self.use_cholesky, False, self.check_singular, **geo)
            self.last_status = status
            return fit.split_lanes(beta, self.nclasses, self.beta_dtype) + (None, None)
        beta, status, enc = self.net._lane_infer(input, self._detect_grid(input), self.zero_rows, self.order, reg, self.y_offset,
                                                 ops.ACT_KINDS[self.activation_name], self.use_cholesky, self.classification_branch)
        self.last_status = status
        if self.check_singular:
            ops._raise_if_singular(status, 1 if self.use_cholesky else 0)
        line = horizon = None
        if self.classification_branch:
            enc = enc.permute(0, 3, 1, 2)             # logical NCHW, channels-last memory (as Net.forward hands it out)
            line, horizon = self.line_classification(enc, folded=True), self.horizon_estimation(enc, folded=True)
        return fit.split_lanes(beta, self.nclasses, self.beta_dtype) + (line, horizon)

    @torch.no_grad()
    def segment(self, input):
        """Image -> the (N, H, W) uint8 arg-max class map of a segmentation-mode model (``end_to_end=False``; 0 = background, k =
        lane k), from the same one call as ``detect`` (``lf_lane_infer_seg`` with its class map requested: 1 B/pixel, the logits
        are not written).  Eval mode only.  ``last_status`` is set; a singular fit does not raise here."""
        self._require_eval_on_device(input, "segment")
        if self.end_to_end or self.pretrained:
            raise RuntimeError("lanefit segment() is for segmentation-mode models (end_to_end=False, not pretrained): this model's "
                               "head 0 has no class channels")
        return self._seg_infer(input, None, True, check=False)[1]

    def detector(self, batch=1, height=None, width=None, thin="auto"):
        """A frozen ``LaneDetector`` of this model for inputs of ``(batch, channels_in, height, width)`` (``height`` / ``width``
        default to ``resize`` / ``2 * resize``): ``det(frame)`` returns ``detect(frame)``'s results bit for bit with the BatchNorm
        fold done once, at construction.  Eval mode only.  See ``LaneDetector``."""
        return LaneDetector(self, batch, self.resize if height is None else height, 2 * self.resize if width is None else width, thin)

    def _require_eval_on_device(self, input, what):
        # (the wrapper, the backbone and the heads: four flags, not a walk over ~300 modules on every call)
        parts = (self, self.net) + ((self.line_classification, self.horizon_estimation) if self.classification_branch else ())
        if any(m.training for m in parts):
            raise RuntimeError("lanefit %s() needs the model, its backbone and its heads in eval mode (model.eval()): it folds "
                               "the BatchNorm running statistics into the convolutions" % what)
        if not input.is_cuda:
            raise erfnet._lib.LaneFitLibraryError("lanefit %s needs its input on the MI355X; there is no CPU path" % what)

    def _detect_grid(self, input):
        """The grid table the fused calls read: the constant one, or (with a homography set) the per-image grid lf_theta_grid makes
        from it -- the bits of the inline route, ``theta_point`` is shared."""
        if self._homography() is None:
            return self.grid_on(input.device)
        return ops.theta_grid(self._geometry(input.device)["theta"], input.shape[2], input.shape[3], self.normalised)

    def _seg_infer(self, input, gt_line, want_classes, check=None):
        """The one-call segmentation-mode path behind ``detect`` and ``segment``: -> (beta (N,lanes,order+1) fp64, class map)."""
        lanes = 2 if self.nclasses < 3 else 4
        reg = 0.0 if (self.use_cholesky and self.cholesky_drops_reg) else self.reg_ls
        flags = ops.seg_flags(gt_line, input.shape[0], lanes, input.device)
        beta, status, classes = self.net._lane_infer_seg(input, self._detect_grid(input), flags, lanes, self.zero_rows, self.order,
                                                         reg, self.y_offset, self.use_cholesky, want_classes)
        self.last_status = status
        if self.check_singular if check is None else check:
            ops._raise_if_singular(status, 1 if self.use_cholesky else 0)
        return beta, classes


# detector(thin="auto"): the largest batch at which the thin fp32 tap-GEMM route measured faster in-stream than fold-once alone,
# beyond the min-max ranges of both, at 256 x 512 and at 320 x 640 (profiles/detector_latency.json, key thin_auto_max_batch;
# tools/detector_latency.py): it won at 1, 2, 4 and 8, and batch 32 has no launch left for it to take.  0 would mean "auto" = off
THIN_AUTO_MAX_BATCH = 8
# ... and of the thin bf16 route (tapgemm_bf16_thin_kernel) in precision mode bf16, by the same rule (profiles/detector_latency_bf16_thin.json):
# it won at 1, 2 and 4 at both sizes; at 8 it won at 256 x 512 (0.723 against 0.842 ms) and lost at 320 x 640 (1.070 against 0.977 ms)
THIN_AUTO_MAX_BATCH_BF16 = 4
# ... and of the --clas heads' conv trunks inside the detector (lf_convchain_infer_folded with LF_INFER_THIN), per precision mode, by the
# same rule at batch 1, 2, 4 and 8 on the BP recipe at 256 x 512 (tools/detector_latency.py --lanes, profiles/detector_lanes_latency.json,
# key heads_thin_auto_max_batch_by_precision): thin heads won at all four batches in both modes, behind the hand-written tail and
# behind lf_clas_tail alike (fp32 batch 1: 0.665 against 1.025 ms; bf16 batch 8: 1.071 against 1.118 ms).  None would mean "not
# measured": the heads follow the backbone's flag; 0: "auto" never routes them.  thin=True always asks for it
THIN_AUTO_MAX_BATCH_HEADS = 8
THIN_AUTO_MAX_BATCH_HEADS_BF16 = 8

# camera(fused="auto"): the largest batch up to which the fused resize + stem launch (frame_stem_kernel, csrc/lf_frame_stem.hip) measured
# faster in-stream than the two-launch form inside the same call, beyond the min-max ranges of both, at every batch below it too and in
# both geometries, 720 x 1280 -> 256 x 512 (BP --clas, lanes) and -> 320 x 640 (BP 4 lanes, __call__), among 1, 2, 4, 8, 32
# (tools/detector_latency.py --frames, profiles/detector_frames_latency.json, key frame_stem_auto_max_batch_by_precision).  fp32: it
# won at 1, 2, 4 and 8 (one frame 0.684 -> 0.667 ms and 0.785 -> 0.772 ms); at 32 it won at 256 x 512 (5.037 -> 5.025 ms) and the
# ranges overlap at 320 x 640 (7.601 (7.596 - 7.702) against 7.613 (7.607 - 7.617) ms).  0 would mean "auto" = the two-launch form.
# fp32x9 runs the stem launches of fp32 and follows its constant
FRAME_STEM_AUTO_MAX_BATCH = 8
# ... in precision mode bf16 it won at all five batches in both geometries (one frame 0.523 -> 0.508 and 0.559 -> 0.544 ms; 32 frames
# 1.872 -> 1.862 and 1.949 -> 1.898 ms)
FRAME_STEM_AUTO_MAX_BATCH_BF16 = 32
# ... and the frame formats (camera(pixel_format=...)) follow the two constants: a format would get one of its own if its fused form
# were not faster than its own two-launch form beyond both min-max ranges at a batch these route to, and none is
# (tools/detector_latency.py --frames --formats, profiles/detector_frames_formats_latency.json, 720 x 1280 -> 256 x 512, lanes).  bgr,
# nv12 and yuyv won at 1, 2, 4, 8 in fp32 (nv12, one frame: 0.687 (0.687 - 0.687) -> 0.671 (0.670 - 0.671) ms; eight: 1.763 (1.763 -
# 1.764) -> 1.757 (1.756 - 1.757)) and at all five batches in bf16 (nv12, 32 frames: 1.865 (1.864 - 1.865) -> 1.829 (1.828 - 1.829));
# at 32 fp32 frames, where "auto" runs two launches, bgr won and the ranges of nv12 and yuyv overlap

# what LaneDetector.lanes returns
FrameLanes = namedtuple("FrameLanes", ["lanes", "betas", "line", "horizon", "line_flags", "horizon_row"])


class LaneDetector:
    """``model.detector(batch, height, width, thin)``: the model frozen for one input shape -- what a deployment loop calls once
    per camera frame.  ``det(input, gt_line=None)`` returns ``model.detect(input, gt_line)``'s 6-tuple bit for bit (same dtypes,
    shapes and ``None``s; ``model.last_status`` and ``det.last_status`` are set, ``model.check_singular`` raises as in ``detect``),
    ``det.segment(input)`` returns ``model.segment(input)``'s class map for a segmentation-mode model.

    What is done ONCE, at construction and in ``refresh()``, instead of on every call: the engine plan and its precision mode
    (``model.net.precision`` at that time; the detector owns its plan), ONE persistent workspace with every BatchNorm folded into
    the convolution that feeds it (``lf_erfnet_infer_fold``: the fold-table upload and the fold-and-pack launch), the parameter
    and running-buffer pointer tables, and the grid table (the constant grid, or the ``lf_theta_grid`` table of a homography set
    with ``set_homography``).  A call validates the input's shape, allocates ``beta`` and ``status`` and makes one C call
    (``lf_lane_infer_folded``; segmentation-mode models: ``lf_lane_infer_seg_folded`` at every batch size, the bits of
    ``detect``'s three-step path at batch 1 too).  The ``--clas`` heads run as in ``detect``, on the encoder output inside the
    detector's workspace, frozen too: per head the detector owns a chain plan, a persistent workspace folded in ``refresh()``
    (``lf_convchain_infer_fold``), the pointer tables and the trunk's output buffer, and a call runs the four convolution launches
    alone (``lf_convchain_infer_folded``) -- no fold, no upload, no workspace allocation -- with the detector's thin flag.

    ``det.lanes(input, out=None)`` (BP tree, end-to-end, ``--clas``) goes on to what ``BP/test.py`` writes per frame: the 56
    x-coordinates of every lane in the 1280 x 720 frame, gated by the line-type and horizon heads -- the backbone call, the two
    trunks and ONE fused tail (``lf_clas_tail``: pooling, the fully connected layers, ``horizon_row``, ``line_flags`` and
    ``Projections.decode_lanes`` in three launches).

    ``refresh()`` MUST be called after any change of a parameter, a running statistic, the homography or ``model.net.precision``
    (``load_state_dict``, a training step, ``set_homography``, ``.to()``): nothing is checked per call, and what an un-refreshed
    detector returns after such a change is NOT DEFINED (stale weights, or pointers to freed memory).

    ``thin``: ``True`` / ``False`` route / do not route the tap-GEMM launches whose regular grid cannot fill the device to the thin
    kernel of the precision mode (one 16-pixel tile per wave; the same bits): ``tapgemm_thin_kernel`` in ``fp32``,
    ``tapgemm_bf16_thin_kernel`` in ``bf16``; ``"auto"``: on for batches up to ``THIN_AUTO_MAX_BATCH`` (``fp32``) /
    ``THIN_AUTO_MAX_BATCH_BF16`` (``bf16``); the ``--clas`` heads' trunks follow ``thin`` too, ``"auto"`` up to
    ``THIN_AUTO_MAX_BATCH_HEADS`` / ``THIN_AUTO_MAX_BATCH_HEADS_BF16``.  There is no thin kernel for the split operands of
    ``fp32x9``: there the detector gives fold-once only, whatever ``thin`` says.

    The results of a call live in fresh tensors; the workspace is the detector's, so calls of ONE detector must be issued on one
    stream (or ordered by the caller).  Detectors of one model are independent of each other and of ``detect``."""

    def __init__(self, model, batch, height, width, thin="auto"):
        if thin not in (True, False, "auto"):
            raise ValueError("detector(thin=...) takes True, False or \"auto\"")
        if not model.end_to_end and model.pretrained:
            raise RuntimeError("lanefit detector() does not take a pretrained segmentation-mode model (its segmentation head is the "
                               "decoder's second one, which the one-call path does not run): use detect()")
        self.model = model
        self.shape = (int(batch), int(model.net.in_channels), int(height), int(width))
        self.thin = thin
        self.last_status = None
        # False: det(frame) runs the --clas heads as model.detect does (their fold, upload and workspace on every call) -- the same
        # bits; tests and tools/detector_latency.py --lanes alternate the two in one process
        self.frozen_heads = True
        self._plan = erfnet._Plan(self.shape[0], self.shape[2], self.shape[3], model.net.in_channels, model.net.out_channels,
                                  2 if model.net.pretrained else 1)
        self._cameras = weakref.WeakSet()
        self.refresh()

    def camera(self, frame_hw=(720, 1280), crop=640, fused="auto", pixel_format="rgb", yuv="jfif", layout=None):
        """A ``CameraDetector`` on this detector: the same calls from decoded uint8 camera frames ``(batch, Hf, Wf, 3)`` -- the
        reference's ``LaneTestSet`` pixel work (crop the bottom ``crop`` rows, Pillow BILINEAR resize to the detector's
        ``(height, width)``, ``ToTensor``) inside the one backbone C call.  RGB models only.  ``pixel_format``: ``"rgb"``, ``"bgr"``,
        ``"nv12"`` or ``"yuyv"`` frames, ``yuv``: their YCbCr matrix (``"jfif"``, ``"bt709"`` or six ints); ``layout``: a
        ``pipeline.FrameLayout`` -- decoder surfaces (pitch, plane offsets, plane pointers, ``i420`` / ``rgbx`` / ``bgrx``) read where
        they lie.  See ``CameraDetector``."""
        return CameraDetector(self, frame_hw, crop, fused, pixel_format, yuv, layout)

    @torch.no_grad()
    def refresh(self):
        """Fold again and rebuild the pointer tables and the grid table: after ANY change of the model's parameters, running
        statistics, homography or precision mode (see the class docstring: an un-refreshed detector is not defined)."""
        model, net, lib = self.model, self.model.net, erfnet._lib.load()
        self._require_eval()
        N, _, H, W = self.shape
        self._params = [p.detach() for p in net._ordered_params()]
        for p in self._params:
            if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()):
                raise erfnet._lib.LaneFitLibraryError("lanefit detector() needs the model's parameters as contiguous fp32 tensors on "
                                                      "the MI355X; there is no CPU path")
        dev = self._params[0].device
        self._running = net._running_buffers()
        self._params_host = erfnet._ptr_array(self._params)
        self._running_host = erfnet._ptr_array(self._running)
        self._params_dev = torch.tensor([p.data_ptr() for p in self._params], dtype=torch.int64, device=dev)
        self.precision = net.precision
        self._mode = erfnet._PRECISIONS[self.precision]
        erfnet._lib.check(lib.lf_erfnet_set_precision(self._plan.handle, self._mode), "lf_erfnet_set_precision")
        self._seg = not model.end_to_end
        self._lanes = 2 if model.nclasses < 3 else 4
        self._order = int(model.order)
        if self._seg:
            self._nbytes = lib.lf_lane_infer_seg_workspace_bytes(self._plan.handle, self._mode, self._lanes, self._order)
        else:
            self._nbytes = lib.lf_lane_infer_workspace_bytes(self._plan.handle, self._mode, net.out_channels, self._order)
        if self._nbytes == 0:
            raise erfnet._lib.LaneFitLibraryError("lanefit detector(): unsupported mode / lanes / order (%s, %d)"
                                                  % (self.precision, self._order))
        ws = self.__dict__.get("_ws")
        if ws is None or ws.numel() != self._nbytes or ws.device != dev:
            self._ws = torch.empty(self._nbytes, dtype=torch.uint8, device=dev)
        erfnet._lib.check(lib.lf_erfnet_infer_fold(self._plan.handle, self._params_host, erfnet._lib.ptr(self._params_dev),
                                                   self._running_host, erfnet._lib.ptr(self._ws), self._nbytes,
                                                   erfnet._lib.stream()), "lf_erfnet_infer_fold")
        # the grid table of the fused head + fit kernel: the constant grid, or the per-image grid of the homography (_detect_grid)
        if model._homography() is None:
            grid = model.grid_on(dev)
        else:
            grid = ops.theta_grid(model._geometry(dev)["theta"], H, W, model.normalised).detach()
        grid = grid.contiguous()
        if grid.dtype != torch.float32 or tuple(grid.shape[-2:]) != (H * W, 2):
            raise ValueError("lanefit detector(): the model's grid is %s, the detector's shape needs (%d, 2)"
                             % (tuple(grid.shape), H * W))
        self._grid = grid
        self._gstride = H * W * 2 if grid.dim() == 3 and grid.shape[0] > 1 else 0      # (as ops.WLSFit)
        self._reg = 0.0 if (model.use_cholesky and model.cholesky_drops_reg) else float(model.reg_ls)
        self._zero_rows, self._y_offset = int(model.zero_rows), float(model.y_offset)
        self._act, self._chol = int(ops.ACT_KINDS[model.activation_name]), int(bool(model.use_cholesky))
        auto_max = {"fp32": THIN_AUTO_MAX_BATCH, "bf16": THIN_AUTO_MAX_BATCH_BF16}.get(self.precision)
        thin_on = auto_max is not None and (self.thin is True or (self.thin == "auto" and N <= auto_max))
        self._flags = 1 if thin_on else 0          # LF_INFER_THIN
        self._enc = self._heads = self._lanes_state = None
        if model.classification_branch and not self._seg:
            # the NHWC encoder output: a view of the detector's own workspace; _enc is its logical-NCHW form (as Net.forward hands it out)
            self._enc_nhwc = net._infer_encoder_view(self._plan, self._ws, self._mode)
            self._enc = self._enc_nhwc.permute(0, 3, 1, 2)
            auto_heads = {"fp32": THIN_AUTO_MAX_BATCH_HEADS, "bf16": THIN_AUTO_MAX_BATCH_HEADS_BF16}.get(self.precision)
            if self.thin == "auto" and auto_heads is not None:
                self._head_flags = 1 if N <= auto_heads else 0
            else:
                self._head_flags = self._flags        # (thin=True always asks; an unmeasured "auto" follows the backbone)
            if self.__dict__.get("_frozen") is None:
                eh, ew = self._enc_nhwc.shape[1:3]
                self._frozen = tuple(h.frozen(N, eh, ew) for h in (model.line_classification, model.horizon_estimation))
            for f in self._frozen:
                f.fold(2 if self._enc_nhwc.dtype == torch.bfloat16 else 0, dev)
            self._heads = (model.line_classification, model.horizon_estimation)
        self._dev = dev
        self._ptrs = (erfnet._lib.ptr(self._params_dev), erfnet._lib.ptr(self._grid), erfnet._lib.ptr(self._ws))
        for cam in list(self._cameras):
            cam._refold()

    def _require_eval(self):
        model = self.model
        parts = (model, model.net) + ((model.line_classification, model.horizon_estimation) if model.classification_branch else ())
        if any(m.training for m in parts):
            raise RuntimeError("lanefit detector() needs the model, its backbone and its heads in eval mode (model.eval()): it folds "
                               "the BatchNorm running statistics into the convolutions")

    def _input(self, input):
        self._require_eval()
        if tuple(input.shape) != self.shape:
            raise ValueError("this detector was built for inputs of shape %s, got %s" % (self.shape, tuple(input.shape)))
        if not input.is_cuda:
            raise erfnet._lib.LaneFitLibraryError("lanefit detector needs its input on the MI355X; there is no CPU path")
        if input.dtype != torch.float32 or not input.is_contiguous():
            input = input.contiguous().float()
        return input

    def _finish(self, status, check):
        self.last_status = self.model.last_status = status
        if check:
            ops._raise_if_singular(status, self._chol)

    @torch.no_grad()
    def __call__(self, input, gt_line=None):
        x = self._input(input)
        model, N = self.model, self.shape[0]
        if self._seg:
            beta, _ = self._seg_call(x, ops.seg_flags(gt_line, N, self._lanes, self._dev), False, model.check_singular)
            return fit.split_lanes(beta, model.nclasses, model.beta_dtype) + (None, None)
        beta, status = self._backbone(x)
        self._finish(status, model.check_singular)
        line = horizon = None
        if self._enc is not None and not self.frozen_heads:
            line, horizon = model.line_classification(self._enc, folded=True), model.horizon_estimation(self._enc, folded=True)
        elif self._enc is not None:
            line, horizon = (h._tail(f.run(self._enc_nhwc, self._head_flags)) for h, f in zip(self._heads, self._frozen))
        return fit.split_lanes(beta, model.nclasses, model.beta_dtype) + (line, horizon)

    def _backbone(self, x):
        """The backbone call of one frame: -> (beta (N,K,order+1) fp64, status); the encoder output is left in the workspace."""
        model, lib, N = self.model, erfnet._lib.load(), self.shape[0]
        params_dev, grid, ws = self._ptrs
        K = model.net.out_channels
        beta = torch.empty(N, K, self._order + 1, dtype=torch.float64, device=self._dev)
        status = torch.empty(N * K, dtype=torch.int32, device=self._dev)
        erfnet._lib.check(lib.lf_lane_infer_folded(self._plan.handle, x.data_ptr(), self._params_host, params_dev, self._running_host,
                                                   grid, self._gstride, self._zero_rows, self._order, self._reg, self._y_offset,
                                                   self._act, self._chol, None, beta.data_ptr(), status.data_ptr(), ws, self._nbytes,
                                                   self._flags, erfnet._lib.stream()), "lf_lane_infer_folded")
        return beta, status

    def _lanes_setup(self):
        """What ``lanes`` needs beside the heads, built on its first call after a ``refresh()``: the fully connected layers'
        tensors, the sample heights and M_inv of ``Projections``, the fused tail's workspace."""
        model, lib = self.model, erfnet._lib.load()
        if self._enc is None:
            why = ("a segmentation-mode model (end_to_end=False) has no line-type / horizon heads to gate the lanes with" if self._seg
                   else "the model was built without --clas: there are no line-type / horizon heads to gate the lanes with")
            raise RuntimeError("lanefit detector.lanes(): " + why)
        if model.normalised:
            raise RuntimeError("lanefit detector.lanes() is for the BP tree: the BEV tree's lane decoding is gated by ground-truth "
                               "labels (ProjectionsBEV.decode_lanes)")
        line, hor = self._heads
        fc = [t.detach() for t in (line.fully_connected1.weight, line.fully_connected1.bias, line.fully_connected_line1.weight,
                                   line.fully_connected_line1.bias, hor.fully_connected_horizon.weight, hor.fully_connected_horizon.bias)]
        for t in fc:
            if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
                raise erfnet._lib.LaneFitLibraryError("lanefit detector.lanes() needs the heads' parameters as contiguous fp32 tensors "
                                                      "on the MI355X; there is no CPU path")
        proj = Projections(SimpleNamespace(resize=model.resize, order=model.order))
        y_eval, y_prime = proj._device_consts(self._dev)
        N, eh, ew, C = self._frozen[0].y.shape
        O1, R = fc[0].shape[0], fc[4].shape[0]
        nbytes = lib.lf_clas_tail_workspace_bytes(N, eh, ew, C, O1)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=self._dev)
        self._lanes_state = dict(fc=fc, proj=proj, y_eval=y_eval, y_prime=y_prime, ws=ws, nbytes=nbytes, dims=(N, eh, ew, C, O1, R),
                                 S=proj.num_heights)
        return self._lanes_state

    @torch.no_grad()
    def lanes(self, input, out=None):
        """One frame -> ``FrameLanes(lanes, betas, line, horizon, line_flags, horizon_row)``: what ``BP/test.py`` writes per frame.
        ``lanes`` (N, L, 56) int32: the x-coordinates of every lane at the heights 160, 170, .. 710 of the 1280 x 720 frame, -2 where
        ``test_model`` writes -2 (line-type flag 0, above the horizon row, outside the frame); ``out``: a contiguous (N, L, 56) int32
        device tensor of the caller's (a slice of a buffer for the whole test set, say) that receives them in place.  ``betas``
        (the four per-lane tensors), ``line`` (N, 4) and ``horizon`` (N, resize) are ``det(input)``'s, bit for bit;
        ``line_flags`` (N, 4) fp32 is ``clas.line_flags(line)``, ``horizon_row`` (N) int32 ``clas.horizon_row(horizon)`` with the
        sum of sigmoids taken in fp64.  BP-tree end-to-end ``--clas`` models only (``RuntimeError`` otherwise).  ``last_status``
        and ``check_singular`` behave as in ``det(input)``.  The call: ``lf_lane_infer_folded``, two ``lf_convchain_infer_folded``
        and ``lf_clas_tail``."""
        x = self._input(input)
        st = self._lanes_state or self._lanes_setup()
        model, lib = self.model, erfnet._lib.load()
        beta, status = self._backbone(x)
        self._finish(status, model.check_singular)
        y_line, y_hor = (f.run(self._enc_nhwc, self._head_flags) for f in self._frozen)
        N, eh, ew, C, O1, R = st["dims"]
        L, S, dev = beta.shape[1], st["S"], self._dev
        if L > 4:
            raise RuntimeError("lanefit detector.lanes(): %d lanes, the line-type head flags 4" % L)
        line = torch.empty(N, 4, dtype=torch.float32, device=dev)
        horizon = torch.empty(N, R, dtype=torch.float32, device=dev)
        flags = torch.empty(N, 4, dtype=torch.float32, device=dev)
        row = torch.empty(N, dtype=torch.int32, device=dev)
        if out is None:
            out = torch.empty(N, L, S, dtype=torch.int32, device=dev)
        elif not (out.is_cuda and out.dtype == torch.int32 and tuple(out.shape) == (N, L, S) and out.is_contiguous()):
            raise ValueError("detector.lanes(out=...) takes a contiguous (%d, %d, %d) int32 tensor on the device" % (N, L, S))
        w1, b1, wl, bl, wh, bh = st["fc"]
        erfnet._lib.check(lib.lf_clas_tail(y_line.data_ptr(), y_hor.data_ptr(), int(y_line.dtype == torch.bfloat16), N, eh, ew, C,
                                           w1.data_ptr(), b1.data_ptr(), O1, wl.data_ptr(), bl.data_ptr(), wh.data_ptr(), bh.data_ptr(),
                                           R, beta.data_ptr(), L, self._order, st["y_eval"].data_ptr(), st["y_prime"].data_ptr(), S,
                                           st["proj"]._minv, 2.5, 0.0, 1279.0, -2.0, line.data_ptr(), horizon.data_ptr(),
                                           flags.data_ptr(), row.data_ptr(), out.data_ptr(), st["ws"].data_ptr(), st["nbytes"],
                                           erfnet._lib.stream()), "lf_clas_tail")
        return FrameLanes(out, fit.split_lanes(beta, model.nclasses, model.beta_dtype), line, horizon, flags, row)

    @torch.no_grad()
    def segment(self, input):
        """``model.segment(input)``: the (N, H, W) uint8 arg-max class map of a segmentation-mode model, from the folded call."""
        if not self._seg:
            raise RuntimeError("lanefit segment() is for segmentation-mode models (end_to_end=False, not pretrained): this model's "
                               "head 0 has no class channels")
        return self._seg_call(self._input(input), None, True, False)[1]

    def _seg_call(self, x, flags, want_classes, check):
        lib, (N, _, H, W) = erfnet._lib.load(), self.shape
        params_dev, grid, ws = self._ptrs
        beta = torch.empty(N, self._lanes, self._order + 1, dtype=torch.float64, device=self._dev)
        status = torch.empty(N * self._lanes, dtype=torch.int32, device=self._dev)
        classes = torch.empty(N, H, W, dtype=torch.uint8, device=self._dev) if want_classes else None
        erfnet._lib.check(lib.lf_lane_infer_seg_folded(self._plan.handle, x.data_ptr(), self._params_host, params_dev,
                                                       self._running_host, grid, self._gstride, erfnet._lib.ptr(flags), self._lanes,
                                                       self._zero_rows, self._order, self._reg, self._y_offset, self._chol,
                                                       erfnet._lib.ptr(classes), beta.data_ptr(), status.data_ptr(), ws,
                                                       self._nbytes, self._flags, erfnet._lib.stream()), "lf_lane_infer_seg_folded")
        self._finish(status, check)
        return beta, classes


class CameraDetector(LaneDetector):
    """``det.camera(frame_hw=(720, 1280), crop=640, fused="auto")``: a view on a ``LaneDetector`` that starts from what a camera (and
    the reference's ``LaneTestSet.__getitem__``, BP/Dataloader/Load_Data_new.py:55-65) delivers -- decoded uint8 HWC frames.
    ``cam(frames_u8, gt_line=None)``, ``cam.lanes(frames_u8, out=None)`` and ``cam.segment(frames_u8)`` return exactly what
    ``det(x)``, ``det.lanes(x)`` and ``det.segment(x)`` return for ``x = InputPipeline(resize, tree, frame_hw=frame_hw,
    crop=crop)(frames_u8)[0]``: the same tuples and ``FrameLanes``, dtypes, ``None``s, ``last_status`` (on the camera and the model)
    and ``check_singular`` behaviour.  Each is ONE backbone C call (``lf_lane_infer_folded_u8`` / ``lf_lane_infer_seg_folded_u8``);
    no fp32 image tensor is allocated.

    The camera owns its ``lf_pipeline_plan`` (``frame_hw``, ``crop`` -> the detector's ``(height, width)``), the uploaded tables and a
    workspace of its own, folded once like the detector's; everything else (the engine plan, pointer tables, grid, the frozen
    ``--clas`` heads, the thin flags) is the detector's.  ``det.refresh()`` refreshes its cameras too (``cam.refresh()`` is
    ``det.refresh()``): the detector's contract -- refresh after ANY change of the model -- covers them.  Calls of a camera and of
    its detector must be issued on one stream; cameras of one detector are independent of each other (own workspace, fresh results).

    ``cam.fused``: ``True`` -- crop, resize, ``ToTensor`` and the stem in one launch (``frame_stem_kernel``: the resized image
    stays in LDS); ``False`` -- ``resize_bilinear_kernel`` into an image slot of the workspace, then the stem, two launches inside the
    same call; the same bits.  ``"auto"`` (default): fused for batches up to ``FRAME_STEM_AUTO_MAX_BATCH`` (``fp32``, ``fp32x9``) /
    ``FRAME_STEM_AUTO_MAX_BATCH_BF16`` (``bf16``).  A geometry whose source window does not fit the kernel's LDS tile (1280 x 640 ->
    128 x 64) raises ``ValueError`` for ``True`` and runs as two launches for ``"auto"``.

    Input: a contiguous uint8 tensor ``(batch, Hf, Wf, 3)`` on the device (``ValueError`` otherwise; ``LaneFitLibraryError`` for a
    CPU tensor).  Eval mode only, as the detector.

    ``pixel_format`` / ``yuv``: what the frames hold (``pipeline.PIXEL_FORMATS``, ``pipeline.YUV_PRESETS``) -- ``"rgb"`` (default) or
    ``"bgr"`` ``(batch, Hf, Wf, 3)``; ``"nv12"`` ``(batch, Hf * 3 // 2, Wf)``, the Y plane and then the interleaved CbCr rows, as video
    and JPEG decoders write it (``Hf``, ``Wf`` even); ``"yuyv"`` ``(batch, Hf, Wf, 2)``, as USB / CSI cameras deliver it (``Wf`` even).
    ``cam.frame_shape`` is the shape expected.  The staging of the source window converts in registers: chroma replicated, YCbCr ->
    RGB by the Q16 integers of ``yuv`` (``"jfif"``: full-range BT.601, libjpeg's decoder bit for bit; ``"bt709"``: limited-range
    BT.709; or six ints), and EVERY result equals that of an ``"rgb"`` camera on the RGB frames this definition makes
    (include/lanefit.h, "additions since 5 -- frame formats").  Unknown names raise ``ValueError``; ``"auto"`` routes every format
    as ``"rgb"`` (measured per format, see ``FRAME_STEM_AUTO_MAX_BATCH``).

    ``layout``: a ``pipeline.FrameLayout`` for ``frame_hw`` -- the frames are decoder surfaces (include/lanefit.h, "additions since 5
    -- surfaces": pitched rows, planes at offsets or in allocations of their own, a frame stride, ``"i420"`` / ``"rgbx"`` /
    ``"bgrx"``), read where they lie; the same bit contract.  The layout carries the format (a ``pixel_format`` other than the
    default with it is a ``ValueError``), ``yuv`` works as above, ``cam.frame_shape`` is ``None``.  A contiguous layout takes a
    contiguous uint8 device tensor of any shape with at least ``layout.batch_bytes(batch)`` elements (a decoder's buffer may be
    larger).  A ``plane_pointers`` layout takes the ``SurfaceTable`` of ``cam.bind(surfaces)`` -- ``batch`` items, each a plane tensor
    or a tuple of plane tensors, checked and uploaded ONCE (surface pools recycle): calls with the table cost nothing extra.
    ``fused`` / ``"auto"`` behave as for ``"rgb"``."""

    def __init__(self, det, frame_hw=(720, 1280), crop=640, fused="auto", pixel_format="rgb", yuv="jfif", layout=None):
        if type(det) is not LaneDetector:
            raise TypeError("camera() is a method of a LaneDetector")
        lib = erfnet._lib.load()
        det._require_eval()
        if det.shape[1] != 3:
            raise RuntimeError("lanefit camera() needs an RGB model (channels_in = 3): camera frames are (batch, Hf, Wf, 3) uint8, this "
                               "model takes %d channel(s)" % det.shape[1])
        Hf, Wf = int(frame_hw[0]), int(frame_hw[1])
        N, _, H, W = det.shape
        self._det = det
        self.layout = None if layout is None else pipeline._as_layout(layout, (Hf, Wf), pixel_format)
        self.frame_hw = (Hf, Wf)
        self.frame_shape = pipeline.frames_shape(pixel_format, N, (Hf, Wf)) if layout is None else None
        pipeline.yuv_coefficients(yuv)
        self.pixel_format = pixel_format if layout is None else layout.pixel_format
        self.last_status = None
        self._pipe = lib.lf_pipeline_plan_create(Hf, Wf, Hf - int(crop), int(crop), H, W)
        if not self._pipe:
            raise erfnet._lib.LaneFitLibraryError("lf_pipeline_plan_create failed: %s" % lib.lf_last_error().decode())
        self._pipe = ctypes.c_void_p(self._pipe)
        if layout is None:
            pipeline.set_plan_format(self._pipe, pixel_format, yuv)
        else:
            layout.apply(self._pipe, yuv)
        self.fits = bool(lib.lf_pipeline_frame_stem_ok(self._pipe))
        self.fused = fused
        self._tables = self._ws = None
        self._refold()
        det._cameras.add(self)

    def __getattr__(self, name):
        # what the camera does not own is the detector's (the engine plan, pointer tables, grid, heads, flags)
        det = self.__dict__.get("_det")
        if det is None or name.startswith("__"):
            raise AttributeError(name)
        return getattr(det, name)

    def __del__(self):
        try:
            erfnet._lib.load().lf_pipeline_plan_destroy(self._pipe)
        except Exception:
            pass

    @property
    def fused(self):
        return self._fused

    @fused.setter
    def fused(self, value):
        if value not in (True, False, "auto"):
            raise ValueError("camera(fused=...) takes True, False or \"auto\"")
        if value is True and not self.fits:
            raise ValueError("camera(fused=True): the source window of a tile does not fit the fused kernel's LDS budget at %s -> %s; "
                             "use \"auto\" or False (two launches inside the call)" % (self.frame_shape[1:3] if self.frame_shape else self.frame_hw, self._det.shape[2:]))
        self._fused = value

    def camera(self, *args, **kwargs):
        raise RuntimeError("camera() is a method of the LaneDetector, not of one of its cameras")

    def refresh(self):
        """``det.refresh()``: the detector and every camera of it fold again."""
        self._det.refresh()

    @torch.no_grad()
    def _refold(self):
        det, lib = self._det, erfnet._lib.load()
        dev = det._dev
        K = det._lanes if det._seg else det.model.net.out_channels
        query = lib.lf_lane_infer_seg_u8_workspace_bytes if det._seg else lib.lf_lane_infer_u8_workspace_bytes
        self._nbytes = query(det._plan.handle, det._mode, K, det._order)
        if self._nbytes == 0:
            raise erfnet._lib.LaneFitLibraryError("lanefit camera(): unsupported mode / lanes / order (%s, %d)" % (det.precision, det._order))
        if self._tables is None or self._tables.device != dev:
            self._tables = torch.empty(lib.lf_pipeline_table_bytes(self._pipe), dtype=torch.uint8, device=dev)
            erfnet._lib.check(lib.lf_pipeline_upload(self._pipe, erfnet._lib.ptr(self._tables), erfnet._lib.stream()), "lf_pipeline_upload")
        if self._ws is None or self._ws.numel() != self._nbytes or self._ws.device != dev:
            self._ws = torch.empty(self._nbytes, dtype=torch.uint8, device=dev)
        erfnet._lib.check(lib.lf_erfnet_infer_fold(det._plan.handle, det._params_host, erfnet._lib.ptr(det._params_dev),
                                                   det._running_host, erfnet._lib.ptr(self._ws), self._nbytes, erfnet._lib.stream()),
                          "lf_erfnet_infer_fold")
        self._enc = self._enc_nhwc = self._lanes_state = None
        if det._enc is not None:
            self._enc_nhwc = det.model.net._infer_encoder_view(det._plan, self._ws, det._mode)
            self._enc = self._enc_nhwc.permute(0, 3, 1, 2)
        self._ptrs = (erfnet._lib.ptr(det._params_dev), erfnet._lib.ptr(det._grid), erfnet._lib.ptr(self._ws))

    def _u8_flags(self):
        det = self._det
        if self._fused == "auto":
            auto_max = FRAME_STEM_AUTO_MAX_BATCH_BF16 if det.precision == "bf16" else FRAME_STEM_AUTO_MAX_BATCH
            on = self.fits and det.shape[0] <= auto_max
        else:
            on = self._fused
        return det._flags | (0 if on else 2)          # LF_INFER_FRAME_TWO_LAUNCH

    def bind(self, surfaces):
        """``plane_pointers`` layouts: ``batch`` surfaces (a plane tensor or a tuple of plane tensors each) -> the ``SurfaceTable`` the
        calls take.  Every plane is checked here (uint8, on the device, row stride = the layout's pitch, the plane's span reachable,
        base alignment); the table keeps the tensors alive and holds their pointers on the device."""
        if self.layout is None:
            raise ValueError("bind() is for a camera built with layout=FrameLayout(..., plane_pointers=True)")
        return self.layout.bind(surfaces, self._det.shape[0])

    def _input(self, frames):
        self._det._require_eval()
        if self.layout is not None:
            lay, N = self.layout, self._det.shape[0]
            if isinstance(frames, pipeline.SurfaceTable):
                if frames.layout is not lay or frames.n != N:
                    raise ValueError("this SurfaceTable was bound for another layout or batch (%d surface(s), the camera's batch is %d)"
                                     % (frames.n, N))
                return frames
            lay.check_batch(frames, "camera(layout=)")
            if frames.numel() < lay.batch_bytes(N):
                raise ValueError("camera(layout=): %d frame(s) need %d bytes, the tensor holds %d" % (N, lay.batch_bytes(N), frames.numel()))
            return frames
        if tuple(frames.shape) != self.frame_shape:
            raise ValueError("this camera was built for frames of shape %s, got %s" % (self.frame_shape, tuple(frames.shape)))
        if not frames.is_cuda:
            raise erfnet._lib.LaneFitLibraryError("lanefit camera needs its frames on the MI355X; there is no CPU path")
        if frames.dtype != torch.uint8 or not frames.is_contiguous():
            raise ValueError("camera frames are contiguous uint8 %s tensors, got %s%s"
                             % ("(batch, Hf, Wf, 3)" if self.frame_shape[3:] == (3,) else "%s (%s)" % (self.frame_shape, self.pixel_format),
                                frames.dtype, "" if frames.is_contiguous() else ", not contiguous"))
        return frames

    def _backbone(self, x):
        det, lib = self._det, erfnet._lib.load()
        N, K = det.shape[0], det.model.net.out_channels
        params_dev, grid, ws = self._ptrs
        beta = torch.empty(N, K, det._order + 1, dtype=torch.float64, device=det._dev)
        status = torch.empty(N * K, dtype=torch.int32, device=det._dev)
        erfnet._lib.check(lib.lf_lane_infer_folded_u8(det._plan.handle, self._pipe, self._tables.data_ptr(), x.data_ptr(),
                                                      det._params_host, params_dev, det._running_host, grid, det._gstride,
                                                      det._zero_rows, det._order, det._reg, det._y_offset, det._act, det._chol, None,
                                                      beta.data_ptr(), status.data_ptr(), ws, self._nbytes, self._u8_flags(),
                                                      erfnet._lib.stream()), "lf_lane_infer_folded_u8")
        return beta, status

    def _seg_call(self, x, flags, want_classes, check):
        det, lib = self._det, erfnet._lib.load()
        N, _, H, W = det.shape
        params_dev, grid, ws = self._ptrs
        beta = torch.empty(N, det._lanes, det._order + 1, dtype=torch.float64, device=det._dev)
        status = torch.empty(N * det._lanes, dtype=torch.int32, device=det._dev)
        classes = torch.empty(N, H, W, dtype=torch.uint8, device=det._dev) if want_classes else None
        erfnet._lib.check(lib.lf_lane_infer_seg_folded_u8(det._plan.handle, self._pipe, self._tables.data_ptr(), x.data_ptr(),
                                                          det._params_host, params_dev, det._running_host, grid, det._gstride,
                                                          erfnet._lib.ptr(flags), det._lanes, det._zero_rows, det._order, det._reg,
                                                          det._y_offset, det._chol, erfnet._lib.ptr(classes), beta.data_ptr(),
                                                          status.data_ptr(), ws, self._nbytes, self._u8_flags(), erfnet._lib.stream()),
                          "lf_lane_infer_seg_folded_u8")
        self._finish(status, check)
        return beta, classes


class BEVNet(_LaneFitNet):
    """``Net(args)``; ``forward(input, end_to_end) ->
    (beta0, beta1, beta2, beta3, masked, M, output, line, horizon)`` (BEV/Networks/LSQ_layer.py:290-326);
    with ``--clas`` the line output is (N, 3, 4) (four 3-way heads, ``ClassificationBEV``)."""
    classification_cls = ClassificationBEV

    def __init__(self, args):
        super().__init__()
        M, _ = geometry.bev_homography()
        self._common_init(args, M, erfnet.Net)
        self.M = torch.from_numpy(M).unsqueeze(0).expand(args.batch_size, 3, 3).float().cuda()

    def set_homography(self, theta):
        """Fit through ``theta`` -- a (3, 3) or per-image (N, 3, 3) tensor or ``nn.Parameter`` -- instead of the constant grid:
        ``forward`` computes the grid inline from it (``lf_wls_fwd_theta``), returns it in the tuple's ``M`` slot and lets the
        gradient reach it (the reference's ``ProjectiveGridGenerator.forward(M)`` on every step, LSQ_layer.py:84-87,318); ``detect``
        uses it too.  A Parameter is registered as ``homography`` (optimisers and ``state_dict`` see it).  ``None`` restores the
        constant grid."""
        self._parameters.pop("homography", None)
        self._theta = None
        if theta is None:
            return
        if not torch.is_tensor(theta) or theta.dim() not in (2, 3) or tuple(theta.shape[-2:]) != (3, 3):
            raise ValueError("set_homography takes a (3, 3) or (N, 3, 3) tensor, or None")
        if isinstance(theta, nn.Parameter):
            self.register_parameter("homography", theta)
        else:
            self._theta = theta

    def forward(self, input, end_to_end):
        shared_encoder, output = self.net(input, end_to_end * self.pretrained)
        line, horizon = self._heads(shared_encoder, end_to_end)
        (b0, b1, b2, b3), masked = self._fit(output, end_to_end)
        theta = self._homography()
        M = self.M if theta is None else theta
        return b0, b1, b2, b3, masked, M, output, line, horizon


class _BPBackbone(erfnet.Net):
    three_outputs = True


class BPNet(_LaneFitNet):
    """``Net(args)``; ``forward(input, gt_line, end_to_end, early_return=False, gt=None) ->
    (beta0..3, masked, output, line, horizon, output_seg)`` or bare ``output``
    (BP/Networks/LSQ_layer.py:269-315).  Pixel coordinates, ``255 - y``, orders 0..3, fp64 betas."""
    normalised = False
    y_offset = 255.0
    beta_dtype = torch.float64
    max_order = 3
    cholesky_drops_reg = True

    def __init__(self, args):
        super().__init__()
        M, _ = geometry.get_homography(args.resize, getattr(args, "no_mapping", False))
        self._common_init(args, M, _BPBackbone)
        self.net.export_encoder_output = True        # output_seg IS the encoder output in this tree (BP/Networks/ERFNet.py:143-163)

    def forward(self, input, gt_line, end_to_end, early_return=False, gt=None):
        shared_encoder, output, output_seg = self.net(input, end_to_end * self.pretrained)
        if early_return:
            return output
        line, horizon = self._heads(shared_encoder, end_to_end)
        (b0, b1, b2, b3), masked = self._fit(output, end_to_end, gt_line)
        return b0, b1, b2, b3, masked, output, line, horizon, output_seg
