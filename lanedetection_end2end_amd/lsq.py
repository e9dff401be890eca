"""The reference's ``LSQ_layer.Net`` wrappers (backbone -> activation -> row mask -> grid -> WLS),
BEV flavour (normalised coordinates, fp32 betas) and BP flavour (pixel coordinates, fp64 betas).

Reference: BEV/Networks/LSQ_layer.py:231-326, BP/Networks/LSQ_layer.py:210-315.
"""
from math import ceil

import numpy as np
import torch
import torch.nn as nn

from . import erfnet, fit, geometry, ops
from .clas import Classification, ClassificationBEV


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
