"""The ``--clas`` line-type / horizon heads and the inference-side lane decoding.

``Classification`` mirrors BP/Networks/LSQ_layer.py:150-207: four Conv-BatchNorm-ReLU blocks on the encoder output, a
pooling layer, fully connected layers.  The BEV tree's class (BEV/Networks/LSQ_layer.py:170-228) has the same trunk and
the same horizon head but a DIFFERENT line head -- four ``fully_connected_line{1..4}`` ``Linear(128, 3)`` whose outputs
are concatenated to (N, 3, 4), consumed by ``nn.CrossEntropyLoss`` (BEV/main.py:88,252) -- ``ClassificationBEV`` below.
The conv trunk runs as ONE C-ABI call per direction (``lf_convchain_forward`` / ``_backward``) directly on
the NHWC encoder output inside the backbone's workspace; pooling + NCHW flatten is ``lf_poolflat_*``; the
``nn.Linear`` layers are plain library GEMMs.  The trunk follows the storage type of its input: on the bf16 encoder output of
the backbone's ``precision = "bf16"`` it runs in the chain's precision mode 2 (bf16 tensors on the bf16 matrix cores,
``lf_convchain_set_precision``) and pooling reads bf16 (``lf_poolflat_bf16_*``); the features, the ``nn.Linear`` tails and
the head outputs are fp32 in every mode.

``FrozenHead`` is a head's trunk frozen for one input shape -- folded once into a persistent workspace, then the convolution launches
alone per frame (``lf_convchain_infer_fold`` / ``lf_convchain_infer_folded``) -- which ``lsq.LaneDetector`` owns per head; its
``lanes()`` runs everything behind the two trunks, down to the decoded lanes, as ``lf_clas_tail``.

``Projections`` mirrors BP/test.py:128-186 and ``decode_lanes`` fuses ``compute_coordinates`` for all lanes
with the gating of ``test_model`` (BP/test.py:72-88) into one launch (``lf_lane_decode``).

``ProjectionsBEV`` is the BEV tree's counterpart: ``decode_lanes`` is ``write_lsq_results`` (BEV/Dataloader/Load_Data_new.py:334-420,
the tail of ``validate()``, BEV/main.py:445-488) for a batch -- normalised coordinates, every lane gated by the extent of its own
ground-truth lane in the resident label table -- in one launch (``lf_lane_decode_bev``).

``LaneLabels`` holds a TuSimple label file as a resident device table and ``lane_eval`` / ``Projections.score_lanes`` score
decoded lanes against it as ``LaneEval.bench`` does (BP/eval_lane.py:15-57), one wave per image (``lf_lane_eval``).
"""
import ctypes
import json
import os

import numpy as np
import torch
import torch.nn as nn

from . import _lib, geometry, ops


def _ptr_array(tensors):
    arr = (ctypes.c_void_p * len(tensors))()
    for i, t in enumerate(tensors):
        arr[i] = None if t is None else t.data_ptr()
    return arr


class _ChainPlan:
    def __init__(self, N, H, W, channels, ksize):
        lib = _lib.load()
        ch = (ctypes.c_int * len(channels))(*channels)
        ks = (ctypes.c_int * len(ksize))(*ksize)
        self.handle = lib.lf_convchain_plan_create(N, H, W, len(ksize), ch, ks)
        if not self.handle:
            raise _lib.LaneFitLibraryError("lf_convchain_plan_create failed: %s" % lib.lf_last_error().decode())
        self.shape = (N, H, W)
        self.channels = tuple(channels)
        # one plan serves both precision modes (0: fp32 tensors, 2: bf16 tensors); the mode is set per call
        self.ws_bytes = lib.lf_convchain_workspace_bytes_for(self.handle, 0)
        self.ws_bytes_bf16 = lib.lf_convchain_workspace_bytes_for(self.handle, 2)

    def workspace_bytes(self, mode):
        return self.ws_bytes_bf16 if mode == 2 else self.ws_bytes

    def __del__(self):
        try:
            _lib.load().lf_convchain_plan_destroy(self.handle)
        except Exception:
            pass


class _ConvChainFn(torch.autograd.Function):
    """x: (N,H,W,C0) NHWC -> relu(bn_L(conv_L(... relu(bn_1(conv_1(x)))))) NHWC, of x's dtype: fp32 (precision mode 0) or bf16
    (mode 2)."""

    @staticmethod
    def forward(ctx, mod, plan, x, training, *params):
        lib = _lib.load()
        N, H, W = plan.shape
        mode = 2 if x.dtype == torch.bfloat16 else 0
        assert x.dtype in (torch.float32, torch.bfloat16) and x.is_contiguous()
        _lib.check(lib.lf_convchain_set_precision(plan.handle, mode), "lf_convchain_set_precision")
        ws_bytes = plan.workspace_bytes(mode)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
        y = torch.empty(N, H, W, plan.channels[-1], dtype=x.dtype, device=x.device)
        params = [p.detach() for p in params]
        for p in params:
            assert p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()
        bns = mod._batchnorms()
        running = _ptr_array([b for bn in bns for b in (bn.running_mean, bn.running_var)])
        _lib.check(lib.lf_convchain_forward(plan.handle, _lib.ptr(x), _ptr_array(params), _lib.ptr(mod._ptr_table(params)),
                                            running, int(training), float(bns[0].momentum), float(bns[0].eps), _lib.ptr(y),
                                            _lib.ptr(ws), ws_bytes, _lib.stream()), "lf_convchain_forward")
        ctx.plan, ctx.ws, ctx.x, ctx.y, ctx.params, ctx.mode = plan, ws, x, y, params, mode
        ctx.training = int(training)
        return y

    @staticmethod
    def backward(ctx, gy):
        lib = _lib.load()
        plan, params = ctx.plan, ctx.params
        gy = gy.to(ctx.y.dtype).contiguous()
        flat = torch.empty(sum(p.numel() for p in params), dtype=torch.float32, device=gy.device)
        grads, off = [], 0
        for p in params:
            grads.append(flat[off: off + p.numel()].view(p.shape))
            off += p.numel()
        gx = torch.empty_like(ctx.x) if ctx.needs_input_grad[2] else None
        _lib.check(lib.lf_convchain_set_precision(plan.handle, ctx.mode), "lf_convchain_set_precision")      # (plans are shared)
        _lib.check(lib.lf_convchain_backward(plan.handle, _lib.ptr(ctx.x), _lib.ptr(ctx.y), _lib.ptr(gy), _ptr_array(params),
                                             _ptr_array(grads), _lib.ptr(gx), ctx.training, _lib.ptr(ctx.ws),
                                             plan.workspace_bytes(ctx.mode), _lib.stream()), "lf_convchain_backward")
        ctx.ws = None
        return (None, None, gx, None) + tuple(grads)


class _PoolFlatFn(torch.autograd.Function):
    """NHWC (N,H,W,C) fp32 or bf16 -> (N, features) fp32 in NCHW flatten order; mode 0 = MaxPool2d(2,2), 1 = AvgPool2d((1,W))."""

    @staticmethod
    def forward(ctx, y, mode):
        lib = _lib.load()
        N, H, W, C = y.shape
        feat = C * (H // 2) * (W // 2) if mode == 0 else C * H
        out = torch.empty(N, feat, dtype=torch.float32, device=y.device)
        fwd = lib.lf_poolflat_bf16_fwd if y.dtype == torch.bfloat16 else lib.lf_poolflat_fwd
        _lib.check(fwd(_lib.ptr(y), N, H, W, C, mode, _lib.ptr(out), _lib.stream()), "lf_poolflat_fwd")
        ctx.save_for_backward(y)
        ctx.mode = mode
        return out

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        (y,) = ctx.saved_tensors
        N, H, W, C = y.shape
        gy = torch.empty_like(y)
        bwd = lib.lf_poolflat_bf16_bwd if y.dtype == torch.bfloat16 else lib.lf_poolflat_bwd
        _lib.check(bwd(_lib.ptr(y), _lib.ptr(g.contiguous()), N, H, W, C, ctx.mode, _lib.ptr(gy), _lib.stream()),
                   "lf_poolflat_bwd")
        return gy, None


class Classification(nn.Module):
    """``Classification(class_type, size, channels_in, resize)`` with the reference's submodule names, so its
    state_dict loads into / from the reference's."""

    def __init__(self, class_type, size, channels_in, resize):
        super().__init__()
        self.class_type = class_type
        self.conv1 = nn.Conv2d(channels_in, 128, 1, stride=1, padding=0, bias=True)
        self.conv1_bn = nn.BatchNorm2d(128)
        self.conv2 = nn.Conv2d(128, 128, 3, stride=1, padding=1, bias=True)
        self.conv2_bn = nn.BatchNorm2d(128)
        self.conv3 = nn.Conv2d(128, 64, 3, stride=1, padding=1, bias=True)
        self.conv3_bn = nn.BatchNorm2d(64)
        self.conv4 = nn.Conv2d(64, 64, 3, stride=1, padding=1, bias=True)
        self.conv4_bn = nn.BatchNorm2d(64)
        rows, cols = size
        self.size = (rows, cols)
        self.avgpool = nn.AvgPool2d((1, cols))
        self.maxpool = nn.MaxPool2d((2, 2), stride=2)
        if class_type == 'line':
            self.fully_connected1 = nn.Linear(64 * rows * cols // 4, 128)
            self._make_line_heads()
        else:
            self.fully_connected_horizon = nn.Linear(64 * rows, resize)
        self._channels = (channels_in, 128, 128, 64, 64)
        self._plans = {}
        self._ptr_cache = (None, None)
        # eval mode under no_grad: the trunk with its BatchNorms folded in (lf_convchain_infer); opt-in like erfnet.Net's switch
        # (use_inference_engine, or LANEFIT_INFERENCE_ENGINE=1 when the module is built)
        self.inference_engine = os.environ.get("LANEFIT_INFERENCE_ENGINE", "") == "1"

    def _make_line_heads(self):
        """BP: one 4-way head (BP/Networks/LSQ_layer.py:186-187)."""
        self.fully_connected_line1 = nn.Linear(128, 4)

    def _line_logits(self, f):
        return ops.linear(f, self.fully_connected_line1.weight, self.fully_connected_line1.bias)

    def _batchnorms(self):
        return [self.conv1_bn, self.conv2_bn, self.conv3_bn, self.conv4_bn]

    def _trunk_params(self):
        out = []
        for conv, bn in zip((self.conv1, self.conv2, self.conv3, self.conv4), self._batchnorms()):
            out += [conv.weight, conv.bias, bn.weight, bn.bias]
        return out

    def _ptr_table(self, params):
        key = tuple(p.data_ptr() for p in params)
        if self._ptr_cache[0] != key:
            self._ptr_cache = (key, torch.tensor(key, dtype=torch.int64, device=params[0].device))
        return self._ptr_cache[1]

    def _trunk_infer(self, plan, xh):
        """The eval-mode trunk with every BatchNorm folded into its convolution (lf_convchain_infer): nothing saved."""
        lib = _lib.load()
        N, H, W = plan.shape
        mode = 2 if xh.dtype == torch.bfloat16 else 0
        _lib.check(lib.lf_convchain_set_precision(plan.handle, mode), "lf_convchain_set_precision")
        nbytes = lib.lf_convchain_infer_workspace_bytes(plan.handle, mode)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=xh.device)
        y = torch.empty(N, H, W, plan.channels[-1], dtype=xh.dtype, device=xh.device)
        params = [p.detach() for p in self._trunk_params()]
        for p in params:
            assert p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()
        bns = self._batchnorms()
        running = _ptr_array([b for bn in bns for b in (bn.running_mean, bn.running_var)])
        _lib.check(lib.lf_convchain_infer(plan.handle, _lib.ptr(xh), _ptr_array(params), _lib.ptr(self._ptr_table(params)), running,
                                          float(bns[0].eps), _lib.ptr(y), _lib.ptr(ws), nbytes, _lib.stream()), "lf_convchain_infer")
        return y

    def trunk(self, x, folded=None):
        """conv1..conv4 (+BN+ReLU) on a logical-NCHW tensor; returns NHWC (N,H,W,64), bf16 on a bf16 input (the encoder output
        of the backbone's bf16 mode, read in place), fp32 otherwise.  In eval mode with gradients disabled the BatchNorm-folded
        trunk runs when ``inference_engine`` is on (``folded``: override the switch for this call)."""
        if not x.is_cuda:
            raise _lib.LaneFitLibraryError("lanefit Classification needs its input on the MI355X; there is no CPU path")
        xh = x.permute(0, 2, 3, 1)
        if not xh.is_contiguous():           # the backbone hands out channels-last memory: normally a no-op
            xh = xh.contiguous()
        if xh.dtype != torch.bfloat16:
            xh = xh.float()
        N, H, W, C = xh.shape
        assert C == self._channels[0]
        key = (N, H, W)
        if key not in self._plans:
            self._plans[key] = _ChainPlan(N, H, W, self._channels, (1, 3, 3, 3))
        if not self.training and not torch.is_grad_enabled() and (self.inference_engine if folded is None else folded):
            return self._trunk_infer(self._plans[key], xh)
        y = _ConvChainFn.apply(self, self._plans[key], xh, self.training, *self._trunk_params())
        if self.training:
            torch._foreach_add_([m.num_batches_tracked for m in self._batchnorms()], 1)
        return y

    def forward(self, x, folded=None):
        return self._tail(self.trunk(x, folded))

    def frozen(self, N, H, W):
        """This head frozen for (N, H, W, channels_in) NHWC encoder outputs: see ``FrozenHead`` (``lsq.LaneDetector`` owns one per
        head)."""
        return FrozenHead(self, N, H, W)

    def _tail(self, y):
        """Pooling + the fully connected layers on the trunk's NHWC output."""
        if self.class_type == 'line':
            f = _PoolFlatFn.apply(y, 0)
            f = ops.linear(f, self.fully_connected1.weight, self.fully_connected1.bias, relu=True)      # F.relu(fc1(f)), one launch
            return self._line_logits(f)
        f = _PoolFlatFn.apply(y, 1)
        return ops.linear(f, self.fully_connected_horizon.weight, self.fully_connected_horizon.bias)


class FrozenHead:
    """The conv trunk of one ``Classification`` head frozen for one input shape (``lf_convchain_infer_fold`` /
    ``lf_convchain_infer_folded``): a chain plan of its own, ONE persistent workspace with every BatchNorm folded into its
    convolution, the pointer tables and the trunk's output buffer.  ``fold(mode, device)`` does the fold-table upload and the
    fold-and-pack launch (after any change of a parameter, a running statistic or the precision mode); ``run(xh, flags)`` is the
    four convolution launches alone -- no fold, no upload, no allocation -- and returns the NHWC output buffer, which the next
    ``run`` overwrites.  The bits are ``Classification.trunk(folded=True)``'s."""

    def __init__(self, head, N, H, W):
        self.head = head
        self.plan = _ChainPlan(N, H, W, head._channels, (1, 3, 3, 3))
        self.mode = None
        self._ws = self.y = None

    @torch.no_grad()
    def fold(self, mode, device):
        lib, head, plan = _lib.load(), self.head, self.plan
        N, H, W = plan.shape
        self.mode = mode
        _lib.check(lib.lf_convchain_set_precision(plan.handle, mode), "lf_convchain_set_precision")
        self.nbytes = lib.lf_convchain_infer_workspace_bytes(plan.handle, mode)
        dtype = torch.bfloat16 if mode == 2 else torch.float32
        if self._ws is None or self._ws.numel() != self.nbytes or self._ws.device != device:
            self._ws = torch.empty(self.nbytes, dtype=torch.uint8, device=device)
        if self.y is None or self.y.dtype != dtype or self.y.device != device:
            self.y = torch.empty(N, H, W, plan.channels[-1], dtype=dtype, device=device)
        self._params = [p.detach() for p in head._trunk_params()]
        for p in self._params:
            if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()):
                raise _lib.LaneFitLibraryError("lanefit detector() needs the heads' parameters as contiguous fp32 tensors on the "
                                               "MI355X; there is no CPU path")
        bns = head._batchnorms()
        self._running = [b for bn in bns for b in (bn.running_mean, bn.running_var)]
        self._params_dev = torch.tensor([p.data_ptr() for p in self._params], dtype=torch.int64, device=device)
        _lib.check(lib.lf_convchain_infer_fold(plan.handle, _ptr_array(self._params), _lib.ptr(self._params_dev),
                                               _ptr_array(self._running), float(bns[0].eps), _lib.ptr(self._ws), self.nbytes,
                                               _lib.stream()), "lf_convchain_infer_fold")
        self._ptrs = (self.y.data_ptr(), self._ws.data_ptr())

    def run(self, xh, flags):
        """``xh``: the contiguous NHWC input of the plan's shape, fp32 (mode 0) or bf16 (mode 2); ``flags``: LF_INFER_THIN or 0."""
        y, ws = self._ptrs
        _lib.check(_lib.load().lf_convchain_infer_folded(self.plan.handle, xh.data_ptr(), y, ws, self.nbytes, flags, _lib.stream()),
                   "lf_convchain_infer_folded")
        return self.y


class ClassificationBEV(Classification):
    """The BEV tree's ``Classification`` (BEV/Networks/LSQ_layer.py:170-228): same trunk and horizon head; the line
    head is four 3-way classifiers ``fully_connected_line1..4`` (``Linear(128, 3)`` each, :198-205) whose logits are
    stacked to (N, 3, 4) -- class axis 1, lane axis 2 (:218-226) -- for ``nn.CrossEntropyLoss`` (BEV/main.py:88,252).
    The four heads keep their own parameters (``state_dict`` keys of the reference) and run as ONE (128 -> 12) GEMM."""

    def _make_line_heads(self):
        for i in range(1, 5):
            setattr(self, "fully_connected_line%d" % i, nn.Linear(128, 3))

    def _line_logits(self, f):
        heads = [getattr(self, "fully_connected_line%d" % i) for i in range(1, 5)]
        y = torch.stack([ops.linear(f, h.weight, h.bias) for h in heads], 2)      # four (N, 3) GEMVs (lf_linear_fwd) -> (N, 3, 4)
        return y


def resize_coordinates(array):
    """BP/test.py:20-21."""
    return array * 2.5


class Projections:
    """``Projections(options)``: sample heights 160..710 step 10 of the 1280x720 frame mapped into the
    bird's-eye view; ``compute_coordinates(params)`` evaluates one lane's polynomial there and projects
    back (BP/test.py:128-186).  ``decode_lanes`` does all lanes + the test-time gating in one launch."""

    def __init__(self, options):
        M, M_inv = geometry.get_homography(resize=options.resize, no_mapping=False)
        self.M, self.M_inv = torch.from_numpy(M), torch.from_numpy(M_inv)
        self.order = options.order
        if self.order < 0 or self.order > 3:
            raise NotImplementedError(
                'Requested order {} for polynomial fit is not implemented'.format(self.order))
        start, delta = 160, 10
        self.num_heights = (720 - start) // delta
        self.y_d = (torch.arange(start, 720, delta) - 80).double() / 2.5
        self.y_prime = (self.M[1, 1:2] * self.y_d + self.M[1, 2:]) / (self.M[2, 1:2] * self.y_d + self.M[2, 2:])
        self.y_eval = 255 - self.y_prime
        self._minv = (ctypes.c_double * 9)(*[float(v) for v in self.M_inv.double().reshape(-1)])
        self._dev = None

    def _device_consts(self, device):
        if self._dev is None or self._dev[0].device != device:
            self._dev = (self.y_eval.to(device).contiguous(), self.y_prime.double().to(device).contiguous())
        return self._dev

    def _decode(self, beta, line_flag, bound, lo, hi, fill, want_int, out_int=None):
        lib = _lib.load()
        if not beta.is_cuda:
            raise _lib.LaneFitLibraryError("lanefit Projections needs its input on the MI355X; there is no CPU path")
        N, L, K = beta.shape
        assert K == self.order + 1
        beta = beta.double().contiguous()
        y_eval, y_prime = self._device_consts(beta.device)
        S = self.num_heights
        # (out_int: the caller's (N, L, S) int32 rows, written in place; the fp64 copy is then not made)
        x = torch.empty(N, L, S, dtype=torch.float64, device=beta.device) if out_int is None else None
        xi = torch.empty(N, L, S, dtype=torch.int32, device=beta.device) if want_int and out_int is None else out_int
        if out_int is not None:
            assert out_int.is_cuda and out_int.dtype == torch.int32 and tuple(out_int.shape) == (N, L, S)
        if line_flag is not None:
            line_flag = line_flag.float().contiguous()
        if bound is not None:
            bound = bound.to(torch.int32).contiguous()
        _lib.check(lib.lf_lane_decode(_lib.ptr(beta), _lib.ptr(y_eval), _lib.ptr(y_prime), self._minv, 2.5,
                                      _lib.ptr(line_flag), _lib.ptr(bound), lo, hi, fill, N, L, S, self.order,
                                      _lib.ptr(x), _lib.ptr(xi), _lib.stream()), "lf_lane_decode")
        return x, xi

    def compute_coordinates(self, params):
        """params (N, order+1, 1) fp64 -> x coordinates (N, 56) in the 1280-wide frame."""
        x, _ = self._decode(params.reshape(params.size(0), 1, -1), None, None, 1.0, 0.0, -2.0, False)
        return x[:, 0]

    def decode_lanes(self, betas, line_pred=None, horizon_pred=None, out_int=None):
        """``betas``: the per-lane (N, order+1, 1) tensors in model order; ``line_pred`` (N, 4) the rounded
        line-type sigmoid in the dataset's order (re-indexed [1,2,0,3] as test_model does);
        ``horizon_pred`` (N,) int horizon row.  Returns (lanes (N,L,56) fp64, rounded int32 copy) with -2
        wherever test_model writes -2 (BP/test.py:77-88).  ``out_int``: a contiguous (N, L, 56) int32 device tensor (a slice
        of a buffer for the whole test set, say) to receive the rounded lanes in place; the return is then (None, out_int)."""
        beta = torch.stack([b.reshape(b.size(0), -1) for b in betas], 1)
        flag = None if line_pred is None else line_pred[:, [1, 2, 0, 3]][:, : beta.size(1)]
        bound = None
        if horizon_pred is not None:
            bound = torch.div(horizon_pred.to(torch.int64) - 160, 10, rounding_mode='trunc')
        return self._decode(beta, flag, bound, 0.0, 1279.0, -2.0, True, out_int)

    def score_lanes(self, lanes_int, labels, index=None, out=None, bad_index=None):
        """``decode_lanes``' int32 lanes (N, L, 56), read in place -> per-image (N, 3) fp64 accuracy / fp / fn on the device,
        image n against label ``index[n]`` (int32 device tensor; default: label n) of ``labels`` (a ``LaneLabels``), with
        test_model's ``run_time`` of 20.  ``out`` / ``bad_index``: see ``lane_eval``; nothing is read back here."""
        if lanes_int.size(2) != labels.S:
            raise ValueError("score_lanes: lanes of %d samples against labels of %d" % (lanes_int.size(2), labels.S))
        return lane_eval(lanes_int, labels, index=index, out=out, bad_index=bad_index)[0]


class ProjectionsBEV:
    """``ProjectionsBEV(options)``: the lane decoding of the BEV tree's ``write_lsq_results`` (BEV/Dataloader/Load_Data_new.py:334-420)
    on the device.  M / M_inv are the normalised-coordinate homography of the fitting head (``geometry.bev_homography``: the same
    four point pairs); ``options.resize`` gives ``factor = 640 / resize`` of the horizon bound, ``options.nclasses`` the number of
    output rows per image."""

    def __init__(self, options):
        M, M_inv = geometry.bev_homography()
        self.M, self.M_inv = torch.from_numpy(M), torch.from_numpy(M_inv)
        self.resize = options.resize
        self.factor = 640 / options.resize
        self.nclasses = getattr(options, "nclasses", 4)
        self._m = (ctypes.c_double * 9)(*[float(v) for v in M.reshape(-1)])
        self._minv = (ctypes.c_double * 9)(*[float(v) for v in M_inv.reshape(-1)])

    def decode_lanes(self, betas, labels, index=None, line_pred=None, horizon_pred=None, all_branches_ready=False, horizon_on=False,
                     no_ortho=False, out_int=None, bad_index=None):
        """``betas``: the per-lane (N, K, 1) tensors of the model's 9-tuple (K <= 3 coefficients, highest power first; fp32 as the BEV
        model makes them, or fp64), image n decoded against label ``index[n]`` (int32 device tensor; default n) of ``labels`` (a
        ``LaneLabels``).  ``line_pred`` (N, 4): the arg-max over the BEV line head (needed with ``all_branches_ready``);
        ``horizon_pred`` (N, resize): the rounded horizon sigmoid (needed with ``horizon_on`` as well).
        -> (lanes (N, nclasses, S) int32, bad_index): -2 wherever write_lsq_results writes -2, rows past the lanes given all -2.
        ``out_int``: a contiguous (N, nclasses, S) int32 device tensor (a slice of a buffer for the whole validation set, say) written in
        place.  ``bad_index``: as for ``lane_eval`` -- an image whose index lies outside the table gets -2 everywhere and is counted.
        One launch, nothing read back."""
        lib = _lib.load()
        betas = [b for b in betas if b is not None]
        if any(b.dim() < 2 or b.size(1) > 3 for b in betas):
            raise ValueError("ProjectionsBEV.decode_lanes: a lane has more than 3 coefficients (a, b, c)")
        if not betas[0].is_cuda:
            raise _lib.LaneFitLibraryError("lanefit ProjectionsBEV needs its input on the MI355X; there is no CPU path")
        beta = torch.stack([b.reshape(b.size(0), -1) for b in betas], 1)
        if beta.dtype != torch.float32:
            beta = beta.double()
        beta = beta.contiguous()
        N, L, K = beta.shape
        dev = beta.device
        gt, gt_count, hs, h_stride = labels.on(dev)
        M, G = gt.shape[:2]
        S = labels.S
        if L > self.nclasses or L > MAX_LANES:
            raise ValueError("ProjectionsBEV.decode_lanes: %d lanes into %d rows (at most %d lanes)" % (L, self.nclasses, MAX_LANES))
        if all_branches_ready and line_pred is None:
            raise ValueError("ProjectionsBEV.decode_lanes: all_branches_ready needs line_pred")
        if all_branches_ready and horizon_on and horizon_pred is None:
            raise ValueError("ProjectionsBEV.decode_lanes: horizon_on needs horizon_pred")
        if line_pred is not None:
            assert tuple(line_pred.shape) == (N, 4)
            line_pred = line_pred.to(torch.int32).contiguous()
        R = 0
        if horizon_pred is not None:
            assert horizon_pred.dim() == 2 and horizon_pred.size(0) == N
            horizon_pred = horizon_pred.float().contiguous()
            R = horizon_pred.size(1)
        assert index is None or (index.is_cuda and index.dtype == torch.int32 and index.numel() == N and index.is_contiguous())
        lanes = torch.empty(N, self.nclasses, S, dtype=torch.int32, device=dev) if out_int is None else out_int
        assert lanes.is_cuda and lanes.dtype == torch.int32 and tuple(lanes.shape) == (N, self.nclasses, S) and lanes.is_contiguous()
        if bad_index is None:
            bad_index = torch.zeros(1, dtype=torch.int32, device=dev)
        assert bad_index.is_cuda and bad_index.dtype == torch.int32
        _lib.check(lib.lf_lane_decode_bev(_lib.ptr(beta), 0 if beta.dtype == torch.float32 else 1, _lib.ptr(gt), _lib.ptr(gt_count),
                                          _lib.ptr(index), _lib.ptr(hs), h_stride, _lib.ptr(line_pred), _lib.ptr(horizon_pred), R,
                                          self.factor, self._m, self._minv, N, M, L, G, S, K - 1, self.nclasses,
                                          int(bool(all_branches_ready)), int(bool(horizon_on)), int(bool(no_ortho)), _lib.ptr(lanes),
                                          _lib.ptr(bad_index), _lib.stream()), "lf_lane_decode_bev")
        return lanes, bad_index

    def score_lanes(self, lanes_int, labels, index=None, out=None, bad_index=None):
        """``decode_lanes``' int32 lanes, read in place -> per-image (N, 3) fp64 accuracy / fp / fn on the device (``lane_eval`` with
        write_lsq_results' ``run_time`` of 20); nothing is read back here."""
        if lanes_int.size(2) != labels.S:
            raise ValueError("score_lanes: lanes of %d samples against labels of %d" % (lanes_int.size(2), labels.S))
        return lane_eval(lanes_int, labels, index=index, out=out, bad_index=bad_index)[0]


MAX_LANES, MAX_SAMPLES = 8, 256      # lf_lane_eval's limits


class LaneLabels:
    """A TuSimple label file -- one JSON object per line with ``lanes``, ``h_samples`` and ``raw_file`` -- parsed once:
    ``lanes`` (M, G, S) int32 padded with -2, ``counts`` (M) int32, ``h_samples`` (S) when every label has the same heights
    (``shared``) or (M, S) fp64.  S is the first label's, G the file's maximum (at least 1).  ``on(device)`` uploads the table
    once; ``labels`` keeps the parsed dicts (test_model writes its predictions file from them).  ``source``: a path, or the
    parsed dicts."""

    def __init__(self, source):
        if isinstance(source, (str, os.PathLike)):
            with open(source, 'r') as f:
                source = [json.loads(line) for line in f if line.strip()]
        self.labels = list(source)
        if not self.labels:
            raise ValueError("LaneLabels: no labels")
        self.S = S = len(self.labels[0]['h_samples'])
        if S < 1 or S > MAX_SAMPLES:
            raise ValueError("LaneLabels: %d sample heights, the scoring kernel takes 1..%d" % (S, MAX_SAMPLES))
        for i, l in enumerate(self.labels):
            if len(l['h_samples']) != S:
                raise ValueError("LaneLabels: label %d has %d sample heights, the first has %d" % (i, len(l['h_samples']), S))
            if any(len(lane) != S for lane in l['lanes']):
                raise Exception('Format of lanes error.')
            if len(l['lanes']) > MAX_LANES:
                raise ValueError("LaneLabels: label %d has %d lanes, the scoring kernel takes %d" % (i, len(l['lanes']), MAX_LANES))
        self.M = M = len(self.labels)
        self.G = G = max(1, max(len(l['lanes']) for l in self.labels))
        self.lanes = np.full((M, G, S), -2, np.int32)
        self.counts = np.zeros(M, np.int32)
        h = np.zeros((M, S), np.float64)
        for i, l in enumerate(self.labels):
            self.counts[i] = len(l['lanes'])
            if l['lanes']:
                self.lanes[i, :len(l['lanes'])] = _int_coordinates(l['lanes'])
            h[i] = l['h_samples']
        self.shared = bool((h == h[0]).all())
        self.h_samples = h[0].copy() if self.shared else h
        self._dev = None

    def on(self, device):
        """-> (lanes, counts, h_samples, y_stride) on ``device``, uploaded on first use."""
        device = torch.device(device)
        if self._dev is None or self._dev[0].device != device:
            self._dev = (torch.from_numpy(self.lanes).to(device), torch.from_numpy(self.counts).to(device),
                         torch.from_numpy(self.h_samples).to(device), 0 if self.shared else self.S)
        return self._dev

    def rows_by_raw_file(self):
        """``raw_file`` -> row, the last label winning a repeated name as in ``bench_one_submit``'s dict."""
        return {l['raw_file']: i for i, l in enumerate(self.labels)}


def _int_coordinates(lanes):
    """Lane lists -> int32; the scoring kernel is integer-only (TuSimple's coordinates are, and test_model rounds its own)."""
    a = np.asarray(lanes)
    if a.dtype.kind not in 'iu':
        if a.dtype.kind != 'f' or not (a == np.rint(a)).all():
            raise ValueError("lane coordinates must be integers")
    return a.astype(np.int32)


def lane_eval(pred, labels, index=None, pred_count=None, run_time=None, pixel_thresh=20, pt_thresh=0.85, out=None, bad_index=None,
              want_best=False, want_totals=False):
    """``LaneEval.bench`` (BP/eval_lane.py:33-57) for N images in one launch (``lf_lane_eval``): ``pred`` (N, P, S) int32 on the
    device, image n scored against label ``index[n]`` (int32 device tensor; default n) of ``labels`` (a ``LaneLabels``);
    ``pred_count`` (N) int32 (default: P lanes each); ``run_time`` (N) fp32 (default 20).
    -> (per_image (N, 3) fp64 = accuracy, fp, fn; best_acc (N, G) fp64; best_pred (N, G) int32; totals (3) fp64 sums; bad_index),
    the middle three ``None`` unless asked for.  ``out``: an (N, 3) fp64 device tensor to write.  ``bad_index``: an int32 device word
    that counts the images whose index lies outside the table -- they score (0, 0, 1); it is the caller's to read (one is made,
    zeroed, when not given)."""
    lib = _lib.load()
    if not pred.is_cuda:
        raise _lib.LaneFitLibraryError("lanefit lane_eval needs its input on the MI355X; there is no CPU path")
    assert pred.dtype == torch.int32 and pred.dim() == 3 and pred.is_contiguous()
    N, P, S = pred.shape
    dev = pred.device
    gt, gt_count, ys, y_stride = labels.on(dev)
    M, G = gt.shape[:2]
    if S != labels.S:
        raise ValueError("lane_eval: lanes of %d samples against labels of %d" % (S, labels.S))
    for name, t, dtype in (("index", index, torch.int32), ("pred_count", pred_count, torch.int32), ("run_time", run_time, torch.float32)):
        assert t is None or (t.is_cuda and t.dtype == dtype and t.numel() == N and t.is_contiguous()), name
    per_image = torch.empty(N, 3, dtype=torch.float64, device=dev) if out is None else out
    assert per_image.dtype == torch.float64 and tuple(per_image.shape) == (N, 3)
    if bad_index is None:
        bad_index = torch.zeros(1, dtype=torch.int32, device=dev)
    assert bad_index.is_cuda and bad_index.dtype == torch.int32
    best_acc = torch.empty(N, G, dtype=torch.float64, device=dev) if want_best else None
    best_pred = torch.empty(N, G, dtype=torch.int32, device=dev) if want_best else None
    totals = torch.empty(3, dtype=torch.float64, device=dev) if want_totals else None
    _lib.check(lib.lf_lane_eval(_lib.ptr(pred), _lib.ptr(pred_count), _lib.ptr(gt), _lib.ptr(gt_count), _lib.ptr(index), _lib.ptr(ys),
                                y_stride, _lib.ptr(run_time), N, M, P, G, S, float(pixel_thresh), float(pt_thresh),
                                _lib.ptr(per_image), _lib.ptr(best_acc), _lib.ptr(best_pred), _lib.ptr(totals), _lib.ptr(bad_index),
                                _lib.stream()), "lf_lane_eval")
    return per_image, best_acc, best_pred, totals, bad_index


def horizon_row(outputs_horizon):
    """BP/test.py:62-63: sigmoid row votes -> horizon row in the 720-high frame, snapped to the 10 px grid."""
    pred = torch.sigmoid(outputs_horizon).sum(dim=1)
    return (torch.round((resize_coordinates(pred) + 80) / 10) * 10).int()


def line_flags(outputs_line):
    """BP/test.py:64."""
    return torch.round(torch.sigmoid(outputs_line))
