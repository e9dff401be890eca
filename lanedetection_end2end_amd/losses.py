"""Loss modules with the reference's names and call signatures (BEV/Loss_crit.py, BP/Loss_crit.py),
computed by liblanefit_hip.so."""
import collections

import numpy as np
import torch
import torch.nn as nn

from . import _lib, geometry, ops


class polynomial():
    """Trapezoid-rule area metric of the reference (BEV/Loss_crit.py:12-35), vectorised.

    Works on whatever device the coefficients live on (the reference calls it on ``.cpu()``
    tensors after every step, BEV/main.py:273-280; passing GPU tensors removes those syncs).
    """

    def __init__(self, coeffs, a=0, b=0.7, n=100):
        c = coeffs.reshape(coeffs.shape[0], -1)
        self.a1, self.b1, self.c1 = c[:, 0], c[:, 1], c[:, 2]
        self.a, self.b, self.n = a, b, n

    def calc_pol(self, x):
        return self.a1 * x ** 2 + self.b1 * x + self.c1

    def trapezoidal(self, other):
        if self.a1.is_cuda:
            # one launch, no host sync: sums in the reference's order and dtype (lf_trapezoid)
            lib = _lib.load()
            dt = self.a1.dtype if self.a1.dtype in (torch.float32, torch.float64) else torch.float32
            p = torch.stack((self.a1, self.b1, self.c1), 1).to(dt).contiguous()
            q = torch.stack((other.a1, other.b1, other.c1), 1).to(dt).to(p.device).contiguous()
            out = torch.empty(p.shape[0], dtype=dt, device=p.device)
            _lib.check(lib.lf_trapezoid(_lib.ptr(p), _lib.ptr(q), p.shape[0], float(self.a), float(self.b), int(self.n),
                                        int(dt == torch.float64), _lib.ptr(out), _lib.stream()), "lf_trapezoid")
            return out
        # host tensors (the reference calls this on .cpu() copies, BEV/main.py:274-279): same rule, vectorised
        h = float(self.b - self.a) / self.n
        xs = self.a + h * torch.arange(0, self.n + 1, device=self.a1.device, dtype=self.a1.dtype)
        d = (self.calc_pol(xs[:, None]) - other.calc_pol(xs[:, None])).abs()
        w = torch.ones_like(xs)
        w[0] = w[-1] = 0.5
        return (d * w[:, None]).sum(0) * h


class Area_Loss(nn.Module):
    """Integral of the squared x-difference between fitted and ground-truth curves over
    y in [0, 0.7], three weightings; ``forward(params, gt_params, compute=True)``
    (BEV/Loss_crit.py:78-134).  Deviation: when no lane is kept the reference returns the
    Python int 0; this returns a zero tensor (still differentiable, gradient 0)."""

    def __init__(self, order, weight_funct):
        super().__init__()
        if order not in (1, 2):
            raise NotImplementedError('The requested order is not implemented')
        if weight_funct not in ops.WEIGHT_FUNCTS:
            raise NotImplementedError('The requested weight function is not implemented')
        self.order = order
        self.weight_funct = weight_funct

    def forward(self, params, gt_params, compute=True):
        return ops.AreaLossFn.apply(params, gt_params, self.order, ops.WEIGHT_FUNCTS[self.weight_funct])


class MSE_Loss(nn.Module):
    """``--loss_policy mse``: ``nn.MSELoss()`` of ``params.squeeze(-1)`` against ``gt_params`` -- the mean over all
    N x (order + 1) elements (BEV/Loss_crit.py:137-150, BP/Loss_crit.py:147-160); ``forward(params, gt_params, compute=True)``.
    One launch for the loss and its gradient (``lf_mse_loss``); like ``nn.MSELoss`` it wants equal shapes after the squeeze."""

    def __init__(self, options=None):
        super().__init__()

    def forward(self, params, gt_params, compute=True):
        return ops.MSELossFn.apply(params.squeeze(-1), gt_params)


class CrossEntropyLoss2d(nn.Module):
    """Class-weighted pixel cross entropy (BEV/Loss_crit.py:61-75): weights [1, w, w],
    target = targets[:, 0].  ``nclasses`` generalises to BP's [1] + [w]*nclasses (:64)."""

    def __init__(self, weight=None, size_average=True, seg=False, nclasses=2):
        super().__init__()
        w = [1.0] + [float(weight)] * nclasses if seg else [1.0] * (nclasses + 1)
        self.register_buffer("weights", torch.tensor(w, dtype=torch.float32), persistent=False)
        # A label outside [0, C) raises like nn.NLLLoss's device assert does -- and, like it, not inside the offending call:
        # the kernel counts such labels (they carry weight 0); the count of call k is copied to pinned host memory right behind
        # the kernel (``_lib.DeferredRead``) and read at the START of call k + 1 (or by flush()), waiting for that copy's event
        # only -- the loss adds no host sync to the step.  "always": read it in the call itself (one sync per step);
        # False: never (the count stays in ops.CrossEntropy2dFn.last_acc[2]).
        # The LAST call of a loop is inspected by flush(): the mirrors' loops call it after the last batch; train() / eval()
        # on the criterion flush too.
        self.check_targets = True
        self._pending = None

    def flush(self):
        """Raise now if the previous call saw a label outside [0, C)."""
        pend, self._pending = self._pending, None
        if pend is not None:
            acc = pend[0].get()
            if float(acc[2]) != 0.0:
                raise RuntimeError("cross entropy: %d target value(s) outside [0, %d)" % (int(acc[2]), pend[1]))

    def train(self, mode=True):
        self.flush()
        return super().train(mode)

    def forward(self, inputs, targets):
        if targets.dim() == 4:
            targets = targets[:, 0, :, :]
        if self.check_targets:
            self.flush()
        loss = ops.CrossEntropy2dFn.apply(inputs, targets.long(), self.weights, self.check_targets == "always")
        if self.check_targets:
            self._pending = (_lib.DeferredRead(ops.CrossEntropy2dFn.last_acc), inputs.shape[1])
        return loss


class backprojection_loss(nn.Module):
    """MSE in image space after back-projecting 56 sampled curve points through M^-1
    (BP/Loss_crit.py:161-218).  ``forward(params, x_gt, valid_samples) -> (loss, x_cal*valid)``."""

    def __init__(self, options):
        super().__init__()
        M, M_inv = geometry.get_homography(options.resize, getattr(options, "no_mapping", False))
        self.M, self.M_inv = torch.from_numpy(M), np.ascontiguousarray(M_inv, dtype=np.float64)
        order = options.order
        if order < 0 or order > 3:
            raise NotImplementedError(
                'Requested order {} for polynomial fit is not implemented'.format(order))
        y_d = (torch.arange(160, 720, 10) - 80).double() / 2.5           # :170-173 (literal 80 / 2.5)
        y_prime = (M[1, 1] * y_d + M[1, 2]) / (M[2, 1] * y_d + M[2, 2])   # :175
        y_eval = 255 - y_prime                                            # :176 (literal 255)
        Y = torch.stack([y_eval ** (order - j) for j in range(order + 1)], 1)
        dev = "cpu" if getattr(options, "no_cuda", False) else "cuda"
        self.Y = Y.contiguous().to(dev)
        self.y_prime = y_prime.contiguous().to(dev)
        self.order = order

    def forward(self, params, x_gt, valid_samples):
        return ops.BackprojLossFn.apply(params, x_gt, valid_samples, self.Y, self.y_prime, self.M_inv)


StepLoss = collections.namedtuple("StepLoss", "loss loss_fit loss_line loss_horizon acc_line acc_horizon x_cal")


class StepMeters:
    """Device-side ``AverageMeter`` sums of a ``StepCriterion`` (``crit.meters()``): every following call of the criterion adds
    ``update(loss, N)``, ``update(loss_fit, N)``, ``update(acc_line)`` and ``update(acc_horizon)`` inside its launch.  ``read()`` is
    the one host synchronisation: the averages as a dict, and the accumulators start over."""
    names = ("loss", "loss_fit", "acc_line", "acc_horizon")

    def __init__(self):
        self.buf = None

    def on(self, device):
        if self.buf is None or self.buf.device != device:
            self.buf = torch.zeros(8, dtype=torch.float64, device=device)
        return self.buf

    def read(self):
        if self.buf is None:
            return {n: 0.0 for n in self.names}
        v = self.buf.tolist()
        self.buf.zero_()
        return {n: (v[2 * i] / v[2 * i + 1] if v[2 * i + 1] else 0.0) for i, n in enumerate(self.names)}


class StepCriterion(nn.Module):
    """The whole criterion of one training / validation step as one launch: the K lane losses of ``options.loss_policy``, their
    combination (BP: sum / nclasses, BP/main.py:296-305; BEV: sum, with the lane-present mask on lanes 2 and 3, BEV/main.py:223-237),
    the line and horizon head losses, ``loss * weight_fit + (loss_line + loss_horizon) * weight_class`` (BP/main.py:321-326,
    BEV/main.py:247-253) and the two validation accuracies (BP/main.py:491-497, BEV/main.py:421-427) -- values and gradients from
    ``lf_step_loss``, nothing read back to the host.

        BP:   crit(betas, lanes, valid_points, outputs_line=None, outputs_horizon=None, gt_line=None, gt_horizon=None)
        BEV:  crit(betas, params, outputs_line=None, outputs_horizon=None, gt_line=None, gt_horizon=None)

    ``betas`` is the model's 4-tuple (``None`` entries end the lane list); ``lanes`` / ``valid_points`` (N, >=K, 56) with the
    backprojection policy, coefficient targets (N, >=K, order + 1) otherwise.  Returns a ``StepLoss`` of device tensors (``x_cal``: a
    tuple of per-lane (N, S) views, BP with the backprojection policy; else None); fp64 in the BP tree, the coefficients' dtype in
    the BEV tree.  Without the heads the total is the fit loss.  ``meters()`` starts device-side running means.  A line label
    outside [0, 3) (BEV) carries weight 0 and raises one call late or on ``flush()``, as ``CrossEntropyLoss2d`` does."""

    def __init__(self, options, tree):
        super().__init__()
        if tree not in ops.TREES:
            raise ValueError("tree must be 'bp' or 'bev', not %r" % (tree,))
        policy = options.loss_policy
        if policy not in ops.LANE_KINDS or (policy == "backproject" and tree != "bp"):
            raise NotImplementedError('The requested loss criterion is not implemented')
        self.tree, self.loss_policy, self.kind_is_backproject = tree, policy, policy == "backproject"
        self.nclasses = int(options.nclasses)
        self.weight_fit = float(getattr(options, "weight_fit", 1.0))
        self.weight_class = float(getattr(options, "weight_class", 1.0))
        self.weight_funct = getattr(options, "weight_funct", "none")
        self.order = options.order
        self.Y = self.y_prime = self.M_inv = None
        if policy == "backproject":
            bp = backprojection_loss(options)
            self.Y, self.y_prime, self.M_inv = bp.Y, bp.y_prime, bp.M_inv
        elif policy == "area":
            Area_Loss(options.order, self.weight_funct)          # (its checks of order and weight function)
        self.check_targets = True
        self._pending = None
        self._ws = None
        self._meters = None

    def workspace(self, device):
        if self._ws is None or self._ws.device != device:        # zeroed once: every call leaves the ticket at zero
            self._ws = torch.zeros(_lib.load().lf_step_loss_workspace_bytes(), dtype=torch.uint8, device=device)
        return self._ws

    def meter_buffer(self, device):
        return None if self._meters is None else self._meters.on(device)

    def meters(self):
        self._meters = StepMeters()
        return self._meters

    def flush(self):
        """Raise now if the previous call saw a line label outside [0, 3)."""
        pend, self._pending = self._pending, None
        if pend is not None:
            bad = float(pend.get()[6])
            if bad != 0.0:
                raise RuntimeError("cross entropy: %d target value(s) outside [0, %d)" % (int(bad), 3))

    def train(self, mode=True):
        self.flush()
        return super().train(mode)

    def forward(self, betas, *args, **kw):
        names = (("lanes", "valid_points") if self.tree == "bp" else ("params",)) + \
            ("outputs_line", "outputs_horizon", "gt_line", "gt_horizon")
        if len(args) > len(names):
            raise TypeError("StepCriterion: too many arguments")
        a = dict(zip(names, args))
        for k, v in kw.items():
            if k not in names or k in a:
                raise TypeError("StepCriterion: unexpected argument %r" % k)
            a[k] = v
        target = a.get("lanes") if self.tree == "bp" else a.get("params")
        if target is None:
            raise TypeError("StepCriterion: the lane targets are missing")
        lanes = []
        for b in betas:
            if b is None:
                break
            lanes.append(b)
        heads = [a.get(n) for n in names[-4:]]
        if any(h is None for h in heads):
            if any(h is not None for h in heads):
                raise TypeError("StepCriterion: the heads take outputs_line, outputs_horizon, gt_line and gt_horizon together")
            heads = [None] * 4
        line, horizon, gt_line, gt_horizon = heads
        check = self.check_targets and self.tree == "bev" and line is not None
        if self.check_targets:
            self.flush()
        loss, values, xcal = ops.StepLossFn.apply(self, target, a.get("valid_points"), line, gt_line, horizon, gt_horizon, *lanes)
        if check:
            self._pending = _lib.DeferredRead(values)
        if self.tree == "bev" and lanes[0].dtype != torch.float64:      # the BEV loop's loss has the coefficients' dtype
            loss, values = loss.to(lanes[0].dtype), values.to(lanes[0].dtype)
        return StepLoss(loss, values[1], values[2], values[3], values[4], values[5],
                        None if xcal is None else tuple(xcal.unbind(1)))


SegStepLoss = collections.namedtuple("SegStepLoss", "loss metric betas status maps")


class SegStepMeters:
    """Device-side running means of a ``SegStepCriterion`` (``crit.meters()``): ``update(loss, N)`` inside every following call's
    finish launch, ``update(metric, N)`` inside its ``lf_step_loss`` launch.  ``read()`` is the one host synchronisation: the two
    averages as a dict, and the accumulators start over."""
    names = ("loss", "metric")

    def __init__(self, step_meters):
        self.buf = None
        self.step = step_meters

    def on(self, device):
        if self.buf is None or self.buf.device != device:
            self.buf = torch.zeros(2, dtype=torch.float64, device=device)
        return self.buf

    def read(self):
        bufs = [b for b in (self.buf, self.step.buf) if b is not None]
        if not bufs:
            return {n: 0.0 for n in self.names}
        v = torch.cat([b[:2] for b in bufs]).tolist()            # one copy, one synchronisation
        for b in bufs:
            b.zero_()
        res, k = {}, 0
        for n, b in zip(self.names, (self.buf, self.step.buf)):
            res[n] = 0.0
            if b is not None:
                res[n] = v[k] / v[k + 1] if v[k + 1] else 0.0
                k += 2
        return res


class SegStepCriterion(nn.Module):
    """The criterion of an ``end_to_end=False`` step -- ``criterion_seg(output_net, gt)`` with its gradient, the arg-max lane maps,
    their fit and the lane metric the loops compute under ``no_grad`` (BP/main.py:306-318, :470-482; BEV/main.py:241-244, :413-415)
    -- in one pass over the logits (``lf_seg_step``) and one ``lf_step_loss`` launch, nothing read back to the host.  Use it with
    ``model.defer_seg_fit = True`` (the forward then leaves the maps and the fit to this call).

        BP :  crit(output_net, gt, lanes, valid_points, gt_line=None, fit=True) -> SegStepLoss
        BEV:  crit(output_net, gt, params, fit=True)                            -> SegStepLoss

    ``SegStepLoss`` is ``(loss, metric, betas, status, maps)``: ``loss`` the fp64 cross-entropy scalar (class weights
    ``[1] + [weight_seg] * nclasses``, as ``CrossEntropyLoss2d``) and the only field with a gradient; ``betas`` the reference's
    4-tuple with the tree's dtypes; ``metric`` the BP tree's ``(sum of lane losses) / nclasses`` or the BEV tree's sum of the two lane
    losses, from one ``StepCriterion`` call on ``betas``; ``maps`` None unless ``return_maps``.  ``fit=False`` is the ``skip`` /
    ``early_return=True`` case: cross entropy only, the other fields None.  The fit's geometry (grid or ``set_homography``'s theta
    through ``ops.theta_grid``, ``zero_rows``, ``order``, ``reg_ls``, ``use_cholesky``, ``y_offset``) is read from ``model`` at call
    time.  ``meters()`` starts device-side running means.  A label outside [0, C) carries weight 0 and raises one call late or on
    ``flush()`` (``check_targets`` as on ``CrossEntropyLoss2d``); ``check_singular=True`` reads ``status`` and raises as ``forward``
    does, ``False`` leaves it in ``last_status`` without a synchronisation."""

    def __init__(self, options, model):
        super().__init__()
        from . import lsq
        self._model = (model,)                     # (in a tuple: the criterion's train() / cuda() must not reach the model)
        self.tree = "bp" if isinstance(model, lsq.BPNet) else "bev"
        self.nclasses = int(options.nclasses)
        nw = self.nclasses if self.tree == "bp" else 2           # define_loss_crit: the BEV tree's criterion_seg has three weights
        self.register_buffer("weights", torch.tensor([1.0] + [float(options.weight_seg)] * nw, dtype=torch.float32),
                             persistent=False)
        self.step = StepCriterion(options, self.tree)
        self.check_targets = True
        self.check_singular = True
        self.return_maps = False
        self.last_status = None
        self._pending = None
        self._ws = None
        self._meters = None
        # the fit's constants, refreshed from the model by every call
        self.lanes, self.order, self.zero_rows, self.reg, self.y_offset, self.solver = 2, options.order, 0, 0.0, 1.0, 0

    def workspace(self, device, nbytes):
        if self._ws is None or self._ws.device != device or self._ws.numel() != nbytes:      # zeroed once: lf_seg_step leaves the label counts at zero
            self._ws = torch.zeros(nbytes, dtype=torch.uint8, device=device)
        return self._ws

    def meter_buffer(self, device):
        return None if self._meters is None else self._meters.on(device)

    def meters(self):
        self._meters = SegStepMeters(self.step.meters())
        return self._meters

    def flush(self):
        """Raise now if the previous call saw a label outside [0, C)."""
        pend, self._pending = self._pending, None
        if pend is not None:
            bad = float(pend[0].get()[3])
            if bad != 0.0:
                raise RuntimeError("cross entropy: %d target value(s) outside [0, %d)" % (int(bad), pend[1]))

    def train(self, mode=True):
        self.flush()
        return super().train(mode)

    def forward(self, output_net, gt, *args, **kw):
        names = (("lanes", "valid_points", "gt_line") if self.tree == "bp" else ("params",)) + ("fit",)
        if len(args) > len(names):
            raise TypeError("SegStepCriterion: too many arguments")
        a = dict(zip(names, args))
        for k, v in kw.items():
            if k not in names or k in a:
                raise TypeError("SegStepCriterion: unexpected argument %r" % k)
            a[k] = v
        fit = bool(a.get("fit", True))
        model = self._model[0]
        if gt.dim() == 4:
            gt = gt[:, 0, :, :]
        if self.check_targets:
            self.flush()
        grid = flags = None
        if fit:
            target = a.get("lanes") if self.tree == "bp" else a.get("params")
            if target is None:
                raise TypeError("SegStepCriterion: the lane targets are missing (or pass fit=False)")
            N, _, H, W = output_net.shape
            self.lanes = 2 if model.nclasses < 3 else 4
            self.order, self.zero_rows, self.y_offset = model.order, model.zero_rows, model.y_offset
            self.reg = 0.0 if (model.use_cholesky and model.cholesky_drops_reg) else model.reg_ls
            self.solver = 1 if model.use_cholesky else 0
            theta = model._homography()
            grid = model.grid_on(output_net.device) if theta is None else \
                ops.theta_grid(theta.detach().to(output_net.device), H, W, model.normalised)
            gt_line = a.get("gt_line")
            if gt_line is not None:
                flags = gt_line.to(device=output_net.device, dtype=torch.float32).contiguous()
                if tuple(flags.shape) != (N, self.lanes):
                    # (as ops.seg_maps: the reference's expand_as fails here, but only when gt_line.sum() != 0 lets it get that far)
                    if float(flags.sum()) != 0:
                        raise RuntimeError("seg-mode fit: gt_line %s cannot be expanded to the (%d, %d) lane maps"
                                           % (tuple(flags.shape), N, self.lanes))
                    flags = None
        want_grad = torch.is_grad_enabled() and output_net.requires_grad
        loss, out, beta, status, maps = ops.SegStepFn.apply(self, output_net, gt.long(), grid, flags, want_grad)
        if self.check_targets == "always":
            bad = float(out[3])
            if bad != 0.0:
                raise RuntimeError("cross entropy: %d target value(s) outside [0, %d)" % (int(bad), output_net.shape[1]))
        elif self.check_targets:
            self._pending = (_lib.DeferredRead(out), output_net.shape[1])
        if not fit:
            return SegStepLoss(loss, None, None, None, None)
        self.last_status = status
        if self.check_singular:
            ops._raise_if_singular(status, self.solver)
        from . import fit as fit_mod
        betas = fit_mod.split_lanes(beta, model.nclasses, model.beta_dtype)
        with torch.no_grad():
            if self.tree == "bp":
                metric = self.step(betas, target, a.get("valid_points")).loss
            else:
                metric = self.step(betas[:2] + (None, None), target).loss
        return SegStepLoss(loss, metric, betas, status, maps)


def define_loss_crit_bev(options):
    """BEV/Loss_crit.py:45-58."""
    if options.loss_policy == 'mse':
        crit = MSE_Loss(options)
    elif options.loss_policy == 'area':
        crit = Area_Loss(options.order, options.weight_funct)
    else:
        return NotImplementedError('The requested loss criterion is not implemented')
    seg = CrossEntropyLoss2d(options.weight_seg, seg=True)
    return crit, (seg if getattr(options, "no_cuda", False) else seg.cuda())


def define_loss_crit_bp(options):
    """BP/Loss_crit.py:47-67."""
    if options.loss_policy == 'mse':
        crit = MSE_Loss(options)
    elif options.loss_policy == 'backproject':
        crit = backprojection_loss(options)
    elif options.loss_policy == 'area':
        crit = Area_Loss(options.order, options.weight_funct)
    else:
        return NotImplementedError('The requested loss criterion is not implemented')
    seg = CrossEntropyLoss2d(options.weight_seg, seg=True, nclasses=options.nclasses)
    return crit, (seg if getattr(options, "no_cuda", False) else seg.cuda())
