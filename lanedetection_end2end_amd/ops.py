"""torch.autograd.Function wrappers around the C ABI (fitting head and losses).

Each Function only marshals pointers: all arithmetic happens in liblanefit_hip.so.
"""
import ctypes

import torch

from . import _lib, geometry

ACT_KINDS = {"square": 0, "abs": 1, "relu": 2, "sigmoid": 3, "softplus": 4, "none": 5}
WEIGHT_FUNCTS = {"none": 0, "linear": 1, "quadratic": 2}


class SingularMatrixError(RuntimeError):
    """Raised like torch.inverse's error so `except RuntimeError` in the reference's main.py
    (BEV/main.py:213-219) keeps skipping the batch."""


def _raise_if_singular(status, solver):
    bad = int(status.max().item())       # D2H sync, by design: the reference raises synchronously
    if bad:
        idx = int((status != 0).nonzero()[0, 0])
        if bad == 2:
            raise SingularMatrixError("lanefit WLS: normal matrix of (image,lane) #%d is not positive-definite "
                                      "(Cholesky/GELS path)" % idx)
        raise SingularMatrixError("lanefit WLS: normal matrix of (image,lane) #%d is singular, the inversion "
                                  "could not be completed" % idx)


def _fit_outputs(lib, logits, order, want_masked):
    """The tensors a fit forward writes: -> (beta, zinv, status, masked | None, workspace)."""
    (N, K), D, dev = logits.shape[:2], order + 1, logits.device
    return (torch.empty(N, K, D, dtype=torch.float64, device=dev), torch.empty(N, K, D * D, dtype=torch.float64, device=dev),
            torch.empty(N * K, dtype=torch.int32, device=dev), torch.empty_like(logits) if want_masked else None,
            torch.empty(lib.lf_wls_workspace_bytes(N, K, order), dtype=torch.uint8, device=dev))


def _fit_finish(ctx, saved, status, masked, solver, check):
    """After the forward call of either fit Function: raise on a singular system, save, mark what has no gradient."""
    if check:
        _raise_if_singular(status, solver)
    ctx.save_for_backward(*saved)
    ctx.status = status
    # (no zero tensors for the outputs nobody differentiates: autograd otherwise fills an (N, K, H, W) fp32 gradient for `masked`
    # every step -- 205 MB, 27 us at config 3)
    ctx.set_materialize_grads(False)
    if masked is not None:
        ctx.mark_non_differentiable(masked)


class WLSFit(torch.autograd.Function):
    """(logits NCHW fp32, grid (P,2)|(N,P,2) fp32) -> beta (N,K,order+1) fp64 [, masked (N,K,H,W) fp32]."""

    @staticmethod
    def forward(ctx, logits, grid, zero_rows, order, reg, y_offset, act_kind, solver, want_masked, check):
        logits = logits.contiguous()
        assert logits.dtype == torch.float32 and logits.dim() == 4
        N, K, H, W = logits.shape
        grid = grid.contiguous()
        assert grid.dtype == torch.float32 and grid.shape[-2:] == (H * W, 2), (grid.shape, H, W)
        gbs = H * W * 2 if grid.dim() == 3 and grid.shape[0] > 1 else 0
        if grid.dim() == 3 and grid.shape[0] > 1:
            assert grid.shape[0] >= N
        lib = _lib.load()
        beta, zinv, status, masked, ws = _fit_outputs(lib, logits, order, want_masked)
        _lib.check(lib.lf_wls_fwd(_lib.ptr(logits), _lib.ptr(grid), gbs, N, K, H, W, zero_rows, order, float(reg),
                                  float(y_offset), act_kind, solver, _lib.ptr(beta), _lib.ptr(zinv),
                                  _lib.ptr(masked), _lib.ptr(ws), _lib.ptr(status), _lib.stream()), "lf_wls_fwd")
        ctx.cfg = (gbs, zero_rows, order, float(y_offset), act_kind)
        _fit_finish(ctx, (logits, grid, beta, zinv), status, masked, solver, check)
        return beta, masked, status

    @staticmethod
    def backward(ctx, gbeta, _gm, _gs):
        lib = _lib.load()
        logits, grid, beta, zinv = ctx.saved_tensors
        gbs, zero_rows, order, y_offset, act_kind = ctx.cfg
        N, K, H, W = logits.shape
        want_grid = ctx.needs_input_grad[1]
        if gbeta is None:          # (the coefficients were not used downstream)
            return (torch.zeros_like(logits), torch.zeros_like(grid) if want_grid else None) + (None,) * 8
        gbeta = gbeta.to(torch.float64).contiguous()
        gl = torch.empty_like(logits)
        _lib.check(lib.lf_wls_bwd(_lib.ptr(logits), _lib.ptr(grid), gbs, N, K, H, W, zero_rows, order, y_offset,
                                  act_kind, _lib.ptr(beta), _lib.ptr(zinv), _lib.ptr(gbeta), _lib.ptr(gl),
                                  _lib.stream()), "lf_wls_bwd")
        gg = None
        if want_grid:              # (a shared grid -- (P, 2) or (1, P, 2) -- collects every image and lane)
            gg = torch.empty_like(grid)
            if gbs and grid.shape[0] > N:          # (grids of images beyond the batch took no part)
                gg[N:].zero_()
            _lib.check(lib.lf_wls_bwd_grid(_lib.ptr(logits), _lib.ptr(grid), gbs, N, K, H, W, zero_rows, order, y_offset,
                                           act_kind, _lib.ptr(beta), _lib.ptr(zinv), _lib.ptr(gbeta), _lib.ptr(gg),
                                           _lib.stream()), "lf_wls_bwd_grid")
        return gl, gg, None, None, None, None, None, None, None, None


def _theta32(theta, N=None):
    """theta (3,3) | (1,3,3) | (N,3,3) of any float dtype -> (contiguous fp32 tensor, batch stride 0 | 9, number of matrices)."""
    if theta.dim() not in (2, 3) or tuple(theta.shape[-2:]) != (3, 3):
        raise ValueError("lanefit: a homography is (3, 3) or (N, 3, 3), got %s" % (tuple(theta.shape),))
    n = theta.shape[0] if theta.dim() == 3 else 1
    if N is not None and n not in (1, N):
        raise ValueError("lanefit: %d homographies for a batch of %d" % (n, N))
    return theta.detach().to(torch.float32).contiguous(), (9 if n > 1 else 0), n


class ThetaGrid(torch.autograd.Function):
    """theta (3,3) | (N,3,3) -> grid (1 | N, H*W, 2) fp32 (``lf_theta_grid``); backward = the theta reduction of
    ``lf_theta_grid_bwd`` on the incoming grid gradient, cast to theta's dtype."""

    @staticmethod
    def forward(ctx, theta, H, W, normalised):
        lib = _lib.load()
        t32, tbs, n = _theta32(theta)
        xs, ys = geometry.base_tables_on(t32.device, H, W, normalised)
        grid = torch.empty(n, H * W, 2, dtype=torch.float32, device=t32.device)
        _lib.check(lib.lf_theta_grid(_lib.ptr(t32), tbs, _lib.ptr(xs), _lib.ptr(ys), n, H, W, _lib.ptr(grid), _lib.stream()),
                   "lf_theta_grid")
        ctx.save_for_backward(t32, xs, ys)
        ctx.cfg = (tbs, n, H, W, theta.shape, theta.dtype)
        return grid

    @staticmethod
    def backward(ctx, ggrid):
        lib = _lib.load()
        t32, xs, ys = ctx.saved_tensors
        tbs, n, H, W, shape, dtype = ctx.cfg
        ggrid = ggrid.to(torch.float32).contiguous()
        gt = torch.empty(n, 3, 3, dtype=torch.float64, device=t32.device)
        ws = torch.empty(lib.lf_theta_grid_bwd_workspace_bytes(n), dtype=torch.uint8, device=t32.device)
        _lib.check(lib.lf_theta_grid_bwd(_lib.ptr(t32), tbs, _lib.ptr(xs), _lib.ptr(ys), _lib.ptr(ggrid), n, H, W, _lib.ptr(gt),
                                         _lib.ptr(ws), _lib.stream()), "lf_theta_grid_bwd")
        return gt.view(shape).to(dtype), None, None, None


def theta_grid(theta, H, W, normalised=True):
    """The projective grid of ``theta`` on the device: (1, H*W, 2) for a (3,3) theta, (N, H*W, 2) for (N,3,3); differentiable."""
    return ThetaGrid.apply(theta, int(H), int(W), bool(normalised))


class WLSFitTheta(torch.autograd.Function):
    """``WLSFit`` with the grid computed inline from a homography: (logits NCHW fp32, theta (3,3) | (N,3,3)) -> the same outputs.
    Backward writes the logits gradient and the theta gradient in one pass (``lf_wls_bwd_theta``); no grid tensor exists."""

    @staticmethod
    def forward(ctx, logits, theta, normalised, zero_rows, order, reg, y_offset, act_kind, solver, want_masked, check):
        logits = logits.contiguous()
        assert logits.dtype == torch.float32 and logits.dim() == 4
        N, K, H, W = logits.shape
        t32, tbs, n = _theta32(theta, N)
        xs, ys = geometry.base_tables_on(logits.device, H, W, normalised)
        lib = _lib.load()
        beta, zinv, status, masked, ws = _fit_outputs(lib, logits, order, want_masked)
        _lib.check(lib.lf_wls_fwd_theta(_lib.ptr(logits), _lib.ptr(t32), tbs, _lib.ptr(xs), _lib.ptr(ys), N, K, H, W, zero_rows,
                                        order, float(reg), float(y_offset), act_kind, solver, _lib.ptr(beta), _lib.ptr(zinv),
                                        _lib.ptr(masked), _lib.ptr(ws), _lib.ptr(status), _lib.stream()), "lf_wls_fwd_theta")
        ctx.cfg = (tbs, n, zero_rows, order, float(y_offset), act_kind, theta.shape, theta.dtype)
        _fit_finish(ctx, (logits, t32, xs, ys, beta, zinv), status, masked, solver, check)
        return beta, masked, status

    @staticmethod
    def backward(ctx, gbeta, _gm, _gs):
        lib = _lib.load()
        logits, t32, xs, ys, beta, zinv = ctx.saved_tensors
        tbs, n, zero_rows, order, y_offset, act_kind, tshape, tdtype = ctx.cfg
        N, K, H, W = logits.shape
        want_theta = ctx.needs_input_grad[1]
        if gbeta is None:          # (the coefficients were not used downstream)
            return (torch.zeros_like(logits),
                    torch.zeros(tshape, dtype=tdtype, device=logits.device) if want_theta else None) + (None,) * 9
        gbeta = gbeta.to(torch.float64).contiguous()
        gl = torch.empty_like(logits)
        gt = torch.empty(n, 3, 3, dtype=torch.float64, device=logits.device)
        ws = torch.empty(lib.lf_wls_bwd_theta_workspace_bytes(N, K), dtype=torch.uint8, device=logits.device)
        _lib.check(lib.lf_wls_bwd_theta(_lib.ptr(logits), _lib.ptr(t32), tbs, _lib.ptr(xs), _lib.ptr(ys), N, K, H, W, zero_rows,
                                        order, y_offset, act_kind, _lib.ptr(beta), _lib.ptr(zinv), _lib.ptr(gbeta), _lib.ptr(gl),
                                        _lib.ptr(gt), _lib.ptr(ws), _lib.stream()), "lf_wls_bwd_theta")
        return (gl, gt.view(tshape).to(tdtype) if want_theta else None) + (None,) * 9


class AreaLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, params, gt, order, weight_funct):
        lib = _lib.load()
        p = params.squeeze(-1) if params.dim() == 3 else params
        if p.stride(1) != 1:       # (rows of one lane out of an (N, K, D) tensor go in as they are: the kernel takes the row stride)
            p = p.contiguous()
        gt = gt.to(p.dtype).contiguous()
        assert p.dtype in (torch.float32, torch.float64) and p.shape == gt.shape and p.shape[1] == order + 1
        loss = torch.empty((), dtype=p.dtype, device=p.device)
        grad = torch.empty(p.shape, dtype=p.dtype, device=p.device)
        _lib.check(lib.lf_area_loss(_lib.ptr(p, rows=True), p.stride(0), _lib.ptr(gt), p.shape[0], order, weight_funct,
                                    1 if p.dtype == torch.float64 else 0, _lib.ptr(loss), _lib.ptr(grad),
                                    _lib.stream()), "lf_area_loss")
        ctx.save_for_backward(grad)
        ctx.pshape = params.shape
        return loss

    @staticmethod
    def backward(ctx, gout):
        (grad,) = ctx.saved_tensors
        return (grad * gout).view(ctx.pshape), None, None, None


class MSELossFn(torch.autograd.Function):
    """mean((params - gt)^2) over all elements and its gradient in one launch (lf_mse_loss)."""

    @staticmethod
    def forward(ctx, params, gt):
        lib = _lib.load()
        p = params.contiguous()
        q = gt.to(p.dtype).contiguous()
        if p.dtype not in (torch.float32, torch.float64) or p.shape != q.shape:
            raise RuntimeError("MSE_Loss: params %s %s vs gt %s" % (tuple(p.shape), p.dtype, tuple(q.shape)))
        loss = torch.empty((), dtype=p.dtype, device=p.device)
        grad = torch.empty_like(p)
        _lib.check(lib.lf_mse_loss(_lib.ptr(p), _lib.ptr(q), p.numel(), 1 if p.dtype == torch.float64 else 0, _lib.ptr(loss),
                                   _lib.ptr(grad), _lib.stream()), "lf_mse_loss")
        ctx.save_for_backward(grad)
        return loss

    @staticmethod
    def backward(ctx, gout):
        (grad,) = ctx.saved_tensors
        return grad * gout, None


class BackprojLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, params, x_gt, valid, Y, y_prime, minv):
        lib = _lib.load()
        p = params.squeeze(-1) if params.dim() == 3 else params
        p = p.to(torch.float64)
        if p.stride(1) != 1:       # (a lane's rows out of an (N, K, D) tensor go in as they are: beta_stride)
            p = p.contiguous()
        x_gt = x_gt.to(torch.float64).contiguous()
        valid = valid.to(torch.float64).contiguous()
        N, D = p.shape
        S = x_gt.shape[1]
        loss = torch.empty((), dtype=torch.float64, device=p.device)
        xcv = torch.empty(N, S, dtype=torch.float64, device=p.device)
        grad = torch.empty(N, D, dtype=torch.float64, device=p.device)
        m = (ctypes.c_double * 9)(*[float(v) for v in minv.reshape(-1)])
        _lib.check(lib.lf_backproj_loss(_lib.ptr(p, rows=True), p.stride(0), _lib.ptr(x_gt), _lib.ptr(valid), _lib.ptr(Y),
                                        _lib.ptr(y_prime), ctypes.cast(m, ctypes.c_void_p), N, S, D - 1,
                                        _lib.ptr(loss), _lib.ptr(xcv), _lib.ptr(grad), _lib.stream()),
                   "lf_backproj_loss")
        ctx.save_for_backward(grad)
        ctx.pshape, ctx.pdtype = params.shape, params.dtype
        ctx.mark_non_differentiable(xcv)
        ctx.set_materialize_grads(False)       # (no zero-filled (N, S) gradient for xcv on every call)
        return loss, xcv

    @staticmethod
    def backward(ctx, gout, _gx):
        (grad,) = ctx.saved_tensors
        if gout is None:
            return torch.zeros(ctx.pshape, dtype=ctx.pdtype, device=grad.device), None, None, None, None, None
        return (grad * gout).view(ctx.pshape).to(ctx.pdtype), None, None, None, None, None


class CrossEntropy2dFn(torch.autograd.Function):
    """``check_targets``: read back the kernel's count of labels outside [0, C) (one D2H sync) and raise like torch's
    NLLLoss does; with False the count stays in ``CrossEntropy2dFn.last_acc[2]`` for the caller to inspect."""
    last_acc = None

    @staticmethod
    def forward(ctx, logits, target, weights, check_targets=True):
        lib = _lib.load()
        logits = logits.contiguous()
        target = target.contiguous()
        weights = weights.to(device=logits.device, dtype=torch.float32).contiguous()
        assert logits.dtype == torch.float32 and target.dtype == torch.int64
        N, C, H, W = logits.shape
        assert target.shape == (N, H, W), (target.shape, logits.shape)
        acc = torch.empty(3, dtype=torch.float64, device=logits.device)
        loss = torch.empty((), dtype=torch.float32, device=logits.device)
        _lib.check(lib.lf_ce2d_fwd(_lib.ptr(logits), _lib.ptr(target), _lib.ptr(weights), N, C, H, W,
                                   _lib.ptr(acc), _lib.ptr(loss), _lib.stream()), "lf_ce2d_fwd")
        CrossEntropy2dFn.last_acc = acc
        if check_targets and float(acc[2]) != 0.0:
            raise RuntimeError("cross entropy: %d target value(s) outside [0, %d)" % (int(acc[2]), C))
        ctx.save_for_backward(logits, target, weights, acc)
        return loss

    @staticmethod
    def backward(ctx, gout):
        lib = _lib.load()
        logits, target, weights, acc = ctx.saved_tensors
        N, C, H, W = logits.shape
        up = gout.to(torch.float32).reshape(1).contiguous()
        g = torch.empty_like(logits)
        _lib.check(lib.lf_ce2d_bwd(_lib.ptr(logits), _lib.ptr(target), _lib.ptr(weights), N, C, H, W,
                                   _lib.ptr(acc), _lib.ptr(up), _lib.ptr(g), _lib.stream()), "lf_ce2d_bwd")
        return g, None, None, None


TREES = {"bp": 0, "bev": 1}
LANE_KINDS = {"backproject": 0, "area": 1, "mse": 2}


class StepLossFn(torch.autograd.Function):
    """The whole criterion of one step in one launch (lf_step_loss): ``apply(cfg, target, valid, line, gt_line, horizon, gt_horizon,
    *betas)`` -> ``(loss, values, x_cal)``.  ``cfg`` is the ``losses.StepCriterion`` (tree, lane kind, constants, weights, workspace,
    meters); ``betas`` are the K lanes' (N, D, 1) | (N, D) coefficients -- the unbind views of one (N, K, D) tensor are read in place.
    ``loss`` is the fp64 total; ``values`` the ten fp64 words of ``out`` (total, fit, line, horizon, acc_line, acc_horizon, bad line
    labels, line hits, horizon hits, 0); ``x_cal`` (N, K, S) fp64 with the backprojection kind, else None.  Only ``loss`` carries a
    gradient; backward is one launch that multiplies the flat gradient buffer of the forward by the upstream scalar."""

    @staticmethod
    def forward(ctx, cfg, target, valid, line, gt_line, horizon, gt_horizon, *betas):
        lib = _lib.load()
        ps = [b.squeeze(-1) if b.dim() == 3 else b for b in betas]
        K, (N, D), dt, dev = len(ps), ps[0].shape, ps[0].dtype, ps[0].device
        assert 1 <= K <= 4 and dt in (torch.float32, torch.float64)
        if any(p.shape != (N, D) or p.dtype != dt or p.stride(1) != 1 or p.stride(0) != ps[0].stride(0) for p in ps):
            ps = list(torch.stack([p.to(dt) for p in ps], 1).unbind(1))
        kind, bp = LANE_KINDS[cfg.loss_policy], cfg.kind_is_backproject
        tdt = torch.float64 if bp else dt
        target = target.to(tdt).contiguous()
        assert target.dim() == 3 and target.shape[0] == N and target.shape[1] >= K, (target.shape, N, K)
        S = target.shape[2]
        if bp:
            valid = valid.to(torch.float64).contiguous()
            assert valid.shape == target.shape and cfg.Y.shape == (S, D), (valid.shape, target.shape, cfg.Y.shape)
        else:
            assert S == D, "coefficient targets %s for order %d" % (tuple(target.shape), D - 1)
            valid = None
        heads = line is not None
        R = n_line = n_hor = 0
        if heads:
            line, horizon = line.contiguous(), horizon.contiguous()
            gt_horizon = gt_horizon.to(torch.float32).contiguous()
            gt_line = (gt_line.to(torch.int64) if cfg.tree == "bev" else gt_line.to(torch.float32)).contiguous()
            R = horizon.shape[1]
            assert line.dtype == torch.float32 and horizon.dtype == torch.float32
            assert tuple(line.shape) == ((N, 3, 4) if cfg.tree == "bev" else (N, 4)) and tuple(gt_line.shape) == (N, 4), line.shape
            assert tuple(horizon.shape) == (N, R) and gt_horizon.shape == horizon.shape
            n_line, n_hor = line.numel(), horizon.numel()
        out = torch.empty(10, dtype=torch.float64, device=dev)
        xcal = torch.empty(N, K, S, dtype=torch.float64, device=dev) if bp else None
        nb = N * K * D * ps[0].element_size()
        grad = torch.empty(nb + 4 * (n_line + n_hor), dtype=torch.uint8, device=dev)
        lanes = (ctypes.c_void_p * K)(*[p.data_ptr() for p in ps])
        m = None if cfg.M_inv is None else (ctypes.c_double * 9)(*[float(v) for v in cfg.M_inv.reshape(-1)])
        _lib.check(lib.lf_step_loss(
            TREES[cfg.tree], kind, K, N, D - 1, WEIGHT_FUNCTS[cfg.weight_funct] if kind == 1 else 0, int(cfg.nclasses),
            ctypes.cast(lanes, ctypes.c_void_p), ps[0].stride(0), 1 if dt == torch.float64 else 0,
            _lib.ptr(target), _lib.ptr(valid), target.stride(0), S,
            _lib.ptr(cfg.Y) if bp else None, _lib.ptr(cfg.y_prime) if bp else None, ctypes.cast(m, ctypes.c_void_p) if bp else None,
            _lib.ptr(line), _lib.ptr(gt_line), _lib.ptr(horizon), _lib.ptr(gt_horizon), R,
            float(cfg.weight_fit), float(cfg.weight_class), _lib.ptr(out), _lib.ptr(xcal), _lib.ptr(grad),
            _lib.ptr(cfg.meter_buffer(dev)), _lib.ptr(cfg.workspace(dev)), _lib.stream()), "lf_step_loss")
        ctx.save_for_backward(grad)
        ctx.cfg = (N, K, D, dt, nb, n_line, n_hor, [b.shape for b in betas], None if line is None else line.shape)
        loss = out[0]
        ctx.mark_non_differentiable(*([out] if xcal is None else [out, xcal]))
        ctx.set_materialize_grads(False)       # (no zero-filled gradients for the values nobody differentiates)
        return loss, out, xcal

    @staticmethod
    def backward(ctx, gloss, _gv, _gx):
        N, K, D, dt, nb, n_line, n_hor, bshapes, lshape = ctx.cfg
        if gloss is None:
            return (None,) * (7 + K)
        lib = _lib.load()
        (grad,) = ctx.saved_tensors
        up = gloss.to(torch.float64).reshape(1).contiguous()
        g = torch.empty_like(grad)
        _lib.check(lib.lf_step_loss_bwd(_lib.ptr(grad), 1 if dt == torch.float64 else 0, N * K * D, n_line + n_hor, _lib.ptr(up),
                                        _lib.ptr(g), _lib.stream()), "lf_step_loss_bwd")
        gb = g[:nb].view(dt).view(N, K, D)
        gl = gh = None
        if n_line:
            gl = g[nb:nb + 4 * n_line].view(torch.float32).view(lshape)
            gh = g[nb + 4 * n_line:].view(torch.float32).view(N, -1)
        return (None, None, None, gl, None, gh, None) + tuple(gb[:, k].view(bshapes[k]) for k in range(K))


class SegStepFn(torch.autograd.Function):
    """The segmentation-mode step behind the backbone in three launches (lf_seg_step): ``apply(cfg, logits, target, grid, flags,
    want_grad)`` -> ``(loss, out, beta, status, maps)``.  ``cfg`` is the ``losses.SegStepCriterion`` (class weights, the fit's
    constants, workspace, meters); ``grid`` None = cross entropy only (``beta``, ``status``, ``maps`` None).  ``loss`` is the fp64
    cross-entropy scalar and the only output with a gradient; ``out`` the four fp64 words (loss, weighted sum, weight sum, labels
    outside [0, C)).  The logits' gradient is written by the forward -- only with ``want_grad`` (the caller's grad mode: inside
    ``forward`` it is always off) -- and backward multiplies it by the upstream scalar in place (``lf_seg_step_bwd``: nothing is
    touched when that is 1, the loops' ``loss.backward()``), so one forward serves one backward."""

    @staticmethod
    def forward(ctx, cfg, logits, target, grid, flags, want_grad):
        lib = _lib.load()
        logits = logits.contiguous()
        target = target.contiguous()
        assert logits.dtype == torch.float32 and logits.dim() == 4 and target.dtype == torch.int64
        N, C, H, W = logits.shape
        assert target.shape == (N, H, W), (target.shape, logits.shape)
        dev = logits.device
        weights = cfg.weights.to(device=dev, dtype=torch.float32).contiguous()
        if weights.numel() != C:
            raise RuntimeError("seg-mode criterion: %d class weights for %d logit planes" % (weights.numel(), C))
        fit = grid is not None
        L, order, gbs = (cfg.lanes, cfg.order, 0) if fit else (0, 0, 0)
        beta = status = maps = None
        if fit:
            grid = grid.detach().contiguous()
            assert grid.dtype == torch.float32 and grid.shape[-2:] == (H * W, 2), (grid.shape, H, W)
            if grid.dim() == 3 and grid.shape[0] > 1:
                assert grid.shape[0] >= N
                gbs = H * W * 2
            beta = torch.empty(N, L, order + 1, dtype=torch.float64, device=dev)
            status = torch.empty(N * L, dtype=torch.int32, device=dev)
            maps = torch.empty(N, L, H, W, dtype=torch.float32, device=dev) if cfg.return_maps else None
        out = torch.empty(4, dtype=torch.float64, device=dev)
        grad = torch.empty_like(logits) if want_grad else None
        ws = cfg.workspace(dev, lib.lf_seg_step_workspace_bytes(N, C, L, H, W, order))
        _lib.check(lib.lf_seg_step(_lib.ptr(logits), _lib.ptr(target), _lib.ptr(weights), _lib.ptr(grid), gbs, _lib.ptr(flags),
                                   N, C, L, H, W, int(cfg.zero_rows), order, float(cfg.reg), float(cfg.y_offset), int(cfg.solver),
                                   _lib.ptr(grad), _lib.ptr(maps), _lib.ptr(beta), _lib.ptr(status), _lib.ptr(out),
                                   _lib.ptr(cfg.meter_buffer(dev)), _lib.ptr(ws), _lib.stream()), "lf_seg_step")
        ctx.grad = grad
        ctx.scaled = False
        loss = out[0]
        ctx.mark_non_differentiable(*[t for t in (out, beta, status, maps) if t is not None])
        ctx.set_materialize_grads(False)
        return loss, out, beta, status, maps

    @staticmethod
    def backward(ctx, gloss, _go, _gb, _gs, _gm):
        grad = ctx.grad
        if gloss is None or grad is None:
            return (None,) * 6
        if ctx.scaled:
            raise RuntimeError("seg-mode criterion: its gradient buffer was scaled in place by an earlier backward; call the "
                               "criterion again")
        ctx.scaled = True
        up = gloss.to(torch.float32).reshape(1).contiguous()
        _lib.check(_lib.load().lf_seg_step_bwd(_lib.ptr(grad), grad.numel(), _lib.ptr(up), _lib.stream()), "lf_seg_step_bwd")
        return None, grad, None, None, None, None


class LinearFn(torch.autograd.Function):
    """``act(x @ w.T + b)`` with ``act`` = identity or ReLU: the nn.Linear tails of the --clas heads on lf_linear_fwd / lf_linear_bwd
    (fp32, fixed summation order) instead of F.linear / rocBLAS."""

    @staticmethod
    def forward(ctx, x, w, b, relu):
        lib = _lib.load()
        x2 = x.reshape(-1, x.shape[-1]).contiguous()
        w = w.contiguous()
        assert x2.dtype == torch.float32 and w.dtype == torch.float32 and w.shape[1] == x2.shape[1]
        N, K = x2.shape
        O = w.shape[0]
        bb = None if b is None else b.contiguous()
        y = torch.empty(N, O, dtype=torch.float32, device=x2.device)
        _lib.check(lib.lf_linear_fwd(_lib.ptr(x2), _lib.ptr(w), _lib.ptr(bb), _lib.ptr(y), N, K, O, int(bool(relu)), _lib.stream()),
                   "lf_linear_fwd")
        ctx.save_for_backward(x2, w, y)
        ctx.relu, ctx.xshape, ctx.has_bias = bool(relu), x.shape, b is not None
        return y.view(*x.shape[:-1], O)

    @staticmethod
    def backward(ctx, gy):
        lib = _lib.load()
        x2, w, y = ctx.saved_tensors
        N, K = x2.shape
        O = w.shape[0]
        gy2 = gy.reshape(N, O).to(torch.float32).contiguous()
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]
        gx = torch.empty_like(x2) if need_x else None
        gw = torch.empty_like(w) if (need_w or need_b) else None
        gb = torch.empty(O, dtype=torch.float32, device=w.device) if need_b else None
        _lib.check(lib.lf_linear_bwd(_lib.ptr(x2), _lib.ptr(w), _lib.ptr(y), _lib.ptr(gy2), _lib.ptr(gx), _lib.ptr(gw), _lib.ptr(gb),
                                     N, K, O, int(ctx.relu), _lib.stream()), "lf_linear_bwd")
        return (gx.view(ctx.xshape) if need_x else None), (gw if need_w else None), gb, None


def linear(x, w, b=None, relu=False):
    return LinearFn.apply(x, w, b, relu)


def seg_flags(gt_line, N, lanes, device):
    """``gt_line`` as the (N, lanes) fp32 device flags lf_seg_maps / lf_head_fit_seg read, or None when nothing is borrowed."""
    if gt_line is None:
        return None
    flags = gt_line.to(device=device, dtype=torch.float32).contiguous()
    if tuple(flags.shape) != (N, lanes):
        # the reference's expand_as(masked) fails here -- but only when gt_line.sum() != 0 lets it get that far
        if float(flags.sum()) != 0:
            raise RuntimeError("seg-mode fit: gt_line %s cannot be expanded to the (%d, %d) lane maps" % (tuple(flags.shape), N, lanes))
        return None
    return flags


def seg_maps(logits, gt_line, zero_rows, lanes):
    """Segmentation-mode fit input (lf_seg_maps): arg-max of the class logits -> per-lane maps valued k at class k, masked rows
    zeroed, lanes flagged in ``gt_line`` (N, lanes; BP only) overwritten with map [0, 0].  No gradient (the reference detaches)."""
    lib = _lib.load()
    logits = logits.detach().contiguous()
    assert logits.dtype == torch.float32 and logits.dim() == 4
    N, C, H, W = logits.shape
    flags = seg_flags(gt_line, N, lanes, logits.device)
    maps =torch.empty(N, lanes, H, W, dtype=torch.float32, device=logits.device)
    _lib.check(lib.lf_seg_maps(_lib.ptr(logits), _lib.ptr(flags), _lib.ptr(maps), N, C, lanes, H, W, int(zero_rows), _lib.stream()),
               "lf_seg_maps")
    return maps
