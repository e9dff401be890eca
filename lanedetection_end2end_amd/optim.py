"""Fused optimizer steps for the hot path's 226 trainable tensors: one HIP launch per step (``lf_adam_step`` /
``lf_sgd_step`` / ``lf_rmsprop_step``) -- the three optimizers the reference's ``define_optim`` builds
(BEV/Networks/utils.py:411-420): Adam, SGD(momentum 0.9), RMSprop(momentum 0.9); ``define_optim`` below mirrors it.

Same update rule and state names as ``torch.optim.Adam`` (``exp_avg``, ``exp_avg_sq``, ``step``), which is what the
reference's ``define_optim('adam', ...)`` returns (BEV/Networks/utils.py:411-420); amsgrad / maximize are not
supported.  Parameters without a gradient (``encoder.output_conv``) are skipped like torch does, and the step count
is PER PARAMETER like torch's: a tensor that gets its first gradient late (``decoder.output_conv`` when the reference's
pretrained schedule flips ``end_to_end`` under one optimizer, BEV/main.py get_flags) starts its own bias correction at 1.
A ``torch.optim.Adam`` state_dict (tensor-valued ``step``) loads as is.

Gradient-norm clipping (``nn.utils.clip_grad_norm(model.parameters(), args.clip_grad_norm)``, BP/main.py:334-335) comes in two
forms on the same kernels.  ``max_grad_norm`` of the optimizers (``define_optim(..., clip_grad_norm=...)``): ``step()`` reads the
gradients once for the global norm (``lf_grad_sumsq`` per param group, one ``lf_grad_norm_finish``) and the ``lf_*_step_clipped``
launches pick the clip coefficient up from device memory; the gradients stay as they are and ``optimizer.last_grad_norm`` is a
0-dim device tensor.  ``clip_grad_norm_`` is the drop-in with torch's semantics: it rewrites the gradients in place and returns the
norm.  Both leave the same bits in the parameters; neither makes the host wait.
"""
import numpy as np
import torch

from . import _lib


def _upload(host_array, device):
    """A small host table to the device WITHOUT stalling the stream: pinned staging + non-blocking copy.  (The engine hands out
    parameter gradients as views of a flat buffer that the caching allocator alternates between two addresses, so the record
    table is rebuilt every step; a pageable `.to(device)` there is a synchronous copy queued behind the whole backward pass --
    the host then waits for the GPU once per step and the next forward's launches start late: ~0.5 ms per step in
    `bench.py --workload epoch`, round 4.)  Returns (device tensor, pinned tensor to keep alive with it)."""
    pinned = torch.from_numpy(host_array).pin_memory()
    return pinned.to(device, non_blocking=True), pinned


def _work_list(numels, chunk, device, cache):
    """(tensor, chunk) work items for tensors of these sizes: depends on the sizes only, cached."""
    key = (tuple(numels), chunk, device)
    hit = cache.get(key)
    if hit is None:
        work = np.array([(i, c) for i, n in enumerate(numels) for c in range((n + chunk - 1) // chunk)], dtype=np.int32).reshape(-1, 2)
        dev, pin = _upload(work, device)
        hit = cache[key] = (dev, pin, len(work))
    return hit


def _require_aligned(who, rec, plist, group_params):
    """The kernels take 16-byte vector loads and stores on the parameter and on its state buffers (only the gradient, a view
    at an arbitrary element offset of the flat buffer, has a scalar form): refuse anything else before it is launched on."""
    if not ((rec[:, 0] | rec[:, 2] | rec[:, 3]) & 15).any():
        return
    for row, p in zip(rec, plist):
        for name, addr in zip(("parameter", "first state buffer", "second state buffer"), (row[0], row[2], row[3])):
            if int(addr) % 16:
                index = next(j for j, q in enumerate(group_params) if q is p)
                raise _lib.LaneFitLibraryError("%s: the %s of tensor %d (%d elements) is not 16-byte aligned"
                                               % (who, name, index, p.numel()))


def _build_tables(who, plist, group_params, rows, works):
    """Device tables for these tensors: the records {p, g, m, v, numel, step[2]} of ``rows`` (refused unless 16-byte aligned where
    the kernels need it) uploaded without a stall, and the cached (tensor, chunk) work list -> (t_rec, t_work, nwork, pinned)."""
    rec = np.zeros((len(plist), 7), dtype=np.int64)
    for i, row in enumerate(rows):
        rec[i] = row
    _require_aligned(who, rec, plist, group_params)
    dev = plist[0].device
    t_work, _, nwork = _work_list([p.numel() for p in plist], _lib.load().lf_adam_chunk(), dev, works)
    t_rec, pin = _upload(rec, dev)
    return t_rec, t_work, nwork, pin


class _GradNorm:
    """The partials of every param group's ``lf_grad_sumsq`` and the {total_norm, coef} pair ``lf_grad_norm_finish`` writes; the
    buffers are allocated once and kept (the partials grow when the work lists do)."""

    def __init__(self, keep_out=True):
        self.partials = None
        self.out = None
        self.keep_out = keep_out

    def run(self, tables, grad_scale, max_norm):
        """``tables``: (t_rec, t_work, nblocks) per group.  Enqueues the sums and the finish -> out (2 fp32 on the device)."""
        lib = _lib.load()
        total = sum(t[2] for t in tables)
        dev = tables[0][0].device
        if self.partials is None or self.partials.numel() < total or self.partials.device != dev:
            self.partials = torch.empty(lib.lf_grad_norm_workspace_bytes(total) // 8, dtype=torch.float64, device=dev)
        if self.out is None or not self.keep_out or self.out.device != dev:
            self.out = torch.empty(2, dtype=torch.float32, device=dev)
        slot = 0
        for t_rec, t_work, nblocks in tables:
            _lib.check(lib.lf_grad_sumsq(_lib.ptr(t_rec), _lib.ptr(t_work), nblocks, slot, _lib.ptr(self.partials), _lib.stream()),
                       "lf_grad_sumsq")
            slot += nblocks
        _lib.check(lib.lf_grad_norm_finish(_lib.ptr(self.partials), total, grad_scale, max_norm, _lib.ptr(self.out), _lib.stream()),
                   "lf_grad_norm_finish")
        return self.out


class FusedAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, grad_scale=1.0, max_grad_norm=0.0):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self.grad_scale = float(grad_scale)
        self.max_grad_norm = float(max_grad_norm)     # 0: no clipping, the launches of an optimizer built without it
        self.last_grad_norm = None                    # 0-dim fp32 device tensors after a clipped step: the norm of the gradients
        self.last_clip_coef = None                    # the step used, and the coefficient it multiplied them by
        self._norm = _GradNorm()
        self._tables = {}
        self._works = {}

    def load_state_dict(self, state_dict):
        """A loaded state replaces ``exp_avg`` / ``exp_avg_sq`` / ``step``: the cached device tables hold the OLD buffers' addresses
        and the old device-side step counts, so they are dropped (mid-run resume / rollback)."""
        super().load_state_dict(state_dict)
        self._tables = {}

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        self._tables = {}

    def _table(self, gi, plist):
        """Device tables for one param group: records {p, g, m, v, numel, step[2]} and the (tensor, chunk) work list.  Rebuilt --
        with the step counts of ``self.state`` in BOTH slots -- when the set of tensors with a gradient or any buffer address
        (parameter, gradient, moments) changed; between rebuilds the kernel advances the counts on the device (slot parity
        alternates per launch)."""
        key = tuple((p.data_ptr(), p.grad.data_ptr(), self.state[p]["exp_avg"].data_ptr(), self.state[p]["exp_avg_sq"].data_ptr())
                    for p in plist)
        cached = self._tables.get(gi)
        if cached is not None and cached[0] == key:
            return cached
        rows = []
        for p in plist:
            st = self.state[p]
            n = int(st["step"])
            rows.append((p.data_ptr(), p.grad.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel(), n, n))
        t_rec, t_work, nwork, pin = _build_tables("FusedAdam", plist, self.param_groups[gi]["params"], rows, self._works)
        cached = [key, t_rec, t_work, nwork, 0, pin]
        self._tables[gi] = cached
        return cached

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = _lib.load()
        clip = self.max_grad_norm != 0
        ready = [self._prepare(gi, group) for gi, group in enumerate(self.param_groups)] if clip else None
        coef = _clip_coef(self, ready) if clip else None
        for gi, group in enumerate(self.param_groups):
            plist, tab = ready[gi] if clip else self._prepare(gi, group)
            if not plist:
                continue
            _, t_rec, t_work, nblocks, parity = tab[:5]
            b1, b2 = group["betas"]
            if clip:
                _lib.check(lib.lf_adam_step_clipped(_lib.ptr(t_rec), _lib.ptr(t_work), nblocks, group["lr"], b1, b2, group["eps"],
                                                    group["weight_decay"], parity, self.grad_scale, _lib.ptr(coef), _lib.stream()),
                           "lf_adam_step_clipped")
            else:
                _lib.check(lib.lf_adam_step(_lib.ptr(t_rec), _lib.ptr(t_work), nblocks, group["lr"], b1, b2, group["eps"],
                                            group["weight_decay"], parity, self.grad_scale, _lib.stream()), "lf_adam_step")
            tab[4] = parity ^ 1
            for p in plist:
                self.state[p]["step"] += 1
        return loss

    def _prepare(self, gi, group):
        """The tensors of one group that take this step and their device table (state created, everything the kernels cannot
        take refused) -> (plist, table), ([], None) for a group without gradients."""
        plist = [p for p in group["params"] if p.grad is not None]
        if not plist:
            return plist, None
        for p in plist:
            if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() and p.grad.is_contiguous()):
                raise _lib.LaneFitLibraryError("FusedAdam needs contiguous fp32 parameters on the GPU")
            st = self.state[p]
            if not st:
                st["step"] = 0
                st["exp_avg"] = torch.zeros_like(p)
                st["exp_avg_sq"] = torch.zeros_like(p)
            elif torch.is_tensor(st["step"]):              # a loaded torch.optim.Adam state
                st["step"] = int(st["step"])
        return plist, self._table(gi, plist)


def _clip_coef(opt, ready):
    """The global norm over ALL param groups (as torch's is over model.parameters()) of the gradients the step will use, and the
    clip coefficient, enqueued ahead of the clipped steps -> the one-element device tensor holding the coefficient (None: no
    gradient anywhere, nothing launched)."""
    tables = [(tab[1], tab[2], tab[3]) for plist, tab in ready if plist]
    if not tables:
        return None
    out = opt._norm.run(tables, opt.grad_scale, opt.max_grad_norm)
    opt.last_grad_norm, opt.last_clip_coef = out[0], out[1]
    return out[1:]


class _FusedMomentum(torch.optim.Optimizer):
    """Shared plumbing of FusedSGD / FusedRMSprop: state buffers, device tables (the layout of FusedAdam's), one launch."""
    _state_names = ()

    def __init__(self, params, defaults, grad_scale, max_grad_norm=0.0):
        super().__init__(params, defaults)
        self.grad_scale = float(grad_scale)
        self.max_grad_norm = float(max_grad_norm)     # as FusedAdam's
        self.last_grad_norm = None
        self.last_clip_coef = None
        self._norm = _GradNorm()
        self._tables = {}
        self._works = {}

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)      # new state buffers: the cached device tables point at the old ones
        self._tables = {}

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        self._tables = {}

    def _table(self, gi, plist):
        key = tuple((p.data_ptr(), p.grad.data_ptr()) + tuple(self.state[p][n].data_ptr() for n in self._state_names) for p in plist)
        cached = self._tables.get(gi)
        if cached is not None and cached[0] == key:
            return cached
        rows = []
        for p in plist:
            st = self.state[p]
            m = st["momentum_buffer"]
            v = st["square_avg"] if "square_avg" in st else m
            rows.append((p.data_ptr(), p.grad.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), 0, 0))
        t_rec, t_work, nwork, pin = _build_tables(type(self).__name__, plist, self.param_groups[gi]["params"], rows, self._works)
        cached = (key, t_rec, t_work, nwork, pin)
        self._tables[gi] = cached
        return cached

    def _launch(self, group, t_rec, t_work, nblocks, coef):
        """One launch for one group; ``coef``: device tensor holding the clip coefficient, None without clipping."""
        raise NotImplementedError

    def _prepare(self, gi, group):
        """As FusedAdam._prepare."""
        plist = [p for p in group["params"] if p.grad is not None]
        if not plist:
            return plist, None
        for p in plist:
            if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() and p.grad.is_contiguous()):
                raise _lib.LaneFitLibraryError("fused optimizers need contiguous fp32 parameters on the GPU")
            st = self.state[p]
            for name in self._state_names:
                if st.get(name) is None:
                    st[name] = torch.zeros_like(p)
        return plist, self._table(gi, plist)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        clip = self.max_grad_norm != 0
        ready = [self._prepare(gi, group) for gi, group in enumerate(self.param_groups)] if clip else None
        coef = _clip_coef(self, ready) if clip else None
        for gi, group in enumerate(self.param_groups):
            plist, tab = ready[gi] if clip else self._prepare(gi, group)
            if not plist:
                continue
            _, t_rec, t_work, nblocks = tab[:4]
            self._launch(group, t_rec, t_work, nblocks, coef)
            for p in plist:
                self.state[p]["step"] = self.state[p].get("step", 0) + 1
        return loss


class FusedSGD(_FusedMomentum):
    """``torch.optim.SGD(params, lr, momentum=0.9, weight_decay)`` as the reference builds it (utils.py:414-415): dampening 0,
    no Nesterov.  State name ``momentum_buffer`` as torch's."""
    _state_names = ("momentum_buffer",)

    def __init__(self, params, lr=1e-3, momentum=0.9, weight_decay=0.0, grad_scale=1.0, max_grad_norm=0.0):
        super().__init__(params, dict(lr=lr, momentum=momentum, weight_decay=weight_decay), grad_scale, max_grad_norm)

    def _launch(self, group, t_rec, t_work, nblocks, coef):
        lib = _lib.load()
        if coef is not None:
            _lib.check(lib.lf_sgd_step_clipped(_lib.ptr(t_rec), _lib.ptr(t_work), nblocks, group["lr"], group["momentum"],
                                               group["weight_decay"], self.grad_scale, _lib.ptr(coef), _lib.stream()),
                       "lf_sgd_step_clipped")
            return
        _lib.check(lib.lf_sgd_step(_lib.ptr(t_rec), _lib.ptr(t_work), nblocks, group["lr"], group["momentum"],
                                   group["weight_decay"], self.grad_scale, _lib.stream()), "lf_sgd_step")


class FusedRMSprop(_FusedMomentum):
    """``torch.optim.RMSprop(params, lr, momentum=0.9, weight_decay)`` (utils.py:416-417): alpha 0.99, eps 1e-8, not centered.
    State names ``square_avg`` / ``momentum_buffer`` as torch's."""
    _state_names = ("square_avg", "momentum_buffer")

    def __init__(self, params, lr=1e-2, alpha=0.99, eps=1e-8, momentum=0.9, weight_decay=0.0, grad_scale=1.0, max_grad_norm=0.0):
        super().__init__(params, dict(lr=lr, alpha=alpha, eps=eps, momentum=momentum, weight_decay=weight_decay), grad_scale,
                         max_grad_norm)

    def _launch(self, group, t_rec, t_work, nblocks, coef):
        lib = _lib.load()
        if coef is not None:
            _lib.check(lib.lf_rmsprop_step_clipped(_lib.ptr(t_rec), _lib.ptr(t_work), nblocks, group["lr"], group["alpha"],
                                                   group["eps"], group["momentum"], group["weight_decay"], self.grad_scale,
                                                   _lib.ptr(coef), _lib.stream()), "lf_rmsprop_step_clipped")
            return
        _lib.check(lib.lf_rmsprop_step(_lib.ptr(t_rec), _lib.ptr(t_work), nblocks, group["lr"], group["alpha"],
                                       group["eps"], group["momentum"], group["weight_decay"], self.grad_scale,
                                       _lib.stream()), "lf_rmsprop_step")


def define_optim(optim, params, lr, weight_decay, clip_grad_norm=0):
    """The reference's optimizer factory (BEV/Networks/utils.py:411-420) on the fused steps: same names, same settings.
    ``clip_grad_norm`` (not an argument of the reference's; 0 = off) folds ``nn.utils.clip_grad_norm(model.parameters(),
    args.clip_grad_norm)`` of BP/main.py:334-335 into ``optimizer.step()``."""
    if optim == 'adam':
        return FusedAdam(params, lr=lr, weight_decay=weight_decay, max_grad_norm=clip_grad_norm)
    if optim == 'sgd':
        return FusedSGD(params, lr=lr, momentum=0.9, weight_decay=weight_decay, max_grad_norm=clip_grad_norm)
    if optim == 'rmsprop':
        return FusedRMSprop(params, lr=lr, momentum=0.9, weight_decay=weight_decay, max_grad_norm=clip_grad_norm)
    raise KeyError("The requested optimizer: {} is not implemented".format(optim))


_drop_in = {"key": None, "tables": None, "works": {}, "norm": _GradNorm(keep_out=False)}


@torch.no_grad()
def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None, grad_scale=1.0):
    """``torch.nn.utils.clip_grad_norm_`` on the device (the drop-in for BP/main.py:334-335): the 2-norm of all gradients in one
    read, then every gradient rewritten in place as fl32(fl32(g * grad_scale) * coef), coef = min(1, max_norm / (norm + 1e-6)) with
    a NaN kept.  Returns the norm (of the ``grad_scale``-scaled gradients) as a 0-dim device tensor; nothing is read back, so
    ``error_if_nonfinite`` cannot be honoured and non-finite gradients behave as under torch's default.  Parameters without a
    gradient are skipped; with none at all the norm is a host zero, as torch's, and nothing is launched."""
    if float(norm_type) != 2.0:
        raise NotImplementedError("clip_grad_norm_: only the 2-norm is implemented (norm_type=%r)" % (norm_type,))
    if error_if_nonfinite:
        raise NotImplementedError("clip_grad_norm_: error_if_nonfinite needs the norm on the host")
    if torch.is_tensor(parameters):
        parameters = [parameters]
    params = list(parameters)
    plist = [p for p in params if p.grad is not None]
    if not plist:
        return torch.tensor(0.0)
    for p in plist:
        if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() and p.grad.is_contiguous()):
            raise _lib.LaneFitLibraryError("clip_grad_norm_ needs contiguous fp32 parameters on the GPU")
    key = tuple((p.data_ptr(), p.grad.data_ptr(), p.numel()) for p in plist)
    if _drop_in["key"] != key:
        # the record's state slots are not read by these kernels: they repeat the parameter's address
        rows = [(p.data_ptr(), p.grad.data_ptr(), p.data_ptr(), p.data_ptr(), p.numel(), 0, 0) for p in plist]
        _drop_in["tables"] = _build_tables("clip_grad_norm_", plist, params, rows, _drop_in["works"])
        _drop_in["key"] = key
    t_rec, t_work, nblocks, _ = _drop_in["tables"]
    out = _drop_in["norm"].run([(t_rec, t_work, nblocks)], float(grad_scale), float(max_norm))
    _lib.check(_lib.load().lf_grad_scale_inplace(_lib.ptr(t_rec), _lib.ptr(t_work), nblocks, float(grad_scale), _lib.ptr(out[1:]),
                                                 _lib.stream()), "lf_grad_scale_inplace")
    return out[0]


clip_grad_norm = clip_grad_norm_        # the name BP/main.py:335 calls
