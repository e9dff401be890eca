#!/usr/bin/env python
"""Every output and gradient of the lane fit on a fixed, seeded list of cases, for bit-for-bit comparison of two checkouts.

    python tools/fit_dump.py --out A.npz           # run from the root of the checkout under test (its package is imported)
    python tools/fit_dump.py --compare A.npz B.npz # array_equal on every array; exit status 1 on any difference

Only the public Python surface is used (``fit.fit_lanes``, ``ops.theta_grid``, ``bp.Networks.gels.GELS`` and the ``lf_head_fit``
binding), so the same file runs on an older checkout.  The fit accumulates in fp64 in a fixed order: two builds that compute the
same thing agree in every bit, and a difference is a moved or re-associated expression.

Cases: orders 0..3; W % 4 == 0 and a ragged width; zero_rows 0 and > 0; the six activations; both solvers with reg 0 and 1e-3;
the masked map requested and not; shared and per-image grid with the grid gradient; shared and per-image theta; the theta-grid
backward on its own; the fused head + fit from fp32 and bf16 input, with and without logits, K odd and even; GELS at D = 1..4.
"""
import argparse
import itertools
import os
import sys

import numpy as np

ACTS = ("square", "abs", "relu", "sigmoid", "softplus", "none")
SOLVERS = ((False, 0.0), (False, 1e-3), (True, 0.0), (True, 1e-3))
N, K, H = 2, 3, 24
WIDTHS = (64, 50)
ZERO_ROWS = (0, 7)


def _theta(gen, n, torch):
    t = torch.eye(3).repeat(n, 1, 1) + 0.05 * torch.randn(n, 3, 3, generator=gen)
    t[:, 2, :2] *= 0.2             # (the denominator stays near 1 on [0, 1)^2)
    return t[0] if n == 1 else t


def dump(path):
    sys.path.insert(0, os.getcwd())
    import torch
    from lanedetection_end2end_amd import _lib, fit, ops
    from lanedetection_end2end_amd.bp.Networks.gels import GELS
    out = {}
    cases = 0

    def put(key, t):
        assert key not in out, key
        out[key] = t.detach().float().cpu().numpy() if t.dtype == torch.bfloat16 else t.detach().cpu().numpy()

    gen = torch.Generator().manual_seed(1234)
    for order, W, zr, (ai, act), (si, (chol, reg)) in itertools.product(range(4), WIDTHS, ZERO_ROWS, enumerate(ACTS),
                                                                        enumerate(SOLVERS)):
        want_masked = (ai + si) % 2 == 0
        logits0 = torch.randn(N, K, H, W, generator=gen).cuda()
        gbeta = torch.randn(N, K, order + 1, generator=gen, dtype=torch.float64).cuda()
        grids = torch.rand(N, H * W, 2, generator=gen).cuda()
        thetas = _theta(gen, N, torch).cuda()
        sources = {"grid1": dict(grid=grids[0].clone()), "gridN": dict(grid=grids.clone()),
                   "theta1": dict(theta=thetas[0].clone()), "thetaN": dict(theta=thetas.clone())}
        for name, kw in sources.items():
            key = "fit/o%d/W%d/zr%d/%s/chol%d/reg%g/%s" % (order, W, zr, act, chol, reg, name)
            logits = logits0.clone().requires_grad_(True)
            src = next(iter(kw.values())).requires_grad_(True)
            beta, masked, status = fit.fit_lanes(logits, zero_rows=zr, order=order, reg_ls=reg, y_offset=1.0, activation=act,
                                                 use_cholesky=chol, return_masked=want_masked, check_singular=False, **kw)
            (beta * gbeta).sum().backward()
            put(key + "/beta", beta)
            put(key + "/status", status)
            if want_masked:
                put(key + "/masked", masked)
            put(key + "/grad_logits", logits.grad)
            put(key + "/grad_source", src.grad)
            cases += 1

    for W, n, normalised in itertools.product(WIDTHS, (1, N), (True, False)):
        key = "theta_grid/W%d/n%d/norm%d" % (W, n, normalised)
        theta = _theta(gen, n, torch).cuda().requires_grad_(True)
        grid = ops.theta_grid(theta, H, W, normalised)
        gg = torch.randn(grid.shape, generator=gen).cuda()
        gg[:, : 5 * W] = 0          # (rows without a gradient are skipped by the kernel)
        grid.backward(gg)
        put(key + "/grid", grid)
        put(key + "/grad_theta", theta.grad)
        cases += 1

    lib = _lib.load()
    h, w = 12, 20
    for order, bf16, with_logits, Kh, zr, per_image in itertools.product(range(4), (False, True), (False, True), (3, 4), (0, 5, 6),
                                                                         (False, True)):
        key = "head/o%d/bf%d/logits%d/K%d/zr%d/gridN%d" % (order, bf16, with_logits, Kh, zr, per_image)
        x = torch.randn(N, h, w, 16, generator=gen).cuda()
        if bf16:
            x = x.to(torch.bfloat16)
        hw = (torch.randn(16, Kh, 2, 2, generator=gen) * 0.3).cuda()
        hb = torch.randn(Kh, generator=gen).cuda()
        grid = torch.rand(N if per_image else 1, 4 * h * w, 2, generator=gen).cuda()
        D = order + 1
        beta = torch.empty(N, Kh, D, dtype=torch.float64, device="cuda")
        zinv = torch.empty(N, Kh, D * D, dtype=torch.float64, device="cuda")
        part = torch.empty(lib.lf_wls_workspace_bytes(N, Kh, order), dtype=torch.uint8, device="cuda")
        status = torch.empty(N * Kh, dtype=torch.int32, device="cuda")
        logits = torch.empty(N, Kh, 2 * h, 2 * w, device="cuda") if with_logits else None
        _lib.check(lib.lf_head_fit(_lib.ptr(x), int(bf16), _lib.ptr(hw), _lib.ptr(hb), _lib.ptr(grid), 8 * h * w if per_image else 0,
                                   N, h, w, Kh, zr, order, 1e-3 if order == 3 else 0.0, 1.0, ops.ACT_KINDS["square"], order % 2,
                                   _lib.ptr(logits), _lib.ptr(beta), _lib.ptr(zinv), _lib.ptr(part), _lib.ptr(status),
                                   _lib.stream()), "lf_head_fit")
        put(key + "/beta", beta)
        put(key + "/zinv", zinv)
        put(key + "/status", status)
        if with_logits:
            put(key + "/logits", logits)
        cases += 1

    for D, P in itertools.product((1, 2, 3, 4), (1000, 4099)):
        key = "gels/D%d/P%d" % (D, P)
        A = torch.randn(N, P, D, generator=gen).cuda().requires_grad_(True)
        b = torch.randn(N, P, 1, generator=gen).cuda().requires_grad_(True)
        x = GELS.apply(A, b)
        (x * torch.randn(N, D, 1, generator=gen).cuda()).sum().backward()
        put(key + "/x", x)
        put(key + "/grad_A", A.grad)
        put(key + "/grad_b", b.grad)
        cases += 1

    torch.cuda.synchronize()
    np.savez_compressed(path, cases=np.int64(cases), **out)
    print("fit_dump: %d cases, %d arrays -> %s" % (cases, len(out), path))


def compare(a_path, b_path):
    a, b = np.load(a_path), np.load(b_path)
    assert sorted(a.files) == sorted(b.files), "the two dumps hold different arrays"
    bad = [k for k in a.files if not (a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k], equal_nan=True))]
    finite = sum(bool(np.isfinite(a[k]).all()) for k in a.files)
    for k in bad[:20]:
        print("DIFFERENT %s: max |a - b| = %g" % (k, float(np.nanmax(np.abs(a[k].astype(np.float64) - b[k].astype(np.float64))))))
    print('{"cases": %d, "arrays": %d, "arrays_all_finite": %d, "different": %d}' % (int(a["cases"]), len(a.files) - 1, finite - 1,
                                                                                 len(bad)))
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    if not args.out:
        ap.error("one of --out and --compare is required")
    dump(args.out)
