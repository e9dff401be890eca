#!/usr/bin/env python
"""Generate tests/golden/homography.npz: the REAL reference ``ProjectiveGridGenerator`` + ``Weighted_least_squares`` with a
per-image homography that requires a gradient (authoring container only; needs the reference tree):

    python tools/gen_golden_homography.py

theta = M * (1 + 0.02 * randn) per image and entry, rounded to fp32 (both runs read the same values); logits, gradients of
beta and the row mask as ``oracle/gen_golden.py`` makes them.  For each case and run (fp32 = the reference as shipped, fp64 = the
same modules in double) the file holds theta, beta, the theta gradient, and the grid and logits gradients sampled ``[::4, ::4]``
over the map (``[::8, ::8]`` for the 256 x 512 logits gradient).
BEV: N=3, K=2, 64x128, orders 0..2, reg 0 and 1e-3.  BP (pixel coordinates, fp64 only): N=2, K=4, 256x512, orders 2 and 3.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import fit_oracle, inputs, ref_shims  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "homography.npz")
PERTURBATION = 0.02
BEV = dict(N=3, K=2, H=64, W=128, logits_seed=11, gbeta_seed=5, theta_seed=17, step=(4, 4))
BP = dict(N=2, K=4, H=256, W=512, logits_seed=12, gbeta_seed=6, theta_seed=18, step=(4, 8))


def perturbed_theta(M, N, seed):
    """(N, 3, 3) fp32: M * (1 + 0.02 * randn), one draw per image and entry."""
    rng = np.random.default_rng(seed)
    return (np.asarray(M, np.float64)[None] * (1 + PERTURBATION * rng.standard_normal((N, 3, 3)))).astype(np.float32)


def _t(a, dtype):
    return torch.from_numpy(np.asarray(a)).to(dtype)


def run_case(grid_of, ls, cfg, theta32, order, dtype, key, out):
    N, K, H, W = cfg["N"], cfg["K"], cfg["H"], cfg["W"]
    zero_rows = fit_oracle.zero_rows_of(H, 0.3)
    ls.tensor_ones = ls.tensor_ones.to(dtype)
    ls.reg_ls = ls.reg_ls.to(dtype)
    theta = _t(theta32, dtype).requires_grad_(True)
    grid = grid_of(theta)
    grid.retain_grad()
    assert bool(torch.isfinite(grid).all()), "a pole of the perturbed homography inside the map"
    o = _t(inputs.lane_like_logits(N, K, H, W, seed=cfg["logits_seed"]), dtype).requires_grad_(True)
    masked = (o ** 2).index_fill(2, torch.arange(zero_rows), 0)
    betas = [b for b in ls(masked, grid) if b is not None]
    gb = _t(np.random.default_rng(cfg["gbeta_seed"]).standard_normal((K, N, order + 1, 1)), dtype)
    sum((b.to(dtype) * g).sum() for b, g in zip(betas, gb)).backward()
    sg, sl = cfg["step"]
    out[key + "_theta"] = theta.detach().numpy()
    out[key + "_beta"] = np.stack([b.detach().numpy() for b in betas], 1)[..., 0]
    out[key + "_grad_theta"] = theta.grad.numpy()
    out[key + "_grad_grid"] = grid.grad.numpy().reshape(N, H, W, 2)[:, ::sg, ::sg].copy()
    out[key + "_grad_logits"] = o.grad.numpy()[:, :, ::sl, ::sl].copy()
    out[key + "_grid_absmax"] = np.array(float(grid.detach().abs().max()))


def gen_bev(ref, out):
    cfg = BEV
    N, K, H, W = cfg["N"], cfg["K"], cfg["H"], cfg["W"]
    size = torch.Size([N, K, H, W])
    _, M, _ = ref.LSQ_layer.Init_Projective_transform(K, N, H)
    theta32 = perturbed_theta(M[0].double().numpy(), N, cfg["theta_seed"])
    for dtype, tag in ((torch.float32, "f32"), (torch.float64, "f64")):
        gridgen = ref.LSQ_layer.ProjectiveGridGenerator(size, _t(theta32, dtype), True)
        gridgen.base_grid = gridgen.base_grid.to(dtype)
        for order in (0, 1, 2):
            for reg in (0.0, 1e-3):
                ls = ref.LSQ_layer.Weighted_least_squares(size, K, order, True, reg, False)
                run_case(gridgen, ls, cfg, theta32, order, dtype, "bev_o%d_r%g_%s" % (order, reg, tag), out)


def gen_bp(ref, out):
    cfg = BP
    N, K, H, W = cfg["N"], cfg["K"], cfg["H"], cfg["W"]
    size = torch.Size([N, K, H, W])
    M, _ = ref.utils.get_homography(H, False)
    theta32 = perturbed_theta(M, N, cfg["theta_seed"])
    for order in (2, 3):
        ls = ref.LSQ_layer.Weighted_least_squares(size, K, order, True, 0.0, False)
        run_case(lambda th: ref.LSQ_layer.ProjectiveGridGenerator(size, th, True), ls, cfg, theta32, order, torch.float64,
                 "bp_o%d_f64" % order, out)


def main():
    assert ref_shims.available(), "needs the reference tree"
    torch.set_num_threads(8)
    out = {}
    gen_bev(ref_shims.load("bev"), out)
    gen_bp(ref_shims.load("bp"), out)
    np.savez_compressed(OUT, **out)
    print(OUT, "%.1f KB" % (os.path.getsize(OUT) / 1024), len(out), "arrays",
          "max |grid| %.1f" % max(float(v) for k, v in out.items() if k.endswith("_grid_absmax")))


if __name__ == "__main__":
    sys.exit(main())
