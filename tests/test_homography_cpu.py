"""Homography through the lane fit, the part that needs no GPU: the C surface (exports, header, ABI number), the code-object
metadata of the new kernels, and the closed form of the grid / theta gradients -- restated here in numpy fp64 -- against the
fp64 run of the real reference modules (tests/golden/homography.npz, tools/gen_golden_homography.py).

The restatement (``fit_through_theta``) is the oracle of tests/test_homography_gpu.py.  Notation of ``wls_bwd_kernel``:
v = Z^-1 gbeta, q = Y.v, r = x - Y.beta, s = w^2, y = y_off - gy; per pixel and lane
    dL/dgx = s q,   dL/dgy = -sum_k s (r v_k - q beta_k) (d - k) y^(d-k-1)
and with (a, b, c) = theta [px, py, 1], gx = a / c, gy = b / c
    dL/dtheta_0 = sum (dgx / c) p,  dL/dtheta_1 = sum (dgy / c) p,  dL/dtheta_2 = sum -((dgx gx + dgy gy) / c) p.
"""
import ctypes
import glob
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN
from oracle import fit_oracle, inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

NEW_SYMBOLS = ("lf_theta_grid", "lf_theta_grid_bwd_workspace_bytes", "lf_theta_grid_bwd", "lf_wls_fwd_theta",
               "lf_wls_bwd_theta_workspace_bytes", "lf_wls_bwd_theta", "lf_wls_bwd_grid")
# name prefix -> instantiations: orders 0..3; the two fit kernels in both vector widths, from both grid sources
NEW_KERNELS = {"theta_grid_kernel": 1, "theta_grid_bwd_kernel": 1, "theta_finish_kernel": 1, "wls_moments_kernel<": 16,
               "wls_bwd_kernel<": 16, "wls_bwd_grid_kernel<": 4}

BEV_CASES = [(order, reg) for order in (0, 1, 2) for reg in (0.0, 1e-3)]
BEV = dict(N=3, K=2, H=64, W=128, logits_seed=11, gbeta_seed=5, y_off=1.0, normalised=True, step=(4, 4))
BP = dict(N=2, K=4, H=256, W=512, logits_seed=12, gbeta_seed=6, y_off=255.0, normalised=False, step=(4, 8))


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(((a - b) ** 2).sum() / max((b ** 2).sum(), 1e-300)))


# ---- the oracle ---------------------------------------------------------------------------------------------------------

def base_tables(H, W, normalised):
    """The reference's own fp32 ``torch.linspace`` base coordinates (BEV LSQ_layer.py:70-71, BP :53-54), as fp64 arrays."""
    import torch
    if normalised:
        xs, ys = torch.linspace(0, 1 - 1 / W, W), torch.linspace(0, 1 - 1 / H, H)
    else:
        xs, ys = torch.linspace(0, W - 1, W), torch.linspace(0, H - 1, H)
    return xs.double().numpy(), ys.double().numpy()


def grid_from_theta(theta, H, W, normalised):
    """theta (N,3,3) -> (gx, gy, c, px, py), each (N, H*W) fp64 (px, py: (H*W))."""
    xs, ys = base_tables(H, W, normalised)
    px, py = np.tile(xs, H), np.repeat(ys, W)
    t = np.asarray(theta, np.float64).reshape(-1, 3, 3)
    a = t[:, 0, 0, None] * px + t[:, 0, 1, None] * py + t[:, 0, 2, None]
    b = t[:, 1, 0, None] * px + t[:, 1, 1, None] * py + t[:, 1, 2, None]
    c = t[:, 2, 0, None] * px + t[:, 2, 1, None] * py + t[:, 2, 2, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        return a / c, b / c, c, px, py


def fit_through_theta(logits, theta, gbeta, zero_rows, order, reg, y_off, normalised, act="square", grid=None):
    """fp64 fit of (N,K,H,W) logits through a per-image (N,3,3) or shared (3,3) theta, and every gradient of
    L = sum(gbeta * beta): dict(beta (N,K,D), grad_logits (N,K,H,W), grad_grid (N,H*W,2), grad_theta (N,3,3); a shared theta's
    gradient is grad_theta.sum(0)).  ``grid`` (N | 1, H*W, 2): use these coordinates -- e.g. the device's own fp32 grid -- in the
    place of theta's (c still comes from theta).  Masked rows are skipped, as in the kernels."""
    o = np.asarray(logits, np.float64)
    N, K, H, W = o.shape
    D = order + 1
    theta = np.broadcast_to(np.asarray(theta, np.float64).reshape(-1, 3, 3), (N, 3, 3))
    gx, gy, c, px, py = grid_from_theta(theta, H, W, normalised)
    if grid is not None:
        g = np.broadcast_to(np.asarray(grid, np.float64).reshape(-1, H * W, 2), (N, H * W, 2))
        gx, gy = g[..., 0], g[..., 1]
    live = np.arange(H * W) >= zero_rows * W
    gx, gy, c, px, py = gx[:, live], gy[:, live], c[:, live], px[live], py[live]
    ol = o.reshape(N, K, -1)[:, :, live]
    w = fit_oracle.activation(ol, act)
    s = w * w
    y = y_off - gy                                                          # (N, P')
    Y = np.stack([y ** (order - k) for k in range(D)], -1)                  # (N, P', D)
    Z = np.einsum("nkp,npi,npj->nkij", s, Y, Y) + reg * np.eye(D)
    X = np.einsum("nkp,np,npi->nki", s, gx, Y)
    Zi = np.linalg.inv(Z)
    beta = np.einsum("nkij,nkj->nki", Zi, X)
    v = np.einsum("nkij,nkj->nki", Zi, np.asarray(gbeta, np.float64))
    q = np.einsum("npi,nki->nkp", Y, v)
    r = gx[:, None] - np.einsum("npi,nki->nkp", Y, beta)
    gl = np.zeros((N, K, H * W))
    gl[:, :, live] = 2 * w * q * r * fit_oracle.activation_grad(ol, act)
    dgx = (s * q).sum(1)                                                    # lanes of an image summed: (N, P')
    dgy = np.zeros_like(dgx)
    for k in range(order):
        u = r * v[:, :, k, None] - q * beta[:, :, k, None]
        dgy -= (s * u * (order - k) * y[:, None] ** (order - k - 1)).sum(1)
    gg = np.zeros((N, H * W, 2))
    gg[:, live, 0], gg[:, live, 1] = dgx, dgy
    p = np.stack([np.broadcast_to(px, c.shape), np.broadcast_to(py, c.shape), np.ones_like(c)], -1)     # (N, P', 3)
    rows = np.stack([dgx / c, dgy / c, -(dgx * gx + dgy * gy) / c], -1)                                 # (N, P', 3)
    gt = np.einsum("npi,npj->nij", rows, p)
    return dict(beta=beta, grad_logits=gl.reshape(N, K, H, W), grad_grid=gg, grad_theta=gt)


def theta_grad_of_grid_grad(theta, grad_grid, H, W, normalised):
    """The backward of the grid alone: grad_grid (N,H*W,2) -> grad_theta (N,3,3); pixels with a zero gradient are skipped."""
    gx, gy, c, px, py = grid_from_theta(theta, H, W, normalised)
    g = np.asarray(grad_grid, np.float64)
    dgx, dgy = g[..., 0], g[..., 1]
    live = (dgx != 0) | (dgy != 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        rows = np.stack([dgx / c, dgy / c, -(dgx * gx + dgy * gy) / c], -1)
    rows[~live] = 0
    p = np.stack([np.broadcast_to(px, c.shape), np.broadcast_to(py, c.shape), np.ones_like(c)], -1)
    return np.einsum("npi,npj->nij", rows, p)


def case_inputs(cfg, order):
    N, K, H, W = cfg["N"], cfg["K"], cfg["H"], cfg["W"]
    o = inputs.lane_like_logits(N, K, H, W, seed=cfg["logits_seed"])
    gb = np.random.default_rng(cfg["gbeta_seed"]).standard_normal((K, N, order + 1, 1))[..., 0].transpose(1, 0, 2)
    return o, np.ascontiguousarray(gb), fit_oracle.zero_rows_of(H, 0.3)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "homography.npz"), allow_pickle=False)


# ---- the C surface --------------------------------------------------------------------------------------------------------

def test_new_symbols_exported_and_declared():
    from lanedetection_end2end_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "lanefit.h")).read()
    additions = header[header.index("additions since 5 -- homography through the fit"):]
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), "%s is not exported by liblanefit_hip.so" % name
        assert re.search(r"\b%s\(" % name, additions), "%s is not declared in the header's additions block" % name
        assert name in _lib.exported_symbols()
    assert lib.lf_abi_version() == 5
    assert "#define LF_ABI_VERSION 5" in header
    lib.lf_wls_bwd_theta_workspace_bytes.restype = ctypes.c_size_t
    lib.lf_theta_grid_bwd_workspace_bytes.restype = ctypes.c_size_t
    assert lib.lf_wls_bwd_theta_workspace_bytes(3, 2) == 3 * 2 * 64 * 9 * 8
    assert lib.lf_theta_grid_bwd_workspace_bytes(3) == 3 * 64 * 9 * 8


def test_new_kernels_do_not_spill(tmp_path):
    from lanedetection_end2end_amd import build
    import isa_meta
    src = os.path.join(build.CSRC, "lf_fit.hip")
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + build.FLAGS + ["-c", src, "-o", str(tmp_path / "lf_fit.o"), "-save-temps=obj"]
    subprocess.check_call(cmd, cwd=str(tmp_path))
    asm = glob.glob(str(tmp_path / "*gfx950*.s"))
    assert asm, "no device assembly produced"
    kernels = isa_meta.kernels(asm[0])
    for prefix, count in NEW_KERNELS.items():
        mine = [k for k in kernels if k["name"].startswith(prefix)]
        assert len(mine) == count, (prefix, [k["name"] for k in mine])
        if count == 16:         # eight on the homography, eight on the constant grid
            assert sum("GridTheta>" in k["name"] for k in mine) == 8 and sum("GridTable>" in k["name"] for k in mine) == 8, mine
        for k in mine:
            assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, k
            assert k["vgpr"] + k["agpr"] <= 128, k          # four waves per SIMD at least


# ---- the closed form against the reference's autograd ---------------------------------------------------------------------

def _check_against_reference(golden, cfg, key, order, reg):
    N, H, W = cfg["N"], cfg["H"], cfg["W"]
    o, gb, zr = case_inputs(cfg, order)
    theta = golden[key + "_theta"]
    assert theta.dtype == np.float64 and np.array_equal(theta, theta.astype(np.float32))      # fp32 values, both runs
    # (the reference keeps reg_ls * eye(order + 1) as an fp32 tensor and casts it up: its 1e-3 is float32(1e-3))
    c = fit_through_theta(o, theta, gb, zr, order, float(np.float32(reg)), cfg["y_off"], cfg["normalised"])
    sg, sl = cfg["step"]
    e = dict(beta=rel_l2(c["beta"], golden[key + "_beta"]),
             grad_theta=rel_l2(c["grad_theta"], golden[key + "_grad_theta"]),
             grad_grid=rel_l2(c["grad_grid"].reshape(N, H, W, 2)[:, ::sg, ::sg], golden[key + "_grad_grid"]),
             grad_logits=rel_l2(c["grad_logits"][:, :, ::sl, ::sl], golden[key + "_grad_logits"]))
    print(key, " ".join("%s %.2e" % kv for kv in e.items()))
    # the grid's backward on its own gives the same theta gradient as the fused sums
    alone = theta_grad_of_grid_grad(theta, c["grad_grid"], H, W, cfg["normalised"])
    assert rel_l2(alone, c["grad_theta"]) < 1e-12
    return e


@pytest.mark.parametrize("order,reg", BEV_CASES)
def test_closed_form_matches_reference_bev(golden, order, reg):
    e = _check_against_reference(golden, BEV, "bev_o%d_r%g_f64" % (order, reg), order, reg)
    assert e["beta"] < 1e-9 and e["grad_theta"] < 1e-9 and e["grad_grid"] < 1e-9 and e["grad_logits"] < 1e-9, e


@pytest.mark.parametrize("order", [2, 3])
def test_closed_form_matches_reference_bp(golden, order):
    """Pixel coordinates, 256 x 512, four lanes, orders 2 and 3 (fp64 run only)."""
    e = _check_against_reference(golden, BP, "bp_o%d_f64" % order, order, 0.0)
    assert e["beta"] < 1e-9 and e["grad_theta"] < 1e-9 and e["grad_grid"] < 1e-9 and e["grad_logits"] < 1e-9, e


def test_shared_theta_is_the_sum_over_images():
    """A (3,3) theta shared by the batch: its gradient is the per-image gradients added (central differences agree)."""
    o = inputs.lane_like_logits(2, 2, 16, 32, seed=3)
    gb = np.random.default_rng(1).standard_normal((2, 2, 3))
    M, _ = fit_oracle.bev_homography()
    f = lambda th: float((fit_through_theta(o, th, gb, 5, 2, 0.0, 1.0, True)["beta"] * gb).sum())
    g = fit_through_theta(o, M, gb, 5, 2, 0.0, 1.0, True)["grad_theta"].sum(0)
    num = np.zeros((3, 3))
    for i in range(3):
        for j in range(3):
            d = np.zeros((3, 3))
            d[i, j] = 1e-5 * max(abs(M[i, j]), 0.1)
            num[i, j] = (f(M + d) - f(M - d)) / (2 * d[i, j])
    assert rel_l2(g, num) < 1e-6, (g, num)


@pytest.mark.parametrize("tree", ["bev", "bp"])
def test_grid_generator_follows_a_changed_theta(tree):
    """``ProjectiveGridGenerator`` called twice with different constant thetas returns different grids, each the host-made grid
    of its own theta; a theta that needs the device route is refused on the host, loudly."""
    import torch
    from lanedetection_end2end_amd import geometry
    mod = __import__("lanedetection_end2end_amd.%s.Networks.LSQ_layer" % tree, fromlist=["ProjectiveGridGenerator"])
    N, H, W = 2, 16, 32
    size = torch.Size([N, 2, H, W])
    M = (geometry.bev_homography() if tree == "bev" else geometry.get_homography(H))[0]
    a = torch.from_numpy(M).unsqueeze(0).expand(N, 3, 3).float()
    b = a * 1.01
    gen = mod.ProjectiveGridGenerator(size, a, True) if tree == "bev" else (lambda th: mod.ProjectiveGridGenerator(size, th, True))
    ga, gb_, ga2 = gen(a), gen(b), gen(a)
    assert ga.shape == (N, H * W, 2) and not torch.equal(ga, gb_) and torch.equal(ga, ga2)
    assert torch.equal(ga[0], geometry.projective_grid(H, W, M, tree == "bev"))
    assert torch.equal(gb_[1], geometry.projective_grid(H, W, b[0].double().numpy(), tree == "bev"))
    with pytest.raises(RuntimeError):
        gen(a.clone().requires_grad_(True))
