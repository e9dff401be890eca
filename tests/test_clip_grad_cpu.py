"""Gradient-norm clipping without a device: the C surface, the resources of its kernels, the Python surface, and the NumPy statement
of the clip (tests/clip_ref.py) pinned to ``torch.nn.utils.clip_grad_norm_``."""
import ctypes
import glob
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
import clip_ref as C
import optim_ref as R

sys.path.insert(0, os.path.join(ROOT, "tools"))

SYMBOLS = ("lf_grad_norm_workspace_bytes", "lf_grad_sumsq", "lf_grad_norm_finish", "lf_grad_scale_inplace",
           "lf_adam_step_clipped", "lf_sgd_step_clipped", "lf_rmsprop_step_clipped")


def test_symbols_exported_and_declared():
    from lanedetection_end2end_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "lanefit.h")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "additions since 5 (gradient-norm clipping): lf_grad_norm_workspace_bytes" in header
    block = header[header.index("additions since 5 -- gradient-norm clipping"):]
    block = block[:block.index("lf_rmsprop_step_clipped(") + 400]
    assert "BP/main.py:334-335" in block and "error_if_nonfinite=False" in block
    exported = _lib.exported_symbols()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in exported, name
        assert re.search(r"\b(int|size_t) %s\(" % name, block), name
        assert name in integration, name
    assert "#define LF_ABI_VERSION 5" in header and lib.lf_abi_version() == 5
    assert lib.lf_grad_norm_workspace_bytes(0) == 0
    lib.lf_grad_norm_workspace_bytes.restype = ctypes.c_size_t
    assert lib.lf_grad_norm_workspace_bytes(700) == 700 * 8


def test_refusals_come_before_any_launch():
    """Bad arguments return an error from the host side of the entry points (no device is present here, so a launch would fail
    differently): null tables, no blocks, a null coefficient, a misaligned workspace."""
    from lanedetection_end2end_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(16)
    f = ctypes.c_float
    assert lib.lf_grad_sumsq(None, one, 1, 0, one, None) != 0 and b"lf_grad_sumsq: bad arguments" in lib.lf_last_error()
    assert lib.lf_grad_sumsq(one, one, 0, 0, one, None) != 0
    assert lib.lf_grad_sumsq(one, one, 1, -1, one, None) != 0
    assert lib.lf_grad_sumsq(one, one, 1, 0, ctypes.c_void_p(20), None) != 0
    assert lib.lf_grad_norm_finish(one, 0, f(1), f(1), one, None) != 0 and b"lf_grad_norm_finish" in lib.lf_last_error()
    assert lib.lf_grad_norm_finish(one, 1, f(1), f(1), None, None) != 0
    assert lib.lf_grad_scale_inplace(one, one, 1, f(1), None, None) != 0 and b"lf_grad_scale_inplace" in lib.lf_last_error()
    assert lib.lf_adam_step_clipped(one, one, 1, f(1), f(.9), f(.999), f(1e-8), f(0), 0, f(1), None, None) != 0
    assert lib.lf_adam_step_clipped(one, one, 1, f(1), f(.9), f(.999), f(1e-8), f(0), 2, f(1), one, None) != 0
    assert lib.lf_sgd_step_clipped(one, one, 1, f(1), f(.9), f(0), f(1), None, None) != 0
    assert lib.lf_rmsprop_step_clipped(one, one, 0, f(1), f(.99), f(1e-8), f(.9), f(0), f(1), one, None) != 0


def test_clip_kernels_do_not_spill(tmp_path):
    from lanedetection_end2end_amd import build
    import isa_meta
    src = os.path.join(build.CSRC, "lf_optim.hip")
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + build.FLAGS + ["-c", src, "-o", str(tmp_path / "lf_optim.o"), "-save-temps=obj"]
    subprocess.check_call(cmd, cwd=str(tmp_path))
    asm = glob.glob(str(tmp_path / "*gfx950*.s"))
    assert asm, "no device assembly produced"
    ks = {k["name"]: k for k in isa_meta.kernels(asm[0])}
    want = ["grad_sumsq_kernel", "grad_norm_finish_kernel", "grad_scale_inplace_kernel"] + \
           ["opt_kernel<%d, %s>" % (op, flag) for op in (0, 1, 2) for flag in ("false", "true")]
    assert sorted(ks) == sorted(want)
    for name in want:
        k = ks[name]
        assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, k
        assert k["vgpr"] + k["agpr"] <= 128, k


def test_python_surface():
    from lanedetection_end2end_amd import optim
    p = [torch.nn.Parameter(torch.ones(3))]
    assert list(inspect.signature(optim.define_optim).parameters)[:4] == ["optim", "params", "lr", "weight_decay"]
    for kind, cls in (("adam", optim.FusedAdam), ("sgd", optim.FusedSGD), ("rmsprop", optim.FusedRMSprop)):
        opt = optim.define_optim(kind, p, 1e-3, 1e-2)                   # the reference's four-argument call
        assert type(opt) is cls and opt.max_grad_norm == 0 and opt.last_grad_norm is None
        assert optim.define_optim(kind, p, 1e-3, 1e-2, clip_grad_norm=1).max_grad_norm == 1.0
        assert cls(p, max_grad_norm=2.5).max_grad_norm == 2.5 and cls(p).max_grad_norm == 0
    assert optim.clip_grad_norm is optim.clip_grad_norm_
    assert list(inspect.signature(optim.clip_grad_norm_).parameters)[:3] == ["parameters", "max_norm", "norm_type"]
    with pytest.raises(NotImplementedError):
        optim.clip_grad_norm_(p, 1.0, norm_type=1)
    with pytest.raises(NotImplementedError):
        optim.clip_grad_norm_(p, 1.0, norm_type=float("inf"))
    # no parameter has a gradient: a zero norm, nothing launched (there is no device here to launch on)
    total = optim.clip_grad_norm_(p, 1.0)
    assert float(total) == 0.0 and float(optim.clip_grad_norm_(p[0], 1.0, 2)) == 0.0
    # a host gradient is refused, not computed somewhere else
    p[0].grad = torch.ones(3)
    from lanedetection_end2end_amd._lib import LaneFitLibraryError
    with pytest.raises(LaneFitLibraryError):
        optim.clip_grad_norm_(p, 1.0)


def _torch_clip(grads, max_norm, dtype):
    params = [torch.nn.Parameter(torch.zeros(len(g), dtype=dtype)) for g in grads]
    for p, g in zip(params, grads):
        p.grad = torch.from_numpy(np.array(g)).to(dtype)
    total = torch.nn.utils.clip_grad_norm_(params, max_norm)
    return total, [p.grad.numpy() for p in params]


@pytest.mark.parametrize("max_norm", [1e-3, 1.0, 100.0, 1e4])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["fp64", "fp32"])
def test_statement_is_torchs_clip(max_norm, dtype):
    """torch's routine on CPU tensors against the statement, in float64 and in the kernels' float32.  The norm: to 1e-14 in fp64
    (torch adds per-tensor norms, the statement all squares at once).  From torch's own norm, the clipped gradients are
    ``g * coef`` bit for bit once the coefficient is rounded the way torch rounds it (reciprocal, then product); the statement's
    coefficient is the correctly rounded quotient, at most 3 rounding units u from torch's, so the gradients agree within 5 u (two
    more for the two products)."""
    u = 2.0 ** (-53 if dtype is np.float64 else -24)
    grads = [t["g"].astype(dtype) for t in R.make_inputs(0)]
    total, after = _torch_clip(grads, max_norm, torch.float64 if dtype is np.float64 else torch.float32)
    total = dtype(float(total))
    want = C.norm_f64(grads)
    assert abs(want - 2730.2) < 0.05
    if dtype is np.float64:
        assert abs(float(total) - want) <= 1e-14 * want
    else:
        ratio = abs(float(total) - want) / (C.NORM_TOL * want)
        print("torch fp32 clip_grad_norm_: |norm - fp64| = %.2f of the GPU test's gate" % ratio)
        assert abs(float(np.float32(want)) - want) <= 0.5 * C.NORM_TOL * want   # the correctly rounded norm: half the gate at most
    c_torch, c = C.coef_as_torch_rounds_it(total, max_norm, dtype), C.coef(total, max_norm, dtype)
    assert type(c) is dtype and abs(float(c) - float(c_torch)) <= 3 * u * float(c)
    assert (c == 1.0) == (max_norm > want) == (c_torch == 1.0)
    for g, a in zip(grads, after):
        assert np.array_equal(a, C.effective(g, 1.0, c_torch))
        assert (np.abs(a.astype(np.float64) - C.effective(g, 1.0, c).astype(np.float64)) <= 5 * u * np.abs(a)).all()
    # the whole statement from the gradients alone
    t2, c2, clipped = C.clip(grads, max_norm)
    assert type(t2) is dtype and abs(float(t2) - want) <= u * want + 1e-14 * want
    if dtype is np.float64:
        for a, b in zip(after, clipped):
            assert np.allclose(a, b, rtol=1e-13, atol=0)


def test_two_roundings_differ_from_one():
    """fl(fl(g * s) * c) is not fl(g * (s * c)): the statement keeps the two products apart, as torch's in-place rewrite after a
    scaled gradient does, and the bit-equality tests on the GPU can tell the two."""
    g = np.concatenate([t["g"] for t in R.make_inputs(0)])
    s, c = np.float32(0.125), np.float32(0.3662737)
    two = C.effective(g, s, c)
    assert np.array_equal(two, (g * s) * c)
    s3 = np.float32(1.0 / 3.0)
    assert (C.effective(g, s3, c) != g * np.float32(s3 * c)).mean() > 0.1


def test_non_finite_semantics_are_torchs():
    g = [np.array([1.0, -2.0, np.inf, 3.0], np.float32), np.array([0.5], np.float32)]
    total, after = _torch_clip(g, 1.0, torch.float32)
    t, c, mine = C.clip(g, 1.0)
    assert np.isinf(float(total)) and np.isinf(t) and c == 0
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(after, mine))
    assert np.isnan(mine[0][2]) and (mine[0][[0, 1, 3]] == 0).all()
    g[0][2] = np.nan
    total, after = _torch_clip(g, 1.0, torch.float32)
    t, c, mine = C.clip(g, 1.0)
    assert np.isnan(float(total)) and np.isnan(t) and np.isnan(c)
    assert all(np.isnan(a).all() and np.isnan(b).all() for a, b in zip(after, mine))
    z = [np.zeros(5, np.float32)]
    total, after = _torch_clip(z, 1.0, torch.float32)
    t, c, mine = C.clip(z, 1.0)
    assert float(total) == 0 and t == 0 and c == 1 and not np.isnan(mine[0]).any()
    # 1e30 and -3e30: the squares overflow fp32, the fp64 statement does not
    big = [np.array([1e30, -3e30], np.float32)]
    assert np.isinf(np.float32(1e30) * np.float32(1e30))
    assert abs(C.norm_f64(big) - 3.1623e30) < 1e26
