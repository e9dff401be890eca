"""Input-image gradient, the part that needs no GPU: the fp64 reference of the stem's data gradient (tests/input_grad_ref.py)
against torch autograd, the two C entries (header block, library, ctypes table), and the register use of every
``stem_bwd_data_kernel`` instantiation."""
import glob
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from input_grad_ref import input_grad_ref

SYMBOLS = ("lf_stem_bwd_data", "lf_erfnet_backward_input")
BLOCK = "additions since 5 -- input-image gradient"


def _autograd(gcat, img, w):
    x = torch.from_numpy(img).double().requires_grad_(True)
    cat = torch.cat([F.conv2d(x, torch.from_numpy(w).double(), stride=2, padding=1), F.max_pool2d(x, 2)], 1)
    cat.backward(torch.from_numpy(gcat).double().permute(0, 3, 1, 2))
    return x.grad.numpy()


@pytest.mark.parametrize("shape", [(2, 3, 6, 32), (1, 4, 10, 18)])
def test_reference_equals_autograd(shape):
    N, Cin, H, W = shape
    rng = np.random.default_rng(7 + H)
    img = rng.standard_normal(shape)
    gcat = rng.standard_normal((N, H // 2, W // 2, 16))
    w = rng.standard_normal((16 - Cin, Cin, 3, 3))
    R, S = input_grad_ref(gcat, img, w)
    ref = _autograd(gcat, img, w)
    # the same <= 61 products per element, summed in another order, in fp64
    assert np.all(np.abs(R - ref) <= 64 * 2.0 ** -53 * S)
    assert np.all(S >= np.abs(R)) and S.min() > 0


def test_ties_go_to_the_first_pixel_of_the_window():
    """An image of constant 2x2 windows: all four values tie, and the pooled gradient lands on the window's first pixel."""
    N, Cin, H, W = 2, 3, 6, 32
    rng = np.random.default_rng(11)
    img = np.repeat(np.repeat(rng.standard_normal((N, Cin, H // 2, W // 2)), 2, axis=2), 2, axis=3)
    gcat = rng.standard_normal((N, H // 2, W // 2, 16))
    w = rng.standard_normal((16 - Cin, Cin, 3, 3))
    R, S = input_grad_ref(gcat, img, w)
    assert np.all(np.abs(R - _autograd(gcat, img, w)) <= 64 * 2.0 ** -53 * S)
    # the pool term alone (zero weights): the first pixel of every window holds the pooled channel's gradient, the others exactly 0
    R0, _ = input_grad_ref(gcat, img, np.zeros_like(w))
    assert np.array_equal(R0[:, :, 0::2, 0::2], gcat[..., 16 - Cin:].transpose(0, 3, 1, 2))
    assert not R0[:, :, 0::2, 1::2].any() and not R0[:, :, 1::2, :].any()
    assert np.array_equal(R0, _autograd(gcat, img, np.zeros_like(w)))


def test_entries_in_header_block_library_table_and_integration():
    from lanedetection_end2end_amd import _lib
    header = open(os.path.join(ROOT, "include", "lanefit.h")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "additions since 5 (input-image gradient): lf_stem_bwd_data, lf_erfnet_backward_input" in header
    start = header.index(BLOCK)
    nxt = header.find("additions since 5 --", start + len(BLOCK))
    block = header[start: nxt if nxt >= 0 else len(header)]
    lib = _lib.load()
    table = _lib.exported_symbols()
    for name in SYMBOLS:
        assert re.search(r"\bint %s\(" % name, block), name
        assert len(re.findall(r"\bint %s\(" % name, header)) == 1, name
        assert hasattr(lib, name), name
        assert name in table, name
        assert name in integration, name
    # the reference lines the block answers
    assert "BEV/Networks/ERFNet.py:11-22,66" in block and "BEV/main.py:264-266" in block
    assert re.search(r"#define LF_ABI_VERSION 5\b", header) and lib.lf_abi_version() == 5
    assert "gx is not produced for first = 0" not in header


def test_stem_bwd_data_kernels_do_not_spill(tmp_path):
    from lanedetection_end2end_amd import build
    import isa_meta
    src = os.path.join(build.CSRC, "lf_stem.hip")
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + build.FLAGS + ["-c", src, "-o", str(tmp_path / "lf_stem.o"), "-save-temps=obj"]
    subprocess.check_call(cmd, cwd=str(tmp_path))
    asm = glob.glob(str(tmp_path / "*gfx950*.s"))
    assert asm, "no device assembly produced"
    mine = [k for k in isa_meta.kernels(asm[0]) if "stem_bwd_data_kernel" in k["mangled"]]
    # in_channels 1..4, fp32 and bf16 gradient tensors
    assert len(mine) == 8, sorted(k["mangled"] for k in mine)
    for k in sorted(mine, key=lambda k: k["mangled"]):
        print("%-80s vgpr %3d agpr %3d lds %5d" % (k["mangled"], k["vgpr"], k["agpr"], k["lds"]))
        assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0 and k["loop_scratch"] == 0, k
        assert k["vgpr"] + k["agpr"] <= 256, k           # one 256-thread workgroup per SIMD row at the least
