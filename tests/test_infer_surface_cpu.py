"""The inference engine beyond the whole-network call, as far as a machine without a GPU can check it: the new C entries (header,
library, ctypes table), the sizes of their workspaces against the inference and the training ones, the fused head + fit kernel's
register use, and the Python switches (``use_inference_engine`` reaches the ``--clas`` heads, ``detect`` refuses train mode)."""
import glob
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

ENTRIES = ("lf_erfnet_infer_range_workspace_bytes", "lf_erfnet_infer_range", "lf_convchain_infer_workspace_bytes",
           "lf_convchain_infer", "lf_head_fit", "lf_lane_infer_workspace_bytes", "lf_lane_infer")
# layer ranges of the plan (module order): encoder, decoder, one block of each kind
RANGES = {"encoder": (0, 16), "decoder": (16, 22), "stem": (0, 1), "down": (1, 2), "nb64": (2, 3), "nb128": (8, 9), "up": (16, 17),
          "nb16": (20, 21)}


def test_entries_in_header_library_and_table():
    from lanedetection_end2end_amd import _lib
    header = open(os.path.join(ROOT, "include", "lanefit.h")).read()
    lib = _lib.load()
    table = _lib.exported_symbols()
    for name in ENTRIES:
        assert re.search(r"\b%s\(" % name, header), name
        assert hasattr(lib, name), name
        assert name in table, name
    assert "additions since 5" in header and lib.lf_abi_version() == 5


@pytest.mark.parametrize("mode", [0, 2, 3])
def test_range_workspace_sizes(mode):
    from lanedetection_end2end_amd import _lib
    from lanedetection_end2end_amd.erfnet import _Plan
    lib = _lib.load()
    N, H, W = 32, 256, 512
    plan = _Plan(N, H, W, 3, 2, 1)
    assert lib.lf_erfnet_num_layers(plan.handle) == 22
    whole = lib.lf_erfnet_infer_workspace_bytes(plan.handle, mode)
    import ctypes
    io = (ctypes.c_int * 6)()
    for name, (first, last) in RANGES.items():
        got = lib.lf_erfnet_infer_range_workspace_bytes(plan.handle, first, last, mode)
        # NCHW <-> NHWC staging of the range's input and output, in the mode's storage type
        lib.lf_erfnet_layer_io(plan.handle, first, io)
        staging = N * io[0] * io[1] * io[2]
        lib.lf_erfnet_layer_io(plan.handle, last - 1, io)
        staging += N * io[3] * io[4] * io[5]
        staging *= 2 if mode == 2 else 4
        assert 0 < got <= whole + staging, (name, got, whole, staging)
        assert got < lib.lf_erfnet_range_workspace_bytes(plan.handle, first, last), (name, got)
    for first, last in ((3, 3), (5, 2), (-1, 4), (0, 23)):
        assert lib.lf_erfnet_infer_range_workspace_bytes(plan.handle, first, last, mode) == 0
    for bad in (1, 4, 7, -1):
        assert lib.lf_erfnet_infer_range_workspace_bytes(plan.handle, 0, 16, bad) == 0


def test_convchain_and_lane_infer_sizes():
    from lanedetection_end2end_amd import _lib
    from lanedetection_end2end_amd.clas import _ChainPlan
    from lanedetection_end2end_amd.erfnet import _Plan
    lib = _lib.load()
    chain = _ChainPlan(32, 32, 64, (128, 128, 128, 64, 64), (1, 3, 3, 3))
    for mode in (0, 2):
        got = lib.lf_convchain_infer_workspace_bytes(chain.handle, mode)
        assert 0 < got < lib.lf_convchain_workspace_bytes_for(chain.handle, mode), (mode, got)
    assert lib.lf_convchain_infer_workspace_bytes(chain.handle, 2) < lib.lf_convchain_infer_workspace_bytes(chain.handle, 0)
    assert lib.lf_convchain_infer_workspace_bytes(chain.handle, 3) == 0
    plan = _Plan(32, 256, 512, 3, 2, 1)
    for mode in (0, 2, 3):
        for order in (0, 1, 2, 3):
            got = lib.lf_lane_infer_workspace_bytes(plan.handle, mode, 2, order)
            whole = lib.lf_erfnet_infer_workspace_bytes(plan.handle, mode)
            # the inference workspace + the chunk partials + the saved inverse: well under 1 MiB on top
            assert whole < got < whole + (1 << 20), (mode, order, got, whole)
    assert lib.lf_lane_infer_workspace_bytes(plan.handle, 1, 2, 2) == 0
    assert lib.lf_lane_infer_workspace_bytes(plan.handle, 0, 3, 2) == 0          # K is the plan's out_channels
    assert lib.lf_lane_infer_workspace_bytes(plan.handle, 0, 2, 4) == 0


@pytest.fixture(scope="module")
def fit_kernels(tmp_path_factory):
    from lanedetection_end2end_amd import build
    import isa_meta
    d = tmp_path_factory.mktemp("isa_fit")
    src = os.path.join(build.CSRC, "lf_fit.hip")
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + build.FLAGS + ["-c", src, "-o", str(d / "lf_fit.o"), "-save-temps=obj"]
    subprocess.check_call(cmd, cwd=str(d))
    asm = glob.glob(str(d / "*gfx950*.s"))
    assert asm, "no device assembly produced"
    return isa_meta.kernels(asm[0])


def test_head_moments_kernels_have_no_spills(fit_kernels):
    found = [k for k in fit_kernels if "head_moments_kernel" in k["name"]]
    names = sorted(k["name"] for k in found)
    assert len(found) == 8, names            # orders 0..3, fp32 and bf16 input
    for k in found:
        assert k["vgpr_spill"] == 0 and k["scratch"] == 0 and k["loop_scratch"] == 0, k
        # the head's weights stay in LDS inside the pixel loop: at least two 256-thread workgroups per CU (512 registers per lane)
        assert k["vgpr"] + k["agpr"] <= 256, k


def test_switch_reaches_the_heads_and_detect_needs_eval(monkeypatch):
    import torch
    import torch.nn as nn
    import lanedetection_end2end_amd as pkg
    from lanedetection_end2end_amd import clas, lsq
    monkeypatch.delenv("LANEFIT_INFERENCE_ENGINE", raising=False)
    head = clas.Classification('horizon', size=(32, 64), channels_in=128, resize=256)
    assert head.inference_engine is False
    outer = nn.ModuleDict({"h": head})
    pkg.use_inference_engine(outer)
    assert head.inference_engine is True
    pkg.use_inference_engine(outer, False)
    assert head.inference_engine is False
    monkeypatch.setenv("LANEFIT_INFERENCE_ENGINE", "1")
    assert clas.ClassificationBEV('line', size=(32, 64), channels_in=128, resize=256).inference_engine is True
    assert head.inference_engine is False
    # detect: on both wrappers' common base, and only in eval mode
    assert callable(getattr(lsq._LaneFitNet, "detect"))

    class Stub(lsq._LaneFitNet):
        def __init__(self):
            nn.Module.__init__(self)
            self.net = nn.Module()
            self.classification_branch = False
    m = Stub()
    m.train()
    with pytest.raises(RuntimeError, match="eval"):
        m.detect(torch.zeros(1, 3, 64, 128))
