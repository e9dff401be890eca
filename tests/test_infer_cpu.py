"""The inference engine's CPU-checkable surface: the C entries (header, library, ctypes table), the size of its workspace against
the training engine's, the compiled-in bias + residual + ReLU epilogues of the forward convolutions (spills, registers), and the
``inference_engine`` switch of the ERFNet module (default, environment variable, ``use_inference_engine``)."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

ENTRIES = ("lf_erfnet_infer_workspace_bytes", "lf_erfnet_infer_encoder_offset", "lf_erfnet_infer")
BRES = 4 | 1 | 64        # LF_EPI_ADD | LF_EPI_RELU | LF_EPI_BIAS (csrc/lf_conv.h)


def test_entries_in_header_library_and_table():
    from lanedetection_end2end_amd import _lib
    header = open(os.path.join(ROOT, "include", "lanefit.h")).read()
    lib = _lib.load()
    table = _lib.exported_symbols()
    for name in ENTRIES:
        assert re.search(r"\b%s\(" % name, header), name
        assert hasattr(lib, name), name
        assert name in table, name


def test_workspace_is_a_fraction_of_the_training_one():
    from lanedetection_end2end_amd import _lib
    from lanedetection_end2end_amd.erfnet import _Plan
    lib = _lib.load()
    plan = _Plan(32, 256, 512, 3, 2, 1)
    f32 = lib.lf_erfnet_infer_workspace_bytes(plan.handle, 0)
    bf16 = lib.lf_erfnet_infer_workspace_bytes(plan.handle, 2)
    x9 = lib.lf_erfnet_infer_workspace_bytes(plan.handle, 3)
    assert f32 > 0 and bf16 > 0 and x9 > 0
    assert f32 * 8 <= lib.lf_erfnet_workspace_bytes_for(plan.handle, 0), (f32, lib.lf_erfnet_workspace_bytes_for(plan.handle, 0))
    assert bf16 <= f32
    assert lib.lf_erfnet_infer_workspace_bytes(plan.handle, 1) == 0 and lib.lf_erfnet_infer_workspace_bytes(plan.handle, 7) == 0
    # the encoder output (N, H/8, W/8, 128) lies inside the workspace in every mode
    off = lib.lf_erfnet_infer_encoder_offset(plan.handle)
    assert off >= 0 and 4 * off + 2 * 32 * 32 * 64 * 128 <= bf16 and 4 * off + 4 * 32 * 32 * 64 * 128 <= f32


@pytest.fixture(scope="module")
def conv_kernels(tmp_path_factory):
    import isa_meta
    return isa_meta.compile_kernels(["lf_conv.hip", "lf_conv_bf16.hip"], tmp_path_factory.mktemp("isa_infer"))


def test_bias_residual_epilogues_are_compiled_in(conv_kernels):
    by = {k["name"]: k for k in conv_kernels}
    want = {
        "tapgemm_kernel<4, 0, %d, true, false>" % BRES: 256,      # fp32 64-channel slab, whole-row waves
        "tapgemm_kernel<4, 0, %d, false, false>" % BRES: 256,     # ... ragged rows
        "tapgemm_lean_kernel<1, 0, %d>" % BRES: 128,              # fp32 16 channels
        "tapgemm_bf16_wv_kernel<%d>" % BRES: 256,                 # bf16 64 channels
        "tapgemm_bf16_wl_kernel<4, %d, 0>" % BRES: 256,           # bf16 128 channels
        "tapgemm_bf16_lean_kernel<0, %d>" % BRES: 128,            # bf16 16 channels
    }
    for name, budget in want.items():
        assert name in by, (name, sorted(n for n in by if str(BRES) in n))
        k = by[name]
        regs = k["vgpr"] if budget == 128 else k["vgpr"] + k["agpr"]
        assert regs <= budget, (name, k["vgpr"], k["agpr"])
        assert k["vgpr_spill"] == 0 and k["scratch"] == 0 and k["loop_scratch"] == 0, (name, k)


def test_inference_engine_switch(monkeypatch):
    import torch.nn as nn
    import lanedetection_end2end_amd as pkg
    from lanedetection_end2end_amd.erfnet import Net
    monkeypatch.delenv("LANEFIT_INFERENCE_ENGINE", raising=False)
    net = Net(layers=18, in_channels=3, out_channels=2)
    assert net.inference_engine is False
    monkeypatch.setenv("LANEFIT_INFERENCE_ENGINE", "1")
    assert Net(layers=18, in_channels=3, out_channels=2).inference_engine is True
    assert net.inference_engine is False                 # read when a Net is built, not later
    monkeypatch.setenv("LANEFIT_INFERENCE_ENGINE", "0")
    assert Net(layers=18, in_channels=3, out_channels=2).inference_engine is False
    outer = nn.Sequential(nn.Module(), nn.ModuleDict({"net": net}))
    assert pkg.use_inference_engine(outer) is outer
    assert net.inference_engine is True
    pkg.use_inference_engine(outer, False)
    assert net.inference_engine is False
