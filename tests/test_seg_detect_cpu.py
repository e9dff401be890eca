"""One-call detect for segmentation-mode models, the part that needs no GPU: the three C entries (header block, library, ctypes
table), the size of the call's workspace, the register use of every ``segfit_kernel`` instantiation, and the Python guards
(``detect`` / ``segment`` refuse train mode, ``segment`` refuses an end-to-end model)."""
import glob
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

ENTRIES = ("lf_head_fit_seg", "lf_lane_infer_seg_workspace_bytes", "lf_lane_infer_seg")
BLOCK = "additions since 5 -- segmentation-mode detect"


def test_entries_in_header_block_library_and_table():
    from lanedetection_end2end_amd import _lib
    header = open(os.path.join(ROOT, "include", "lanefit.h")).read()
    assert BLOCK in header
    start = header.index(BLOCK)
    # the last block of the header: every "additions since 5 --" heading lies before it
    assert start == max(m.start() for m in re.finditer(r"additions since 5 --", header))
    lib = _lib.load()
    table = _lib.exported_symbols()
    for name in ENTRIES:
        m = re.search(r"\b%s\(" % name, header)
        assert m and m.start() > start, name
        assert hasattr(lib, name), name
        assert name in table, name
    # ... and the list at the top names them
    top = header[:header.index("*/", header.index("#define LF_ABI_VERSION"))]
    assert "segmentation-mode detect" in top and all(name in top for name in ENTRIES)
    assert re.search(r"#define LF_ABI_VERSION 5\b", header) and lib.lf_abi_version() == 5


def test_workspace_sizes():
    from lanedetection_end2end_amd import _lib
    from lanedetection_end2end_amd.erfnet import _Plan
    lib = _lib.load()
    plan = _Plan(32, 256, 512, 3, 3, 1)
    for mode in (0, 2, 3):
        whole = lib.lf_erfnet_infer_workspace_bytes(plan.handle, mode)
        for order in (0, 1, 2, 3):
            for L in (1, 2, 4):
                got = lib.lf_lane_infer_seg_workspace_bytes(plan.handle, mode, L, order)
                # the inference workspace + the chunk partials + the saved inverses of N * L lanes: under 1 MiB on top
                assert whole < got < whole + (1 << 20), (mode, order, L, got, whole)
    assert lib.lf_lane_infer_seg_workspace_bytes(plan.handle, 1, 2, 2) == 0
    assert lib.lf_lane_infer_seg_workspace_bytes(plan.handle, 0, 2, 4) == 0
    assert lib.lf_lane_infer_seg_workspace_bytes(plan.handle, 0, 0, 2) == 0
    assert lib.lf_lane_infer_seg_workspace_bytes(plan.handle, 0, 5, 2) == 0


def test_segfit_kernels_fit_two_workgroups_per_cu(tmp_path):
    from lanedetection_end2end_amd import build
    import isa_meta
    src = os.path.join(build.CSRC, "lf_fit.hip")
    cmd = ([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + build.FLAGS +
           ["-c", src, "-o", str(tmp_path / "lf_fit.o"), "-save-temps=obj"])
    subprocess.check_call(cmd, cwd=str(tmp_path))
    asm = glob.glob(str(tmp_path / "*gfx950*.s"))
    assert asm, "no device assembly produced"
    found = [k for k in isa_meta.kernels(asm[0]) if "segfit_kernel" in k["mangled"]]
    # orders 0..3, fp32 and bf16 input, 1 / 2 / 4 lanes per workgroup
    assert len(found) == 24, sorted(k["mangled"] for k in found)
    for k in sorted(found, key=lambda k: k["mangled"]):
        print("%-90s vgpr %3d agpr %3d lds %5d" % (k["mangled"], k["vgpr"], k["agpr"], k["lds"]))
        assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0 and k["loop_scratch"] == 0, k
        # two 256-thread workgroups per CU (512 registers per lane), the bound head_moments_kernel is held to
        assert k["vgpr"] + k["agpr"] <= 256, k


def _stub(end_to_end, training):
    import torch.nn as nn
    from lanedetection_end2end_amd import lsq

    class Stub(lsq._LaneFitNet):
        def __init__(self):
            nn.Module.__init__(self)
            self.net = nn.Module()
            self.classification_branch = False
            self.end_to_end = end_to_end
            self.pretrained = False
    m = Stub()
    return m.train() if training else m.eval()


def test_detect_and_segment_need_eval_mode():
    import torch
    from lanedetection_end2end_amd import lsq
    assert lsq._LaneFitNet.fused_seg_detect is True
    m = _stub(False, True)
    assert m.fused_seg_detect is True
    x = torch.zeros(1, 3, 64, 128)
    with pytest.raises(RuntimeError, match="eval"):
        m.detect(x)
    with pytest.raises(RuntimeError, match="eval"):
        m.segment(x)
    m.eval()
    m.net.train()                    # the backbone alone in train mode is refused too
    with pytest.raises(RuntimeError, match="eval"):
        m.segment(x)


def test_segment_refuses_an_end_to_end_model():
    import torch

    class OnDevice:                  # (what the guards look at of an input; nothing is launched)
        is_cuda = True
        shape = torch.Size((1, 3, 64, 128))
    m = _stub(True, False)
    with pytest.raises(RuntimeError, match="segmentation-mode"):
        m.segment(OnDevice())
