"""The frozen single-frame detector, the part that needs no GPU: the new C entries and debug hooks (headers, library, ctypes table),
the registers of every ``tapgemm_thin_kernel`` instantiation beside the instantiations ``tests/test_infer_cpu.py`` names, the size of a
one-frame workspace, and the guards of ``detector()`` that fire before anything is launched."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

ENTRIES = ("lf_erfnet_infer_fold", "lf_lane_infer_folded", "lf_lane_infer_seg_folded")
HOOKS = ("lf_debug_set_thin", "lf_debug_thin_launches", "lf_debug_fold_pack_launches")
BLOCK = "additions since 5 -- frozen single-frame detector"
RELU, BRES = 1, 4 | 1 | 64        # LF_EPI_RELU; LF_EPI_ADD | LF_EPI_RELU | LF_EPI_BIAS (csrc/lf_conv.h)


def test_entries_and_hooks_in_headers_library_and_table():
    from lanedetection_end2end_amd import _lib
    header = open(os.path.join(ROOT, "include", "lanefit.h")).read()
    debug = open(os.path.join(ROOT, "lanedetection_end2end_amd", "csrc", "lf_debug.h")).read()
    lib = _lib.load()
    table = _lib.exported_symbols()
    start = header.index(BLOCK)
    nxt = header.find("additions since 5 --", start + len(BLOCK))
    block = header[start: nxt if nxt >= 0 else len(header)]
    for name in ENTRIES:
        assert re.search(r"\bint %s\(" % name, block), name
        assert hasattr(lib, name) and name in table, name
    assert re.search(r"\bLF_INFER_THIN = 1\b", block)
    for name in HOOKS:
        assert re.search(r"\b%s\(" % name, debug), name
        assert hasattr(lib, name) and name in table, name
    # the ABI number stays, the list at the top names the additions
    top = header[:header.index("*/", header.index("#define LF_ABI_VERSION"))]
    assert "additions since 5 (frozen single-frame detector): " + ", ".join(ENTRIES[:2]) in top and ENTRIES[2] in top
    assert re.search(r"#define LF_ABI_VERSION 5\b", header) and lib.lf_abi_version() == 5


@pytest.fixture(scope="module")
def conv_kernels(tmp_path_factory):
    import isa_meta
    return isa_meta.compile_kernels(["lf_conv.hip"], tmp_path_factory.mktemp("isa_thin"))


def test_thin_kernels_do_not_spill(conv_kernels):
    thin = {k["name"]: k for k in conv_kernels if k["name"].startswith("tapgemm_thin_kernel<")}
    want = {"tapgemm_thin_kernel<%d, %d>" % (nt, e) for nt in (1, 2, 3, 4) for e in (RELU, BRES)}
    assert set(thin) == want, sorted(thin)
    for name, k in sorted(thin.items()):
        print("%-40s vgpr %3d agpr %3d lds %5d" % (name, k["vgpr"], k["agpr"], k["lds"]))
        assert k["vgpr_spill"] == 0 and k["scratch"] == 0 and k["loop_scratch"] == 0, (name, k)
        assert k["vgpr"] + k["agpr"] <= 256, (name, k["vgpr"], k["agpr"])


def test_regular_instantiations_keep_their_budgets(conv_kernels):
    """What tests/test_infer_cpu.py names of lf_conv.hip: still there, within the same budgets."""
    by = {k["name"]: k for k in conv_kernels}
    want = {"tapgemm_kernel<4, 0, %d, true, false>" % BRES: 256, "tapgemm_kernel<4, 0, %d, false, false>" % BRES: 256,
            "tapgemm_lean_kernel<1, 0, %d>" % BRES: 128}
    for name, budget in want.items():
        assert name in by, name
        k = by[name]
        regs = k["vgpr"] if budget == 128 else k["vgpr"] + k["agpr"]
        assert regs <= budget, (name, k["vgpr"], k["agpr"])
        assert k["vgpr_spill"] == 0 and k["scratch"] == 0 and k["loop_scratch"] == 0, (name, k)


def test_one_frame_workspace():
    from lanedetection_end2end_amd import _lib
    from lanedetection_end2end_amd.erfnet import _Plan
    lib = _lib.load()
    one, full = _Plan(1, 256, 512, 3, 2, 1), _Plan(32, 256, 512, 3, 2, 1)
    for mode in (0, 2, 3):
        a, b = lib.lf_lane_infer_workspace_bytes(one.handle, mode, 2, 2), lib.lf_lane_infer_workspace_bytes(full.handle, mode, 2, 2)
        assert 0 < a < b, (mode, a, b)
        # the folded region is the common prefix of the three workspaces
        whole = lib.lf_erfnet_infer_workspace_bytes(one.handle, mode)
        assert whole <= a and whole <= lib.lf_lane_infer_seg_workspace_bytes(one.handle, mode, 2, 2)


def _stub(end_to_end, pretrained, training):
    import torch.nn as nn
    from lanedetection_end2end_amd import lsq

    class Stub(lsq._LaneFitNet):
        def __init__(self):
            nn.Module.__init__(self)
            self.net = nn.Module()
            self.net.in_channels, self.net.out_channels, self.net.pretrained = 3, 2, pretrained
            self.classification_branch = False
            self.end_to_end = end_to_end
            self.pretrained = pretrained
            self.resize = 64
    m = Stub()
    return m.train() if training else m.eval()


def test_detector_guards():
    from lanedetection_end2end_amd import lsq
    assert isinstance(lsq.THIN_AUTO_MAX_BATCH, int) and 0 <= lsq.THIN_AUTO_MAX_BATCH <= 8
    with pytest.raises(RuntimeError, match="detect"):
        _stub(False, True, False).detector()          # pretrained segmentation-mode: the one form detect keeps off the one-call path
    with pytest.raises(RuntimeError, match="eval"):
        _stub(True, False, True).detector()
    with pytest.raises(ValueError, match="thin"):
        _stub(True, False, False).detector(thin="yes")
