"""The thin bf16 tap-GEMM, the part that needs no GPU: its two debug hooks (header, library, ctypes table), the registers of every
``tapgemm_bf16_thin_kernel`` instantiation beside the bf16 instantiations ``tests/test_infer_cpu.py`` names, and the detector's
constant."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

HOOKS = ("lf_debug_set_thin_bf16", "lf_debug_thin_bf16_launches")
RELU, BRES = 1, 4 | 1 | 64        # LF_EPI_RELU; LF_EPI_ADD | LF_EPI_RELU | LF_EPI_BIAS (csrc/lf_conv.h)


def test_hooks_in_header_library_and_table():
    from lanedetection_end2end_amd import _lib
    debug = open(os.path.join(ROOT, "lanedetection_end2end_amd", "csrc", "lf_debug.h")).read()
    lib = _lib.load()
    table = _lib.exported_symbols()
    assert re.search(r"\bvoid lf_debug_set_thin_bf16\(int mode, int nt\);", debug)
    assert re.search(r"\blong lf_debug_thin_bf16_launches\(void\);", debug)
    for name in HOOKS:
        assert hasattr(lib, name) and name in table, name
    # separate from the fp32 pair, which stays
    for name in ("lf_debug_set_thin", "lf_debug_thin_launches"):
        assert re.search(r"\b%s\(" % name, debug) and hasattr(lib, name) and name in table, name
    # the counter answers without a device; the switch takes any pair
    lib.lf_debug_set_thin_bf16(0, 0)
    assert lib.lf_debug_thin_bf16_launches() >= 0
    assert lib.lf_abi_version() == 5


@pytest.fixture(scope="module")
def bf16_kernels(tmp_path_factory):
    import isa_meta
    return isa_meta.compile_kernels(["lf_conv_bf16.hip"], tmp_path_factory.mktemp("isa_thin_bf16"))


def test_thin_kernels_do_not_spill(bf16_kernels):
    thin = {k["name"]: k for k in bf16_kernels if k["name"].startswith("tapgemm_bf16_thin_kernel<")}
    want = {"tapgemm_bf16_thin_kernel<%d, %d>" % (nt, e) for nt in (1, 2, 3, 4) for e in (RELU, BRES)}
    assert set(thin) == want, sorted(thin)
    for name, k in sorted(thin.items()):
        print("%-40s vgpr %3d agpr %3d lds %5d" % (name, k["vgpr"], k["agpr"], k["lds"]))
        assert k["vgpr_spill"] == 0 and k["scratch"] == 0 and k["loop_scratch"] == 0, (name, k)
        assert k["vgpr"] + k["agpr"] <= 256, (name, k["vgpr"], k["agpr"])
        assert k["lds"] == 4 * 9 * 64 * 4, (name, k["lds"])        # the tap table only: [waves][LF_MAX_TAPS][64] words


def test_regular_bf16_instantiations_keep_their_budgets(bf16_kernels):
    """What tests/test_infer_cpu.py names of lf_conv_bf16.hip: still there, within the same budgets."""
    by = {k["name"]: k for k in bf16_kernels}
    want = {"tapgemm_bf16_wv_kernel<%d>" % BRES: 256, "tapgemm_bf16_wl_kernel<4, %d, 0>" % BRES: 256,
            "tapgemm_bf16_lean_kernel<0, %d>" % BRES: 128}
    for name, budget in want.items():
        assert name in by, name
        k = by[name]
        regs = k["vgpr"] if budget == 128 else k["vgpr"] + k["agpr"]
        assert regs <= budget, (name, k["vgpr"], k["agpr"])
        assert k["vgpr_spill"] == 0 and k["scratch"] == 0 and k["loop_scratch"] == 0, (name, k)


def test_no_thin_kernel_of_the_fp32_name_in_the_bf16_file(bf16_kernels):
    assert not [k["name"] for k in bf16_kernels if k["name"].startswith("tapgemm_thin_kernel<")]


def test_auto_constant():
    from lanedetection_end2end_amd import lsq
    assert isinstance(lsq.THIN_AUTO_MAX_BATCH_BF16, int) and 0 <= lsq.THIN_AUTO_MAX_BATCH_BF16 <= 8
    assert lsq.THIN_AUTO_MAX_BATCH == 8
