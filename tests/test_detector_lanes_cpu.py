"""The frozen --clas heads and the frame -> lanes call, the part that needs no GPU: the four entry points in the header, the library
and the ctypes table (ABI version unchanged), the registers of every kernel of ``lf_clas_tail.hip``, and the detector's constants."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

SYMBOLS = ("lf_convchain_infer_fold", "lf_convchain_infer_folded", "lf_clas_tail_workspace_bytes", "lf_clas_tail")


def test_symbols_in_header_library_and_table():
    from lanedetection_end2end_amd import _lib
    header = open(os.path.join(ROOT, "include", "lanefit.h")).read()
    lib = _lib.load()
    table = _lib.exported_symbols()
    for name in SYMBOLS:
        assert re.search(r"^(int|size_t) %s\(" % name, header, re.M), name
        assert hasattr(lib, name) and name in table, name
    assert re.search(r"additions since 5 \(frozen --clas heads\): lf_convchain_infer_fold, lf_convchain_infer_folded,\s+"
                     r"lf_clas_tail_workspace_bytes, lf_clas_tail", header)
    assert "#define LF_ABI_VERSION 5 " in header and lib.lf_abi_version() == 5
    stub = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in SYMBOLS:
        assert name in stub, name
    # the size query answers without a device: three 256-byte-aligned regions
    assert lib.lf_clas_tail_workspace_bytes(1, 32, 64, 64, 128) == 4 * (64 * 16 * 32 + 64 * 32 + 128)
    assert lib.lf_clas_tail_workspace_bytes(1, 2, 2, 16, 8) == 3 * 256
    assert lib.lf_clas_tail_workspace_bytes(0, 2, 2, 16, 8) == 0


@pytest.fixture(scope="module")
def tail_kernels(tmp_path_factory):
    import isa_meta
    return isa_meta.compile_kernels(["lf_clas_tail.hip"], tmp_path_factory.mktemp("isa_clas_tail"))


def test_tail_kernels_do_not_spill(tail_kernels):
    by = {k["name"]: k for k in tail_kernels}
    # (by mangled name: the demangler at hand does not know the __bf16 instantiation's type code)
    mangled = sorted(k["mangled"] for k in tail_kernels)
    assert len(by) == 4 and all("clas_tail_" in m for m in mangled), mangled
    assert sum("clas_tail_pool_kernelI" in m for m in mangled) == 2                     # fp32 and bf16 trunk outputs
    assert sum("clas_tail_gemv_kernel" in m for m in mangled) == 1 and sum("clas_tail_finish_kernel" in m for m in mangled) == 1
    for name, k in sorted(by.items()):
        print("%-40s vgpr %3d agpr %3d lds %5d" % (name, k["vgpr"], k["agpr"], k["lds"]))
        assert k["vgpr_spill"] == 0 and k["scratch"] == 0 and k["loop_scratch"] == 0, (name, k)
        assert k["vgpr"] + k["agpr"] <= 128, (name, k["vgpr"], k["agpr"])
        assert k["lds"] <= 64, (name, k["lds"])           # the four-wave partials of the block sums


def test_constants():
    from lanedetection_end2end_amd import lsq
    for name in ("THIN_AUTO_MAX_BATCH_HEADS", "THIN_AUTO_MAX_BATCH_HEADS_BF16"):
        v = getattr(lsq, name)
        assert v is None or (isinstance(v, int) and not isinstance(v, bool) and 0 <= v <= 8), (name, v)
    assert lsq.FrameLanes._fields == ("lanes", "betas", "line", "horizon", "line_flags", "horizon_row")
    assert lsq.THIN_AUTO_MAX_BATCH == 8 and isinstance(lsq.THIN_AUTO_MAX_BATCH_BF16, int)
