"""Register and LDS budgets of tapbwd16_kernel (csrc/lf_bwd16.hip), from the code-object metadata alone: each of the four compiled
forms runs without scratch and fits TWO 256-thread workgroups per CU (8 waves: these launches live on bytes in flight) -- registers
for two waves per SIMD, static + dynamic LDS within half of the CU's 160 KB.

Compiles the TU for gfx950 with -save-temps (hipcc cross-compiles without a GPU), as tests/test_isa_cpu.py does."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# (prologue, epilogue flags) -> 1 KB tiles per ring stage, stages: B16Cfg in lf_bwd16.hip (g and x at three taps, + residual, + BN operand)
FORMS = {(0, 2): (6, 3), (1, 48): (6, 3), (0, 38): (8, 2), (0, 4): (7, 2)}


@pytest.fixture(scope="module")
def bwd16_kernels(tmp_path_factory):
    import isa_meta
    out = {}
    for k in isa_meta.compile_kernels(["lf_bwd16.hip"], tmp_path_factory.mktemp("isa_bwd16")):
        m = re.search(r"tapbwd16_kernelILb(\d)ELi(\d+)E", k["mangled"])
        if m:
            out[(int(m.group(1)), int(m.group(2)))] = k
    return out


def test_the_four_forms_exist(bwd16_kernels):
    assert sorted(bwd16_kernels) == sorted(FORMS)


@pytest.mark.parametrize("form", sorted(FORMS))
def test_no_scratch_and_two_workgroups_per_cu(bwd16_kernels, form):
    k = bwd16_kernels[form]
    tiles, stages = FORMS[form]
    assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, k
    assert k["vgpr"] + k["agpr"] <= 256, k
    dynamic = 4 * stages * tiles * 1024            # four waves' private rings
    assert k["lds"] + dynamic <= 80 * 1024, (form, k["lds"], dynamic)
