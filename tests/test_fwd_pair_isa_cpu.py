"""Register and LDS budgets of tappair_kernel (csrc/lf_conv_pair.hip: a non_bottleneck_1d block's 3x1 -> 1x3 forward pair in one
launch), from the code-object metadata alone: every instantiation the launcher references exists, runs without scratch, fits the
two waves per SIMD of its one 512-thread workgroup per CU, and both convolutions' weights fit that CU's LDS.

Compiles the TU for gfx950 with -save-temps (hipcc cross-compiles without a GPU), as tests/test_fp32_stream_isa_cpu.py does."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# the (channels, conv_a prologue, 4-wave groups) lf_tappair_launch instantiates: tappair_kernel<64, pro, 2>, tappair128_kernel<pro>
VARIANTS = [(64, 0, 2), (64, 1, 2), (128, 0, 2), (128, 1, 2)]
WORKGROUPS_PER_CU = 1
LDS_PER_CU = 160 * 1024
REGS_PER_SIMD_LANE = 512           # VGPR + AGPR of one SIMD lane, shared by the waves resident on the SIMD


@pytest.fixture(scope="module")
def pair_kernels(tmp_path_factory):
    import isa_meta
    out = {}
    for k in isa_meta.compile_kernels(["lf_conv_pair.hip"], tmp_path_factory.mktemp("isa_pair")):
        m = re.search(r"tappair_kernelILi(\d+)ELi(\d+)ELi(\d+)E", k["mangled"])
        key = tuple(int(v) for v in m.groups()) if m else None
        m = re.search(r"tappair128_kernelILi(\d+)E", k["mangled"])
        if m:
            key = (128, int(m.group(1)), 2)
        if key:
            out[key] = dict(agpr=k["agpr"], vgpr=k["vgpr"], spill=k["vgpr_spill"], sgpr_spill=k["sgpr_spill"],
                                                          scratch=k["scratch"], lds=k["lds"])
    return out


def test_every_launched_instantiation_exists(pair_kernels):
    assert sorted(pair_kernels) == sorted(VARIANTS)


@pytest.mark.parametrize("variant", VARIANTS)
def test_no_scratch_and_register_and_lds_budgets(pair_kernels, variant):
    k = pair_kernels[variant]
    C, pro, groups = variant
    assert k["spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, k
    # a workgroup of `groups` 4-wave groups puts `groups` waves on each of the CU's four SIMDs
    waves_per_simd = groups * WORKGROUPS_PER_CU
    assert (k["vgpr"] + k["agpr"]) * waves_per_simd <= REGS_PER_SIMD_LANE, k
    # dynamic LDS, 64 channels (launch_tappair): two 64-output-channel weight slices [3 * C/16 K-steps][4][64] float4, + scale and
    # shift [2][C]; 128 channels (PAIR128_LDS): the tap tables, 8 waves x 3 taps x 64 lanes x (16 + 4) bytes
    dynamic = 2 * 3 * (C // 16) * 4096 + (2 * C * 4 if pro else 0) if C == 64 else 8 * 3 * 64 * 20
    assert (k["lds"] + dynamic) * WORKGROUPS_PER_CU <= LDS_PER_CU, (variant, k["lds"], dynamic)
