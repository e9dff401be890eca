"""Register and LDS budgets of tapstream_kernel (csrc/lf_conv.hip), from the code-object metadata alone: every instantiation the
launcher references runs two waves per SIMD without scratch, and its weights fit the CU's LDS at the workgroups per CU it is
launched with (64 channels: two 256-thread workgroups; 128 channels: one 512-thread workgroup).

Compiles the TU for gfx950 with -save-temps (hipcc cross-compiles without a GPU), as tests/test_isa_cpu.py does."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# the (channels, prologue, epilogue flags, 4-wave groups) the launcher instantiates: route_tapstream<64 / 128> in lf_conv.hip
VARIANTS = [(c, pro, epi, 1 if c == 64 else 2) for c in (64, 128) for pro, epi in ((0, 1), (0, 8), (0, 2), (1, 1))] + [(64, 0, 48, 1), (64, 0, 38, 1)]


@pytest.fixture(scope="module")
def stream_kernels(tmp_path_factory):
    import isa_meta
    out = {}
    for k in isa_meta.compile_kernels(["lf_conv.hip"], tmp_path_factory.mktemp("isa_stream")):
        m = re.search(r"tapstream_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)E", k["mangled"])
        if m:
            out[tuple(int(v) for v in m.groups())] = dict(agpr=k["agpr"], vgpr=k["vgpr"], spill=k["vgpr_spill"], scratch=k["scratch"], lds=k["lds"])
    return out


def test_every_launched_instantiation_exists(stream_kernels):
    assert sorted(stream_kernels) == sorted(VARIANTS)


@pytest.mark.parametrize("variant", VARIANTS)
def test_two_waves_per_simd_and_lds_budget(stream_kernels, variant):
    k = stream_kernels[variant]
    C, pro, epi, groups = variant
    assert k["spill"] == 0 and k["scratch"] == 0, k
    assert k["vgpr"] + k["agpr"] <= 256, k
    # dynamic LDS of launch_tapstream: the 64-output-channel weight slice [3 * C/16 K-steps][4][64] float4, + scale and shift [2][C]
    dynamic = 3 * (C // 16) * 4096 + (2 * C * 4 if pro else 0)
    total = k["lds"] + dynamic
    assert total <= (80 if C == 64 else 160) * 1024, (variant, k["lds"], dynamic)
