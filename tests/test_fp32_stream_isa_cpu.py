"""Register and LDS budgets of tapstream_kernel (csrc/lf_conv.hip), from the code-object metadata alone: every instantiation the
launcher references runs two waves per SIMD without scratch, and its weights fit the CU's LDS at the workgroups per CU it is
launched with (64 channels: two 256-thread workgroups; 128 channels: one 512-thread workgroup).

Compiles the TU for gfx950 with -save-temps (hipcc cross-compiles without a GPU), as tests/test_isa_cpu.py does."""
import glob
import os
import re
import subprocess

import pytest

# the (channels, prologue, epilogue flags, 4-wave groups) the launcher instantiates: route_tapstream<64 / 128> in lf_conv.hip
VARIANTS = [(c, pro, epi, 1 if c == 64 else 2) for c in (64, 128) for pro, epi in ((0, 1), (0, 8), (0, 2), (1, 1))] + [(64, 0, 48, 1), (64, 0, 38, 1)]


@pytest.fixture(scope="module")
def stream_kernels(tmp_path_factory):
    from lanedetection_end2end_amd import build
    d = tmp_path_factory.mktemp("isa_stream")
    src = os.path.join(build.CSRC, "lf_conv.hip")
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + build.FLAGS + ["-c", src, "-o", str(d / "lf_conv.o"), "-save-temps=obj"]
    subprocess.check_call(cmd, cwd=str(d))
    asm = glob.glob(str(d / "*gfx950*.s"))
    assert asm, "no device assembly produced"
    s = open(asm[0]).read()
    md = s[s.index("amdhsa.kernels:"):]                  # the metadata note: nothing of the instruction stream is read
    out = {}
    for b in md.split("\n  - .agpr_count:")[1:]:
        g = lambda k: re.search(r"\." + k + r":\s+(\S+)", b).group(1)
        m = re.search(r"tapstream_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)E", g("name"))
        if m:
            out[tuple(int(v) for v in m.groups())] = dict(agpr=int(b.split("\n")[0].strip()), vgpr=int(g("vgpr_count")), spill=int(g("vgpr_spill_count")),
                                                         scratch=int(g("private_segment_fixed_size")), lds=int(g("group_segment_fixed_size")))
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
