"""CPU checks of the --clas heads / only_encode in the bf16 precision mode (no GPU needed).

The bf16 forms of the trunk's pooling and of encoder.output_conv are new kernel instantiations: compiled for gfx950 with
-save-temps (as tests/test_isa_cpu.py does) none of them may spill or use a private segment.  The library exports the new
entry points the header declares, and the conv-chain plan sizes a bf16 workspace of its own without a device.
"""
import glob
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

NEW_SYMBOLS = ("lf_convchain_set_precision", "lf_convchain_workspace_bytes_for", "lf_poolflat_bf16_fwd", "lf_poolflat_bf16_bwd",
               "lf_pointwise_bf16_fwd", "lf_pointwise_bf16_bwd")


def _compile(src_name, d):
    from lanedetection_end2end_amd import build
    import isa_meta
    src = os.path.join(build.CSRC, src_name)
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + build.FLAGS + ["-c", src, "-o", str(d / (src_name + ".o")),
                                                                            "-save-temps=obj"]
    subprocess.check_call(cmd, cwd=str(d))
    asm = glob.glob(str(d / ("%s-*gfx950*.s" % src_name[:-4])))
    assert asm, "no device assembly produced for " + src_name
    return isa_meta.kernels(asm[0])


@pytest.fixture(scope="module")
def new_kernels(tmp_path_factory):
    d = tmp_path_factory.mktemp("isa_clas_bf16")
    return _compile("lf_convchain.hip", d) + _compile("lf_eltwise.hip", d)


def test_bf16_pool_and_pointwise_kernels_do_not_spill(new_kernels):
    want = ("poolflat_max_fwd_kernel", "poolflat_max_bwd_kernel", "poolflat_avg_fwd_kernel", "poolflat_avg_bwd_kernel",
            "pointwise_fwd_kernel", "pointwise_bwd_data_kernel", "pointwise_wgrad_kernel")

    def of(k):
        return [w for w in want if w + "<" in k["name"] or w + "I" in k["mangled"]]
    # (c++filt leaves the __bf16 instantiations mangled: template argument DF16b)
    bf16 = [k for k in new_kernels if of(k) and "IDF16b" in k["mangled"]]
    f32 = [k for k in new_kernels if of(k) and k["name"].endswith("<float>")]
    assert len(bf16) == len(want) and len(f32) == len(want), sorted(k["name"] for k in bf16 + f32)
    bad = [(k["name"], k["vgpr_spill"], k["scratch"]) for k in bf16 + f32 if k["vgpr_spill"] != 0 or k["scratch"] != 0]
    assert not bad, "kernels spilling / using a private segment: %r" % bad


def test_library_exports_the_bf16_head_entry_points():
    from lanedetection_end2end_amd import _lib
    lib = _lib.load()
    txt = open(os.path.join(ROOT, "include", "lanefit.h")).read()
    declared = set(re.findall(r"\b(lf_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", txt, flags=re.S)))
    for s in NEW_SYMBOLS:
        assert s in declared, s + " is not declared in include/lanefit.h"
        assert hasattr(lib, s), "liblanefit_hip.so does not export " + s
    assert set(NEW_SYMBOLS) <= set(_lib.exported_symbols())


def test_chain_plan_precision_modes():
    from lanedetection_end2end_amd import _lib, clas
    lib = _lib.load()
    plan = clas._ChainPlan(4, 32, 64, (128, 128, 128, 64, 64), (1, 3, 3, 3))
    f32, b16 = plan.workspace_bytes(0), plan.workspace_bytes(2)
    assert f32 == plan.ws_bytes == lib.lf_convchain_workspace_bytes(plan.handle)       # mode 0 is the default
    assert b16 > f32                        # + the bf16 weight copy and the bf16 weight-gradient partial rows
    assert lib.lf_convchain_set_precision(plan.handle, 2) == 0 and lib.lf_convchain_workspace_bytes(plan.handle) == b16
    assert lib.lf_convchain_workspace_bytes_for(plan.handle, 0) == f32                # named mode: independent of the setting
    for bad in (1, 3, 4, -1):
        assert lib.lf_convchain_set_precision(plan.handle, bad) != 0
        assert b"mode must be 0" in lib.lf_last_error()
        assert lib.lf_convchain_workspace_bytes_for(plan.handle, bad) == 0
    assert lib.lf_convchain_workspace_bytes(plan.handle) == b16                         # a refused mode leaves the setting
    assert lib.lf_convchain_set_precision(plan.handle, 0) == 0 and lib.lf_convchain_workspace_bytes(plan.handle) == f32
