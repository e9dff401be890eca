"""The whole-step criterion without a device: the C surface of ``lf_step_loss``, its Python names and the resources of its kernels."""
import ctypes
import glob
import inspect
import os
import re
import subprocess
import sys

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))

SYMBOLS = ("lf_step_loss", "lf_step_loss_workspace_bytes", "lf_step_loss_bwd")


def test_symbols_exported_and_declared():
    from lanedetection_end2end_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "lanefit.h")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "additions since 5 (whole-step criterion): lf_step_loss, lf_step_loss_workspace_bytes" in header
    block = header[header.index("additions since 5 -- whole-step criterion"):]
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in _lib.exported_symbols(), name
        assert re.search(r"\b(int|size_t) %s\(" % name, block), name
        assert name in integration, name
    # the reference lines the block answers
    for cite in ("BP/main.py:296-326", "BEV/main.py:223-253", "BP/Loss_crit.py:202-218", "BEV/Loss_crit.py:98-134"):
        assert cite in block[:block.index("lf_step_loss_bwd(")], cite
    assert "#define LF_ABI_VERSION 5" in header and lib.lf_abi_version() == 5
    lib.lf_step_loss_workspace_bytes.restype = ctypes.c_size_t
    assert 80 <= lib.lf_step_loss_workspace_bytes() <= 4096


def test_python_surface():
    from lanedetection_end2end_amd import losses, ops
    from lanedetection_end2end_amd.bp import Loss_crit as bp_crit
    from lanedetection_end2end_amd.bev import Loss_crit as bev_crit
    assert bp_crit.StepCriterion is losses.StepCriterion and bev_crit.StepCriterion is losses.StepCriterion
    assert losses.StepLoss._fields == ("loss", "loss_fit", "loss_line", "loss_horizon", "acc_line", "acc_horizon", "x_cal")
    assert list(inspect.signature(losses.StepCriterion.__init__).parameters) == ["self", "options", "tree"]
    assert issubclass(ops.StepLossFn, __import__("torch").autograd.Function)
    assert callable(losses.StepCriterion.meters) and callable(losses.StepMeters.read) and callable(losses.StepCriterion.flush)
    # the existing names are untouched
    for m, names in ((bp_crit, ("Area_Loss", "CrossEntropyLoss2d", "MSE_Loss", "backprojection_loss", "polynomial", "define_loss_crit")),
                     (bev_crit, ("Area_Loss", "CrossEntropyLoss2d", "MSE_Loss", "polynomial", "define_loss_crit"))):
        for n in names:
            assert hasattr(m, n), (m.__name__, n)


def test_step_loss_kernels_do_not_spill(tmp_path):
    from lanedetection_end2end_amd import build
    import isa_meta
    src = os.path.join(build.CSRC, "lf_criterion.hip")
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + build.FLAGS + ["-c", src, "-o", str(tmp_path / "lf_criterion.o"), "-save-temps=obj"]
    subprocess.check_call(cmd, cwd=str(tmp_path))
    asm = glob.glob(str(tmp_path / "*gfx950*.s"))
    assert asm, "no device assembly produced"
    mine = isa_meta.kernels(asm[0])
    assert sorted(k["name"] for k in mine) == ["step_loss_kernel<double>", "step_loss_kernel<float>",
                                               "step_scale_kernel<double>", "step_scale_kernel<float>"]
    for k in mine:
        assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, k
        assert k["vgpr"] + k["agpr"] <= 128, k
