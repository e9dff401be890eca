"""The segmentation-mode step criterion without a device: the C surface of ``lf_seg_step``, its Python names, the ``defer_seg_fit``
switch and the resources of its kernels."""
import ctypes
import glob
import inspect
import os
import re
import subprocess
import sys
from argparse import Namespace

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))

SYMBOLS = ("lf_seg_step_workspace_bytes", "lf_seg_step", "lf_seg_step_bwd")


def test_symbols_exported_and_declared():
    from lanedetection_end2end_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "lanefit.h")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "additions since 5 (segmentation-mode step criterion): lf_seg_step, lf_seg_step_workspace_bytes" in header
    block = header[header.index("additions since 5 -- segmentation-mode step criterion"):]
    table = _lib._declare(lib)
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in _lib.exported_symbols(), name
        assert re.search(r"\b(int|size_t) %s\(" % name, block), name
        assert name in integration, name
    # the ctypes table has one entry per parameter of the declaration
    for name in SYMBOLS:
        decl = re.search(r"\b(?:int|size_t) %s\(([^;]*)\);" % name, block).group(1)
        assert len(table[name][1]) == len([p for p in decl.split(",") if p.strip()]), name
    assert table["lf_seg_step_workspace_bytes"][0] is ctypes.c_size_t
    # the reference lines the block answers
    for cite in ("BP/Networks/LSQ_layer.py:279-314", "BEV/Loss_crit.py:61-75"):
        assert cite in block[:block.index("lf_seg_step_bwd(")], cite
    assert "#define LF_ABI_VERSION 5" in header and lib.lf_abi_version() == 5


def test_workspace_bytes():
    """128 bytes of label counts, one loss slot per workgroup, L * (3 * order + 2) moment slots per workgroup with the fit; one
    workgroup per 4096 pixels of an image, 128 per image at the most."""
    from lanedetection_end2end_amd import _lib
    ws = _lib.load().lf_seg_step_workspace_bytes
    assert ws(2, 3, 0, 8, 16, 2) == 128 + 2 * 8
    assert ws(2, 3, 2, 8, 16, 2) == 128 + 2 * 8 * (1 + 2 * 8)
    assert ws(3, 5, 4, 64, 128, 3) == 128 + 3 * 2 * 8 * (1 + 4 * 11)
    assert ws(16, 3, 0, 512, 1024, 0) == 128 + 16 * 128 * 8
    assert ws(0, 3, 0, 8, 16, 0) == 0


def test_python_surface():
    import torch
    from lanedetection_end2end_amd import losses, ops
    from lanedetection_end2end_amd.bp import Loss_crit as bp_crit
    from lanedetection_end2end_amd.bev import Loss_crit as bev_crit
    assert bp_crit.SegStepCriterion is losses.SegStepCriterion and bev_crit.SegStepCriterion is losses.SegStepCriterion
    assert bp_crit.SegStepLoss is losses.SegStepLoss and bev_crit.SegStepLoss is losses.SegStepLoss
    assert losses.SegStepLoss._fields == ("loss", "metric", "betas", "status", "maps")
    assert list(inspect.signature(losses.SegStepCriterion.__init__).parameters) == ["self", "options", "model"]
    assert issubclass(ops.SegStepFn, torch.autograd.Function)
    for n in ("meters", "flush", "train"):
        assert callable(getattr(losses.SegStepCriterion, n)), n
    assert losses.SegStepMeters.names == ("loss", "metric") and callable(losses.SegStepMeters.read)
    # the existing names are untouched
    for m, names in ((bp_crit, ("Area_Loss", "CrossEntropyLoss2d", "MSE_Loss", "backprojection_loss", "polynomial", "define_loss_crit",
                                "StepCriterion", "StepLoss")),
                     (bev_crit, ("Area_Loss", "CrossEntropyLoss2d", "MSE_Loss", "polynomial", "define_loss_crit", "StepCriterion",
                                 "StepLoss"))):
        for n in names:
            assert hasattr(m, n), (m.__name__, n)


def test_defer_seg_fit_defaults_to_false():
    from lanedetection_end2end_amd import lsq
    from lanedetection_end2end_amd.bp.Networks.LSQ_layer import Net
    args = Namespace(batch_size=2, nclasses=4, resize=64, end_to_end=False, mod="erfnet", layers=18, channels_in=3, pretrained=False,
                     pool=True, activation_layer="square", no_cuda=False, order=2, reg_ls=0.0, use_cholesky=False,
                     mask_percentage=0.2, clas=False, no_mapping=False, loss_policy="backproject", weight_seg=30, weight_funct="none")
    model = Net(args)                                  # (the BP wrapper is built on the host; nothing runs)
    assert model.defer_seg_fit is False
    # both trees share the constructor path that sets it, and the forward consults it for end_to_end=False only
    assert re.search(r"self\.defer_seg_fit = False\b", inspect.getsource(lsq._LaneFitNet._common_init))
    assert "self.defer_seg_fit and not end_to_end" in inspect.getsource(lsq._LaneFitNet._fit)


def test_criterion_takes_its_constants_from_the_options():
    """Construction needs no device: class weights [1] + [weight_seg] * nclasses (BP) / [1, w, w] (BEV), the tree from the wrapper."""
    import torch
    from lanedetection_end2end_amd import losses, lsq

    class _BP(lsq.BPNet):
        def __init__(self):
            torch.nn.Module.__init__(self)

    class _BEV(lsq.BEVNet):
        def __init__(self):
            torch.nn.Module.__init__(self)

    opt = Namespace(nclasses=4, weight_seg=30, loss_policy="backproject", order=2, resize=64, no_mapping=False, no_cuda=True)
    crit = losses.SegStepCriterion(opt, _BP())
    assert crit.tree == "bp" and crit.weights.tolist() == [1.0, 30.0, 30.0, 30.0, 30.0]
    assert crit.check_targets is True and crit.check_singular is True and crit.return_maps is False
    assert not any(isinstance(m, lsq._LaneFitNet) for m in crit.modules())          # the model is not a child of the criterion
    opt = Namespace(nclasses=2, weight_seg=7, loss_policy="area", weight_funct="none", order=2)
    crit = losses.SegStepCriterion(opt, _BEV())
    assert crit.tree == "bev" and crit.weights.tolist() == [1.0, 7.0, 7.0]
    assert crit.meters().read() == {"loss": 0.0, "metric": 0.0}


def test_seg_step_kernels_use_no_scratch(tmp_path):
    from lanedetection_end2end_amd import build
    import isa_meta
    src = os.path.join(build.CSRC, "lf_seg_step.hip")
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + build.FLAGS + ["-c", src, "-o", str(tmp_path / "lf_seg_step.o"), "-save-temps=obj"]
    subprocess.check_call(cmd, cwd=str(tmp_path))
    asm = glob.glob(str(tmp_path / "*gfx950*.s"))
    assert asm, "no device assembly produced"
    mine = isa_meta.kernels(asm[0])
    names = sorted(k["name"] for k in mine)
    # the streaming pass: cross entropy alone, and orders 0..3 x (2 | 4 lanes), each with 16-byte and with scalar accesses
    want = ["seg_step_kernel<-1, 1, %d>" % v for v in (1, 4)] + \
           ["seg_step_kernel<%d, %d, %d>" % (o, l, v) for o in range(4) for l in (2, 4) for v in (1, 4)]
    assert [n for n in names if n.startswith("seg_step_kernel")] == sorted(want)
    assert set(n for n in names if not n.startswith("seg_step_kernel")) == \
        {"seg_label_kernel", "seg_flag_maps_kernel", "seg_scale_kernel"} | {"seg_finish_kernel<%d>" % o for o in range(-1, 4)}
    for k in mine:
        assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, k
        assert k["vgpr"] + k["agpr"] <= 256, k
