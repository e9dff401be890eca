"""BEV lane decoding without a device: the numpy restatement of ``write_lsq_results`` (tests/bev_lanes_ref.py) against goldens from
the real reference, the homography, the C surface of ``lf_lane_decode_bev``, the resources of its kernels, the mirror's import
shadowing and the arguments the mirror refuses."""
import ctypes
import glob
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
import bev_lanes_ref
import laneeval_ref

sys.path.insert(0, os.path.join(ROOT, "tools"))

FLAGS = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 0, 1), (1, 1, 1)]


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "bev_lanes.npz"), allow_pickle=False)


case_line = bev_lanes_ref.golden_line


def restate(golden, c, **kw):
    l = case_line(golden, c)
    abr, hon, no = (bool(v) for v in golden["flags"][c])
    return bev_lanes_ref.decode(l["params"], l["lanes"], l["h_samples"], l["line_id"], l["horizon_est"], golden["M"], golden["M_inv"],
                                int(golden["nclasses"]), int(golden["resize"]), abr, hon, no, **kw)


def test_restatement_equals_the_reference_on_every_golden(golden):
    for c in range(len(golden["S"])):
        S = int(golden["S"][c])
        got = restate(golden, c)
        assert np.array_equal(got, golden["lanes"][c, :, :S]), (c, golden["flags"][c])
        assert np.array_equal(restate(golden, c, int32=True), got)          # nothing in the goldens reaches the int32 bounds
        l = case_line(golden, c)
        assert laneeval_ref.bench(got.tolist(), l["lanes"], l["h_samples"], 20) == tuple(golden["scores"][c]), c
        args = (l["params"], l["lanes"], l["h_samples"], l["line_id"], l["horizon_est"], golden["M"], golden["M_inv"], int(golden["resize"]))
        assert bev_lanes_ref.tie_margin(*args, *(bool(v) for v in golden["flags"][c])) >= 1e-6, c


def test_golden_covers_the_cases_it_claims(golden):
    S, flags, gt, gc, lanes = golden["S"], golden["flags"], golden["gt"], golden["gt_count"], golden["lanes"]
    assert os.path.getsize(os.path.join(GOLDEN, "bev_lanes.npz")) <= os.path.getsize(os.path.join(GOLDEN, "laneeval.npz"))
    assert {(tuple(int(v) for v in f), int(s)) for f, s in zip(flags, S)} == {(f, s) for f in FLAGS for s in (48, 56, 130)}
    assert golden["params"].dtype == np.float32 and lanes.dtype == np.int32 and golden["scores"].dtype == np.float64
    c48, c56, c130 = (list(S).index(s) for s in (48, 56, 130))
    assert list(golden["h_samples"][c48, :48]) == list(range(240, 720, 10)) and list(golden["h_samples"][c56, :56]) == list(range(160, 720, 10))
    h130 = golden["h_samples"][c130, :130]
    assert len(set(h130)) == 130 and np.any(np.diff(h130) < 0)                # more than one sample per wave lane, unsorted
    for f in FLAGS:                                                           # every special under every flag combination
        mine = [c for c in range(len(S)) if tuple(flags[c]) == f]
        valid = [(gt[c, :4, :S[c]] != -2).sum(1) for c in mine]
        assert any((v == 0).any() for v in valid) and any((v == 1).any() for v in valid)
        holes = False
        for c in mine:
            for g in range(4):
                ok = np.nonzero(gt[c, g, :S[c]] != -2)[0]
                holes |= len(ok) > 1 and ok[-1] - ok[0] + 1 > len(ok) and S[c] != 130
        assert holes
        assert any(golden["line_id"][c, 0] == 0 for c in mine) and any(golden["line_id"][c, 3] == 0 for c in mine)
        minimum = golden["horizon"][mine].sum(1) * (640 / int(golden["resize"])) + 80
        assert minimum.min() < 210 < minimum.max()
        assert {1, 2, 3} <= set(golden["params_len"][mine].reshape(-1))
        inside = np.concatenate([lanes[c, :, :S[c]].reshape(-1) for c in mine])
        inside = inside[inside != -2]
        assert inside.min() < 0 and inside.max() > 1279
        assert set(gc[mine]) == {4, 5}
    assert golden["triple"].shape == (15, 3) and np.any(golden["scores"][:, 0] > 0.5) and np.any(golden["scores"][:, 2] > 0)
    # the skip rules are visible in the stored lanes: lane 2 / 3 with line_id 0 under all_branches_ready, an empty gt lane without it
    for c in range(len(S)):
        abr = bool(flags[c, 0])
        empty = (gt[c, :4, :S[c]] != -2).sum(1) == 0
        for j in range(4):
            skipped = ((j == 2 and golden["line_id"][c, 0] == 0) or (j == 3 and golden["line_id"][c, 3] == 0)) if abr else bool(empty[j])
            if skipped:
                assert (lanes[c, j] == -2).all(), (c, j)


def test_geometry_bev_homography_equals_the_reference(golden):
    from lanedetection_end2end_amd import geometry
    M, M_inv = geometry.bev_homography()
    assert np.abs(M - golden["M"]).max() <= 1e-12 and np.abs(M_inv - golden["M_inv"]).max() <= 1e-12
    assert golden["M"].dtype == np.float64 and abs(golden["M"][2, 2] - 1) <= 1e-12


def test_symbol_exported_and_declared():
    from lanedetection_end2end_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "lanefit.h")).read()
    assert hasattr(lib, "lf_lane_decode_bev") and "lf_lane_decode_bev" in _lib.exported_symbols()
    assert "additions since 5 (BEV lane decoding): lf_lane_decode_bev" in header
    body = header[header.index("additions since 5 -- BEV lane decoding"):]
    assert re.search(r"\bint lf_lane_decode_bev\(", body)
    assert "BEV/Dataloader/Load_Data_new.py:334-420" in body and "BEV/main.py:445-488" in body
    assert "#define LF_ABI_VERSION 5" in header and lib.lf_abi_version() == 5
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "lf_lane_decode_bev" in integration and "Not exercised as files: the argparse / scheduler / logging plumbing of `main.py:31-198` and `write_lsq_results`" not in integration


def test_lane_decode_bev_kernels_do_not_spill(tmp_path):
    from lanedetection_end2end_amd import build
    import isa_meta
    src = os.path.join(build.CSRC, "lf_lanes.hip")
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + build.FLAGS + ["-c", src, "-o", str(tmp_path / "lf_lanes.o"), "-save-temps=obj"]
    subprocess.check_call(cmd, cwd=str(tmp_path))
    asm = glob.glob(str(tmp_path / "*gfx950*.s"))
    assert asm, "no device assembly produced"
    mine = [k for k in isa_meta.kernels(asm[0]) if k["name"].startswith("lane_decode_bev")]
    assert sorted(k["name"] for k in mine) == ["lane_decode_bev_kernel<double>", "lane_decode_bev_kernel<float>"]
    for k in mine:
        assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0 and k["lds"] == 0, k
        assert k["vgpr"] + k["agpr"] <= 128, k


def _run(code):
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-1500:]


def test_mirror_shadows_dataloader_and_eval_lane(tmp_path):
    """``from Dataloader.Load_Data_new import get_loader, write_lsq_results`` and ``from eval_lane import LaneEval`` (BEV/main.py:20-22)
    with the mirror's tree ahead of a stand-in reference tree: the loader comes from the reference's file, ``write_lsq_results`` and
    ``LaneEval`` from the mirror."""
    d = "Birds_Eye_View_Loss"
    ref = tmp_path / "reference"
    (ref / d / "Dataloader").mkdir(parents=True)
    (ref / d / "Dataloader" / "Load_Data_new.py").write_text(
        "import json\nMARK = 'reference'\n\ndef get_loader(*a):\n    return 'dummy loader'\n\n"
        "def write_lsq_results(*a, **k):\n    raise ImportError('the reference write_lsq_results was called')\n\ndef _private():\n    pass\n")
    (ref / d / "eval_lane.py").write_text("raise ImportError('reference eval_lane imported instead of the mirror')\n")
    mirror = os.path.join(ROOT, "lanedetection_end2end_amd", "bev")
    _run(r'''
import os, sys
sys.path.insert(0, %r)
os.environ["LANEFIT_REFERENCE_ROOT"] = %r
sys.path.insert(0, os.path.join(%r, %r))
sys.path.insert(0, %r)
from Dataloader.Load_Data_new import get_loader, write_lsq_results
from eval_lane import LaneEval
import Dataloader.Load_Data_new as m
assert get_loader() == "dummy loader" and m.MARK == "reference" and not hasattr(m, "_private")
assert "lanedetection_end2end_amd" in m.__file__ and write_lsq_results.__module__ == "Dataloader.Load_Data_new"
assert write_lsq_results.__code__.co_filename == m.__file__
assert "lanedetection_end2end_amd" in sys.modules["eval_lane"].__file__ and LaneEval.pixel_thresh == 20
assert "get_loader" in m.__all__ and "ujson" not in sys.modules
print("ok")
''' % (ROOT, str(ref), str(ref), d, mirror))
    # without the variable only write_lsq_results exists
    _run(r'''
import os, sys
sys.path.insert(0, %r)
os.environ.pop("LANEFIT_REFERENCE_ROOT", None)
sys.path.insert(0, %r)
from Dataloader.Load_Data_new import write_lsq_results
import Dataloader.Load_Data_new as m
assert m.__all__ == ["write_lsq_results"] and not hasattr(m, "get_loader")
try:
    from Dataloader.Load_Data_new import get_loader
except ImportError:
    print("ok")
''' % (ROOT, mirror))


def test_refpath_extend_is_unchanged_and_loader_is_private(tmp_path, monkeypatch):
    from lanedetection_end2end_amd import _refpath
    (tmp_path / "T" / "Networks").mkdir(parents=True)
    (tmp_path / "T" / "x.py").write_text("VALUE = 7\n")
    monkeypatch.delenv("LANEFIT_REFERENCE_ROOT", raising=False)
    path = []
    _refpath.extend(path, "T")
    assert path == [] and _refpath.load_reference_module("T", "x.py", "_lanefit_test_private_x") is None
    monkeypatch.setenv("LANEFIT_REFERENCE_ROOT", str(tmp_path))
    _refpath.extend(path, "T")
    assert path == [str(tmp_path / "T" / "Networks")]
    try:
        m = _refpath.load_reference_module("T", "x.py", "_lanefit_test_private_x")
        assert m.VALUE == 7 and sys.modules["_lanefit_test_private_x"] is m and "x" not in sys.modules
        assert _refpath.load_reference_module("T", "missing.py", "_lanefit_test_private_y") is None
    finally:
        sys.modules.pop("_lanefit_test_private_x", None)


def test_signature_and_refused_arguments(golden, tmp_path):
    import inspect
    from lanedetection_end2end_amd.bev.Dataloader.Load_Data_new import write_lsq_results
    from lanedetection_end2end_amd.bev import eval_lane
    from lanedetection_end2end_amd.bp.eval_lane import LaneEval
    assert eval_lane.LaneEval is LaneEval
    sig = inspect.signature(write_lsq_results)
    assert list(sig.parameters) == ["src_file", "dst_file", "nclasses", "all_branches_ready", "horizon_on", "resize", "no_ortho",
                                    "calc_intersection", "draw_image", "path_test_set", "test_phase"]
    assert [sig.parameters[k].default for k in ("calc_intersection", "draw_image", "path_test_set", "test_phase")] == [False, False, '../../../', False]
    src, dst = tmp_path / "src.json", tmp_path / "dst.json"
    src.write_text(json.dumps(case_line(golden, 0)) + "\n")
    for name in ("calc_intersection", "draw_image", "test_phase"):
        with pytest.raises(NotImplementedError, match=name):
            write_lsq_results(str(src), str(dst), 4, False, False, 256, False, **{name: True})
    line = case_line(golden, 0)
    line["params"][1] = [0., 0., 0., .5]
    src.write_text(json.dumps(line) + "\n")
    with pytest.raises(ValueError):
        write_lsq_results(str(src), str(dst), 4, False, False, 256, False)
    assert not dst.exists()
    with pytest.raises(ValueError):
        bev_lanes_ref.decode(line["params"], line["lanes"], line["h_samples"], line["line_id"], line["horizon_est"], golden["M"],
                             golden["M_inv"], 4, 256)
    import torch
    from lanedetection_end2end_amd.clas import LaneLabels, ProjectionsBEV
    from argparse import Namespace
    with pytest.raises(ValueError):
        ProjectionsBEV(Namespace(resize=256, nclasses=4)).decode_lanes([torch.zeros(2, 4, 1)], LaneLabels([case_line(golden, 0)] * 2))


def test_restatement_int32_rule():
    """What the device stores where the reference's int64 does not fit: saturation, and INT32_MIN for NaN."""
    h = list(range(160, 720, 10))
    gt = [[100] * 56]
    M = M_inv = np.eye(3)
    for c, want in ((1e12, bev_lanes_ref.INT32_MAX), (-1e12, bev_lanes_ref.INT32_MIN), (float("nan"), bev_lanes_ref.INT32_MIN)):
        got = bev_lanes_ref.decode([[c]], gt, h, [1] * 4, [0.] * 4, M, M_inv, 2, 256, no_ortho=True, int32=True)
        assert (got[0][np.array(h) >= 210] == want).all() and (got[0][np.array(h) < 210] == -2).all() and (got[1] == -2).all()
    wide = bev_lanes_ref.decode([[1e12]], gt, h, [1] * 4, [0.] * 4, M, M_inv, 2, 256, no_ortho=True)
    assert wide[0, -1] == 1279 * 10 ** 12
