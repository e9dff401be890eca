"""Lane scoring without a device: the numpy restatement of ``LaneEval.bench`` against goldens from the real reference, the
``LaneLabels`` table, the C surface of ``lf_lane_eval`` and the resources of its kernels."""
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
import laneeval_ref

sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "laneeval.npz"), allow_pickle=False)


def test_golden_covers_the_cases_it_claims(golden):
    gc, pc, S, e, kind = golden["gt_count"], golden["pred_count"], golden["S"], golden["expected"], golden["kind"]
    assert len(gc) >= 300 and os.path.getsize(os.path.join(GOLDEN, "laneeval.npz")) < 100 * 1000
    assert golden["pred"].dtype == np.int16 and golden["gt"].dtype == np.int16 and e.dtype == np.float64
    assert {(g, p) for g, p in zip(gc, pc)} >= {(g, p) for g in range(7) for p in range(6)}
    assert set(S) == {48, 56} and set(golden["run_time"]) == {20., 250.}
    assert list(golden["y_samples"][list(S).index(56)]) == list(range(160, 720, 10))
    assert np.any(gc + 2 < pc) and np.any((gc > 4) & (e[:, 2] > 0)) and np.any((gc > 4) & (e[:, 2] == 0) & (gc + 2 >= pc))
    valid = (golden["gt"] >= 0).sum(2)
    assert np.any([(valid[c, :gc[c]] == 1).any() for c in range(len(gc))]) and np.any([(valid[c, :gc[c]] == 0).any() for c in range(len(gc))])
    assert {"exact_20_vertical", "exact_20_single", "both_all_invalid"} <= set(kind)


def test_restatement_equals_the_reference_on_every_golden(golden):
    for c in range(len(golden["S"])):
        S = int(golden["S"][c])
        pred = laneeval_ref.unpack_case(golden["pred"][c], golden["pred_count"][c], S)
        gt = laneeval_ref.unpack_case(golden["gt"][c], golden["gt_count"][c], S)
        got = laneeval_ref.bench(pred, gt, [int(v) for v in golden["y_samples"][c, :S]], float(golden["run_time"][c]))
        assert got == tuple(golden["expected"][c]), (c, golden["kind"][c], got, golden["expected"][c])


def test_exactly_twenty_pixels_is_not_a_hit(golden):
    c = list(golden["kind"]).index("exact_20_vertical")
    S = int(golden["S"][c])
    pred = laneeval_ref.unpack_case(golden["pred"][c], 3, S)
    gt = laneeval_ref.unpack_case(golden["gt"][c], 3, S)
    ys = list(golden["y_samples"][c, :S])
    assert laneeval_ref.threshold(gt[0], ys) == 20.0
    assert laneeval_ref.line_accuracy(pred[0], gt[0], 20.0) == 0.0 and laneeval_ref.line_accuracy(pred[1], gt[0], 20.0) == 1.0


def _label(lanes, h, name):
    return dict(lanes=lanes, h_samples=h, raw_file=name)


def _write(path, labels):
    path.write_text("".join(json.dumps(l) + "\n" for l in labels))
    return str(path)


def test_lane_labels_table(tmp_path):
    from lanedetection_end2end_amd.clas import LaneLabels
    h = [10, 20, 30, 40]
    labels = [_label([[1, 2, 3, 4], [-2, -2, 7, 8]], h, "a"), _label([], h, "b"), _label([[5, 6, 7, 8], [1, 1, 1, 1], [9, 9, -2, 9]], h, "c")]
    t = LaneLabels(_write(tmp_path / "l.json", labels))
    assert (t.M, t.G, t.S) == (3, 3, 4) and t.lanes.dtype == np.int32 and t.counts.dtype == np.int32
    assert list(t.counts) == [2, 0, 3] and t.shared and t.h_samples.shape == (4,) and t.h_samples.dtype == np.float64
    assert t.lanes[0].tolist() == [[1, 2, 3, 4], [-2, -2, 7, 8], [-2] * 4] and (t.lanes[1] == -2).all()
    assert t.lanes[2].tolist() == labels[2]["lanes"] and t.labels == labels
    assert t.rows_by_raw_file() == {"a": 0, "b": 1, "c": 2}
    # per-image heights
    labels[1]["h_samples"] = [10, 20, 30, 45]
    t = LaneLabels(labels)
    assert not t.shared and t.h_samples.shape == (3, 4) and t.h_samples[1].tolist() == [10, 20, 30, 45]
    # a file without lanes still has one (empty) lane slot
    t = LaneLabels([_label([], h, "x")])
    assert (t.M, t.G, t.S) == (1, 1, 4) and list(t.counts) == [0]


def test_lane_labels_errors(tmp_path):
    from lanedetection_end2end_amd.clas import LaneLabels
    h = [10, 20, 30, 40]
    with pytest.raises(Exception, match="Format of lanes error.") as e:
        LaneLabels(_write(tmp_path / "a.json", [_label([[1, 2, 3, 4]], h, "a"), _label([[1, 2, 3]], h, "b")]))
    assert type(e.value) is Exception
    with pytest.raises(ValueError):
        LaneLabels(_write(tmp_path / "b.json", [_label([[1, 2, 3, 4]], h, "a"), _label([[1, 2, 3]], h[:3], "b")]))
    with pytest.raises(ValueError):
        LaneLabels(_write(tmp_path / "c.json", [_label([[1, 2, 3, 4]] * 9, h, "a")]))
    LaneLabels([_label([[1, 2, 3, 4]] * 8, h, "a")])
    with pytest.raises(ValueError):
        LaneLabels([_label([[1, 2.5, 3, 4]], h, "a")])


def test_symbol_exported_and_declared():
    from lanedetection_end2end_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "lanefit.h")).read()
    assert hasattr(lib, "lf_lane_eval") and "lf_lane_eval" in _lib.exported_symbols()
    assert "additions since 5 (scoring of decoded lanes): lf_lane_eval" in header
    assert re.search(r"\bint lf_lane_eval\(", header[header.index("additions since 5 -- scoring of decoded lanes"):])
    assert "#define LF_ABI_VERSION 5" in header and lib.lf_abi_version() == 5
    assert "lf_lane_eval" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_mirror_exports():
    from lanedetection_end2end_amd.bp import eval_lane, test as bp_test
    assert eval_lane.LaneEval.pixel_thresh == 20 and eval_lane.LaneEval.pt_thresh == 0.85
    assert callable(eval_lane.LaneEval.bench) and callable(eval_lane.LaneEval.bench_one_submit)
    import inspect
    assert list(inspect.signature(bp_test.test_model).parameters) == [
        "loader", "model", "criterion", "criterion_seg", "criterion_line_class", "criterion_horizon", "args", "epoch"]
    for f in ("eval_lane.py", "test.py"):
        assert "ujson" not in open(os.path.join(ROOT, "lanedetection_end2end_amd", "bp", f)).read()


def test_lane_eval_kernels_do_not_spill(tmp_path):
    from lanedetection_end2end_amd import build
    import isa_meta
    src = os.path.join(build.CSRC, "lf_lanes.hip")
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + build.FLAGS + ["-c", src, "-o", str(tmp_path / "lf_lanes.o"), "-save-temps=obj"]
    subprocess.check_call(cmd, cwd=str(tmp_path))
    asm = glob.glob(str(tmp_path / "*gfx950*.s"))
    assert asm, "no device assembly produced"
    mine = [k for k in isa_meta.kernels(asm[0]) if k["name"].startswith("lane_eval")]
    assert sorted(k["name"] for k in mine) == ["lane_eval_kernel", "lane_eval_totals_kernel"]
    for k in mine:
        assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, k
        assert k["vgpr"] + k["agpr"] <= 128, k


def test_mirror_shadows_test_and_eval_lane(tmp_path):
    """``from test import test_model`` (BP/main.py:29) and ``from eval_lane import LaneEval`` resolve to the mirror when its tree
    precedes the reference tree on sys.path (set up as tests/test_host_cpu.py::test_mirror_shadows_reference_imports does: the
    stand-in reference's copies refuse to be imported)."""
    d = "Backprojection_Loss"
    ref = tmp_path / "reference"
    nets = ref / d / "Networks"
    nets.mkdir(parents=True)
    for f in [nets / "__init__.py", nets / "LSQ_layer.py", nets / "ERFNet.py", nets / "gels.py", ref / d / "Loss_crit.py",
              ref / d / "test.py", ref / d / "eval_lane.py"]:
        f.write_text("raise ImportError('reference module %s imported instead of the mirror')\n" % f.name)
    (nets / "utils.py").write_text("def define_args():\n    return None\n")
    code = r'''
import os, sys
sys.path.insert(0, %r)
os.environ["LANEFIT_REFERENCE_ROOT"] = %r
sys.path.insert(0, os.path.join(%r, %r))
sys.path.insert(0, %r)
from test import test_model, Projections
from eval_lane import LaneEval
assert test_model.__module__ == "test" and "lanedetection_end2end_amd" in sys.modules["test"].__file__
assert "lanedetection_end2end_amd" in sys.modules["eval_lane"].__file__ and LaneEval.pixel_thresh == 20
assert "ujson" not in sys.modules
print("ok")
''' % (ROOT, str(ref), str(ref), d, os.path.join(ROOT, "lanedetection_end2end_amd", "bp"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-800:]
