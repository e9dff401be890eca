"""Lane scoring on the device (``lf_lane_eval``) against goldens from the real ``LaneEval.bench`` and its numpy restatement
(tests/laneeval_ref.py), the chaining decode -> score, ``LaneEval`` of the mirror and ``test_model`` end to end.

The golden file holds two sample counts (56 and 48) and S is a launch argument, so "all goldens" is one launch per block
(258 and 42 images).  Exact comparisons rest on the tie margin: no |pred - gt| lies within 1e-9 of its threshold (the generator
asserts it for the goldens, ``_assert_margin`` for the batches made here), so the device's fixed-order slope and the restatement's
count the same integer hits."""
import json
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import laneeval_ref
from oracle import clas_oracle, erfnet_oracle, inputs
from oracle.gen_golden_clas import decode_inputs

pytestmark = pytest.mark.gpu

H56 = list(range(160, 720, 10))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "laneeval.npz"), allow_pickle=False)


def _golden_block(golden, S):
    """-> (case numbers, labels, pred (n, 5, S) int32, pred_count, run_time, expected) of the cases with S samples."""
    from lanedetection_end2end_amd.clas import LaneLabels
    cases = np.nonzero(golden["S"] == S)[0]
    labels = LaneLabels([dict(lanes=laneeval_ref.unpack_case(golden["gt"][c], golden["gt_count"][c], S),
                              h_samples=[int(v) for v in golden["y_samples"][c, :S]], raw_file=str(c)) for c in cases]
                        + [dict(lanes=[[-2] * S] * 6, h_samples=[int(v) for v in golden["y_samples"][cases[0], :S]], raw_file="pad")])
    assert labels.G == 6
    pred = np.ascontiguousarray(golden["pred"][cases][:, :, :S]).astype(np.int32)
    return cases, labels, pred, golden["pred_count"][cases].astype(np.int32), golden["run_time"][cases], golden["expected"][cases]


def _run(labels, pred, pred_count=None, run_time=None, index=None, **kw):
    from lanedetection_end2end_amd.clas import lane_eval
    t = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dt).cuda()
    out = lane_eval(t(pred, torch.int32), labels, index=t(index, torch.int32), pred_count=t(pred_count, torch.int32),
                    run_time=t(run_time, torch.float32), want_best=True, want_totals=True, **kw)
    return [o.cpu().numpy() for o in out]


def _restate(labels, pred, pred_count, run_time, index):
    """The restatement over a batch -> (per_image (N, 3), best_acc (N, G), best_pred (N, G))."""
    N, G = len(pred), labels.G
    per, best, arg = np.zeros((N, 3)), np.zeros((N, G)), np.full((N, G), -1, np.int32)
    for n in range(N):
        row = n if index is None else int(index[n])
        l = labels.labels[row]
        p = [[int(v) for v in lane] for lane in pred[n][: (pred.shape[1] if pred_count is None else int(pred_count[n]))]]
        res, accs, args = laneeval_ref.bench_detail(p, l["lanes"], l["h_samples"], 20. if run_time is None else float(run_time[n]))
        per[n] = res
        best[n, :len(accs)] = accs
        arg[n, :len(args)] = args
    return per, best, arg


def _assert_margin(labels, pred, index):
    for n in range(len(pred)):
        l = labels.labels[n if index is None else int(index[n])]
        for g in l["lanes"]:
            thresh = laneeval_ref.threshold(g, l["h_samples"])
            if thresh == 20:
                continue
            gg = np.where(np.array(g) >= 0, np.array(g), -100)
            pp = np.where(pred[n] >= 0, pred[n], -100)
            assert np.abs(np.abs(pp - gg[None]) - thresh).min() >= 1e-9


@pytest.mark.parametrize("S", [56, 48])
def test_goldens(golden, S):
    cases, labels, pred, pc, rt, expected = _golden_block(golden, S)
    per, best, arg, totals, bad = _run(labels, pred, pc, rt)
    wrong = np.nonzero((per != expected).any(1))[0]
    assert wrong.size == 0, [(int(cases[i]), str(golden["kind"][cases[i]]), per[i], expected[i]) for i in wrong[:5]]
    r_per, r_best, r_arg = _restate(labels, pred, pc, rt, None)
    assert np.array_equal(r_per, expected) and np.array_equal(best, r_best) and np.array_equal(arg, r_arg)
    seq = np.zeros(3)
    for row in expected:
        seq = seq + row
    print("totals", totals, "sequential", seq)
    assert np.all(np.abs(totals - seq) <= 1e-12 * np.abs(seq)) and int(bad[0]) == 0
    again = _run(labels, pred, pc, rt)
    for a, b in zip((per, best, arg, totals), again):
        assert a.tobytes() == b.tobytes()


def _random_batch(seed, M, N, S, G, P):
    """Labels with their own sample heights, and preds drawn from the label each image is indexed to."""
    from lanedetection_end2end_amd.clas import LaneLabels
    rng = np.random.default_rng(seed)
    labels = []
    for m in range(M):
        h = np.sort(rng.choice(np.arange(100, 720, 5), S, replace=False))
        gc = [0, G][m] if m < 2 else int(rng.integers(1, G + 1))
        lanes = []
        for _ in range(gc):
            x = np.rint(rng.uniform(200, 1080) + rng.uniform(-1.5, 1.5) * (h - 400) + rng.normal(0, 2, S)).astype(np.int64)
            x[: rng.integers(0, S // 2 + 1)] = -2
            x[(x < 0) | (x > 1279)] = -2
            lanes.append([int(v) for v in x])
        labels.append(dict(lanes=lanes, h_samples=[int(v) for v in h], raw_file="f%d" % m))
    labels = LaneLabels(labels)
    index = rng.permutation(np.arange(N) % M).astype(np.int32)
    pred = np.full((N, P, S), -2, np.int32)
    pc = rng.integers(0, P + 1, N).astype(np.int32)
    pc[:2] = [0, P]
    for n in range(N):
        src = labels.labels[index[n]]["lanes"]
        for p in range(P):                                    # (lanes past pred_count are filled too: they must not be read as preds)
            base = np.array(src[p % len(src)]) if src and rng.uniform() < 0.8 else np.rint(rng.uniform(0, 1279, S)).astype(np.int64)
            x = base + np.rint(rng.normal(0, 12, S)).astype(np.int64)
            x[(base < 0) | (x < 0) | (x > 1279)] = -2
            pred[n, p] = x
    return labels, pred, pc, index


def test_wave_loop_counts_and_index():
    labels, pred, pc, index = _random_batch(5, M=12, N=20, S=70, G=8, P=8)
    assert not labels.shared and labels.G == 8 and set(labels.counts) >= {0, 8} and set(pc) >= {0, 8}
    _assert_margin(labels, pred, index)
    per, best, arg, totals, bad = _run(labels, pred, pc, None, index)
    r_per, r_best, r_arg = _restate(labels, pred, pc, None, index)
    assert np.array_equal(per, r_per) and np.array_equal(best, r_best) and np.array_equal(arg, r_arg) and int(bad[0]) == 0
    assert len({tuple(r) for r in per}) > 8                   # a spread of scores, not one branch


@pytest.mark.parametrize("S", [1, 64, 65, 129, 256])
def test_sample_counts_at_the_wave_boundaries(S):
    labels, pred, pc, index = _random_batch(40 + S, M=5, N=6, S=min(S, 124), G=3, P=3)
    if S > 124:                                               # (only 124 distinct heights in the draw above: tile them, shifted)
        reps = -(-S // 124)
        for l in labels.labels:
            l["h_samples"] = [h + 1000 * r for r in range(reps) for h in l["h_samples"]][:S]
            l["lanes"] = [(lane * reps)[:S] for lane in l["lanes"]]
        from lanedetection_end2end_amd.clas import LaneLabels
        labels = LaneLabels(labels.labels)
        pred = np.ascontiguousarray(np.tile(pred, (1, 1, reps))[:, :, :S])
    _assert_margin(labels, pred, index)
    per, best, arg, _, bad = _run(labels, pred, pc, None, index)
    r_per, r_best, r_arg = _restate(labels, pred, pc, None, index)
    assert np.array_equal(per, r_per) and np.array_equal(best, r_best) and np.array_equal(arg, r_arg) and int(bad[0]) == 0


def test_bad_index(golden):
    cases, labels, pred, pc, rt, expected = _golden_block(golden, 56)
    n = 40
    index = np.arange(n, dtype=np.int32)
    index[[3, 17, 39]] = [labels.M, -1, 2 ** 31 - 1]
    per, best, arg, _, bad = _run(labels, pred[:n], pc[:n], rt[:n], index)
    assert int(bad[0]) == 3
    want = expected[:n].copy()
    want[[3, 17, 39]] = (0., 0., 1.)
    assert np.array_equal(per, want) and (best[[3, 17, 39]] == 0).all() and (arg[[3, 17, 39]] == -1).all()
    # more images than labels without an index: refused before anything is launched
    from lanedetection_end2end_amd import _lib
    with pytest.raises(_lib.LaneFitLibraryError):
        _run(labels, np.concatenate([pred, pred]))


@pytest.mark.parametrize("order", [0, 1, 2, 3])
def test_decode_feeds_score(order):
    from lanedetection_end2end_amd.clas import LaneLabels, Projections
    beta, line, horizon = decode_inputs(order)
    N, L, _ = beta.shape
    proj = Projections(Namespace(resize=256, order=order, batch_size=N))
    bt = torch.from_numpy(beta).cuda()
    _, ints = proj.decode_lanes([bt[:, l, :, None] for l in range(L)], torch.from_numpy(line).cuda(), torch.from_numpy(horizon).cuda())
    host = ints.cpu().numpy()
    rng = np.random.default_rng(300 + order)
    labels = []
    for n in range(N):                       # labels near the decoded lanes: shifted copies, a dropped or an extra lane
        lanes = []
        for l in rng.permutation(L)[: rng.integers(2, L + 1)]:
            x = host[n, l].astype(np.int64) + rng.integers(-30, 31) + np.rint(rng.normal(0, 3, host.shape[2])).astype(np.int64)
            x[(host[n, l] < 0) | (x < 0) | (x > 1279)] = -2
            x[: rng.integers(0, 20)] = -2
            lanes.append([int(v) for v in x])
        labels.append(dict(lanes=lanes, h_samples=H56, raw_file=str(n)))
    labels = LaneLabels(labels)
    index = rng.permutation(N).astype(np.int32)
    _assert_margin(labels, host, index)
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = torch.full((N, 3), -1., dtype=torch.float64, device="cuda")
    got = proj.score_lanes(ints, labels, torch.from_numpy(index).cuda(), out=out, bad_index=bad)
    assert got.data_ptr() == out.data_ptr()
    assert np.array_equal(got.cpu().numpy(), _restate(labels, host, None, None, index)[0]) and int(bad) == 0
    # the in-place form of the decode writes the same lanes
    ints2 = torch.empty_like(ints)
    none, same = proj.decode_lanes([bt[:, l, :, None] for l in range(L)], torch.from_numpy(line).cuda(), torch.from_numpy(horizon).cuda(),
                                   out_int=ints2)
    assert none is None and same is ints2 and torch.equal(ints2, ints)


def _lists(golden, c):
    S = int(golden["S"][c])
    return (laneeval_ref.unpack_case(golden["pred"][c], golden["pred_count"][c], S),
            laneeval_ref.unpack_case(golden["gt"][c], golden["gt_count"][c], S), [int(v) for v in golden["y_samples"][c, :S]],
            float(golden["run_time"][c]))


def test_bench_one_image(golden):
    from lanedetection_end2end_amd.bp.eval_lane import LaneEval
    kinds = list(golden["kind"])
    picks = [0, 5, 41, 100, 207, 215, kinds.index("run_time_250"), kinds.index("exact_20_vertical"), kinds.index("exact_20_single"),
             kinds.index("one_valid_sample")]
    for c in picks:
        got = LaneEval.bench(*_lists(golden, c))
        assert all(type(v) is float for v in got) and got == tuple(golden["expected"][c]), (c, got)
    with pytest.raises(Exception, match="Format of lanes error."):
        LaneEval.bench([[1, 2, 3]], [[1, 2, 3, 4]], [10, 20, 30, 40], 20)


def _dump(path, lines):
    path.write_text("".join(json.dumps(l) + "\n" for l in lines))
    return str(path)


def test_bench_one_submit(golden, tmp_path):
    from lanedetection_end2end_amd.bp.eval_lane import LaneEval
    cases = [c for c in range(0, 210, 7)]
    gts, preds = [], []
    for c in cases:
        p, g, h, rt = _lists(golden, c)
        gts.append(dict(lanes=g, h_samples=h, raw_file="clips/%d.jpg" % c))
        preds.append(dict(raw_file="clips/%d.jpg" % c, lanes=p, run_time=rt))
    preds = preds[::-1]                                       # matched by raw_file, not by position
    gt_file, pred_file = _dump(tmp_path / "gt.json", gts), _dump(tmp_path / "pred.json", preds)
    got = LaneEval.bench_one_submit(pred_file, gt_file)
    want = laneeval_ref.bench_one_submit(pred_file, gt_file)
    seq = np.sum(golden["expected"][cases], 0) / len(cases)
    print("bench_one_submit", got, "restatement", want)
    assert np.allclose(want, seq, rtol=1e-14, atol=0)
    assert all(abs(a - b) <= 1e-12 * abs(b) for a, b in zip(got, want)) and want[0] > 0
    # its exceptions
    with pytest.raises(Exception, match="We do not get the predictions of all the test tasks"):
        LaneEval.bench_one_submit(_dump(tmp_path / "short.json", preds[:-1]), gt_file)
    with pytest.raises(Exception, match="raw_file or lanes or run_time not in some predictions."):
        LaneEval.bench_one_submit(_dump(tmp_path / "nokey.json", [{k: v for k, v in preds[0].items() if k != "run_time"}] + preds[1:]), gt_file)
    with pytest.raises(Exception, match="Some raw_file from your predictions do not exist in the test tasks."):
        LaneEval.bench_one_submit(_dump(tmp_path / "unknown.json", [dict(preds[0], raw_file="nowhere.jpg")] + preds[1:]), gt_file)
    with pytest.raises(Exception, match="Format of lanes error."):
        LaneEval.bench_one_submit(_dump(tmp_path / "fmt.json", [dict(preds[0], lanes=[[1, 2, 3]])] + preds[1:]), gt_file)
    (tmp_path / "broken.json").write_text("{not json\n")
    with pytest.raises(Exception, match="Fail to load json file of the prediction."):
        LaneEval.bench_one_submit(str(tmp_path / "broken.json"), gt_file)


def _bp_args(N, R, K, **kw):
    a = dict(batch_size=N, nclasses=K, resize=R, end_to_end=True, mod="erfnet", layers=18, channels_in=3, pretrained=False, pool=True,
             activation_layer="square", no_cuda=False, order=2, reg_ls=0.0, use_cholesky=False, mask_percentage=0.2, clas=True,
             no_mapping=False, loss_policy="backproject", weight_seg=30, weight_funct="none", val_batch_size=N, draw_testset=False)
    a.update(kw)
    return Namespace(**a)


def _reference_statements(model, proj, x):
    """BP/test.py:60-89 on ``model.detect``'s outputs, with per-lane ``compute_coordinates`` and torch indexing."""
    from lanedetection_end2end_amd.clas import resize_coordinates
    beta0, beta1, beta2, beta3, outputs_line, outputs_horizon = model.detect(x)
    horizon_pred = torch.nn.Sigmoid()(outputs_horizon).sum(dim=1)
    horizon_pred = (torch.round((resize_coordinates(horizon_pred) + 80) / 10) * 10).int()
    line_pred = torch.round(torch.nn.Sigmoid()(outputs_line))
    lanes_pred = torch.stack([proj.compute_coordinates(b) for b in (beta0, beta1, beta2, beta3)], dim=1)
    line_pred = line_pred[:, [1, 2, 0, 3]]
    lanes_pred[(1 - line_pred[:, :, None]).bool().expand_as(lanes_pred)] = -2
    bounds = torch.div(horizon_pred - 160, 10, rounding_mode="trunc")
    for k, bound in enumerate(bounds):
        lanes_pred[k, :, :bound.item()] = -2
    lanes_pred[lanes_pred > 1279] = -2
    lanes_pred[lanes_pred < 0] = -2
    return np.int_(np.round(lanes_pred.data.cpu().numpy())).tolist()


def test_test_model_end_to_end(tmp_path, capsys):
    from lanedetection_end2end_amd.bp import test as bp_test
    from lanedetection_end2end_amd.bp.Networks.LSQ_layer import Net
    N, R, K = 2, 256, 4
    test_dir, save_path = tmp_path / "data", tmp_path / "out"
    test_dir.mkdir()
    save_path.mkdir()
    args = _bp_args(N, R, K, test_dir=str(test_dir), save_path=str(save_path))
    model = Net(args)
    model.net.load_state_dict(erfnet_oracle.make_params(seed=5, out_channels=K))
    model.line_classification.load_state_dict(clas_oracle.make_clas_params("line", seed=11))
    model.horizon_estimation.load_state_dict(clas_oracle.make_clas_params("horizon", seed=12))
    model = model.cuda().train()
    loader = [torch.from_numpy(inputs.images(N, R, 2 * R, seed=400 + i)) for i in range(3)]
    proj = bp_test.Projections(args)
    model.eval()
    expected = [lanes for x in loader for lanes in _reference_statements(model, proj, x.cuda())]
    model.train()                                             # test_model puts it in eval mode itself
    # labels: the lanes the model finds, shifted (some within the threshold, some not), 2..5 of them, plus one empty label
    rng = np.random.default_rng(9)
    labels = []
    for i, lanes in enumerate(expected):
        gt = []
        for l in range(int(rng.integers(2, 6))):
            x = np.array(lanes[l % 4]) + int(rng.integers(-25, 26)) + 40 * (l // 4)
            x[(np.array(lanes[l % 4]) < 0) | (x < 0) | (x > 1279)] = -2
            gt.append([int(v) for v in x])
        labels.append(dict(lanes=gt if i != 4 else [], h_samples=H56, raw_file="clips/%04d/20.jpg" % i))
    gt_file = _dump(test_dir / "test_label.json", labels)

    acc = bp_test.test_model(loader, model, None, None, None, None, args)
    assert not model.training and model.check_singular
    pred_file = str(save_path / "test_set_predictions.json")
    lines = [json.loads(l) for l in open(pred_file).readlines()]
    assert len(lines) == 6
    for line, label, lanes in zip(lines, labels, expected):
        assert line["run_time"] == 20 and line["raw_file"] == label["raw_file"] and line["h_samples"] == H56
        assert list(line.keys()) == ["lanes", "h_samples", "raw_file", "run_time"]
        assert line["lanes"] == lanes
    assert any(v >= 0 for line in lines for lane in line["lanes"] for v in lane), "every lane was gated away: the test checks nothing"
    want = laneeval_ref.bench_one_submit(pred_file, gt_file)
    out = capsys.readouterr().out
    print(out, "restatement", want)
    assert type(acc) is float and acc == want[0]
    assert "===> Average ACC on TESTSET is {:.8} in ".format(want[0]) in out and str(want) in out.splitlines()
    assert json.loads(open(gt_file).readline()) == labels[0]          # the label dicts are not what gets written to

    with pytest.raises(NotImplementedError):
        bp_test.test_model(loader, model, None, None, None, None, _bp_args(N, R, K, test_dir=str(test_dir), save_path=str(save_path),
                                                                         draw_testset=True))
    with pytest.raises(AssertionError):
        bp_test.test_model(loader, model, None, None, None, None, _bp_args(N, R, K, test_dir=str(test_dir), save_path=str(save_path),
                                                                         end_to_end=False))
    with pytest.raises(AssertionError):
        bp_test.test_model(loader, model, None, None, None, None, _bp_args(N, R, K, test_dir=str(test_dir), save_path=str(save_path),
                                                                         clas=False))
    with pytest.raises(IndexError):                           # more images than labels: gt_lanes[im_id] in the reference
        bp_test.test_model(loader + loader[:1], model, None, None, None, None, args)
