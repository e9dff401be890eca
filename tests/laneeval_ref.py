"""numpy restatement of ``LaneEval.bench`` / ``bench_one_submit`` (BP/eval_lane.py:15-95) for the lane-scoring tests.

The reference's two inexact steps are written in closed form here -- the angle is the centred least-squares slope instead of
``sklearn``'s solver, the threshold ``pixel_thresh * sqrt(1 + k^2)`` instead of ``pixel_thresh / cos(arctan k)`` -- and every
other statement is the reference's.  The hits are integer counts, so the three results carry the reference's bits whenever no
sample sits within rounding of its threshold: tools/gen_golden_laneeval.py asserts that margin (1e-9) on every golden case, and
tests/test_laneeval_cpu.py holds this module to the goldens with ``==``.
"""
import json

import numpy as np

PIXEL_THRESH = 20
PT_THRESH = 0.85


def slope(xs, y_samples):
    xs, ys = np.asarray(xs, np.float64), np.asarray(y_samples, np.float64)
    ok = xs >= 0
    xs, ys = xs[ok], ys[ok]
    if len(xs) < 2:
        return 0.
    dy = ys - ys.sum() / len(ys)
    dx = xs - xs.sum() / len(xs)
    syy = float((dy * dy).sum())
    return float((dy * dx).sum()) / syy if syy > 0 else 0.


def threshold(xs, y_samples, pixel_thresh=PIXEL_THRESH):
    k = slope(xs, y_samples)
    return pixel_thresh * np.sqrt(1. + k * k)


def line_accuracy(pred, gt, thresh):
    pred, gt = np.asarray(pred, np.float64), np.asarray(gt, np.float64)
    pred = np.where(pred >= 0, pred, -100.)
    gt = np.where(gt >= 0, gt, -100.)
    return float(np.sum(np.abs(pred - gt) < thresh)) / len(gt)


def bench_detail(pred, gt, y_samples, running_time, pixel_thresh=PIXEL_THRESH, pt_thresh=PT_THRESH):
    """-> ((accuracy, fp, fn), max_acc per gt lane, pred lane that reached it) -- the lists are empty on the early exit."""
    if any(len(p) != len(y_samples) for p in pred):
        raise Exception('Format of lanes error.')
    if running_time > 200 or len(gt) + 2 < len(pred):
        return (0., 0., 1.), [], []
    line_accs, args = [], []
    fn, matched = 0., 0.
    for x_gts in gt:
        thresh = threshold(x_gts, y_samples, pixel_thresh)
        accs = [line_accuracy(x_preds, x_gts, thresh) for x_preds in pred]
        max_acc = max(accs) if accs else 0.
        args.append(accs.index(max_acc) if accs else -1)
        if max_acc < pt_thresh:
            fn += 1
        else:
            matched += 1
        line_accs.append(max_acc)
    fp = len(pred) - matched
    if len(gt) > 4 and fn > 0:
        fn -= 1
    s = 0.
    for a in line_accs:         # (the reference's sum() adds numpy scalars one by one; on Python floats sum() would compensate)
        s = s + a
    if len(gt) > 4:
        s -= min(line_accs)
    return ((s / max(min(4.0, len(gt)), 1.), fp / len(pred) if len(pred) > 0 else 0., fn / max(min(len(gt), 4.), 1.)),
            line_accs, args)


def bench(pred, gt, y_samples, running_time):
    return bench_detail(pred, gt, y_samples, running_time)[0]


def bench_one_submit(pred_file, gt_file):
    json_pred = [json.loads(line) for line in open(pred_file).readlines()]
    json_gt = [json.loads(line) for line in open(gt_file).readlines()]
    assert len(json_gt) == len(json_pred)
    gts = {l['raw_file']: l for l in json_gt}
    accuracy, fp, fn = 0., 0., 0.
    for pred in json_pred:
        gt = gts[pred['raw_file']]
        a, p, n = bench(pred['lanes'], gt['lanes'], gt['h_samples'], pred['run_time'])
        accuracy += a
        fp += p
        fn += n
    num = len(gts)
    return [accuracy / num, fp / num, fn / num]


def unpack_case(lanes, count, S):
    """Rows of a padded (L, Smax) array -> the list-of-lists ``bench`` takes."""
    return [[int(v) for v in lanes[l, :S]] for l in range(int(count))]
