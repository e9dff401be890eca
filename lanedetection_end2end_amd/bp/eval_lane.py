"""``eval_lane`` of the BP tree (BP/eval_lane.py): ``LaneEval`` with the reference's names, scoring on the device
(``lf_lane_eval``).  Integer coordinates only, at most 8 lanes a side and 256 sample heights (``ValueError`` beyond)."""
import json

import numpy as np
import torch

from lanedetection_end2end_amd import _lib
from lanedetection_end2end_amd.clas import MAX_LANES, LaneLabels, _int_coordinates, lane_eval


def _device():
    if not torch.cuda.is_available():
        raise _lib.LaneFitLibraryError("lanefit LaneEval scores on the MI355X; there is no CPU path")
    return torch.device("cuda", torch.cuda.current_device())


def _pred_table(preds, S, device):
    """Lists of pred lanes (each lane S long) -> ((N, P, S) int32, (N) counts) on the device."""
    P = max(1, max(len(p) for p in preds))
    if P > MAX_LANES:
        raise ValueError("LaneEval: %d predicted lanes, the scoring kernel takes %d" % (P, MAX_LANES))
    table = np.full((len(preds), P, S), -2, np.int32)
    counts = np.zeros(len(preds), np.int32)
    for i, p in enumerate(preds):
        counts[i] = len(p)
        if p:
            table[i, :len(p)] = _int_coordinates(p)
    return torch.from_numpy(table).to(device), torch.from_numpy(counts).to(device)


class LaneEval(object):
    pixel_thresh = 20
    pt_thresh = 0.85

    @staticmethod
    def bench(pred, gt, y_samples, running_time):
        """One image: -> (accuracy, fp, fn) as Python floats, one launch and one host read."""
        if any(len(p) != len(y_samples) for p in pred):
            raise Exception('Format of lanes error.')
        dev = _device()
        labels = LaneLabels([dict(lanes=gt, h_samples=y_samples, raw_file='')])
        table, counts = _pred_table([pred], labels.S, dev)
        run_time = torch.tensor([float(running_time)], dtype=torch.float32, device=dev)
        per_image = lane_eval(table, labels, pred_count=counts, run_time=run_time, pixel_thresh=LaneEval.pixel_thresh,
                              pt_thresh=LaneEval.pt_thresh)[0]
        a, p, n = per_image[0].tolist()
        return a, p, n

    @staticmethod
    def bench_one_submit(pred_file, gt_file):
        """-> [accuracy, fp, fn] averaged over the label file: both files parsed on the host, one launch pair (scores, then
        their fixed-order sums) and one host read.  The sums come from a tree, so they agree with the reference's running sum
        to fp64 rounding (1e-12 relative), not to the bit; ``test_model`` adds the per-image scores in the reference's order."""
        try:
            json_pred = [json.loads(line) for line in open(pred_file).readlines()]
        except BaseException:
            raise Exception('Fail to load json file of the prediction.')
        json_gt = [json.loads(line) for line in open(gt_file).readlines()]
        if len(json_gt) != len(json_pred):
            raise Exception('We do not get the predictions of all the test tasks')
        gts = {l['raw_file']: l for l in json_gt}
        labels = LaneLabels(list(gts.values()))
        rows = labels.rows_by_raw_file()
        index = np.zeros(len(json_pred), np.int32)
        for i, pred in enumerate(json_pred):
            if 'raw_file' not in pred or 'lanes' not in pred or 'run_time' not in pred:
                raise Exception('raw_file or lanes or run_time not in some predictions.')
            if pred['raw_file'] not in rows:
                raise Exception('Some raw_file from your predictions do not exist in the test tasks.')
            if any(len(p) != labels.S for p in pred['lanes']):
                raise Exception('Format of lanes error.')
            index[i] = rows[pred['raw_file']]
        dev = _device()
        table, counts = _pred_table([p['lanes'] for p in json_pred], labels.S, dev)
        run_time = torch.tensor([float(p['run_time']) for p in json_pred], dtype=torch.float32, device=dev)
        totals = lane_eval(table, labels, index=torch.from_numpy(index).to(dev), pred_count=counts, run_time=run_time,
                           pixel_thresh=LaneEval.pixel_thresh, pt_thresh=LaneEval.pt_thresh, want_totals=True)[3]
        accuracy, fp, fn = totals.tolist()
        num = len(gts)
        return [accuracy / num, fp / num, fn / num]
