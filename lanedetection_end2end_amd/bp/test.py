"""``test`` of the BP tree (BP/test.py): ``test_model`` with the reference's signature, its three stages on the device --
``model.detect`` (image -> lane coefficients, line flags, horizon), ``Projections.decode_lanes`` (coefficients -> 56 x coordinates
per lane with test_model's gates) and ``Projections.score_lanes`` (TuSimple accuracy / FP / FN, ``LaneEval.bench``) -- with no
host synchronisation inside the loop: lanes and scores of every batch land in one device buffer sized for the label file, which is
read once behind the loop; the predictions file is written from that copy."""
import json
import os

import torch

from lanedetection_end2end_amd import ops
from lanedetection_end2end_amd.clas import (LaneLabels, Projections, horizon_row, line_flags,  # noqa: F401
                                            resize_coordinates)


def test_model(loader, model, criterion, criterion_seg, criterion_line_class, criterion_horizon, args, epoch=0):
    """BP/test.py:23-129.  Writes ``args.save_path/test_set_predictions.json`` (each label's dict with ``lanes`` replaced and
    ``run_time`` 20), prints the reference's two lines and returns the TuSimple accuracy.  The per-image scores are added on the
    host in file order, as ``bench_one_submit`` adds them, so the returned value carries the reference's bits.
    ``args.draw_testset`` is not provided (it draws on the frames on disk with OpenCV): ``NotImplementedError``."""
    assert args.end_to_end == True  # noqa: E712  (the reference's statement)
    if getattr(args, "draw_testset", False):
        raise NotImplementedError("lanefit test_model does not draw the test set (args.draw_testset): it needs OpenCV and the frames")
    params = Projections(args)
    gt_file = os.path.join(args.test_dir, 'test_label.json')
    labels = LaneLabels(gt_file)
    test_set_file = os.path.join(args.save_path, 'test_set_predictions.json')
    net = model if hasattr(model, "detect") else model.module            # (nn.DataParallel around the mirror's Net)
    M, L, S = labels.M, 4, params.num_heights
    rows = labels.rows_by_raw_file()             # a prediction is scored against the label of its raw_file (the last of that name)

    model.eval()
    device = torch.device("cuda", torch.cuda.current_device())
    # one buffer for everything read back: (M, 3) fp64 scores | (M, L, S) int32 lanes | 2 int32 words (bad index count, fit status)
    buf = torch.zeros(M * 3 * 8 + (M * L * S + 2) * 4, dtype=torch.uint8, device=device)
    scores = buf[:M * 24].view(torch.float64).view(M, 3)
    ints = buf[M * 24:].view(torch.int32)
    lanes, words = ints[:M * L * S].view(M, L, S), ints[M * L * S:]
    index = torch.tensor([rows[l['raw_file']] for l in labels.labels], dtype=torch.int32, device=device)
    events, done = [], 0
    check_singular, net.check_singular = net.check_singular, False       # (its status read is a host sync: deferred to the end)
    try:
        with torch.no_grad():
            for i, input in enumerate(loader):
                if not args.no_cuda:
                    input = input.cuda(non_blocking=True).float()
                n = input.size(0)
                start = i * args.val_batch_size                          # im_id = i * val_batch_size + j
                if start + n > M:
                    raise IndexError("list index out of range")          # what gt_lanes[im_id] raises
                events.append((torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)))
                events[-1][0].record()
                beta0, beta1, beta2, beta3, outputs_line, outputs_horizon = net.detect(input)
                events[-1][1].record()
                words[1:2].copy_(torch.maximum(words[1:2], net.last_status.max().to(torch.int32).reshape(1)))

                # Horizon task & Line classification task
                if args.clas:
                    horizon_pred = horizon_row(outputs_horizon)
                    line_pred = line_flags(outputs_line)
                else:
                    assert False

                # X coordinates, line type gate, horizon gate, range gate, rounding: one launch, written in place
                params.decode_lanes([beta0, beta1, beta2, beta3], line_pred, horizon_pred, out_int=lanes[start:start + n])
                params.score_lanes(lanes[start:start + n], labels, index[start:start + n], out=scores[start:start + n],
                                   bad_index=words[0:1])
                done = max(done, start + n)
    finally:
        net.check_singular = check_singular

    host = buf.cpu()                                                     # the one copy (and the one synchronisation)
    scores_h = host[:M * 24].view(torch.float64).view(M, 3)
    ints_h = host[M * 24:].view(torch.int32)
    lanes_h, bad, status = ints_h[:M * L * S].view(M, L, S), int(ints_h[M * L * S]), int(ints_h[M * L * S + 1])
    if bad:
        raise IndexError("test_model: %d images were scored against a label outside the label file" % bad)
    if status and check_singular:
        raise ops.SingularMatrixError("lanefit WLS: a normal matrix of the test set is %s" %
                                      ("not positive-definite (Cholesky/GELS path)" if status == 2 else "singular"))
    batch_time = sum(a.elapsed_time(b) for a, b in events) * 1e-3 / max(len(events), 1)

    with open(test_set_file, 'w') as jsonFile:
        for im_id in range(done):
            json_line = dict(labels.labels[im_id])
            json_line["lanes"] = lanes_h[im_id].tolist()
            json_line["run_time"] = 20
            json.dump(json_line, jsonFile)
            jsonFile.write('\n')

    # Calculate accuracy
    if args.clas and args.nclasses > 3:
        if done != M:
            raise Exception('We do not get the predictions of all the test tasks')
        accuracy, fp, fn = 0., 0., 0.
        for a, p, n in scores_h.tolist():
            accuracy += a
            fp += p
            fn += n
        num = len(rows)
        acc_seg = [accuracy / num, fp / num, fn / num]
        print(acc_seg)
        print("===> Average ACC on TESTSET is {:.8} in {:.6}s for a batch".format(acc_seg[0], batch_time))
    return acc_seg[0]
