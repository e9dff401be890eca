#!/usr/bin/env python
"""Time the ``--clas`` tail of the BEV tree's ``validate()`` on an MI355X against the host leg it replaces.

    python tools/bev_lane_time.py [--out profiles/bev_lane_decode_time.json]

362 synthetic labels (10 % of TuSimple's 3 626 training frames, the reference's validation split) drawn like the golden family
(tools/gen_golden_bev_lanes.py: 4 or 5 gt lanes at the 56 heights, 4 predicted lanes fitted to them plus noise), in batches of 32.
* device: per batch ``ProjectionsBEV.decode_lanes`` written into the whole-set buffer and ``score_lanes`` on it in place, timed
  with in-stream event pairs (per batch and over the whole set), median of 5 passes with all of them reported; lanes and scores
  are checked against the restatements.
* host: wall time of what the reference does with the same data -- per batch the ``.tolist()`` of coefficients, line types and
  horizon rows, then one JSON file of the labels with them, ``write_lsq_results`` file to file (timed as the numpy restatement of
  tests/bev_lanes_ref.py) and ``LaneEval.bench_one_submit`` reading both files back (the restatement of tests/laneeval_ref.py:
  closed-form slope, the cheaper stand-in for sklearn's solver).
The baseline is that host leg; the device figures are never compared with themselves.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bev_lanes_ref  # noqa: E402
import gen_golden_bev_lanes as family  # noqa: E402
import laneeval_ref  # noqa: E402
from lanedetection_end2end_amd import geometry  # noqa: E402
from lanedetection_end2end_amd.clas import LaneLabels, ProjectionsBEV  # noqa: E402

FRAMES, BATCH, REPEATS, RESIZE = 362, 32, 5, 256
FLAGS = (False, False, False)            # what validate() passes (BEV/main.py:485-486)
H56 = list(range(160, 720, 10))


def make_set(M):
    lines = []
    for i in range(FRAMES):
        attempt = 0
        while True:
            rng = np.random.default_rng([91, i, attempt])
            line = family.draw_line(rng, H56, 0 if i % 3 == 0 else 6, M, False)
            if bev_lanes_ref.tie_margin(line["params"], line["lanes"], line["h_samples"], line["line_id"], line["horizon_est"], M,
                                        geometry.bev_homography()[1], RESIZE, *FLAGS) >= 1e-6:
                break
            attempt += 1
        line["raw_file"] = "clips/%d.jpg" % i
        lines.append(line)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bev_lane_decode_time.json"))
    a = ap.parse_args()
    M, M_inv = geometry.bev_homography()
    lines = make_set(M)
    labels = LaneLabels(lines)
    dev = torch.device("cuda")
    proj = ProjectionsBEV(argparse.Namespace(resize=RESIZE, nclasses=4))
    beta = torch.tensor([l["params"] for l in lines], dtype=torch.float32).to(dev)                # (FRAMES, 4, 3), the BEV model's dtype
    line_pred = torch.tensor([l["line_id"] for l in lines]).to(dev)
    horizon = torch.tensor([l["horizon_est"] for l in lines], dtype=torch.float32).to(dev)
    lanes = torch.empty(FRAMES, 4, labels.S, dtype=torch.int32, device=dev)
    scores = torch.empty(FRAMES, 3, dtype=torch.float64, device=dev)
    index = torch.arange(FRAMES, dtype=torch.int32, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    starts = list(range(0, FRAMES, BATCH))

    def device_pass():
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in starts]
        whole = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        whole[0].record()
        for (e0, e1), s in zip(ev, starts):
            e = min(s + BATCH, FRAMES)
            e0.record()
            proj.decode_lanes([beta[s:e, l, :, None] for l in range(4)], labels, index=index[s:e], line_pred=line_pred[s:e],
                              horizon_pred=horizon[s:e], out_int=lanes[s:e], bad_index=bad)
            proj.score_lanes(lanes[s:e], labels, index[s:e], out=scores[s:e], bad_index=bad)
            e1.record()
        whole[1].record()
        torch.cuda.synchronize()
        return whole[0].elapsed_time(whole[1]) * 1e-3, [x.elapsed_time(y) * 1e-3 for x, y in ev]

    res = dict(frames=FRAMES, batch=BATCH, batches=len(starts), device=torch.cuda.get_device_name(0))
    device_pass()                                                          # warm-up
    runs = sorted((device_pass() for _ in range(REPEATS)), key=lambda r: r[0])
    whole, per = runs[REPEATS // 2]
    res["device_decode_and_score_set_s"] = whole
    res["device_decode_and_score_batch_kernels_s"] = float(np.median(per))
    res["device_decode_and_score_set_s_all_runs"] = [r[0] for r in runs]
    got_lanes, got_scores = lanes.cpu().numpy(), scores.cpu().numpy()
    assert int(bad) == 0

    # the host leg of the reference's validate() on the same data
    tmp = tempfile.mkdtemp()
    src, dst = os.path.join(tmp, "val_set.json"), os.path.join(tmp, "ls_result.json")
    b3 = beta[:, :, :, None]
    torch.cuda.synchronize()
    t = time.perf_counter()
    params, types, rows = [], [], []
    for s in starts:
        params += torch.cat([b3[s:s + BATCH, l] for l in range(4)], 2).transpose(1, 2).data.tolist()
        types += line_pred[s:s + BATCH].data.tolist()
        rows += horizon[s:s + BATCH].data.tolist()
    res["host_tolist_s"] = time.perf_counter() - t
    t = time.perf_counter()
    with open(src, "w") as f:
        for l, p, ty, r in zip(lines, params, types, rows):
            json_line = dict(l, params=p, line_id=ty, horizon_est=r)
            json.dump(json_line, f)
            f.write("\n")
    res["host_json_write_s"] = time.perf_counter() - t
    t = time.perf_counter()
    bev_lanes_ref.write_lsq_results(src, dst, 4, *FLAGS[:2], RESIZE, FLAGS[2], M, M_inv)
    res["host_write_lsq_results_restatement_s"] = time.perf_counter() - t
    t = time.perf_counter()
    triple = laneeval_ref.bench_one_submit(dst, src)
    res["host_bench_one_submit_restatement_s"] = time.perf_counter() - t
    decoded = [json.loads(l) for l in open(dst).readlines()]
    want_lanes = np.array([l["lanes"] for l in decoded])
    want_scores = np.array([laneeval_ref.bench(l["lanes"], g["lanes"], g["h_samples"], 20) for l, g in zip(decoded, lines)])
    res["device_lanes_equal_restatement"] = bool(np.array_equal(got_lanes, want_lanes))
    res["device_scores_equal_restatement"] = bool(np.array_equal(got_scores, want_scores))
    res["accuracy"] = triple[0]
    res["host_leg_s"] = (res["host_tolist_s"] + res["host_json_write_s"] + res["host_write_lsq_results_restatement_s"]
                         + res["host_bench_one_submit_restatement_s"])
    res["host_leg_over_device_decode_and_score"] = res["host_leg_s"] / res["device_decode_and_score_set_s"]
    res["baseline_note"] = ("the host leg is timed with the numpy restatements of write_lsq_results and LaneEval (closed-form slope): the "
                            "cheaper stand-ins for the reference's own functions")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    assert res["device_lanes_equal_restatement"] and res["device_scores_equal_restatement"], "device results differ from the restatement"


if __name__ == "__main__":
    sys.exit(main())
