#!/usr/bin/env python
"""Time the scoring stage of ``test_model`` on an MI355X against the host leg it replaces.

    python tools/lane_eval_time.py [--out profiles/lane_eval_time.json]

2 782 synthetic labels (the size of TuSimple's test set) and predicted lanes drawn like the golden family
(tools/gen_golden_laneeval.py: 4 pred lanes, 2..5 gt lanes), in batches of 64.
* device: per batch ``decode_lanes`` written into the whole-set buffer and ``score_lanes`` on it in place, timed with in-stream
  event pairs (per batch and over the whole set); the scoring alone on the family's lanes is timed the same way and checked
  against the restatement.
* host: wall time of what the reference's ``test_model`` does with the same data -- ``.cpu().numpy()`` + round + ``.tolist()``
  per batch, the ``bound.item()`` loop per image, and ``LaneEval.bench`` over the set.  ``bench`` is timed as the numpy
  restatement of tests/laneeval_ref.py (closed-form slope: it stands in for sklearn's solver and is the cheaper of the two) and,
  when sklearn imports, with ``LinearRegression.fit`` for the angle as the reference has it.
The baseline is that host leg; the device figures are never compared with themselves.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden_laneeval as family  # noqa: E402
import laneeval_ref  # noqa: E402
from lanedetection_end2end_amd.clas import LaneLabels, Projections  # noqa: E402

FRAMES, BATCH, REPEATS = 2782, 64, 5


def make_set():
    labels, preds = [], []
    for i in range(FRAMES):
        rng = np.random.default_rng([77, i])
        pred, gt, h, _ = family.draw(rng, int(rng.integers(2, 6)), 4, family.H56)
        labels.append(dict(lanes=[[int(v) for v in g] for g in gt], h_samples=list(h), raw_file="clips/%d.jpg" % i))
        preds.append(np.stack(pred))
    return labels, np.stack(preds).astype(np.int32)


def sklearn_bench():
    """``bench`` with the angle from ``LinearRegression.fit``, as the reference computes it; None without sklearn."""
    try:
        from sklearn.linear_model import LinearRegression
    except Exception:
        return None
    lr = LinearRegression()

    def threshold(xs, y_samples, pixel_thresh=20):
        xs, ys = np.array(xs), np.array(y_samples)
        ok = xs >= 0
        k = 0.
        if ok.sum() > 1:
            lr.fit(ys[ok][:, None], xs[ok])
            k = lr.coef_[0]
        return pixel_thresh / np.cos(np.arctan(k))
    return threshold


def host_bench(labels, lanes, threshold=None):
    saved = laneeval_ref.threshold
    if threshold is not None:
        laneeval_ref.threshold = threshold
    try:
        t = time.perf_counter()
        acc = 0.
        for l, p in zip(labels, lanes):
            acc += laneeval_ref.bench(p, l["lanes"], l["h_samples"], 20)[0]
        return time.perf_counter() - t, acc / len(labels)
    finally:
        laneeval_ref.threshold = saved


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lane_eval_time.json"))
    a = ap.parse_args()
    labels_list, pred = make_set()
    labels = LaneLabels(labels_list)
    dev = torch.device("cuda")
    proj = Projections(argparse.Namespace(resize=256, order=2, batch_size=BATCH))
    rng = np.random.default_rng(3)
    beta = np.zeros((FRAMES, 4, 3))
    beta[..., 2], beta[..., 1], beta[..., 0] = rng.uniform(60, 450, (FRAMES, 4)), rng.uniform(-.6, .6, (FRAMES, 4)), rng.uniform(-2e-3, 2e-3, (FRAMES, 4))
    beta = torch.from_numpy(beta).to(dev)
    line = torch.from_numpy((rng.uniform(0, 1, (FRAMES, 4)) > 0.1).astype(np.float32)).to(dev)
    horizon = torch.from_numpy((rng.integers(15, 30, FRAMES) * 10).astype(np.int32)).to(dev)
    lanes = torch.empty(FRAMES, 4, 56, dtype=torch.int32, device=dev)
    scores = torch.empty(FRAMES, 3, dtype=torch.float64, device=dev)
    family_lanes = torch.from_numpy(pred).to(dev)
    index = torch.arange(FRAMES, dtype=torch.int32, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    starts = list(range(0, FRAMES, BATCH))

    def device_pass(decode):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in starts]
        whole = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        whole[0].record()
        for (e0, e1), s in zip(ev, starts):
            e = min(s + BATCH, FRAMES)
            e0.record()
            if decode:
                proj.decode_lanes([beta[s:e, l, :, None] for l in range(4)], line[s:e], horizon[s:e], out_int=lanes[s:e])
                proj.score_lanes(lanes[s:e], labels, index[s:e], out=scores[s:e], bad_index=bad)
            else:
                proj.score_lanes(family_lanes[s:e], labels, index[s:e], out=scores[s:e], bad_index=bad)
            e1.record()
        whole[1].record()
        torch.cuda.synchronize()
        return whole[0].elapsed_time(whole[1]) * 1e-3, [x.elapsed_time(y) * 1e-3 for x, y in ev]

    res = dict(frames=FRAMES, batch=BATCH, batches=len(starts), device=torch.cuda.get_device_name(0))
    for name, decode in (("decode_and_score", True), ("score_only", False)):
        device_pass(decode)                                            # warm-up
        runs = sorted((device_pass(decode) for _ in range(REPEATS)), key=lambda r: r[0])
        whole, per = runs[REPEATS // 2]
        res["device_%s_set_s" % name] = whole
        res["device_%s_batch_kernels_s" % name] = float(np.median(per))
        res["device_%s_set_s_all_runs" % name] = [r[0] for r in runs]
    got = scores.cpu().numpy()                                         # (the last pass scored the family's lanes)
    assert int(bad) == 0

    # the host leg of the reference's test_model on the same data
    x64 = family_lanes.double()
    bounds = torch.div(horizon - 160, 10, rounding_mode="trunc")
    torch.cuda.synchronize()
    t = time.perf_counter()
    lists = []
    for s in starts:
        lists += np.int_(np.round(x64[s:s + BATCH].data.cpu().numpy())).tolist()
    res["host_cpu_numpy_tolist_s"] = time.perf_counter() - t
    t = time.perf_counter()
    for s in starts:
        for k, bound in enumerate(bounds[s:s + BATCH]):
            bound.item()
    res["host_horizon_item_loop_s"] = time.perf_counter() - t
    res["host_bench_restatement_s"], acc = host_bench(labels_list, lists)
    want = np.array([laneeval_ref.bench(p, l["lanes"], l["h_samples"], 20) for l, p in zip(labels_list, lists)])
    res["device_equals_restatement"] = bool(np.array_equal(got, want))
    res["accuracy"] = acc
    thr = sklearn_bench()
    res["sklearn_available"] = thr is not None
    if thr is not None:
        res["host_bench_sklearn_s"], acc_sk = host_bench(labels_list, lists, thr)
        res["sklearn_bench_equals_restatement"] = acc_sk == acc
    res["baseline_note"] = ("host_bench_restatement_s is the numpy restatement of LaneEval.bench (closed-form slope), standing in for "
                            "sklearn's solver; host_bench_sklearn_s, when present, is bench with LinearRegression.fit as the reference has it")
    bench_s = res.get("host_bench_sklearn_s", res["host_bench_restatement_s"])
    res["host_leg_s"] = res["host_cpu_numpy_tolist_s"] + res["host_horizon_item_loop_s"] + bench_s
    res["host_leg_restatement_s"] = res["host_cpu_numpy_tolist_s"] + res["host_horizon_item_loop_s"] + res["host_bench_restatement_s"]
    res["host_leg_over_device_decode_and_score"] = res["host_leg_s"] / res["device_decode_and_score_set_s"]
    res["host_leg_restatement_over_device_decode_and_score"] = res["host_leg_restatement_s"] / res["device_decode_and_score_set_s"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    assert res["device_equals_restatement"], "device scores differ from the restatement"


if __name__ == "__main__":
    sys.exit(main())
