#!/usr/bin/env python
"""Generate tests/golden/laneeval.npz by running the REAL reference ``LaneEval.bench`` (BP/eval_lane.py) on the CPU
(authoring container only; needs the reference tree and sklearn):

    python tools/gen_golden_laneeval.py

Seeded cases: straight gt lanes x = a + k (y - 440) with k in +-1.5 and 2-pixel noise, cut at a random horizon and at the frame's
edges (-2 there, as TuSimple writes them); pred lanes are gt lanes with 12-pixel noise (some shifted far enough to miss) plus
unrelated ones, in shuffled order.
* every G_n in 0..6 times every P_n in 0..5, five draws each at S = 56 (the TuSimple heights 160..710) and one each at S = 48;
  these hold G_n + 2 < P_n and G_n > 4 with and without a miss;
* specials: gt / pred lanes that are all -2, a gt lane with exactly one valid sample and one with none (angle 0, threshold
  exactly 20), run_time 250, and |pred - gt| exactly 20 against a lane with k = 0 (not a hit: the comparison is strict).
Stored: inputs as int16 padded to (6 | 5, 56), counts, S, y_samples, run times, and the reference's three outputs as fp64.

Every case passes the tie margin below before it is stored (a violating draw is resampled): the reference's threshold
``pixel_thresh / cos(arctan k)`` with sklearn's k, and any closed form of it, then count the same hits, so an implementation can
be held to these outputs with ``==``.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import ref_shims  # noqa: E402
import laneeval_ref  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "laneeval.npz")
GMAX, PMAX, SMAX = 6, 5, 56
MARGIN = 1e-9
H56 = list(range(160, 720, 10))
H48 = list(range(240, 720, 10))


def load_reference():
    sys.modules.setdefault("ujson", json)
    sys.path.insert(0, os.path.join(os.environ.get("LANEFIT_REFERENCE_ROOT", ref_shims.REF_ROOT), ref_shims.TREES["bp"]))
    from eval_lane import LaneEval
    return LaneEval


def gt_lane(rng, h):
    h = np.asarray(h, np.float64)
    x = rng.uniform(200, 1080) + rng.uniform(-1.5, 1.5) * (h - 440) + rng.normal(0, 2, len(h))
    x = np.rint(x).astype(np.int64)
    x[: rng.integers(0, 2 * len(h) // 3)] = -2
    x[(x < 0) | (x > 1279)] = -2
    return x


def pred_of(rng, g):
    p = g + np.rint(rng.normal(0, 12, len(g))).astype(np.int64) + (rng.integers(25, 80) if rng.uniform() < 0.3 else 0)
    p[g < 0] = -2
    cut = rng.integers(0, 6)
    if cut:
        p[:cut] = -2
    p[(p < 0) | (p > 1279)] = -2
    return p


def draw(rng, G, P, h):
    gt = [gt_lane(rng, h) for _ in range(G)]
    pred = [pred_of(rng, gt[i]) if i < G else gt_lane(rng, h) for i in range(P)]
    order = rng.permutation(P)
    return [pred[i] for i in order], gt, h, 20.


def special(rng, kind):
    h = H56
    S = len(h)
    pred, gt, h, rt = draw(rng, 3, 3, h)
    if kind == "gt_all_invalid":
        gt = [np.full(S, -2) for _ in gt]
    elif kind == "pred_all_invalid":
        pred = [np.full(S, -2) for _ in pred]
    elif kind == "both_all_invalid":
        gt = [np.full(S, -2) for _ in gt]
        pred = [np.full(S, -2) for _ in pred]
    elif kind == "one_valid_sample":
        gt[1] = np.full(S, -2)
        gt[1][rng.integers(0, S)] = rng.integers(0, 1280)
        pred[0] = gt[1].copy()
    elif kind == "no_valid_sample":
        gt[2] = np.full(S, -2)
        pred[1] = np.full(S, -2)
    elif kind == "run_time_250":
        rt = 250.
    elif kind == "exact_20_vertical":            # a vertical lane: k = 0, threshold exactly 20; 20 away is NOT a hit, 19 is
        gt[0] = np.full(S, rng.integers(100, 1100))
        pred[0] = gt[0] + 20
        pred[1] = gt[0] - 19
        pred[2] = gt[0].copy()
        pred[2][::2] -= 20
    elif kind == "exact_20_single":              # one valid sample: k = 0 by definition
        gt[0] = np.full(S, -2)
        gt[0][10] = 500
        pred[0] = np.full(S, -2)
        pred[0][10] = 520
        pred[1] = np.full(S, -2)
        pred[1][10] = 481
    else:
        raise KeyError(kind)
    return pred, gt, h, rt


def margin_ok(ref, pred, gt, h):
    """||pred - gt| - thresh| >= MARGIN for every (gt lane, pred lane, sample), unless thresh is pixel_thresh exactly."""
    ys = np.array(h)
    for g in gt:
        thresh = ref.pixel_thresh / np.cos(ref.get_angle(np.array(g), ys))
        if thresh == ref.pixel_thresh:
            continue
        gg = np.where(np.array(g) >= 0, np.array(g), -100)
        for p in pred:
            pp = np.where(np.array(p) >= 0, np.array(p), -100)
            if np.any(np.abs(np.abs(pp - gg) - thresh) < MARGIN):
                return False
    return True


def main():
    ref = load_reference()
    plan = []
    for rep in range(5):
        plan += [("grid56", G, P, rep) for G in range(GMAX + 1) for P in range(PMAX + 1)]
    plan += [("grid48", G, P, 0) for G in range(GMAX + 1) for P in range(PMAX + 1)]
    kinds = ["gt_all_invalid", "pred_all_invalid", "both_all_invalid", "one_valid_sample", "no_valid_sample", "run_time_250",
             "exact_20_vertical", "exact_20_single"]
    plan += [(k, 3, 3, rep) for k in kinds for rep in range(6)]
    C = len(plan)
    out = dict(pred=np.full((C, PMAX, SMAX), -2, np.int16), gt=np.full((C, GMAX, SMAX), -2, np.int16),
               pred_count=np.zeros(C, np.int32), gt_count=np.zeros(C, np.int32), S=np.zeros(C, np.int32),
               y_samples=np.zeros((C, SMAX), np.int16), run_time=np.zeros(C, np.float32), expected=np.zeros((C, 3), np.float64),
               kind=np.array([p[0] for p in plan]))
    resampled = 0
    for c, (kind, G, P, rep) in enumerate(plan):
        attempt = 0
        while True:
            rng = np.random.default_rng([2024, c, attempt])
            if kind.startswith("grid"):
                pred, gt, h, rt = draw(rng, G, P, H56 if kind == "grid56" else H48)
            else:
                pred, gt, h, rt = special(rng, kind)
            if margin_ok(ref, pred, gt, h):
                break
            attempt += 1
            resampled += 1
        if kind.startswith("exact_20"):           # gt lane 0 is the k = 0 lane: the reference's threshold is 20 exactly
            assert ref.pixel_thresh / np.cos(ref.get_angle(np.array(gt[0]), np.array(h))) == ref.pixel_thresh
        lists = ([[int(v) for v in p] for p in pred], [[int(v) for v in g] for g in gt], list(h))
        res = ref.bench(lists[0], lists[1], lists[2], rt)
        assert tuple(float(v) for v in res) == laneeval_ref.bench(*lists, rt), (c, kind, res)
        S = len(h)
        for i, p in enumerate(pred):
            out["pred"][c, i, :S] = p
        for i, g in enumerate(gt):
            out["gt"][c, i, :S] = g
        out["pred_count"][c], out["gt_count"][c], out["S"][c] = len(pred), len(gt), S
        out["y_samples"][c, :S] = h
        out["run_time"][c] = rt
        out["expected"][c] = res
    gc, pc, e = out["gt_count"], out["pred_count"], out["expected"]
    assert C >= 300 and set(gc) >= set(range(7)) and set(pc) >= set(range(6))
    assert np.any(gc + 2 < pc) and np.any((gc > 4) & (e[:, 2] > 0)) and np.any((gc > 4) & (e[:, 2] == 0) & (gc + 2 >= pc))
    np.savez_compressed(OUT, **out)
    print(OUT, "%.1f KB" % (os.path.getsize(OUT) / 1024), C, "cases,", resampled, "resampled; mean accuracy %.3f fp %.3f fn %.3f"
          % tuple(e.mean(0)))


if __name__ == "__main__":
    sys.exit(main())
