#!/usr/bin/env python
"""Generate tests/golden/bev_lanes.npz by running the REAL reference ``write_lsq_results`` (BEV/Dataloader/Load_Data_new.py) and
``LaneEval`` (BEV/eval_lane.py) on the CPU (authoring container only; needs the reference tree and sklearn):

    python tools/gen_golden_bev_lanes.py

The reference modules are imported at run time with what this container lacks stood in for: ``cv2`` by the oracle's
``getPerspectiveTransform`` (oracle/ref_shims), empty ``torchvision`` modules (the loader classes are not used), ``json`` as
``ujson`` and ``np.RankWarning``.

One "file" per (all_branches_ready, horizon_on, no_ortho) in FLAGS times the three height sets -- TuSimple's 48 (240..710) and
56 (160..710) and a synthetic, UNSORTED set of 130 (so that a wave lane holds more than one sample and the last iteration is
ragged) -- of LINES label lines each, nclasses = 4, resize = 256.  gt lanes are drawn like tools/gen_golden_laneeval.py's; the
params are least-squares fits of those lanes in the space the decoder evaluates them in, plus noise, rounded to fp32 (the BEV
model's beta is fp32; JSON holds it widened).  Per file the lines hold: a gt lane without a valid sample, one with exactly one, one
with -2 holes in the middle, five gt lanes, ``line_id`` zeros at positions 0 and 3, params of length 1, 2 and 3, constant terms that
push x below 0 and beyond 1279, and horizon sums that put ``minimum`` below and above 210.
Stored: arrays only -- the inputs, the reference's ``lanes``, ``LaneEval.bench`` of every line, ``bench_one_submit`` of every
file, and M / M_inv as the reference computes them.

Every line passes two margins before it is stored (a violating draw is resampled): every in-gate ``1279 x`` lies at least 1e-6
from a half-integer, and no |pred - gt| lies within 1e-9 of its LaneEval threshold.  An implementation can be held to these
outputs with ``==``.
"""
import json
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from oracle import ref_shims  # noqa: E402
import bev_lanes_ref  # noqa: E402
import gen_golden_laneeval as family  # noqa: E402
import laneeval_ref  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "bev_lanes.npz")
FLAGS = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 0, 1), (1, 1, 1)]
H130 = [int(v) for v in np.random.default_rng(130).permutation(np.arange(200, 720, 4))]
HEIGHTS = [family.H48, family.H56, H130]
LINES, NCLASSES, RESIZE, GMAX, SMAX = 6, 4, 256, 5, 130
ROUND_MARGIN = 1e-6


def load_reference():
    """-> (write_lsq_results, LaneEval, M, M_inv) of the reference's BEV tree."""
    ref_shims._install_cv2_stub()
    sys.modules.setdefault("ujson", json)
    for name in ("torchvision", "torchvision.transforms", "torchvision.transforms.functional", "torchvision.utils"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]
    sys.modules["torchvision"].utils = sys.modules["torchvision.utils"]
    sys.modules["torchvision.transforms"].functional = sys.modules["torchvision.transforms.functional"]
    if not hasattr(np, "RankWarning"):
        np.RankWarning = np.exceptions.RankWarning
    sys.path.insert(0, os.path.join(os.environ.get("LANEFIT_REFERENCE_ROOT", ref_shims.REF_ROOT), ref_shims.TREES["bev"]))
    from Dataloader.Load_Data_new import write_lsq_results
    from eval_lane import LaneEval
    import cv2
    src = np.float32([[0.45, 0.3], [0.55, 0.3], [0.1, 1], [0.9, 1]])
    dst = np.float32([[0.45, 0.3], [0.55, 0.3], [0.45, 1], [0.55, 1]])
    return write_lsq_results, LaneEval, cv2.getPerspectiveTransform(src, dst), cv2.getPerspectiveTransform(dst, src)


def fit_params(rng, gt, h, M, no_ortho, length, shift):
    """Coefficients (fp32, highest power first, ``length`` of them) that draw roughly the gt lane: a least-squares parabola through
    its valid samples in the decoder's own coordinates, noise and ``shift`` on the constant term."""
    gt, h = np.asarray(gt, np.float64), np.asarray(h, np.float64)
    ok = gt != -2
    if ok.sum() < 3:
        p = np.array([0., rng.uniform(-.3, .3), rng.uniform(.3, .7)])
    else:
        x, y_d = gt[ok] / 1279, (h[ok] - 80) / 639
        if no_ortho:
            xs, ys = x, 1 - y_d
        else:
            w = M[2, 0] * x + M[2, 1] * y_d + M[2, 2]
            xs = (M[0, 0] * x + M[0, 1] * y_d + M[0, 2]) / w
            ys = 1 - (M[1, 0] * x + M[1, 1] * y_d + M[1, 2]) / w
        p = np.polyfit(ys, xs, 2)
    p[2] += rng.normal(0, 0.004) + shift
    p[1] += rng.normal(0, 0.004)
    return [float(v) for v in p.astype(np.float32)[3 - length:]]


def draw_line(rng, h, k, M, no_ortho):
    """Label line k of a file: the special of that slot on top of an ordinary draw."""
    S = len(h)
    gt = [family.gt_lane(rng, h) for _ in range(5 if k == 0 else 4)]
    lengths, shifts = [3, 3, 3, 3], [0., 0., 0., 0.]
    line_id = [int(v) for v in rng.integers(1, 3, 4)]
    if k == 1:                                   # a gt lane without a valid sample; params of every length
        gt[2] = np.full(S, -2)
        lengths = [1, 2, 3, 3]
    elif k == 2:                                 # exactly one valid sample
        gt[1] = np.full(S, -2)
        gt[1][rng.integers(0, S)] = rng.integers(0, 1280)
        line_id[0] = 0
    elif k == 3:                                 # -2 holes in the middle of a lane that is valid on both sides of them
        gt[0] = np.rint(rng.uniform(300, 900) + rng.uniform(-.3, .3) * (np.asarray(h, np.float64) - 440)).astype(np.int64)
        gt[0][S // 3: S // 2] = -2
        gt[0][S // 2 + 3] = -2
    elif k == 4:
        line_id[0], line_id[3] = 0, 0
        gt[3] = np.full(S, -2)                   # (with all_branches_ready and line_id[3] == 0 this lane is skipped before its extent)
    elif k == 5:                                 # x below 0 and beyond 1279
        shifts = [-.9, .9, -.45, .45]
        line_id[3] = 0
    horizon = np.zeros(RESIZE)
    first = int(rng.integers(0, 100))
    horizon[first: first + (int(rng.integers(20, 50)) if k % 2 else int(rng.integers(56, 110)))] = 1.      # minimum below / above 210
    params = [fit_params(rng, gt[j], h, M, no_ortho, lengths[j], shifts[j]) for j in range(4)]
    return dict(lanes=[[int(v) for v in g] for g in gt], h_samples=list(h), params=params, line_id=line_id,
                horizon_est=[float(v) for v in horizon])


def main():
    write_lsq_results, LaneEval, M, M_inv = load_reference()
    files = [(f, h) for f in FLAGS for h in HEIGHTS]
    C = len(files) * LINES
    out = dict(file_id=np.zeros(C, np.int16), flags=np.zeros((C, 3), np.uint8), S=np.zeros(C, np.int16),
               h_samples=np.zeros((C, SMAX), np.int16), gt=np.full((C, GMAX, SMAX), -2, np.int16), gt_count=np.zeros(C, np.int8),
               params=np.zeros((C, 4, 3), np.float32), params_len=np.zeros((C, 4), np.int8), line_id=np.zeros((C, 4), np.int8),
               horizon=np.zeros((C, RESIZE), np.uint8), lanes=np.full((C, NCLASSES, SMAX), -2, np.int32),
               scores=np.zeros((C, 3), np.float64), triple=np.zeros((len(files), 3), np.float64), M=M, M_inv=M_inv,
               nclasses=np.int32(NCLASSES), resize=np.int32(RESIZE))
    resampled, worst = 0, np.inf
    tmp = tempfile.mkdtemp()
    for f, ((abr, hon, no), h) in enumerate(files):
        lines = []
        for k in range(LINES):
            attempt = 0
            while True:
                rng = np.random.default_rng([2025, f, k, attempt])
                line = draw_line(rng, h, k, M, bool(no))
                args = (line["params"], line["lanes"], h, line["line_id"], line["horizon_est"], M, M_inv)
                margin = bev_lanes_ref.tie_margin(*args, RESIZE, abr, hon, no)
                pred = bev_lanes_ref.decode(*args, NCLASSES, RESIZE, abr, hon, no).tolist()
                if margin >= ROUND_MARGIN and family.margin_ok(LaneEval, pred, line["lanes"], h):
                    break
                attempt += 1
                resampled += 1
            worst = min(worst, margin)
            line["raw_file"] = "clips/%d/%d.jpg" % (f, k)
            lines.append(line)
        src, dst = os.path.join(tmp, "src%d.json" % f), os.path.join(tmp, "dst%d.json" % f)
        with open(src, "w") as fh:
            fh.write("".join(json.dumps(l) + "\n" for l in lines))
        write_lsq_results(src, dst, NCLASSES, bool(abr), bool(hon), RESIZE, bool(no))
        got = [json.loads(l) for l in open(dst).readlines()]
        triple = LaneEval.bench_one_submit(dst, src)
        for k, (line, res) in enumerate(zip(lines, got)):
            c = f * LINES + k
            S = len(h)
            assert sorted(res.keys()) == sorted(list(line.keys()) + ["run_time"]) and res["run_time"] == 20
            lanes = np.array(res["lanes"])
            mine = bev_lanes_ref.decode(line["params"], line["lanes"], h, line["line_id"], line["horizon_est"], M, M_inv, NCLASSES,
                                        RESIZE, abr, hon, no)
            assert lanes.shape == (NCLASSES, S) and np.array_equal(lanes, mine), (c, lanes, mine)
            score = LaneEval.bench(res["lanes"], line["lanes"], h, 20)
            assert tuple(float(v) for v in score) == laneeval_ref.bench(res["lanes"], line["lanes"], h, 20), (c, score)
            out["file_id"][c], out["flags"][c], out["S"][c] = f, (abr, hon, no), S
            out["h_samples"][c, :S] = h
            out["gt_count"][c] = len(line["lanes"])
            out["gt"][c, :len(line["lanes"]), :S] = line["lanes"]
            for j, p in enumerate(line["params"]):
                out["params"][c, j, 3 - len(p):] = p
                out["params_len"][c, j] = len(p)
                assert [float(v) for v in out["params"][c, j, 3 - len(p):]] == p           # fp32 holds them exactly
            out["line_id"][c] = line["line_id"]
            out["horizon"][c] = line["horizon_est"]
            out["lanes"][c, :, :S] = lanes
            out["scores"][c] = score
        out["triple"][f] = triple
    inside = out["lanes"][out["lanes"] != -2]
    assert inside.min() < 0 and inside.max() > 1279 and np.any(out["scores"][:, 0] > 0.5)
    np.savez_compressed(OUT, **out)
    print(OUT, "%.1f KB" % (os.path.getsize(OUT) / 1024), C, "lines in", len(files), "files,", resampled,
          "resampled; smallest rounding margin %.2e; mean accuracy %.3f fp %.3f fn %.3f" % ((worst,) + tuple(out["scores"].mean(0))))


if __name__ == "__main__":
    sys.exit(main())
