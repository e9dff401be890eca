"""numpy restatement of the BEV tree's lane decoding (``write_lsq_results``, BEV/Dataloader/Load_Data_new.py:334-420) for the
BEV lane tests, in the role tests/laneeval_ref.py has for the scoring.

Per label line: every predicted lane j is gated by the extent of gt lane j (lowest and highest sample height among its x != -2),
its polynomial is evaluated in the normalised bird's-eye view (or, with ``no_ortho``, directly in the normalised image), mapped
back through M_inv, scaled by 1279 and rounded half to even.  The only inexact steps are the fp64 evaluation and the homography:
tools/gen_golden_bev_lanes.py asserts that every in-gate ``1279 x`` of a golden lies at least 1e-6 from a half-integer, far
beyond any reordering of those sums, so this module, the device kernel and the reference round to the same integers and
tests/test_bev_lanes_cpu.py holds this module to the goldens with ``==``.
"""
import json

import numpy as np

INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def scaled_x(params, h_samples, M, M_inv, no_ortho):
    """``1279 x`` (S) fp64 of one lane before rounding and gating; ``params`` highest power first, at most three."""
    if len(params) > 3:
        raise ValueError("a lane of %d coefficients: at most 3 (a, b, c)" % len(params))
    a, b, c = [0.] * (3 - len(params)) + [float(v) for v in params]
    y_d = (np.asarray(h_samples, np.float64) - 80) / 639
    if no_ortho:
        y = 1 - y_d
        x = a * y ** 2 + b * y + c
    else:
        yp = (M[1, 1] * y_d + M[1, 2]) / (M[2, 1] * y_d + M[2, 2])
        y = 1 - yp
        xp = a * y ** 2 + b * y + c
        x = (M_inv[0, 0] * xp + M_inv[0, 1] * yp + M_inv[0, 2]) / (M_inv[2, 0] * xp + M_inv[2, 1] * yp + M_inv[2, 2])
    return x * 1279


def lane_extent(gt_lane, h_samples):
    """-> (number of samples with x != -2, their lowest height, their highest); (0, 250, 710) without one."""
    h = np.asarray(h_samples, np.float64)[np.asarray(gt_lane) != -2]
    return (len(h), h.min(), h.max()) if len(h) else (0, 250., 710.)


def gate(h_samples, gt_lane, j, line_id, horizon_est, factor, all_branches_ready, horizon_on):
    """-> boolean (S) mask of the samples lane j writes, or None when the lane is skipped."""
    count, lo, hi = lane_extent(gt_lane, h_samples)
    if all_branches_ready:
        if (j == 2 and line_id[0] == 0) or (j == 3 and line_id[3] == 0):
            return None
        if horizon_on:
            lo = float(np.sum(np.asarray(horizon_est, np.float64))) * factor + 80
    elif count == 0:
        return None
    h = np.asarray(h_samples, np.float64)
    return (h >= max(210, lo)) & (h <= hi)


def decode(params, gt_lanes, h_samples, line_id, horizon_est, M, M_inv, nclasses, resize, all_branches_ready=False, horizon_on=False,
           no_ortho=False, int32=False):
    """One label line -> (nclasses, S) lanes.  int64 as the reference converts (``np.int_``; NaN and values beyond int64 are what
    the platform's conversion gives), or with ``int32`` what the device stores: saturated to int32, NaN -> INT32_MIN.  A gt lane
    the label does not have counts as all -2 (the device's rule; the reference raises IndexError)."""
    S = len(h_samples)
    out = np.full((nclasses, S), -2, np.int64)
    for j, p in enumerate(params):
        gt = gt_lanes[j] if j < len(gt_lanes) else [-2] * S
        keep = gate(h_samples, gt, j, line_id, horizon_est, 640 / resize, all_branches_ready, horizon_on)
        if keep is None:
            continue
        r = np.rint(scaled_x(p, h_samples, M, M_inv, no_ortho))
        with np.errstate(invalid="ignore"):
            if int32:
                v = np.where(np.isnan(r), INT32_MIN, np.clip(np.nan_to_num(r, nan=0.), INT32_MIN, INT32_MAX)).astype(np.int64)
            else:
                v = r.astype(np.int64)
        out[j] = np.where(keep, v, -2)
    return out


def tie_margin(params, gt_lanes, h_samples, line_id, horizon_est, M, M_inv, resize, all_branches_ready, horizon_on, no_ortho):
    """Smallest distance of an in-gate ``1279 x`` from a half-integer over the lanes of one label line (inf without one)."""
    worst = np.inf
    for j, p in enumerate(params):
        gt = gt_lanes[j] if j < len(gt_lanes) else [-2] * len(h_samples)
        keep = gate(h_samples, gt, j, line_id, horizon_est, 640 / resize, all_branches_ready, horizon_on)
        if keep is None or not keep.any():
            continue
        v = scaled_x(p, h_samples, M, M_inv, no_ortho)[keep]
        worst = min(worst, float(np.abs(v - np.floor(v) - 0.5).min()))
    return worst


def golden_line(golden, c):
    """Case c of tests/golden/bev_lanes.npz -> the label line ``write_lsq_results`` reads (lists, as JSON holds them)."""
    S, G = int(golden["S"][c]), int(golden["gt_count"][c])
    return dict(lanes=[[int(v) for v in golden["gt"][c, g, :S]] for g in range(G)], h_samples=[int(v) for v in golden["h_samples"][c, :S]],
                raw_file="clips/%d.jpg" % c,
                params=[[float(v) for v in golden["params"][c, j, 3 - n:]] for j, n in enumerate(golden["params_len"][c])],
                line_id=[int(v) for v in golden["line_id"][c]], horizon_est=[float(v) for v in golden["horizon"][c]])


def write_lsq_results(src_file, dst_file, nclasses, all_branches_ready, horizon_on, resize, no_ortho, M, M_inv):
    """File to file, as the reference's function of that name: every key kept, ``lanes`` replaced, ``run_time`` 20."""
    lines = [json.loads(line) for line in open(src_file).readlines()]
    with open(dst_file, "w") as f:
        for line in lines:
            lanes = decode(line["params"], line["lanes"], line["h_samples"], line["line_id"], line["horizon_est"], M, M_inv, nclasses,
                           resize, all_branches_ready, horizon_on, no_ortho)
            line["run_time"] = 20
            line["lanes"] = lanes.tolist()
            json.dump(line, f)
            f.write("\n")
