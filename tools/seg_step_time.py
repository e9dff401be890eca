#!/usr/bin/env python
"""Time of what a segmentation-mode step does behind the backbone, as the statements stand and as one ``SegStepCriterion`` call,
with in-stream HIP events after warm-up, alternated in one process.

    python tools/seg_step_time.py [--steps 100] [--warmup 10] [--repeats 7] [--json FILE]      -> profiles/seg_step_time.json

Two shapes:
  config5   (16, 3, 512, 1024), fit=False: ``criterion_seg(output_net, gt)`` + ``loss.backward()`` against
            ``SegStepCriterion(..., fit=False)`` + ``loss.backward()`` (BASELINE config 5, the ``skip`` epochs);
  bp_fit    (32, 5, 256, 512), 4 lanes, order 2, BP tree: ``_seg_maps`` + ``fit_lanes`` + ``criterion_seg`` + ``loss.backward()`` + the
            per-lane criterion under ``no_grad`` (BP/main.py:306-318) against ``SegStepCriterion`` + ``loss.backward()``.
Logits are lane-like (a ridge per lane over a background plane), so the arg-max picks lanes where a trained head would.  Neither
side reads anything back to the host inside the timed window (``check_singular`` off; the label check stays deferred).
A third series times the three launches of ``lf_seg_step`` alone, through the C entry point: the two sides above include the host's
work per call (autograd nodes, the deferred label check), which at these sizes is longer than the kernels.  Its required bytes
(logits + target read once, gradient written once) over its time stand beside a device copy of the same bytes; the buffers are
reused from call to call, so both run as warm in the last-level cache as a loop over one batch can be.
"""
import argparse
import json
import os
import sys
from argparse import Namespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def case(name, N, C, R, with_fit):
    from lanedetection_end2end_amd import fit, losses
    from lanedetection_end2end_amd.bp.Networks.LSQ_layer import Net
    from oracle import inputs
    K = C - 1
    args = Namespace(batch_size=N, nclasses=K, resize=R, end_to_end=False, mod="erfnet", layers=18, channels_in=3, pretrained=False,
                     pool=True, activation_layer="square", no_cuda=False, order=2, reg_ls=0.0, use_cholesky=False,
                     mask_percentage=0.2, clas=False, no_mapping=False, loss_policy="backproject", weight_seg=30, weight_funct="none")
    model = Net(args).cuda()                   # (for its geometry; the timed statements start at the logits)
    model.check_singular = False
    H, W = R, 2 * R
    lanes_z = inputs.lane_like_logits(N, K, H, W, seed=1)
    z = torch.from_numpy(np.concatenate([np.full((N, 1, H, W), 0.3, np.float32), lanes_z.astype(np.float32)], 1)).cuda().requires_grad_(True)
    gt = torch.from_numpy(inputs.seg_targets(N, H, W, C, seed=2)).cuda()
    lanes, valid = (torch.from_numpy(a).cuda() for a in inputs.bp_targets(N, 4, R, seed=3))
    gt_line = torch.zeros(N, 4 if K > 3 else 2).cuda()
    criterion, criterion_seg = losses.define_loss_crit_bp(args)
    fused_crit = losses.SegStepCriterion(args, model).cuda()
    fused_crit.check_singular = False
    reg = 0.0

    def statements():
        z.grad = None
        if with_fit:
            maps = model._seg_maps(z, gt_line)
            beta, _, _ = fit.fit_lanes(maps, model.grid_on(z.device), model.zero_rows, model.order, reg, model.y_offset, "none",
                                       model.use_cholesky, False, False)
            betas = fit.split_lanes(beta, K, model.beta_dtype)
        loss = criterion_seg(z, gt)
        loss.backward()
        if with_fit:
            with torch.no_grad():
                ls = [criterion(betas[k], lanes[:, k], valid[:, k])[0] for k in range(len([b for b in betas if b is not None]))]
                return sum(ls) / K
        return loss

    def fused():
        z.grad = None
        res = fused_crit(z, gt, lanes, valid, gt_line, fit=with_fit)
        res.loss.backward()
        return res.metric if with_fit else res.loss

    nbytes = z.numel() * 4 * 2 + gt.numel() * 8            # logits and target read once, the gradient written once
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)

    def copy():
        dst.copy_(src)

    from lanedetection_end2end_amd import _lib
    lib = _lib.load()
    L = (4 if K > 3 else 2) if with_fit else 0
    zd = z.detach()
    grad, out = torch.empty_like(zd), torch.empty(4, dtype=torch.float64, device="cuda")
    beta = torch.empty(N, max(L, 1), 3, dtype=torch.float64, device="cuda")
    status = torch.empty(N * max(L, 1), dtype=torch.int32, device="cuda")
    ws = torch.zeros(lib.lf_seg_step_workspace_bytes(N, C, L, H, W, 2), dtype=torch.uint8, device="cuda")
    weights = fused_crit.weights
    grid = model.grid_on(z.device) if with_fit else None

    def launches():
        _lib.check(lib.lf_seg_step(_lib.ptr(zd), _lib.ptr(gt), _lib.ptr(weights), _lib.ptr(grid), 0, _lib.ptr(gt_line) if with_fit else None,
                                   N, C, L, H, W, model.zero_rows, 2, 0.0, float(model.y_offset), 0, _lib.ptr(grad), None,
                                   _lib.ptr(beta) if with_fit else None, _lib.ptr(status) if with_fit else None, _lib.ptr(out), None,
                                   _lib.ptr(ws), _lib.stream()), "lf_seg_step")
    return name, statements, fused, copy, launches, nbytes, dict(shape=[N, C, H, W], fit=bool(with_fit), lanes=(4 if K > 3 else 2) if with_fit else 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7, help="alternations of the two sides")
    ap.add_argument("--json", default=None, help="result file (default profiles/seg_step_time.json)")
    ap.add_argument("--small", action="store_true", help="quarter-size shapes (a rehearsal, not a measurement)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("seg_step_time needs the MI355X: there is nothing to time without it")
    res = {"steps": a.steps, "warmup": a.warmup, "repeats": a.repeats, "device": torch.cuda.get_device_name(0), "cases": {}}
    shapes = [("config5", 16, 3, 512, False), ("bp_fit", 32, 5, 256, True)]
    if a.small:
        shapes = [("config5", 4, 3, 128, False), ("bp_fit", 4, 5, 64, True)]
    for spec in shapes:
        name, statements, fused, copy, launches, nbytes, info = case(*spec)
        t = {"statements": [], "fused": [], "copy": [], "launches": []}
        for r in range(a.repeats):
            w = a.warmup if r == 0 else 2
            t["statements"].append(timed(statements, a.steps, w))
            t["fused"].append(timed(fused, a.steps, w))
            t["copy"].append(timed(copy, a.steps, w))
            t["launches"].append(timed(launches, a.steps, w))
        c = dict(info)
        for k, v in t.items():
            c[k + "_ms"] = {"median": float(np.median(v)), "min": min(v), "max": max(v), "all": v}
        saved = float(np.median(t["statements"]) - np.median(t["fused"]))
        spread = max(max(t[k]) - min(t[k]) for k in ("statements", "fused"))
        c["saved_ms"], c["widest_range_ms"], c["beyond_range"] = saved, spread, bool(saved > spread)
        c["required_bytes"] = nbytes
        c["launches_GB_per_s"] = nbytes / (np.median(t["launches"]) * 1e-3) / 1e9
        c["copy_GB_per_s"] = nbytes / (np.median(t["copy"]) * 1e-3) / 1e9
        res["cases"][name] = c
        print("%-8s statements %8.3f ms [%.3f, %.3f]   fused %8.3f ms [%.3f, %.3f]   saved %+.3f ms (widest range %.3f)   "
              "the three launches alone %.3f ms = %.0f GB/s of their required bytes, a copy of them %.0f GB/s" % (
                  name, c["statements_ms"]["median"], min(t["statements"]), max(t["statements"]), c["fused_ms"]["median"],
                  min(t["fused"]), max(t["fused"]), saved, spread, c["launches_ms"]["median"], c["launches_GB_per_s"], c["copy_GB_per_s"]))
    print(json.dumps(res))
    out = a.json or os.path.join(ROOT, "profiles", "seg_step_time.json")
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
