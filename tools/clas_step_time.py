#!/usr/bin/env python
"""Step time of the Backprojection_Loss/train.sh recipe (BP Net, --nclasses 4 --order 3 --clas 1) and of its two --clas heads,
in the fp32 and the bf16 precision modes, with in-stream HIP events after warm-up.

    python tools/clas_step_time.py [--batch 32] [--resize 256] [--steps 20] [--warmup 5] [--json FILE]
    python tools/clas_step_time.py --fused-criterion [--repeats 7]      -> profiles/step_criterion_time.json

recipe step = forward, backprojection loss over the four lanes + line / horizon BCE, backward and FusedAdam.step();
heads = line + horizon Classification forward + backward on an encoder-shaped input (N, 128, R/8, R/4) of the mode's dtype.
--fused-criterion: the same recipe step with the per-lane criterion statements (BP/main.py:296-326) and with the one call of
losses.StepCriterion, alternated in one process on one model; both times with their spread over the repeats.
"""
import argparse
import json
import os
import sys
from argparse import Namespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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


def recipe(precision, N, R, K, both=False):
    from lanedetection_end2end_amd.bp.Loss_crit import StepCriterion, backprojection_loss
    from lanedetection_end2end_amd.bp.Networks.LSQ_layer import Net
    from lanedetection_end2end_amd.optim import FusedAdam
    from oracle import inputs
    args = Namespace(batch_size=N, nclasses=K, resize=R, end_to_end=True, mod="erfnet", layers=18, channels_in=3, pretrained=False,
                     pool=True, activation_layer="square", no_cuda=False, order=3, reg_ls=0.0, use_cholesky=False,
                     mask_percentage=0.2, clas=True, no_mapping=False, loss_policy="backproject", weight_seg=30,
                     weight_funct="none", precision=precision)
    torch.manual_seed(0)
    model = Net(args).cuda().train()
    model.check_singular = False
    crit = backprojection_loss(args)
    bce = torch.nn.BCEWithLogitsLoss()
    x = torch.from_numpy(inputs.images(N, R, 2 * R, seed=1)).cuda()
    lanes, valid = inputs.bp_targets(N, K, R, seed=2)
    lt = [torch.from_numpy(lanes[:, k]).cuda() for k in range(K)]
    vt = [torch.from_numpy(valid[:, k]).cuda() for k in range(K)]
    rng = np.random.default_rng(3)
    gt_line = torch.from_numpy((rng.uniform(0, 1, (N, 4)) > 0.5).astype(np.float32)).cuda()
    gt_hor = torch.from_numpy((rng.uniform(0, 1, (N, R)) > 0.5).astype(np.float32)).cuda()
    params = list(model.parameters())
    opt = FusedAdam(params, lr=1e-4)
    gl = torch.zeros(N, K)

    def step():
        out = model(x, gl, True)
        loss = sum(crit(out[k], lt[k], vt[k])[0] for k in range(K)) / K
        loss = loss + (bce(out[6], gt_line) + bce(out[7], gt_hor)).double()
        for p in params:
            p.grad = None
        loss.backward()
        opt.step()
    if not both:
        return step
    fused_crit = StepCriterion(args, "bp")             # weight_fit = weight_class = 1, as the statements above

    def fused():
        out = model(x, gl, True)
        loss = fused_crit(out[:4], lanes_t, valid_t, out[6], out[7], gt_line, gt_hor).loss
        for p in params:
            p.grad = None
        loss.backward()
        opt.step()
    lanes_t, valid_t = torch.from_numpy(lanes).cuda(), torch.from_numpy(valid).cuda()
    return step, fused


def fused_criterion(a):
    """Per-lane and fused recipe steps alternated: median and spread (min, max) over the repeats, in ms."""
    N, R, K = a.batch, a.resize, 4
    res = {"batch": N, "geometry": [R, 2 * R], "lanes": K, "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats,
           "device": torch.cuda.get_device_name(0)}
    for precision in ("fp32", "bf16"):
        step, fused = recipe(precision, N, R, K, both=True)
        t = {"per_lane": [], "fused": []}
        for r in range(a.repeats):
            t["per_lane"].append(timed(step, a.steps, a.warmup if r == 0 else 2))
            t["fused"].append(timed(fused, a.steps, a.warmup if r == 0 else 2))
        for k, v in t.items():
            res["%s_step_ms_%s" % (k, precision)] = {"median": float(np.median(v)), "min": min(v), "max": max(v), "all": v}
        d = float(np.median(t["per_lane"]) - np.median(t["fused"]))
        spread = max(max(v) - min(v) for v in t.values())
        res["saved_ms_" + precision] = d
        res["beyond_spread_" + precision] = bool(d > spread)
        print("%-5s per-lane %8.3f ms [%.3f, %.3f]   fused %8.3f ms [%.3f, %.3f]   saved %+.3f ms (spread %.3f)" % (
            precision, np.median(t["per_lane"]), min(t["per_lane"]), max(t["per_lane"]), np.median(t["fused"]), min(t["fused"]),
            max(t["fused"]), d, spread))
    print(json.dumps(res))
    out = a.json or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "step_criterion_time.json")
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


def heads(precision, N, R):
    from lanedetection_end2end_amd.clas import Classification
    torch.manual_seed(0)
    ms = [Classification(t, size=(R // 8, R // 4), channels_in=128, resize=R).cuda().train() for t in ("line", "horizon")]
    dt = torch.bfloat16 if precision == "bf16" else torch.float32
    enc = torch.relu(torch.randn(N, R // 8, R // 4, 128, device="cuda")).to(dt).permute(0, 3, 1, 2).requires_grad_(True)
    gs = [torch.randn(N, 4, device="cuda"), torch.randn(N, R, device="cuda")]

    def step():
        for m in ms:
            for p in m.parameters():
                p.grad = None
        enc.grad = None
        ys = [m(enc) for m in ms]
        torch.autograd.backward(ys, gs)
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--resize", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None, help="also write the result object to this file")
    ap.add_argument("--fused-criterion", action="store_true",
                    help="time the recipe step with the per-lane criterion calls and with the one StepCriterion call")
    ap.add_argument("--repeats", type=int, default=7, help="--fused-criterion: alternations of the two steps")
    a = ap.parse_args()
    if a.fused_criterion:
        return fused_criterion(a)
    N, R, K = a.batch, a.resize, 4
    res = {"batch": N, "geometry": [R, 2 * R], "lanes": K, "steps": a.steps, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0)}
    for precision in ("fp32", "bf16"):
        res["recipe_step_ms_" + precision] = timed(recipe(precision, N, R, K), a.steps, a.warmup)
        res["heads_fwd_bwd_ms_" + precision] = timed(heads(precision, N, R), a.steps, a.warmup)
    for precision in ("fp32", "bf16"):
        res["heads_share_" + precision] = res["heads_fwd_bwd_ms_" + precision] / res["recipe_step_ms_" + precision]
    res["recipe_speedup_bf16"] = res["recipe_step_ms_fp32"] / res["recipe_step_ms_bf16"]
    for precision in ("fp32", "bf16"):
        print("%-5s recipe step %8.2f ms (%7.1f images/s)   heads fwd+bwd %7.2f ms (%4.1f %% of the step)" % (
            precision, res["recipe_step_ms_" + precision], N * 1e3 / res["recipe_step_ms_" + precision],
            res["heads_fwd_bwd_ms_" + precision], 100 * res["heads_share_" + precision]))
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
