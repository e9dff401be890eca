#!/usr/bin/env python
"""Time of ``clip_grad_norm`` + ``optimizer.step()`` (BP/main.py:334-340) on the real BEV model at the headline geometry (batch 32,
256x512: 226 tensors with a gradient), three forms alternated in one process after one backward pass:

    A  torch.nn.utils.clip_grad_norm_(params, 1) + FusedAdam.step()      what --clip_grad_norm 1 cost before
    B  optim.clip_grad_norm_(params, 1)          + FusedAdam.step()      the drop-in form
    C  FusedAdam(max_grad_norm=1).step()                                  the clip inside the step

    python tools/clip_step_time.py [--steps 20] [--warmup 5] [--repeats 3] [--json FILE]       -> profiles/clip_step_time.json

Two figures per form and repeat, per call: the time between two in-stream HIP events around the timed calls, and the host's wall
time for issuing them (up to, not including, the synchronise): torch's routine walks every gradient on the host.  A and B rewrite
the gradients, so every series starts from a restored copy of the backward pass's gradients (outside the timed window).
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


def timed(fn, restore, steps, warmup):
    restore()
    for _ in range(warmup):
        fn()
    restore()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    host = time.perf_counter() - t0
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps, host * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--json", default=None, help="result file (default profiles/clip_step_time.json)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("clip_step_time needs the MI355X: there is nothing to time without it")
    import bench
    import synthetic_inputs as inputs
    from lanedetection_end2end_amd import optim
    B, R = a.batch, bench.WORKLOADS["bev"]["R"]
    model, crit = bench.build_model(B, seed=0, workload="bev")
    model.check_singular = False
    x = torch.from_numpy(inputs.images(B, R, 2 * R, seed=100)).cuda()
    gt = torch.from_numpy(inputs.bev_gt_params(B, seed=200)).cuda()
    out = model(x, True)
    (crit(out[0], gt[:, 0]) + crit(out[1], gt[:, 1])).backward()
    params = list(model.parameters())
    with_grad = [p for p in params if p.grad is not None]
    saved = [p.grad.clone() for p in with_grad]
    norm0 = float(torch.sqrt(sum((g.double() ** 2).sum() for g in saved)))

    def restore():
        for p, g in zip(with_grad, saved):
            p.grad.copy_(g)

    plain = optim.FusedAdam(params, lr=1e-4)
    clipped = optim.FusedAdam(params, lr=1e-4, max_grad_norm=1.0)

    def form_a():
        torch.nn.utils.clip_grad_norm_(params, 1.0)
        plain.step()

    def form_b():
        optim.clip_grad_norm_(params, 1.0)
        plain.step()

    def form_c():
        clipped.step()

    forms = (("A_torch_clip_then_step", form_a), ("B_drop_in_then_step", form_b), ("C_clip_inside_step", form_c))
    t = {name: {"event_ms": [], "host_ms": []} for name, _ in forms}
    for _ in range(a.repeats):
        for name, fn in forms:
            ev, host = timed(fn, restore, a.steps, a.warmup)
            t[name]["event_ms"].append(ev)
            t[name]["host_ms"].append(host)
    restore()
    clipped.step()
    res = {"steps": a.steps, "warmup": a.warmup, "repeats": a.repeats, "device": torch.cuda.get_device_name(0), "batch": B,
           "tensors_with_gradient": len(with_grad), "gradient_bytes": int(sum(g.numel() for g in saved) * 4),
           "gradient_norm_fp64": norm0, "norm_from_the_device": float(clipped.last_grad_norm), "forms": {}}
    for name, _ in forms:
        res["forms"][name] = {k: {"median": float(np.median(v)), "min": min(v), "max": max(v), "all": v} for k, v in t[name].items()}
    for k in ("event_ms", "host_ms"):
        widest = max(max(t[n][k]) - min(t[n][k]) for n, _ in forms)
        diff = res["forms"]["C_clip_inside_step"][k]["median"] - res["forms"]["A_torch_clip_then_step"][k]["median"]
        res[k + "_widest_range"] = widest
        res[k + "_C_minus_A"] = diff
        res[k + "_C_not_slower_than_A_beyond_range"] = bool(diff <= widest)
    for name, _ in forms:
        f = res["forms"][name]
        print("%-24s in-stream %7.3f ms [%.3f, %.3f]   host %7.3f ms [%.3f, %.3f]" % (
            name, f["event_ms"]["median"], f["event_ms"]["min"], f["event_ms"]["max"],
            f["host_ms"]["median"], f["host_ms"]["min"], f["host_ms"]["max"]))
    print(json.dumps(res))
    with open(a.json or os.path.join(ROOT, "profiles", "clip_step_time.json"), "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
