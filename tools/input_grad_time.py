#!/usr/bin/env python
"""What the input image's gradient costs: forward + backward of the real models with and without ``input.requires_grad_()``,
alternated in one process, and the added launch (``lf_stem_bwd_data``) on its own, at

    headline   BEV model, 32 x 3 x 256 x 512, fp32
    config3    BP model, 4 lanes, 64 x 3 x 320 x 640, bf16

    python tools/input_grad_time.py [--steps 10] [--warmup 3] [--repeats 5] [--json FILE]       -> profiles/input_grad_time.json

Step figures: the time between two in-stream HIP events around ``steps`` steps (forward, criterion, backward), per step; median and
min-max over the repeats; ``added`` = median(with) - median(without), to be read against the ranges.  Kernel figures: the same
events around ``kernel_calls`` back-to-back launches of the kernel through the C ABI on tensors of the geometry's size, and the
kernel's own bytes (gcat read + image read + gimg written) over that time.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def events_ms(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def summary(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "all": [float(t) for t in v]}


def run_config(name, workload, precision, a):
    import bench
    import synthetic_inputs as inputs
    from lanedetection_end2end_amd import _lib
    wl = bench.WORKLOADS[workload]
    B, R, K = wl["batch"], wl["R"], wl["K"]
    model, crit = bench.build_model(B, seed=0, workload=workload)
    model.net.precision = precision
    model.check_singular = False
    x = torch.from_numpy(inputs.images(B, R, 2 * R, seed=100)).cuda()
    if workload == "bev":
        gt = torch.from_numpy(inputs.bev_gt_params(B, seed=200)).cuda()
    else:
        from lanedetection_end2end_amd.bp.Loss_crit import backprojection_loss
        crit = backprojection_loss(model._bench_args)
        lanes_np, valid_np = inputs.bp_targets(B, K, 256, seed=300)
        lanes, valid = torch.from_numpy(lanes_np).cuda(), torch.from_numpy(valid_np).cuda()
        gt_line = torch.zeros(B, K)
    params = list(model.parameters())
    seen = {}

    def step(requires_grad):
        xi = x.detach().requires_grad_(requires_grad)
        if workload == "bev":
            out = model(xi, True)
            loss = crit(out[0], gt[:, 0]) + crit(out[1], gt[:, 1])
        else:
            out = model(xi, gt_line, True)
            loss = sum(crit(out[k], lanes[:, k], valid[:, k])[0] for k in range(K)) / K
        for p in params:
            p.grad = None
        loss.backward()
        seen[requires_grad] = xi.grad

    t = {False: [], True: []}
    for _ in range(a.repeats):
        for rg in (False, True):
            t[rg].append(events_ms(lambda: step(rg), a.steps, a.warmup))
    assert seen[False] is None and seen[True] is not None and bool(torch.isfinite(seen[True]).all())

    # the added launch on its own
    lib = _lib.load()
    H, W, s16 = R, 2 * R, int(precision == "bf16")
    # (four sets of tensors in rotation, 0.5 - 1 GB together: a launch finds none of its bytes in the 256 MB last-level cache)
    sets = []
    for _ in range(4):
        gcat = torch.randn(B, H // 2, W // 2, 16, device="cuda")
        sets.append((gcat.bfloat16() if s16 else gcat, x.clone(), torch.empty_like(x)))
    gcat = sets[0][0]
    w = model.net.encoder.initial_block.conv.weight.detach().contiguous()
    turn = [0]

    def kernel():
        g, xi, gimg = sets[turn[0] & 3]
        turn[0] += 1
        _lib.check(lib.lf_stem_bwd_data(ctypes.c_void_p(g.data_ptr()), _lib.ptr(xi), _lib.ptr(w), B, 3, H, W, s16, _lib.ptr(gimg),
                                        _lib.stream()), "lf_stem_bwd_data")
    tk = [events_ms(kernel, a.kernel_calls, 8) for _ in range(a.repeats)]
    nbytes = gcat.numel() * gcat.element_size() + 2 * x.numel() * 4
    res = {"workload": wl["desc"], "batch": B, "H": H, "W": W, "precision": precision,
           "step_ms_without_input_grad": summary(t[False]), "step_ms_with_input_grad": summary(t[True]),
           "added_ms_per_step": float(np.median(t[True]) - np.median(t[False])),
           "widest_step_range_ms": float(max(max(v) - min(v) for v in t.values())),
           "kernel_us": summary([1e3 * v for v in tk]), "kernel_bytes": int(nbytes),
           "kernel_TB_per_s": nbytes / (float(np.median(tk)) * 1e-3) / 1e12}
    print("%-9s step %8.3f ms [%.3f, %.3f] -> %8.3f ms [%.3f, %.3f] with input.grad (added %.3f ms); lf_stem_bwd_data %.1f us "
          "[%.1f, %.1f], %.1f MB: %.2f TB/s" % (
              name, res["step_ms_without_input_grad"]["median"], min(t[False]), max(t[False]), res["step_ms_with_input_grad"]["median"],
              min(t[True]), max(t[True]), res["added_ms_per_step"], res["kernel_us"]["median"], res["kernel_us"]["min"],
              res["kernel_us"]["max"], nbytes / 1e6, res["kernel_TB_per_s"]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--kernel-calls", type=int, default=200)
    ap.add_argument("--json", default=None, help="result file (default profiles/input_grad_time.json)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("input_grad_time needs the MI355X: there is nothing to time without it")
    res = {"steps": a.steps, "warmup": a.warmup, "repeats": a.repeats, "kernel_calls": a.kernel_calls,
           "device": torch.cuda.get_device_name(0), "configs": {}}
    for name, workload, precision in (("headline", "bev", "fp32"), ("config3", "bp", "bf16")):
        res["configs"][name] = run_config(name, workload, precision, a)
        torch.cuda.empty_cache()
    print(json.dumps(res))
    with open(a.json or os.path.join(ROOT, "profiles", "input_grad_time.json"), "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
