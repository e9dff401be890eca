#!/usr/bin/env python
"""Step time of config 3 (bench.py's "bp" workload in the bf16 precision mode: BP, 4 lanes, 320x640, batch 64) of this checkout
alternated with another built checkout of this repository (e.g. the parent commit), in the scheme of
tools/homography_step_time.py: the two packages share module names, so every run is a fresh child process, and the runs alternate
this, parent, this, parent, ...

    python tools/fast16_step_time.py --parent-root DIR [--rounds 3] [--steps 10] [--blocks 5] [--out profiles/fast16_oob_step_time.json]

Each block is `steps` steps between two synchronisations (ms per step).  Reported per checkout: all blocks of all runs, each run's
median block, the median and the spread (min, max) of the run medians;
not_above_parent_max (this median <= the parent's slowest run) and inside_parent_spread (between its fastest and slowest).
"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))


def run(root, steps, warmup, blocks):
    sys.path.insert(0, root)
    import torch
    import bench
    import synthetic_inputs as inputs
    from lanedetection_end2end_amd.bp.Loss_crit import backprojection_loss
    wl = bench.WORKLOADS["bp"]
    B, R, K = wl["batch"], wl["R"], wl["K"]
    model, _ = bench.build_model(B, seed=0, workload="bp")
    model.net.precision = "bf16"
    model.check_singular = False
    crit = backprojection_loss(model._bench_args)
    x = torch.from_numpy(inputs.images(B, R, 2 * R, seed=100)).cuda()
    lanes_np, valid_np = inputs.bp_targets(B, K, 256, seed=300)
    lanes, valid = torch.from_numpy(lanes_np).cuda(), torch.from_numpy(valid_np).cuda()
    gt_line = torch.zeros(B, K)
    params = list(model.parameters())

    statuses = []

    def step():
        out = model(x, gt_line, True)
        loss = sum(crit(out[k], lanes[:, k], valid[:, k])[0] for k in range(K)) / K
        for p in params:
            p.grad = None
        loss.backward()
        if model.last_status is not None:       # the fit's per-image status, as bench.py collects it
            statuses.append(model.last_status)
        return loss

    for _ in range(warmup):
        step()
    times = []
    for _ in range(blocks):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            loss = step()
        torch.cuda.synchronize()
        times.append(round((time.perf_counter() - t0) / steps * 1e3, 4))
        assert bool(torch.isfinite(loss))
        assert not statuses or int(torch.stack(statuses).abs().sum()) == 0, "singular normal matrix inside the timed region"
        statuses.clear()
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", required=True, help="another built checkout of this repository")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "fast16_oob_step_time.json"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(run(a.child, a.steps, a.warmup, a.blocks)))
        return
    import numpy as np
    roots = {"this": os.path.dirname(HERE), "parent": os.path.abspath(a.parent_root)}
    runs = {"this": [], "parent": []}
    for _ in range(a.rounds):
        for name in ("this", "parent"):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--parent-root", a.parent_root, "--child", roots[name],
                                  "--steps", str(a.steps), "--warmup", str(a.warmup), "--blocks", str(a.blocks)],
                                 capture_output=True, text=True, timeout=300)
            if out.returncode:
                raise SystemExit("the run of '%s' failed:\n%s" % (name, out.stderr[-2000:]))
            runs[name].append(json.loads([l for l in out.stdout.splitlines() if l.startswith("RESULT ")][-1][7:]))
            print(name, runs[name][-1], flush=True)
    res = dict(workload="bp", precision="bf16", steps=a.steps, blocks=a.blocks, rounds=a.rounds, order="this, parent, this, parent, ...")
    for name, rr in runs.items():
        med = [float(np.median(r)) for r in rr]
        res[name] = dict(blocks_ms=rr, run_median_ms=med, ms_per_step_median=float(np.median(med)), min_ms=min(med), max_ms=max(med))
    res["this_over_parent"] = res["this"]["ms_per_step_median"] / res["parent"]["ms_per_step_median"]
    res["not_above_parent_max"] = bool(res["this"]["ms_per_step_median"] <= res["parent"]["max_ms"])
    res["inside_parent_spread"] = bool(res["parent"]["min_ms"] <= res["this"]["ms_per_step_median"] <= res["parent"]["max_ms"])
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
