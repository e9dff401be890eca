#!/usr/bin/env python
"""Time the resident loader on an MI355X (report only, no gate).

    python tools/loader_time.py [--out profiles/loader_time.json]

1. The label statements of ONE batch, two legs alternated in one process, REPEATS times each:
   * host: what INTEGRATION.md prescribed before the loader -- per sample the numpy statements of ``__getitem__`` (the restatement
     tests/loader_ref.py: flips through ``mirror_list`` and the ``flip_params_bev`` / ``flip_lanes_bp`` arithmetic, the BP horizon
     from the lane heights, the validity mask), ``np.stack``, one host -> device copy per tensor.  The leg starts from the PARSED
     JSON LISTS of each sample, as the reference's ``__getitem__`` does, so it also pays the list -> array conversion a host
     loader that kept parsed arrays would not.  Host clock around the leg, ending in a device synchronise.
   * device: ``ResidentDataset.label_batch`` -- one launch.  In-stream event pair around CALLS launches (device time per launch)
     and a host clock around the same calls ending in a synchronise (what the host spends enqueueing one).
   BEV at batch 32, BP at batch 64 (the trees' bench configurations); labels are the golden family of tests/golden/loader.npz.
2. One epoch (3626 frames, batch 32, 113 steps) of the headline BEV training step (bench.py's epoch workload: pipeline -> Net ->
   area loss -> backward -> FusedAdam), three feeds alternated, EPOCH_REPEATS times each, a 128-frame pool indexed modulo:
   * plan: index batches and flips pre-uploaded, labels gathered by ``torch.where`` over a plain and a flipped pool, pixels of the
     image only (exactly what bench.py builds);
   * plan+gt: the same plus the label-map launches (``gt`` and ``horizon``), which every loader batch carries;
   * loader: ``for batch in ResidentLoader`` -- torch's samplers on the host, one upload per epoch, three launches per batch.
Every figure is reported with all of its repeats; the medians are quoted.
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
import loader_ref  # noqa: E402
from lanedetection_end2end_amd.loader import ResidentDataset, ResidentLoader  # noqa: E402

REPEATS, CALLS, EPOCH_REPEATS = 7, 200, 3
EPOCH_FRAMES, POOL, RESIZE = 3626, 128, 256


def golden_labels(tree, M):
    g = np.load(os.path.join(ROOT, "tests", "golden", "loader.npz"), allow_pickle=False)
    labs = [json.loads(str(s)) for s in g[tree + "_label_json"]]
    lines = [json.loads(str(s)) for s in g[tree + "_line_json"]]
    return [labs[i % len(labs)] for i in range(M)], [lines[i % len(lines)] for i in range(M)]


def spread(values):
    values = sorted(values)
    return dict(median=values[len(values) // 2], min=values[0], max=values[-1], all=values)


def label_legs(tree, batch):
    M = 256
    labs, lines = golden_labels(tree, M)
    frames = torch.zeros(M, 48, 64, 3, dtype=torch.uint8, device="cuda")
    maps = torch.ones(M, 48, 64, dtype=torch.uint8, device="cuda")
    kw = dict(lane_labels=labs) if tree == "bp" else dict(param_labels=labs)
    ds = ResidentDataset.from_arrays(tree, RESIZE, frames, maps, list(range(1, M + 1)), lines, nclasses=4, crop=32, **kw)
    rng = np.random.default_rng(1)
    rows = rng.integers(0, M, batch)
    flips = rng.uniform(size=batch) > 0.5
    sel, flip = torch.from_numpy(rows).cuda(), torch.from_numpy(flips).cuda()

    def host_leg():
        t = time.perf_counter()
        if tree == "bp":
            per = [loader_ref.bp_labels(labs[r], lines[r], f, RESIZE) for r, f in zip(rows, flips)]
        else:
            per = [loader_ref.bev_labels(labs[r], lines[r], f) for r, f in zip(rows, flips)]
        out = {k: torch.from_numpy(np.stack([p[k] for p in per])).cuda() for k in per[0]}
        out["idx"] = torch.from_numpy(rows).cuda()
        torch.cuda.synchronize()
        return time.perf_counter() - t, out

    def device_leg():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t = time.perf_counter()
        e0.record()
        for _ in range(CALLS):
            _, out = ds.label_batch(sel, flip)
        e1.record()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / CALLS, e0.elapsed_time(e1) * 1e-3 / CALLS, out

    host_leg(), device_leg()                                                 # warm-up
    host, dev_host, dev_stream = [], [], []
    for _ in range(REPEATS):                                                 # alternated
        h, want = host_leg()
        a, b, got = device_leg()
        host.append(h), dev_host.append(a), dev_stream.append(b)
    equal = all(torch.equal(got[k], want[k]) for k in want if k != "idx")
    res = dict(batch=batch, host_copies=len(want), host_label_statements_s=spread(host),
               device_label_launch_host_s=spread(dev_host), device_label_launch_stream_s=spread(dev_stream),
               device_equals_host=bool(equal))
    res["host_over_device_host_side"] = res["host_label_statements_s"]["median"] / res["device_label_launch_host_s"]["median"]
    return res


def epoch_legs():
    sys.path.insert(0, ROOT)
    import bench
    import synthetic_inputs as inputs
    from lanedetection_end2end_amd.optim import FusedAdam
    from lanedetection_end2end_amd.pipeline import InputPipeline, flip_params_bev
    B = 32
    model, crit = bench.build_model(B, seed=0, workload="bev")
    model.check_singular = False
    params = [p for p in model.parameters()]
    opt = FusedAdam(params, lr=1e-4)
    g = torch.Generator(device="cuda").manual_seed(1234)
    frames = torch.randint(0, 256, (POOL, 720, 1280, 3), dtype=torch.uint8, device="cuda", generator=g)
    maps = torch.randint(0, 5, (POOL, 720, 1280), dtype=torch.uint8, device="cuda", generator=g)
    gt_np = inputs.bev_gt_params(POOL, seed=77)
    gt_pool = torch.from_numpy(gt_np.astype(np.float32)).cuda()
    gt_pool_flipped = torch.from_numpy(np.stack([flip_params_bev(p) for p in gt_np]).astype(np.float32)).cuda()
    pipe = InputPipeline(RESIZE, tree="bev", nclasses=2)
    _, lines = golden_labels("bev", POOL)
    ds = ResidentDataset.from_arrays("bev", RESIZE, frames, maps, list(range(1, POOL + 1)), lines,
                                     param_labels=[dict(poly_params=p.tolist()) for p in gt_np])
    steps = EPOCH_FRAMES // B
    indices = [i % POOL for i in range(steps * B)]
    loader = ResidentLoader(ds, indices, B, True)
    rng = np.random.default_rng(900)

    def step(image, gt):
        b0, b1, _, _, _, _, _, _, _ = model(image, True)
        loss = crit(b0, gt[:, 0]) + crit(b1, gt[:, 1])
        for p in params:
            p.grad = None
        loss.backward()
        opt.step()
        return loss

    def plan_epoch(with_gt):
        torch.cuda.synchronize()
        t = time.perf_counter()
        idx = rng.permutation(steps * B).reshape(steps, B) % POOL
        flip = rng.uniform(size=idx.shape) > 0.5
        sel_e, flip_e = torch.from_numpy(idx).cuda(), torch.from_numpy(flip).cuda()
        for s in range(steps):
            sel, fl = sel_e[s], flip_e[s]
            gt = torch.where(fl[:, None, None], gt_pool_flipped.index_select(0, sel), gt_pool.index_select(0, sel))
            image, _, _ = pipe(frames, maps if with_gt else None, fl, index=sel)
            loss = step(image, gt)
        torch.cuda.synchronize()
        assert torch.isfinite(loss)
        return time.perf_counter() - t

    def loader_epoch():
        torch.cuda.synchronize()
        t = time.perf_counter()
        n = 0
        for image, gt_map, gt, idx, gt_line, horizon in loader:
            loss = step(image, gt)
            n += 1
        torch.cuda.synchronize()
        assert torch.isfinite(loss) and n == steps
        return time.perf_counter() - t

    def loader_host_only():
        """The host side of the loader alone: samplers, draws, the epoch upload -- batches taken, no step."""
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in loader:
            pass
        torch.cuda.synchronize()
        return time.perf_counter() - t

    for s in range(2):                                                       # warm-up: plans, tables, every shape
        sel = torch.arange(B, device="cuda")
        fl = torch.zeros(B, dtype=torch.bool, device="cuda")
        step(pipe(frames, maps, fl, index=sel)[0], gt_pool[:B])
        out = ds.batch(sel, fl)
        step(out[0], out[2])
    legs = dict(plan=[], plan_gt=[], loader=[], loader_batches_only=[])
    for _ in range(EPOCH_REPEATS):                                           # alternated
        legs["plan"].append(plan_epoch(False))
        legs["plan_gt"].append(plan_epoch(True))
        legs["loader"].append(loader_epoch())
        legs["loader_batches_only"].append(loader_host_only())
    ds.flush()
    res = dict(frames=steps * B, batch=B, steps=steps, pool=POOL)
    for k, v in legs.items():
        res[k + "_epoch_s"] = spread(v)
    for k in ("plan", "plan_gt", "loader"):
        res[k + "_images_per_s"] = steps * B / res[k + "_epoch_s"]["median"]
    res["loader_over_plan_gt"] = res["loader_epoch_s"]["median"] / res["plan_gt_epoch_s"]["median"]
    res["loader_over_plan"] = res["loader_epoch_s"]["median"] / res["plan_epoch_s"]["median"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loader_time.json"))
    ap.add_argument("--no-epoch", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/loader_time.py measures on the GPU; none is visible")
    res = dict(device=torch.cuda.get_device_name(0), repeats=REPEATS, calls_per_repeat=CALLS, epoch_repeats=EPOCH_REPEATS,
               labels_bev_batch32=label_legs("bev", 32), labels_bp_batch64=label_legs("bp", 64))
    if not a.no_epoch:
        res["epoch_bev"] = epoch_legs()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    assert res["labels_bev_batch32"]["device_equals_host"] and res["labels_bp_batch64"]["device_equals_host"]


if __name__ == "__main__":
    sys.exit(main())
