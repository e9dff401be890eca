"""Eval-mode forward throughput of the ERFNet backbone: the existing engine (lf_erfnet_forward, training = 0) against the inference
engine (lf_erfnet_infer), alternated in one process, under torch.no_grad(), timed with in-stream events.

    python tools/infer_bench.py [--warmup 5] [--iters 20] [--repeats 3] [--configs a,b,c]

Geometries: (a) BEV 2 lanes, 256 x 512, batch 32, fp32 (the headline); (b) the same in bf16; (c) config 3: BP 4 lanes,
320 x 640, batch 64, bf16.  Per geometry and engine: images/s (median over the repeats, each the mean of --iters timed calls after
--warmup untimed ones) and the rise of torch.cuda.max_memory_allocated() during one call.  Prints one JSON line.

    python tools/infer_bench.py --detect [--configs a,b,c,c_clas]

Image -> lane coefficients (+ line / horizon with the --clas heads) on the LSQ models, three ways alternated in one process with
the same protocol: (A) ``forward`` on the existing engine, (B) ``forward`` with the backbone's inference engine on and the heads as
they were (unfolded), (C) ``detect`` (lf_lane_infer + the BatchNorm-folded heads).  ``c_clas`` is config 3's model with
``--clas 1`` at 256 x 512: the heads are built for a (32, 64) encoder output, so they do not exist at 320 x 640.  With heads, their
own time (both heads on the encoder output, unfolded and folded) is reported too.

    python tools/infer_bench.py --detect --configs seg5,seg4,seg1 [--out profiles/seg_detect_time.json]

Segmentation-mode rows (``end_to_end=False``): ``detect`` with ``fused_seg_detect`` off (the three-step path: inference-engine
forward, lf_seg_maps, the fit -- bit for bit the code ``detect`` ran before the fused call existed, hence the baseline) and
``"always"`` (lf_lane_infer_seg at every batch size, the single image included), alternated in one process.  ``seg5`` is config 5's shard (16 x 512 x 1024, 2 lanes), ``seg4`` the headline
geometry with 4 lanes (32 x 256 x 512, BP tree), ``seg1`` one 512 x 1024 image (``seg_n2`` / ``seg_n4`` / ``seg_n8``: 2, 4, 8 of them).  Reported: images/s, the min-max range of the
repeats, the peak memory of one call.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CONFIGS = {
    "a": dict(name="bev_2lanes_256x512_b32_fp32", N=32, H=256, W=512, K=2, precision="fp32", tree="bev"),
    "b": dict(name="bev_2lanes_256x512_b32_bf16", N=32, H=256, W=512, K=2, precision="bf16", tree="bev"),
    "c": dict(name="bp_4lanes_320x640_b64_bf16", N=64, H=320, W=640, K=4, precision="bf16", tree="bp"),
}


def make_net(cfg):
    from oracle import erfnet_oracle
    if cfg["tree"] == "bev":
        from lanedetection_end2end_amd.bev.Networks.ERFNet import Net
    else:
        from lanedetection_end2end_amd.bp.Networks.ERFNet import Net
    net = Net(layers=18, in_channels=3, out_channels=cfg["K"])
    net.load_state_dict(erfnet_oracle.make_params(seed=3, out_channels=cfg["K"]))
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():           # non-trivial running statistics (the engines' cost does not depend on them)
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.copy_(torch.rand(m.num_features, generator=g) - 0.5)
                m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
    net = net.cuda().eval()
    net.precision = cfg["precision"]
    return net


def time_calls(net, x, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        net(x, True)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def peak_rise(net, x):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = net(x, True)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    del out
    return rise


def run(cfg, warmup, iters, repeats):
    from oracle import inputs
    net = make_net(cfg)
    x = torch.from_numpy(inputs.images(cfg["N"], cfg["H"], cfg["W"], seed=1)).cuda()
    ms = {False: [], True: []}
    mem = {}
    with torch.no_grad():
        for on in (False, True):
            net.inference_engine = on
            for _ in range(warmup):
                net(x, True)
            mem[on] = peak_rise(net, x)
        for _ in range(repeats):
            for on in (False, True):          # alternated: both engines see the same clocks and neighbours
                net.inference_engine = on
                for _ in range(warmup):
                    net(x, True)
                ms[on].append(time_calls(net, x, iters))
    res = {"config": cfg["name"]}
    for on, tag in ((False, "existing"), (True, "inference")):
        med = statistics.median(ms[on])
        res[tag] = {"ms_per_call": round(med, 4), "images_per_s": round(cfg["N"] * 1e3 / med, 1),
                    "ms_all": [round(v, 4) for v in ms[on]], "peak_rise_mb": round(mem[on] / 1e6, 1)}
    res["speedup"] = round(statistics.median(ms[False]) / statistics.median(ms[True]), 4)
    del net, x
    torch.cuda.empty_cache()
    return res


DETECT_CONFIGS = dict(CONFIGS)
DETECT_CONFIGS["c_clas"] = dict(name="bp_4lanes_256x512_b64_bf16_clas", N=64, H=256, W=512, K=4, precision="bf16", tree="bp", clas=True)


SEG_CONFIGS = {
    "seg5": dict(name="seg_bev_2lanes_512x1024_b16_fp32", N=16, H=512, W=1024, K=2, precision="fp32", tree="bev", seg=True),
    "seg4": dict(name="seg_bp_4lanes_256x512_b32_fp32", N=32, H=256, W=512, K=4, precision="fp32", tree="bp", seg=True),
    "seg1": dict(name="seg_bev_2lanes_512x1024_b1_fp32", N=1, H=512, W=1024, K=2, precision="fp32", tree="bev", seg=True),
}
for _n in (2, 4, 8):          # the batches between: seg_n2, seg_n4, seg_n8
    SEG_CONFIGS["seg_n%d" % _n] = dict(SEG_CONFIGS["seg1"], name="seg_bev_2lanes_512x1024_b%d_fp32" % _n, N=_n)
DETECT_CONFIGS.update(SEG_CONFIGS)


def make_model(cfg):
    from argparse import Namespace
    from oracle import clas_oracle, erfnet_oracle
    bp = cfg["tree"] == "bp"
    clas = bool(cfg.get("clas"))
    seg = bool(cfg.get("seg"))
    args = Namespace(batch_size=cfg["N"], nclasses=cfg["K"], resize=cfg["H"], end_to_end=not seg, mod="erfnet", layers=18, channels_in=3,
                     pretrained=False, pool=True, activation_layer="square", no_cuda=False, order=3 if bp else 2, reg_ls=0.0,
                     use_cholesky=bp, mask_percentage=0.2 if bp else 0.3, clas=clas, no_mapping=False, precision=cfg["precision"])
    if bp:
        from lanedetection_end2end_amd.bp.Networks.LSQ_layer import Net
    else:
        from lanedetection_end2end_amd.bev.Networks.LSQ_layer import Net
    model = Net(args)
    model.net.load_state_dict(erfnet_oracle.make_params(seed=3, out_channels=cfg["K"] + int(seg)))
    if clas:
        model.line_classification.load_state_dict(clas_oracle.make_clas_params("line", seed=11, tree=cfg["tree"]))
        model.horizon_estimation.load_state_dict(clas_oracle.make_clas_params("horizon", seed=12))
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.copy_(torch.rand(m.num_features, generator=g) - 0.5)
                m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
    return model.cuda().eval()


def timed(call, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        call()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def run_detect(cfg, warmup, iters, repeats):
    import lanedetection_end2end_amd as pkg
    from oracle import inputs
    model = make_model(cfg)
    x = torch.from_numpy(inputs.images(cfg["N"], cfg["H"], cfg["W"], seed=1)).cuda()
    gt_line = torch.zeros(cfg["N"], cfg["K"])
    fwd = (lambda: model(x, gt_line, True)) if cfg["tree"] == "bp" else (lambda: model(x, True))

    def way(tag):
        pkg.use_inference_engine(model, False)
        model.net.inference_engine = tag != "A"          # (B): the backbone's engine as merged, the heads unfolded
        return (lambda: model.detect(x)) if tag == "C" else fwd
    tags = ("A", "B", "C")
    ms, mem = {t: [] for t in tags}, {}
    with torch.no_grad():
        for t in tags:
            call = way(t)
            for _ in range(warmup):
                call()
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            out = call()
            torch.cuda.synchronize()
            mem[t] = torch.cuda.max_memory_allocated() - base
            del out
        for _ in range(repeats):
            for t in tags:                        # alternated: the three ways see the same clocks and neighbours
                call = way(t)
                for _ in range(warmup):
                    call()
                ms[t].append(timed(call, iters))
        res = {"config": cfg["name"]}
        names = {"A": "existing_forward", "B": "inference_forward", "C": "detect"}
        for t in tags:
            med = statistics.median(ms[t])
            res[names[t]] = {"ms_per_call": round(med, 4), "images_per_s": round(cfg["N"] * 1e3 / med, 1),
                             "ms_all": [round(v, 4) for v in ms[t]], "peak_rise_mb": round(mem[t] / 1e6, 1)}
        res["detect_over_inference_forward"] = round(statistics.median(ms["B"]) / statistics.median(ms["C"]), 4)
        if cfg.get("clas"):
            # the two heads alone on the encoder output, unfolded (as merged) and folded
            model.net.inference_engine = True
            enc = model.net(x, True)[0]
            hm = {False: [], True: []}
            for _ in range(repeats):
                for folded in (False, True):
                    call = lambda: (model.line_classification(enc, folded=folded), model.horizon_estimation(enc, folded=folded))
                    for _ in range(warmup):
                        call()
                    hm[folded].append(timed(call, iters))
            res["heads_ms"] = {"unfolded": round(statistics.median(hm[False]), 4), "folded": round(statistics.median(hm[True]), 4),
                               "unfolded_all": [round(v, 4) for v in hm[False]], "folded_all": [round(v, 4) for v in hm[True]]}
            del enc
    del model, x
    torch.cuda.empty_cache()
    return res


def run_detect_seg(cfg, warmup, iters, repeats):
    """detect of a segmentation-mode model: the three-step path against the fused call, alternated."""
    from oracle import inputs
    model = make_model(cfg)
    model.check_singular = False          # (random weights at a random image: the timing does not depend on the statuses)
    x = torch.from_numpy(inputs.images(cfg["N"], cfg["H"], cfg["W"], seed=1)).cuda()
    call = lambda: model.detect(x)
    tags = (False, "always")
    ms, mem, status = {t: [] for t in tags}, {}, {}
    for t in tags:
        model.fused_seg_detect = t
        for _ in range(warmup):
            out = call()
        status[t] = (model.last_status.clone(), [None if b is None else b.clone() for b in out[:4]])
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = call()
        torch.cuda.synchronize()
        mem[t] = torch.cuda.max_memory_allocated() - base
        del out
    same = torch.equal(status[False][0], status["always"][0]) and all(
        (u is None and v is None) or torch.equal(u.contiguous().view(torch.uint8), v.contiguous().view(torch.uint8)) for u, v in zip(status[False][1], status["always"][1]))
    for _ in range(repeats):
        for t in tags:                        # alternated: both paths see the same clocks and neighbours
            model.fused_seg_detect = t
            for _ in range(warmup):
                call()
            ms[t].append(timed(call, iters))
    res = {"config": cfg["name"], "same_bits": bool(same)}
    for t, tag in ((False, "three_step"), ("always", "fused")):
        med = statistics.median(ms[t])
        res[tag] = {"ms_per_call": round(med, 4), "images_per_s": round(cfg["N"] * 1e3 / med, 1),
                    "ms_min_max": [round(min(ms[t]), 4), round(max(ms[t]), 4)], "ms_all": [round(v, 4) for v in ms[t]],
                    "peak_rise_mb": round(mem[t] / 1e6, 1)}
    res["fused_over_three_step"] = round(statistics.median(ms[False]) / statistics.median(ms["always"]), 4)
    # slower only if the ranges of the repeats do not overlap
    res["fused_slower_beyond_range"] = bool(min(ms["always"]) > max(ms[False]))
    model.fused_seg_detect = True
    res["detect_default_takes"] = "fused" if cfg["N"] > 1 else "three_step"
    del model, x
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--configs", default="a,b,c")
    ap.add_argument("--detect", action="store_true", help="image -> lane coefficients: existing forward / inference forward / detect")
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    args = ap.parse_args()
    assert args.warmup >= 5 and args.iters >= 20, "at least 5 warm-up and 20 timed calls"
    if args.detect:
        cfgs = "a,b,c,c_clas" if args.configs == "a,b,c" else args.configs
        runs = [(run_detect_seg if DETECT_CONFIGS[c].get("seg") else run_detect)(DETECT_CONFIGS[c], args.warmup, args.iters, args.repeats)
                for c in cfgs.split(",")]
        out = {"tool": "infer_bench --detect", "device": torch.cuda.get_device_name(0), "warmup": args.warmup, "iters": args.iters,
               "repeats": args.repeats, "results": runs}
        if any(DETECT_CONFIGS[c].get("seg") for c in cfgs.split(",")):
            out["seg_baseline"] = ("three_step = detect with fused_seg_detect off: the inference-engine forward, lf_seg_maps and the "
                                   "fit of the same build, bit for bit the code detect ran before lf_lane_infer_seg existed")
        print(json.dumps(out))
        if args.out:
            with open(args.out, "w") as f:
                json.dump(out, f, indent=1)
                f.write("\n")
        return
    out = {"tool": "infer_bench", "device": torch.cuda.get_device_name(0), "warmup": args.warmup, "iters": args.iters,
           "repeats": args.repeats, "results": [run(CONFIGS[c], args.warmup, args.iters, args.repeats) for c in args.configs.split(",")]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
