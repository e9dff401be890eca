"""Latency of one call, image -> lane coefficients, at small batch: ``model.detect`` against the frozen detector.

    python tools/detector_latency.py [--out profiles/detector_latency.json] [--batches 1,2,4,8,32] [--configs bev,bp] [--precisions fp32,bf16]
    python tools/detector_latency.py --precisions bf16          (-> profiles/detector_latency_bf16_thin.json)

Three paths alternated in one process: (A) ``model.detect`` (the fold on every call), (B) ``model.detector(thin=False)`` (fold
once), (C) ``model.detector(thin=True)`` (fold once + the thin tap-GEMM route of the precision mode: tapgemm_thin_kernel in fp32,
tapgemm_bf16_thin_kernel in bf16).  Geometries: BEV 2 lanes 256 x 512 and BP 4 lanes order 3 320 x 640, each in fp32 and in
bf16.  Beside (C) the row records the thin launches of one call (``thin_launches_per_call``, the library's counter) and, where
there are any, ``thin_nt_derived``: the slabs per wave of the network's thin launches by output channel count, DERIVED in this
file from the launcher's rule at nt = 0 (lf_tapgemm_thin_pick_nt, csrc/lf_conv.hip), not read back from the launches.  A row
whose (C) took no thin launch ran (B)'s code: it carries no ``thin_wins``.  ``check_singular`` is off on every path (its status
read would synchronise every call).  Protocol: per repeat and path --warmup untimed calls, then --calls
back-to-back calls between two in-stream events and two host clock reads, the second behind one final synchronise; --repeats
repeats; reported: median and min-max of both times per call (ms).  Where the host issues slower than the device runs, the two
agree and the host is the limit.  ``thin_auto_max_batch``: the largest batch among 1, 2, 4, 8 at which (C)'s in-stream time is below
(B)'s beyond the min-max ranges of both, in every geometry measured (0: nowhere), per precision mode -- lsq.THIN_AUTO_MAX_BATCH
(fp32; the top-level key of a run that measured fp32) and lsq.THIN_AUTO_MAX_BATCH_BF16 (the top-level key of a bf16-only run);
``thin_auto_max_batch_by_precision`` has both.  A run of --precisions bf16 alone writes profiles/detector_latency_bf16_thin.json
and leaves the fp32 file as it is.

    python tools/detector_latency.py --lanes [--out profiles/detector_lanes_latency.json] [--precisions fp32,bf16] [--batches 1,2,4,8]

--lanes: one frame -> the lanes BP/test.py writes, on the BP tree's deployment recipe (4 lanes, order 3, --clas, 1 x 256 x 512).  Three
ways alternated in one process by the same protocol: (A) the detector with its --clas heads run as ``model.detect`` runs them (their
fold, upload and workspace on every call: ``frozen_heads = False``), then ``horizon_row`` / ``line_flags`` / ``decode_lanes`` as
``test_model`` issues them; (B) ``det(frame)`` with frozen heads, then the same hand-written tail; (C) ``det.lanes(frame)``.  (B) and
(C) are measured with the heads' trunks on the regular tiling and on the thin route (the backbone is thin="auto" in all five), which
decides lsq.THIN_AUTO_MAX_BATCH_HEADS / _BF16 by the rule above.  ``gain`` is stated only where the min-max ranges do not overlap.

    rocprofv3 --kernel-trace --stats -d DIR -o trace -- python tools/detector_latency.py --trace A|C|L
    python tools/detector_latency.py --launches DB_A DB_C [--out profiles/detector_launches.md]
    python tools/detector_latency.py --lanes-launches DB_L [--out profiles/detector_launches.md]      (appends the list of --trace L)

    python tools/detector_latency.py --frames [--out profiles/detector_frames_latency.json] [--precisions fp32,bf16] [--batches 1,2,4,8,32]

--frames: decoded uint8 720 x 1280 camera frames -> results, three ways alternated in one process by the same protocol: (A)
``InputPipeline`` + ``det(x)`` / ``det.lanes(x)`` (two Python calls, a fresh fp32 image per frame), (B) ``det.camera()`` with the
two-launch form inside the call (``fused=False``), (C) the camera with the fused resize + stem launch (``fused=True``,
frame_stem_kernel).  Geometries: -> 256 x 512 on the BP --clas recipe through ``lanes``, -> 320 x 640 on BP 4 lanes through
``__call__``.  ``fused_wins``: (C)'s in-stream time is below (B)'s beyond the min-max ranges of both.
``frame_stem_auto_max_batch_by_precision``: the largest batch up to which (C) won at every batch and in both geometries (0: nowhere)
-- lsq.FRAME_STEM_AUTO_MAX_BATCH / _BF16.

    python tools/detector_latency.py --frames --formats rgb,bgr,nv12,yuyv [--out profiles/detector_frames_formats_latency.json] [--yuv bt709]
    python tools/detector_latency.py --frames --formats rgb,nv12,nv12@decoder,nv12@pointers,i420,rgbx --batches 1 \
        --out profiles/detector_surfaces_latency.json      # surfaces: camera(layout=...), see SURFACE_SPECS

--frames --formats: ``det.camera(pixel_format=F).lanes(frames)`` on 720 x 1280 -> 256 x 512 (BP --clas) per frame format, the two-launch
and the fused form of each, all alternated in one process by the same protocol.  The yardstick is the ``rgb`` call of the same process
(``against_rgb``, stated only beyond both min-max ranges).  ``frame_stem_auto_max_batch_by_format``: per format and precision the
largest batch up to which its fused form beat its own two-launch form at every batch -- a format for which that is below what
lsq.FRAME_STEM_AUTO_MAX_BATCH / _BF16 route to needs a constant of its own beside them (none does: the comment there).

    rocprofv3 --kernel-trace --stats -d DIR -o trace -- python tools/detector_latency.py --trace F|G
    python tools/detector_latency.py --frames-launches DB_F DB_G [--out profiles/detector_launches.md]   (appends; F fused, G two launches)

The launch table: ten batch-1 calls at 1 x 256 x 512 fp32 of path (A) / (C) under the profiler (no counters), then per-kernel count
and duration of the two runs side by side from their rocpd databases.
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time
from argparse import Namespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CONFIGS = {
    "bev": dict(name="bev_2lanes_256x512", tree="bev", K=2, order=2, H=256, W=512, mask=0.3),
    "bp": dict(name="bp_4lanes_order3_320x640", tree="bp", K=4, order=3, H=320, W=640, mask=0.2),
}


def commit_stamp():
    """The commit the tree is at, as the other profiles carry it: .git_head (tools/stamp_head.sh; where there is no .git) or git."""
    try:
        return open(os.path.join(ROOT, ".git_head")).read().strip()
    except OSError:
        pass
    try:
        return subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=ROOT, text=True).strip()
    except Exception:
        return "unknown"


LANES_CFG = dict(name="bp_4lanes_order3_clas_256x512", tree="bp", K=4, order=3, H=256, W=512, mask=0.2)


def make_model(cfg, precision, N, clas=False):
    import torch
    from oracle import erfnet_oracle
    if cfg["tree"] == "bev":
        from lanedetection_end2end_amd.bev.Networks.LSQ_layer import Net
    else:
        from lanedetection_end2end_amd.bp.Networks.LSQ_layer import Net
    args = Namespace(batch_size=N, nclasses=cfg["K"], resize=cfg["H"], end_to_end=True, mod="erfnet", layers=18, channels_in=3,
                     pretrained=False, pool=True, activation_layer="square", no_cuda=False, order=cfg["order"], reg_ls=0.0,
                     use_cholesky=False, mask_percentage=cfg["mask"], clas=clas, no_mapping=False, loss_policy="backproject",
                     weight_seg=30, weight_funct="none", precision=precision)
    model = Net(args)
    model.net.load_state_dict(erfnet_oracle.make_params(seed=3, out_channels=cfg["K"]))
    if clas:
        from oracle import clas_oracle
        model.line_classification.load_state_dict(clas_oracle.make_clas_params("line", seed=11))
        model.horizon_estimation.load_state_dict(clas_oracle.make_clas_params("horizon", seed=12))
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():           # non-trivial running statistics (the cost does not depend on them)
        for m in model.net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.copy_(torch.rand(m.num_features, generator=g) - 0.5)
                m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
    model = model.cuda().eval()
    model.check_singular = False
    return model


def timed(fn, x, calls):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    for _ in range(calls):
        fn(x)
    b.record()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    return a.elapsed_time(b) / calls, (t1 - t0) * 1e3 / calls


def stats(v):
    return {"median": round(statistics.median(v), 5), "min": round(min(v), 5), "max": round(max(v), 5)}


def thin_launches(precision):
    """the launch counter of the precision mode's thin kernel"""
    from lanedetection_end2end_amd import _lib
    lib = _lib.load()
    return lib.lf_debug_thin_launches() if precision == "fp32" else lib.lf_debug_thin_bf16_launches()


def derived_nt(cfg, N):
    """slabs per wave of the network's thin launches by (stage pixels, output channels), DERIVED from the launcher's rule with no nt
    forced (lf_tapgemm_thin_pick_nt, csrc/lf_conv.hip: the largest of 4, 3, 2, 1 dividing Cd / 16 that still gives one 64-pixel
    workgroup per CU, else 1); which of these launches take the route at this batch is not derived"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    out = {}
    for name, div, cd in (("down_16_to_48", 4, 48), ("conv_64", 4, 64), ("down_64_to_64", 8, 64), ("conv_128", 8, 128), ("up_128_to_64_phase", 8, 64)):
        tiles = -(-(N * (cfg["H"] // div) * (cfg["W"] // div)) // 64)
        slabs = cd // 16
        out[name] = next((nt for nt in (4, 3, 2) if slabs % nt == 0 and tiles * (slabs // nt) >= cus), 1)
    return out


def measure(cfg, precision, N, warmup, calls, repeats):
    import torch
    from oracle import inputs
    model = make_model(cfg, precision, N)
    x = torch.from_numpy(inputs.images(N, cfg["H"], cfg["W"], seed=1)).cuda()
    paths = {"A_detect": model.detect, "B_detector": model.detector(batch=N, height=cfg["H"], width=cfg["W"], thin=False)}
    if precision in ("fp32", "bf16"):
        paths["C_detector_thin"] = model.detector(batch=N, height=cfg["H"], width=cfg["W"], thin=True)
    ref = model.detect(x)
    for name, fn in paths.items():      # the three paths give the same bits
        got = fn(x)
        assert all((u is None and v is None) or torch.equal(u, v) for u, v in zip(got, ref)), name
    ev = {k: [] for k in paths}
    wall = {k: [] for k in paths}
    for _ in range(repeats):
        for name, fn in paths.items():      # alternated: every path sees the same clocks and neighbours
            for _ in range(warmup):
                fn(x)
            e, w = timed(fn, x, calls)
            ev[name].append(e)
            wall[name].append(w)
    row = {"config": cfg["name"], "precision": precision, "batch": N}
    for name in paths:
        row[name] = {"in_stream_ms": stats(ev[name]), "wall_ms": stats(wall[name])}
    if "C_detector_thin" in paths:
        c0 = thin_launches(precision)
        paths["C_detector_thin"](x)
        row["thin_launches_per_call"] = thin_launches(precision) - c0
        if row["thin_launches_per_call"] > 0:      # (none: (C) ran (B)'s code, a difference is the order of the runs)
            row["thin_wins"] = row["C_detector_thin"]["in_stream_ms"]["max"] < row["B_detector"]["in_stream_ms"]["min"]
            row["thin_nt_derived"] = derived_nt(cfg, N)
    del model, paths, x
    torch.cuda.empty_cache()
    return row


def run(args):
    import torch
    rows = []
    for key in args.configs.split(","):
        for precision in args.precisions.split(","):
            for N in [int(b) for b in args.batches.split(",")]:
                rows.append(measure(CONFIGS[key], precision, N, args.warmup, args.calls, args.repeats))
                print(json.dumps(rows[-1]), flush=True)
    bounds = {}
    for precision in args.precisions.split(","):
        bounds[precision] = 0
        for N in (1, 2, 4, 8):
            at = [r for r in rows if r["precision"] == precision and r["batch"] == N]
            if at and all(r.get("thin_wins", False) for r in at):
                bounds[precision] = N
    bf16_only = args.precisions == "bf16"
    bound = bounds["bf16"] if bf16_only else bounds.get("fp32", 0)
    res = {"tool": "detector_latency", "commit": commit_stamp(), "device": torch.cuda.get_device_name(0), "warmup": args.warmup,
           "calls": args.calls, "repeats": args.repeats, "check_singular": False, "thin_auto_max_batch": bound,
           "thin_auto_max_batch_by_precision": bounds, "results": rows}
    default = "detector_latency_bf16_thin.json" if bf16_only else "detector_latency.json"
    with open(args.out or os.path.join(ROOT, "profiles", default), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"thin_auto_max_batch": bound, "by_precision": bounds}))


def lanes_paths(model, N):
    """The five ways of --lanes, each frame -> (N, 4, 56) int32 lanes."""
    import torch
    from lanedetection_end2end_amd import clas
    cfg = LANES_CFG
    proj = clas.Projections(Namespace(resize=cfg["H"], order=cfg["order"]))
    buf = torch.empty(N, cfg["K"], 56, dtype=torch.int32, device="cuda")

    def detector(frozen, heads_thin):
        det = model.detector(batch=N, height=cfg["H"], width=cfg["W"], thin="auto")
        det.frozen_heads = frozen
        det._head_flags = int(heads_thin)          # (tool only: the heads' LF_INFER_THIN apart from the backbone's)
        return det

    def hand_tail(det):
        def call(x):      # the tail of bp/test.py::test_model
            b0, b1, b2, b3, line, horizon = det(x)
            row = clas.horizon_row(horizon)
            flags = clas.line_flags(line)
            proj.decode_lanes([b0, b1, b2, b3], flags, row, out_int=buf)
            return buf
        return call

    def fused(det):
        return lambda x: det.lanes(x, out=buf).lanes
    return {"A_unfrozen_heads_hand_tail": hand_tail(detector(False, False)),
            "B_frozen_heads_hand_tail": hand_tail(detector(True, False)),
            "B_frozen_heads_thin_hand_tail": hand_tail(detector(True, True)),
            "C_lanes": fused(detector(True, False)),
            "C_lanes_heads_thin": fused(detector(True, True))}


def measure_lanes(precision, N, warmup, calls, repeats):
    import torch
    from oracle import inputs
    cfg = LANES_CFG
    model = make_model(cfg, precision, N, clas=True)
    x = torch.from_numpy(inputs.images(N, cfg["H"], cfg["W"], seed=1)).cuda()
    paths = lanes_paths(model, N)
    ref = paths["A_unfrozen_heads_hand_tail"](x).clone()
    for name, fn in paths.items():      # the five ways give the same lanes
        assert torch.equal(fn(x), ref), name
    ev = {k: [] for k in paths}
    wall = {k: [] for k in paths}
    for _ in range(repeats):
        for name, fn in paths.items():
            for _ in range(warmup):
                fn(x)
            e, w = timed(fn, x, calls)
            ev[name].append(e)
            wall[name].append(w)
    row = {"config": cfg["name"], "precision": precision, "batch": N}
    for name in paths:
        row[name] = {"in_stream_ms": stats(ev[name]), "wall_ms": stats(wall[name])}
    a = row["A_unfrozen_heads_hand_tail"]["in_stream_ms"]
    for name in paths:
        if name[0] != "A":      # a gain only where the min-max ranges do not overlap
            s = row[name]["in_stream_ms"]
            row[name]["against_A"] = ("gain" if s["max"] < a["min"] else "loss" if s["min"] > a["max"] else "ranges overlap")
            row[name]["median_ratio_to_A"] = round(s["median"] / a["median"], 4)
    row["heads_thin_wins"] = all(row[t]["in_stream_ms"]["max"] < row[r]["in_stream_ms"]["min"] for r, t in
                                 (("B_frozen_heads_hand_tail", "B_frozen_heads_thin_hand_tail"), ("C_lanes", "C_lanes_heads_thin")))
    del model, paths, x
    torch.cuda.empty_cache()
    return row


def run_lanes(args):
    import torch
    rows = []
    precisions = args.precisions.split(",")
    batches = [int(b) for b in args.batches.split(",") if int(b) <= 8]
    for precision in precisions:
        for N in batches:
            rows.append(measure_lanes(precision, N, args.warmup, args.calls, args.repeats))
            print(json.dumps(rows[-1]), flush=True)
    bounds = {}
    for precision in precisions:      # the rule of thin_auto_max_batch: the largest batch up to which the thin route won at every batch
        bounds[precision] = 0
        for N in (1, 2, 4, 8):
            at = [r for r in rows if r["precision"] == precision and r["batch"] == N]
            if not at or not all(r["heads_thin_wins"] for r in at):
                break
            bounds[precision] = N
    res = {"tool": "detector_latency --lanes", "commit": commit_stamp(), "device": torch.cuda.get_device_name(0), "warmup": args.warmup,
           "calls": args.calls, "repeats": args.repeats, "check_singular": False, "heads_thin_auto_max_batch_by_precision": bounds,
           "results": rows}
    with open(args.out or os.path.join(ROOT, "profiles", "detector_lanes_latency.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"heads_thin_auto_max_batch_by_precision": bounds}))


FRAMES_HW, FRAMES_CROP = (720, 1280), 640


def camera_frames(N):
    import numpy as np
    import torch
    from oracle import pipeline_oracle
    return torch.from_numpy(np.stack([pipeline_oracle.synthetic_frame(3 + n)[0] for n in range(min(N, 4))])[[n % 4 for n in range(N)]]).cuda()


def measure_frames(cfg, through_lanes, precision, N, warmup, calls, repeats):
    import torch
    from lanedetection_end2end_amd.pipeline import InputPipeline
    model = make_model(cfg, precision, N, clas=through_lanes)
    f = camera_frames(N)
    det = model.detector(batch=N, height=cfg["H"], width=cfg["W"], thin="auto")
    pipe = InputPipeline(cfg["H"], "bp", frame_hw=FRAMES_HW, crop=FRAMES_CROP)
    cams = {False: det.camera(FRAMES_HW, FRAMES_CROP, fused=False), True: det.camera(FRAMES_HW, FRAMES_CROP, fused=True)}
    if through_lanes:
        buf = torch.empty(N, cfg["K"], 56, dtype=torch.int32, device="cuda")
        paths = {"A_pipeline_then_detector": lambda u: det.lanes(pipe(u)[0], out=buf).lanes,
                 "B_camera_two_launches": lambda u: cams[False].lanes(u, out=buf).lanes,
                 "C_camera_fused": lambda u: cams[True].lanes(u, out=buf).lanes}
    else:
        paths = {"A_pipeline_then_detector": lambda u: det(pipe(u)[0])[3],
                 "B_camera_two_launches": lambda u: cams[False](u)[3],
                 "C_camera_fused": lambda u: cams[True](u)[3]}
    ref = paths["A_pipeline_then_detector"](f).clone()
    for name, fn in paths.items():      # the three ways give the same bits
        assert torch.equal(fn(f), ref), name
    ev = {k: [] for k in paths}
    wall = {k: [] for k in paths}
    for _ in range(repeats):
        for name, fn in paths.items():
            for _ in range(warmup):
                fn(f)
            e, w = timed(fn, f, calls)
            ev[name].append(e)
            wall[name].append(w)
    row = {"config": cfg["name"], "through": "lanes" if through_lanes else "__call__", "frames": "%dx%d crop %d" % (FRAMES_HW + (FRAMES_CROP,)),
           "precision": precision, "batch": N}
    for name in paths:
        row[name] = {"in_stream_ms": stats(ev[name]), "wall_ms": stats(wall[name])}
    b, c = row["B_camera_two_launches"]["in_stream_ms"], row["C_camera_fused"]["in_stream_ms"]
    row["fused_wins"] = c["max"] < b["min"]
    row["fused_against_two_launches"] = "gain" if c["max"] < b["min"] else "loss" if c["min"] > b["max"] else "ranges overlap"
    row["median_ratio_C_to_B"] = round(c["median"] / b["median"], 4)
    row["median_ratio_B_to_A"] = round(b["median"] / row["A_pipeline_then_detector"]["in_stream_ms"]["median"], 4)
    del model, det, cams, paths, f
    torch.cuda.empty_cache()
    return row


def run_frames(args):
    import torch
    rows = []
    precisions = args.precisions.split(",")
    batches = [int(b) for b in args.batches.split(",")]
    for cfg, through_lanes in ((LANES_CFG, True), (CONFIGS["bp"], False)):
        for precision in precisions:
            for N in batches:
                rows.append(measure_frames(cfg, through_lanes, precision, N, args.warmup, args.calls, args.repeats))
                print(json.dumps(rows[-1]), flush=True)
    bounds = {}
    for precision in precisions:      # the largest batch up to which the fused launch won at every batch, in both geometries
        bounds[precision] = 0
        for N in sorted(set(batches)):
            at = [r for r in rows if r["precision"] == precision and r["batch"] == N]
            if not at or not all(r["fused_wins"] for r in at):
                break
            bounds[precision] = N
    res = {"tool": "detector_latency --frames", "commit": commit_stamp(), "device": torch.cuda.get_device_name(0), "warmup": args.warmup,
           "calls": args.calls, "repeats": args.repeats, "check_singular": False, "frame_stem_auto_max_batch_by_precision": bounds,
           "results": rows}
    with open(args.out or os.path.join(ROOT, "profiles", "detector_frames_latency.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"frame_stem_auto_max_batch_by_precision": bounds}))


def format_frames(rgb, fmt):
    """(N, H, W, 3) uint8 RGB frames re-read as frames in format fmt: the planes of the picture stand in for B G R / Y Cb Cr (the
    cost does not depend on the values; the chroma planes are sub-sampled by dropping, as the layout demands)"""
    import numpy as np
    N, H, W, _ = rgb.shape
    if fmt in ("rgb", "bgr"):
        return np.ascontiguousarray(rgb)
    if fmt == "nv12":
        return np.ascontiguousarray(np.concatenate([rgb[..., 1], rgb[:, ::2, ::2][..., [2, 0]].reshape(N, H // 2, W)], axis=1))
    return np.ascontiguousarray(np.stack([rgb[..., 1], np.where(np.arange(W) % 2 == 0, rgb[..., 2], rgb[..., 0])], axis=-1))


# --formats also takes surfaces (camera(layout=...)): a decoder's NV12 with pitch 1536 and the chroma plane behind 736 rows, the same
# through a pointer table with Y and CbCr in separate allocations, and the formats that exist only with a layout
SURFACE_SPECS = ("nv12@decoder", "nv12@pointers", "i420", "rgbx", "bgrx")
DECODER_PITCH, DECODER_ROWS = 1536, 736


def surface_case(det, spec, rgb, yuv):
    """({fused: camera}, their frames argument, the bytes of one frame's pixels and padding) for a surface spec: both cameras share
    the layout, so one bound table serves them"""
    import numpy as np
    import torch
    from lanedetection_end2end_amd.pipeline import FrameLayout
    N, H, W, _ = rgb.shape
    if spec.startswith("nv12@"):
        pointers = spec == "nv12@pointers"
        lay = FrameLayout("nv12", (H, W), pitch=(DECODER_PITCH, DECODER_PITCH), plane_offsets=None if pointers else (0, DECODER_ROWS * DECODER_PITCH),
                          plane_pointers=pointers)
        tight = format_frames(rgb, "nv12")
        y = np.zeros((N, DECODER_ROWS, DECODER_PITCH), np.uint8)
        c = np.zeros((N, H // 2, DECODER_PITCH), np.uint8)
        y[:, :H, :W], c[:, :, :W] = tight[:, :H], tight[:, H:]
        cams = {fused: det.camera((H, W), FRAMES_CROP, fused=fused, layout=lay, yuv=yuv) for fused in (False, True)}
        if pointers:      # Y and CbCr of every frame in allocations of their own
            arg = cams[True].bind([(torch.from_numpy(y[n]).cuda(), torch.from_numpy(c[n]).cuda()) for n in range(N)])
        else:
            arg = torch.from_numpy(np.concatenate([y, c], axis=1)).cuda()
        return cams, arg, lay.frame_stride
    if spec == "i420":
        planes = [rgb[..., 1].reshape(N, -1), rgb[:, ::2, ::2, 2].reshape(N, -1), rgb[:, ::2, ::2, 0].reshape(N, -1)]
        tight = np.ascontiguousarray(np.concatenate(planes, axis=1))
    else:
        tight = np.ascontiguousarray(np.concatenate([rgb if spec == "rgbx" else rgb[..., ::-1], np.full((N, H, W, 1), 255, np.uint8)], axis=-1))
    lay = FrameLayout(spec, (H, W))
    cams = {fused: det.camera((H, W), FRAMES_CROP, fused=fused, layout=lay, yuv=yuv) for fused in (False, True)}
    return cams, torch.from_numpy(tight).cuda(), lay.frame_stride


def measure_formats(precision, N, formats, yuv, warmup, calls, repeats):
    """--frames --formats: cam.lanes(frames) per frame format or surface, two-launch and fused, all alternated in one process"""
    import torch
    cfg = LANES_CFG
    model = make_model(cfg, precision, N, clas=True)
    det = model.detector(batch=N, height=cfg["H"], width=cfg["W"], thin="auto")
    rgb = camera_frames(N).cpu().numpy()
    buf = torch.empty(N, cfg["K"], 56, dtype=torch.int32, device="cuda")
    paths, frames, nbytes = {}, {}, {}
    for fmt in formats:
        if fmt not in SURFACE_SPECS:
            frames[fmt] = torch.from_numpy(format_frames(rgb, fmt)).cuda()
            nbytes[fmt] = int(frames[fmt][0].numel())
        else:
            cams, frames[fmt], nbytes[fmt] = surface_case(det, fmt, rgb, yuv)
        for fused in (False, True):
            cam = cams[fused] if fmt in SURFACE_SPECS else det.camera(FRAMES_HW, FRAMES_CROP, fused=fused, pixel_format=fmt, yuv=yuv)
            paths[(fmt, fused)] = (lambda c: lambda u: c.lanes(u, out=buf).lanes)(cam)
        # the two forms of a format give the same bits (that they are the bits of the rgb call on the converted frames is the tests')
        assert torch.equal(paths[(fmt, True)](frames[fmt]).clone(), paths[(fmt, False)](frames[fmt])), fmt
    ev = {k: [] for k in paths}
    wall = {k: [] for k in paths}
    for _ in range(repeats):
        for key, fn in paths.items():
            for _ in range(warmup):
                fn(frames[key[0]])
            e, w = timed(fn, frames[key[0]], calls)
            ev[key].append(e)
            wall[key].append(w)
    row = {"config": cfg["name"], "through": "lanes", "frames": "%dx%d crop %d" % (FRAMES_HW + (FRAMES_CROP,)), "yuv": yuv,
           "precision": precision, "batch": N, "formats": {}}
    for fmt in formats:
        b, c = stats(ev[(fmt, False)]), stats(ev[(fmt, True)])
        r = {"frame_bytes": nbytes[fmt],
             "two_launches": {"in_stream_ms": b, "wall_ms": stats(wall[(fmt, False)])},
             "fused": {"in_stream_ms": c, "wall_ms": stats(wall[(fmt, True)])},
             "fused_wins": c["max"] < b["min"],
             "fused_against_two_launches": "gain" if c["max"] < b["min"] else "loss" if c["min"] > b["max"] else "ranges overlap",
             "median_ratio_fused_to_two_launches": round(c["median"] / b["median"], 4)}
        row["formats"][fmt] = r
    for fmt in formats:       # surfaces that move NV12's bytes are held against the tight nv12 call of the same process
        if (fmt.startswith("nv12@") or fmt == "i420") and "nv12" in formats:
            for form in ("two_launches", "fused"):
                s, y = row["formats"][fmt][form]["in_stream_ms"], row["formats"]["nv12"][form]["in_stream_ms"]
                row["formats"][fmt][form]["against_nv12"] = ("inside nv12's range" if y["min"] <= s["median"] <= y["max"] else
                                                             "faster" if s["max"] < y["min"] else "slower" if s["min"] > y["max"] else "ranges overlap")
                row["formats"][fmt][form]["median_ratio_to_nv12"] = round(s["median"] / y["median"], 4)
    if "rgb" in formats:      # the yardstick: the rgb call of the same process
        for fmt in formats:
            for form in ("two_launches", "fused"):
                s, y = row["formats"][fmt][form]["in_stream_ms"], row["formats"]["rgb"][form]["in_stream_ms"]
                row["formats"][fmt][form]["against_rgb"] = "faster" if s["max"] < y["min"] else "slower" if s["min"] > y["max"] else "ranges overlap"
                row["formats"][fmt][form]["median_ratio_to_rgb"] = round(s["median"] / y["median"], 4)
    del model, det, paths, frames
    torch.cuda.empty_cache()
    return row


def run_formats(args):
    import torch
    formats = args.formats.split(",")
    precisions = args.precisions.split(",")
    batches = [int(b) for b in args.batches.split(",")]
    rows = []
    for precision in precisions:
        for N in batches:
            rows.append(measure_formats(precision, N, formats, args.yuv, args.warmup, args.calls, args.repeats))
            print(json.dumps(rows[-1]), flush=True)
    bounds = {}
    for fmt in formats:       # per format: the largest batch up to which its fused form beat its own two-launch form at every batch
        bounds[fmt] = {}
        for precision in precisions:
            bounds[fmt][precision] = 0
            for N in sorted(set(batches)):
                at = [r for r in rows if r["precision"] == precision and r["batch"] == N]
                if not at or not all(r["formats"][fmt]["fused_wins"] for r in at):
                    break
                bounds[fmt][precision] = N
    res = {"tool": "detector_latency --frames --formats", "commit": commit_stamp(), "device": torch.cuda.get_device_name(0),
           "warmup": args.warmup, "calls": args.calls, "repeats": args.repeats, "check_singular": False,
           "frame_stem_auto_max_batch_by_format": bounds, "results": rows}
    with open(args.out or os.path.join(ROOT, "profiles", "detector_frames_formats_latency.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"frame_stem_auto_max_batch_by_format": bounds}))


def trace_frames(fused):
    """ten batch-1 cam.lanes(frame) calls, 720 x 1280 -> 256 x 512 fp32, --clas (run under rocprofv3 --kernel-trace --stats)"""
    import torch
    cfg = LANES_CFG
    model = make_model(cfg, "fp32", 1, clas=True)
    cam = model.detector(thin=True).camera(FRAMES_HW, FRAMES_CROP, fused=fused)
    f = camera_frames(1)
    for _ in range(10):
        cam.lanes(f)
    torch.cuda.synchronize()


def frames_launches(db_f, db_g, out):
    """append the kernels of --trace F (fused) and --trace G (two launches) side by side to the launch table"""
    import sqlite3

    def table(path):
        cur = sqlite3.connect(path).cursor()
        cols = [r[1] for r in cur.execute("pragma table_info(kernels)")]
        name_col = "name" if "name" in cols else [c for c in cols if "name" in c][0]
        agg = {}
        for n, s, e in cur.execute("select %s, start, end from kernels" % name_col).fetchall():
            k = re.sub(r"\(.*$", "", re.sub(r"\(anonymous namespace\)::", "", n)).replace("void ", "")[:80]
            a = agg.setdefault(k, [0, 0])
            a[0] += 1
            a[1] += e - s
        return agg
    tf, tg = table(db_f), table(db_g)
    lines = ["", "# Launches of ten `det.camera().lanes(frame_u8)` calls, 1 x 720 x 1280 x 3 uint8 -> 256 x 512, fp32, BP 4 lanes order 3 --clas", "",
             "commit: `%s`" % commit_stamp(), "",
             "`rocprofv3 --kernel-trace --stats` (no counters) of one process each: the model's set-up and the folds, then ten calls with",
             "(F) `fused=True` (frame_stem_kernel) / (G) `fused=False` (resize_bilinear_kernel + stem_fwd_kernel inside the call).",
             "Per kernel: launches and summed duration (us) over the whole process, sorted by time.", "",
             "| kernel | (F) launches | (F) us | (G) launches | (G) us |", "|---|---:|---:|---:|---:|"]
    for k in sorted(set(tf) | set(tg), key=lambda k: -(tf.get(k, [0, 0])[1] + tg.get(k, [0, 0])[1])):
        a, c = tf.get(k, [0, 0]), tg.get(k, [0, 0])
        lines.append("| `%s` | %d | %.1f | %d | %.1f |" % (k, a[0], a[1] / 1e3, c[0], c[1] / 1e3))
    lines += ["", "total: (F) %d launches, %.1f us; (G) %d launches, %.1f us" %
              (sum(v[0] for v in tf.values()), sum(v[1] for v in tf.values()) / 1e3,
               sum(v[0] for v in tg.values()), sum(v[1] for v in tg.values()) / 1e3), ""]
    with open(out or os.path.join(ROOT, "profiles", "detector_launches.md"), "a") as f:
        f.write("\n".join(lines))


def trace_lanes():
    """ten batch-1 det.lanes(frame) calls at 1 x 256 x 512 fp32, --clas (run under rocprofv3 --kernel-trace --stats)"""
    import torch
    from oracle import inputs
    cfg = LANES_CFG
    model = make_model(cfg, "fp32", 1, clas=True)
    x = torch.from_numpy(inputs.images(1, cfg["H"], cfg["W"], seed=1)).cuda()
    det = model.detector(thin=True)
    for _ in range(10):
        det.lanes(x)
    torch.cuda.synchronize()


def lanes_launches(db, out):
    """append the kernels of --trace L to the launch table"""
    import sqlite3
    cur = sqlite3.connect(db).cursor()
    cols = [r[1] for r in cur.execute("pragma table_info(kernels)")]
    name_col = "name" if "name" in cols else [c for c in cols if "name" in c][0]
    agg = {}
    for n, s, e in cur.execute("select %s, start, end from kernels" % name_col).fetchall():
        k = re.sub(r"\(.*$", "", re.sub(r"\(anonymous namespace\)::", "", n)).replace("void ", "")[:80]
        a = agg.setdefault(k, [0, 0])
        a[0] += 1
        a[1] += e - s
    lines = ["", "# Launches of ten `det.lanes(frame)` calls, 1 x 3 x 256 x 512, fp32, BP 4 lanes order 3 --clas", "",
             "commit: `%s`" % commit_stamp(), "",
             "`rocprofv3 --kernel-trace --stats` (no counters) of one process: the model's set-up and the detector's three folds, then ten",
             "calls of `model.detector(thin=True).lanes(frame)`.  Per kernel: launches and summed duration (us) over the whole process.", "",
             "| kernel | launches | us |", "|---|---:|---:|"]
    for k in sorted(agg, key=lambda k: -agg[k][1]):
        lines.append("| `%s` | %d | %.1f |" % (k, agg[k][0], agg[k][1] / 1e3))
    lines += ["", "total: %d launches, %.1f us" % (sum(v[0] for v in agg.values()), sum(v[1] for v in agg.values()) / 1e3), ""]
    with open(out or os.path.join(ROOT, "profiles", "detector_launches.md"), "a") as f:
        f.write("\n".join(lines))


def trace(path):
    """ten batch-1 calls of one path at 1 x 256 x 512 fp32 (run under rocprofv3 --kernel-trace --stats)"""
    import torch
    from oracle import inputs
    if path == "L":
        return trace_lanes()
    if path in ("F", "G"):
        return trace_frames(path == "F")
    cfg = CONFIGS["bev"]
    model = make_model(cfg, "fp32", 1)
    x = torch.from_numpy(inputs.images(1, cfg["H"], cfg["W"], seed=1)).cuda()
    fn = model.detect if path == "A" else model.detector(thin=True)
    for _ in range(10):
        fn(x)
    torch.cuda.synchronize()


def launches(db_a, db_c, out):
    import sqlite3

    def table(path):
        cur = sqlite3.connect(path).cursor()
        cols = [r[1] for r in cur.execute("pragma table_info(kernels)")]
        name_col = "name" if "name" in cols else [c for c in cols if "name" in c][0]
        agg = {}
        for n, s, e in cur.execute("select %s, start, end from kernels" % name_col).fetchall():
            k = re.sub(r"\(.*$", "", re.sub(r"\(anonymous namespace\)::", "", n)).replace("void ", "")[:80]
            a = agg.setdefault(k, [0, 0])
            a[0] += 1
            a[1] += e - s
        return agg
    ta, tc = table(db_a), table(db_c)
    lines = ["# Launches of ten single-frame calls, 1 x 3 x 256 x 512, fp32", "",
             "commit: `%s`" % commit_stamp(), "",
             "`rocprofv3 --kernel-trace --stats` (no counters) of one process each: the model's set-up, then ten calls of (A) `model.detect`",
             "/ (C) `model.detector(thin=True)`; the first call carries first-launch costs.  Per kernel: launches and summed duration (us)",
             "over the whole process (torch's set-up kernels included), sorted by (A)'s time.", "",
             "| kernel | (A) launches | (A) us | (C) launches | (C) us |", "|---|---:|---:|---:|---:|"]
    for k in sorted(set(ta) | set(tc), key=lambda k: -(ta.get(k, [0, 0])[1] + tc.get(k, [0, 0])[1])):
        a, c = ta.get(k, [0, 0]), tc.get(k, [0, 0])
        lines.append("| `%s` | %d | %.1f | %d | %.1f |" % (k, a[0], a[1] / 1e3, c[0], c[1] / 1e3))
    lines += ["", "total: (A) %d launches, %.1f us; (C) %d launches, %.1f us" %
              (sum(v[0] for v in ta.values()), sum(v[1] for v in ta.values()) / 1e3,
               sum(v[0] for v in tc.values()), sum(v[1] for v in tc.values()) / 1e3), ""]
    with open(out or os.path.join(ROOT, "profiles", "detector_launches.md"), "w") as f:
        f.write("\n".join(lines))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--configs", default="bev,bp")
    ap.add_argument("--precisions", default="fp32,bf16")
    ap.add_argument("--batches", default="1,2,4,8,32")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--trace", choices=["A", "C", "L", "F", "G"])
    ap.add_argument("--lanes", action="store_true")
    ap.add_argument("--frames", action="store_true")
    ap.add_argument("--formats", help="with --frames: frame formats to compare, e.g. rgb,bgr,nv12,yuyv; surfaces too: nv12@decoder (pitch 1536, "
                    "chroma at row 736), nv12@pointers (the same, Y and CbCr in separate allocations), i420, rgbx, bgrx")
    ap.add_argument("--yuv", default="bt709", help="with --formats: the YCbCr preset (the cost does not depend on it)")
    ap.add_argument("--frames-launches", nargs=2, metavar=("DB_F", "DB_G"))
    ap.add_argument("--lanes-launches", metavar="DB_L")
    ap.add_argument("--launches", nargs=2, metavar=("DB_A", "DB_C"))
    args = ap.parse_args()
    if args.trace:
        trace(args.trace)
    elif args.launches:
        launches(args.launches[0], args.launches[1], args.out)
    elif args.lanes_launches:
        lanes_launches(args.lanes_launches, args.out)
    elif args.frames_launches:
        frames_launches(args.frames_launches[0], args.frames_launches[1], args.out)
    elif args.lanes:
        run_lanes(args)
    elif args.frames and args.formats:
        run_formats(args)
    elif args.frames:
        run_frames(args)
    else:
        run(args)
