#!/usr/bin/env python
"""Generate tests/golden/loader.npz by running the REAL ``LaneDataset.__getitem__`` of both reference trees
(BP/Dataloader/Load_Data_new.py, BEV/Dataloader/Load_Data_new.py) on the CPU (authoring container only; needs the reference tree):

    python tools/gen_golden_loader.py

The reference modules are loaded at run time with what this container lacks stood in for: ``torchvision`` by the four calls the
datasets make (``F.crop`` / ``F.resize`` / ``F.hflip`` / ``transforms.ToTensor``) written on PIL, ``cv2`` by the oracle's stub,
``np.RankWarning``.  Nothing of the reference is copied.

The datasets only list their directories and open the files they are asked for, so a temporary directory of EMPTY placeholder files
named ``1.png`` .. ``3626.png`` (BP) / ``2535.png`` (BEV) satisfies the count assertions; the fetched positions hold real 720 x 32
PNGs.  The names are not zero-padded, so the sorted listing is lexicographic and ``target_idx[i] - 1`` is not ``i``: the file-number
bookkeeping is part of what is recorded.  ``lanes_ordered.json`` / ``Curve_parameters.json`` (absent from the reference's tree) are
written in the format the loaders read: ``lanes`` + ``h_samples`` from 4-lane lines of Labels/label_data_0313.json (48 heights)
plus seeded 56-height labels, seeded ``poly_params`` with absent lanes as zeros; ``lines`` from the reference's own label_new.json.

A case = the label dicts in (JSON strings) and every non-pixel output of ``__getitem__`` after ``np.random.seed(k)``; the drawn flip
is recovered by replaying the seed.  BP cases are recorded at resize 256 and at resize 16 (the flipped x and the horizon depend on
it).  The real ``get_loader`` of both trees is also called for num_train 10 and 37, shuffled and not, and its split recorded (the
samplers' index lists, the returned ``valid_idx``, the batches per epoch).  The conditions the tests rely on are asserted on the
fixture at the end.
"""
import importlib.util
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import ref_shims  # noqa: E402
import loader_ref  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "loader.npz")
CASES = 60
COUNT = {"bp": 3626, "bev": 2535}
BP_RESIZES = (256, 16)
BEV_RESIZE = 16
SPLIT_SIZES, SPLIT_BATCH, SPLIT_VAL_BATCH = (10, 37), 4, 2
H48 = list(range(240, 720, 10))
H56 = list(range(160, 720, 10))


def install_torchvision_standin():
    tv, tr, fn, ut = (types.ModuleType(n) for n in ("torchvision", "torchvision.transforms", "torchvision.transforms.functional",
                                                   "torchvision.utils"))

    def crop(img, top, left, height, width):
        return img.crop((left, top, left + width, top + height))

    def resize(img, size, interpolation=Image.BILINEAR):
        return img.resize((size[1], size[0]), interpolation)

    def hflip(img):
        if isinstance(img, np.ndarray):                 # BEV :89 hands the label map over as an array
            return img[:, ::-1].copy()
        return img.transpose(Image.FLIP_LEFT_RIGHT)

    class ToTensor:
        def __call__(self, pic):
            arr = np.array(pic)
            if arr.ndim == 2:
                arr = arr[:, :, None]
            t = torch.from_numpy(arr.transpose(2, 0, 1).copy())
            return t.float().div(255) if t.dtype == torch.uint8 else t

    fn.crop, fn.resize, fn.hflip, tr.ToTensor, tr.functional, tv.transforms, tv.utils = crop, resize, hflip, ToTensor, fn, tr, ut
    for m in (tv, tr, fn, ut):
        sys.modules[m.__name__] = m


def load_reference(tree):
    ref_shims._install_cv2_stub()
    install_torchvision_standin()
    if not hasattr(np, "RankWarning"):
        np.RankWarning = np.exceptions.RankWarning
    root = os.path.join(os.environ.get("LANEFIT_REFERENCE_ROOT", ref_shims.REF_ROOT), ref_shims.TREES[tree])
    spec = importlib.util.spec_from_file_location("_ref_loader_" + tree, os.path.join(root, "Dataloader", "Load_Data_new.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod, root


def seeded_lane(rng, heights, first, last, x0=None):
    """A straight lane present on columns [first, last) of its height list, clipped to the frame like TuSimple's."""
    S = len(heights)
    x0 = rng.uniform(100, 1100) if x0 is None else x0
    k = rng.uniform(-1.2, 1.2)
    x = np.rint(x0 + k * (np.asarray(heights, np.float64) - heights[S // 2])).astype(np.int64)
    lane = np.full(S, -2, np.int64)
    lane[first:last] = x[first:last]
    lane[(lane < 0) | (lane > 1279)] = -2
    return [int(v) for v in lane]


def bp_case_labels(k, natural):
    """Lane label of BP case k: a line of label_data_0313.json, or a seeded special."""
    rng = np.random.default_rng([77, k])
    special = {
        3: ("h56", lambda: dict(lanes=[seeded_lane(rng, H56, 2, 50), seeded_lane(rng, H56, 0, 56, 640), seeded_lane(rng, H56, 10, 40),
                                      seeded_lane(rng, H56, 5, 56)], h_samples=H56)),
        7: ("absent_lane", lambda: dict(lanes=[seeded_lane(rng, H56, 12, 56), [-2] * 56, seeded_lane(rng, H56, 9, 30), [-2] * 56],
                                        h_samples=H56)),
        11: ("all_absent48", lambda: dict(lanes=[[-2] * 48] * 4, h_samples=H48)),
        12: ("all_absent56", lambda: dict(lanes=[[-2] * 56] * 4, h_samples=H56)),
        15: ("x_zero", lambda: dict(lanes=[[0, 3, 1] + [-2] * 53, [-2] * 6 + [0] + seeded_lane(rng, H56, 7, 56)[7:],
                                           seeded_lane(rng, H56, 20, 56), [-2] * 55 + [0]], h_samples=H56)),
        19: ("y_below_zero", lambda: dict(lanes=[seeded_lane(rng, list(range(30, 590, 10)), 0, 56, 600)] +
                                          [seeded_lane(rng, list(range(30, 590, 10)), 9, 40) for _ in range(3)],
                                          h_samples=list(range(30, 590, 10)))),
        23: ("y_above_resize", lambda: dict(lanes=[[-2] * 55 + [640], [-2] * 56, [-2] * 54 + [300, 310], [-2] * 56],
                                            h_samples=list(range(200, 760, 10)))),
        27: ("fractional_heights", lambda: dict(lanes=[seeded_lane(rng, H56, 8, 56), seeded_lane(rng, H56, 3, 56),
                                                       seeded_lane(rng, H56, 30, 56), seeded_lane(rng, H56, 1, 20)],
                                                h_samples=[h + 0.3 for h in H56])),
        35: ("all_lanes_above_resize", lambda: dict(lanes=[[-2] * 55 + [640], [-2] * 55 + [200], [-2] * 55 + [900], [-2] * 55 + [5]],
                                                    h_samples=list(range(180, 730, 10)) + [750])),
        # the zip quirk at its plainest: 48 heights, the only present point in the LAST column -- which the padded lane never pairs
        31: ("zip_quirk", lambda: dict(lanes=[[-2] * 47 + [500], [-2] * 48, [-2] * 40 + [700] + [-2] * 7, [-2] * 48], h_samples=H48)),
    }
    if k in special:
        return special[k][1]()
    if k % 4 == 2:
        return dict(lanes=[seeded_lane(rng, H56, int(rng.integers(0, 14)), int(rng.integers(30, 57))) for _ in range(4)], h_samples=H56)
    lab = natural[k]
    return dict(lanes=lab["lanes"], h_samples=lab["h_samples"])


def bev_case_labels(k):
    rng = np.random.default_rng([78, k])
    params = [[float(rng.normal(0, .2)), float(rng.normal(0, .4)), float(rng.uniform(.1, .9))] for _ in range(4)]
    if k % 5 == 1:
        params[int(rng.integers(0, 4))] = [0, 0, 0]
    if k % 10 == 4:
        params[2], params[3] = [0, 0, 0], [0, 0, 0]
    if k == 13:
        params = [[0.0, 0.0, 0.0]] * 4                   # (floats: an all-integer label is negated as an integer array, -0 = +0)
    return dict(poly_params=params)


def write_png_pair(image_path, gt_path):
    rng = np.random.default_rng(5)
    Image.fromarray(rng.integers(0, 256, (720, 32, 3), dtype=np.uint8)).save(image_path)
    gt = rng.integers(0, 5, (720, 32), dtype=np.uint8)
    gt[:, 3] = 1                                         # (BEV :106 needs a labelled pixel after any resize)
    im = Image.frombytes("P", (32, 720), gt.tobytes())
    im.putpalette([v for i in range(256) for v in (i, i, i)])
    im.save(gt_path)


def main():
    with tempfile.TemporaryDirectory() as tmp:           # ~12 000 placeholder files: removed when the run ends
        out = record(tmp)
    np.savez_compressed(OUT, **out)
    print(OUT, "%.1f KB" % (os.path.getsize(OUT) / 1024), CASES, "cases per tree")


def record(tmp):
    out = {}
    cwd = os.getcwd()
    for tree in ("bp", "bev"):
        mod, root = load_reference(tree)
        count = COUNT[tree]
        names = sorted("%d.png" % i for i in range(1, count + 1))
        target_idx = [int(os.path.splitext(n)[0]) for n in names]
        work = os.path.join(tmp, tree)
        image_dir, gt_dir = os.path.join(work, "images"), os.path.join(work, "gt")
        os.makedirs(image_dir), os.makedirs(gt_dir), os.makedirs(os.path.join(work, "Labels"))
        for n in names:
            open(os.path.join(image_dir, n), "wb").close()
            open(os.path.join(gt_dir, n), "wb").close()
        # positions fetched: spread over the listing; a quarter of them validation, listed in an order of their own
        positions = [int(p) for p in np.random.default_rng(9).choice(count, CASES, replace=False)]
        valid_positions = [positions[c] for c in (17, 4, 41, 8, 29, 0, 53, 36, 22, 12, 47, 58, 33, 26, 50)]
        for p in positions:
            write_png_pair(os.path.join(image_dir, names[p]), os.path.join(gt_dir, names[p]))
        ref_lines = [json.loads(l) for l in open(os.path.join(root, "Labels", "label_new.json")).readlines()]
        natural = [l for l in (json.loads(l) for l in open(os.path.join(root, "Labels", "label_data_0313.json")).readlines())
                   if len(l["lanes"]) == 4 and len(l["h_samples"]) == 48]
        natural = [natural[i] for i in np.random.default_rng(3).choice(len(natural), CASES, replace=False)]
        filler_line = dict(lines=[-1] * 10)
        filler = dict(lanes=[[-2] * 48] * 4, h_samples=H48) if tree == "bp" else dict(poly_params=[[0, 0, 0]] * 4)
        labels, lines = [filler] * count, [filler_line] * count
        line_pick = np.random.default_rng(4).choice(len(ref_lines), CASES, replace=False)
        for c, p in enumerate(positions):
            f = target_idx[p] - 1
            labels[f] = bp_case_labels(c, natural) if tree == "bp" else bev_case_labels(c)
            lines[f] = dict(lines=ref_lines[line_pick[c]]["lines"])
        label_file = os.path.join(work, "lanes_ordered.json" if tree == "bp" else "Curve_parameters.json")
        for path, rows in ((label_file, labels), (os.path.join(work, "Labels", "label_new.json"), lines)):
            with open(path, "w") as fh:
                fh.write("".join(json.dumps(r) + "\n" for r in rows))
        os.chdir(work)                                   # the datasets open 'Labels/label_new.json' relative to the cwd
        try:
            datasets = {}
            for flip_on in (True, False):
                for R in (BP_RESIZES if tree == "bp" else (BEV_RESIZE,)):
                    if tree == "bp":
                        datasets[flip_on, R] = mod.LaneDataset(end_to_end=True, valid_idx=valid_positions, json_file=label_file,
                                                               lanes_file=label_file, image_dir=image_dir, gt_dir=gt_dir,
                                                               flip_on=flip_on, resize=R, nclasses=4)
                    else:
                        datasets[flip_on, R] = mod.LaneDataset(end_to_end=True, valid_idx=valid_positions, json_file=label_file,
                                                               image_dir=image_dir, gt_dir=gt_dir, flip_on=flip_on, resize=R)
            # the real get_loader's split: sampler index lists, the returned valid_idx, batches per epoch (batch 4, BP validation 2)
            splits = {}
            for num_train in SPLIT_SIZES:
                for shuffle in (True, False):
                    if tree == "bp":
                        tl, vl, vi = mod.get_loader(num_train, label_file, label_file, image_dir, gt_dir, True, SPLIT_BATCH,
                                                    SPLIT_VAL_BATCH, shuffle, 0, True, 16, 4)
                    else:
                        tl, vl, vi = mod.get_loader(num_train, label_file, image_dir, gt_dir, True, SPLIT_BATCH, shuffle, 0, True, 16)
                    key = "split_n%d_s%d_" % (num_train, shuffle)
                    splits[key + "train"] = np.array(list(tl.sampler.indices), np.int32)
                    splits[key + "valid"] = np.array(list(vl.sampler.indices), np.int32)
                    splits[key + "returned"] = np.array(list(vi), np.int32)
                    splits[key + "batches"] = np.array([len(tl), len(vl)], np.int32)
        finally:
            os.chdir(cwd)
        rec = dict(position=np.array(positions, np.int32), file_number=np.array([target_idx[p] for p in positions], np.int32),
                   valid_positions=np.array(valid_positions, np.int32), draw=np.zeros(CASES), flip_on=np.zeros(CASES, np.uint8),
                   is_valid=np.zeros(CASES, np.uint8), idx=np.zeros(CASES, np.int64), index=np.full(CASES, -1, np.int64),
                   tuple_len=np.zeros(CASES, np.int8), label_json=[], line_json=[])
        if tree == "bp":
            rec.update(valid_points=np.zeros((CASES, 4, 56)), gt_line=np.zeros((CASES, 4), np.float32))
            for R in BP_RESIZES:
                rec["lanes_R%d" % R] = np.zeros((CASES, 4, 56))
                rec["horizon_R%d" % R] = np.zeros((CASES, R), np.float32)
        else:
            rec.update(params=np.zeros((CASES, 4, 3), np.float32), gt_line=np.zeros((CASES, 4), np.int64))
        for c, p in enumerate(positions):
            flip_on = c % 6 != 5
            np.random.seed(c)
            draw = np.random.uniform(0.0, 1.0)
            f = target_idx[p] - 1
            rec["draw"][c], rec["flip_on"][c] = draw, flip_on
            rec["label_json"].append(json.dumps(labels[f]))
            rec["line_json"].append(json.dumps(lines[f]))
            for R in (BP_RESIZES if tree == "bp" else (BEV_RESIZE,)):
                np.random.seed(c)
                item = datasets[flip_on, R][p]
                is_valid = len(item) == (8 if tree == "bp" else 7)
                assert is_valid == (p in valid_positions)
                rec["is_valid"][c], rec["tuple_len"][c] = is_valid, len(item)
                fl = loader_ref.effective_flip(draw, flip_on, is_valid)
                if tree == "bp":
                    lanes, idx, gt_line, horizon, valid_points = item[2], item[3], item[4], item[5], item[-1]
                    assert lanes.dtype == torch.float64 and gt_line.dtype == torch.float32 and horizon.dtype == torch.float32
                    assert valid_points.dtype == torch.float64 and tuple(horizon.shape) == (R,)
                    mine = loader_ref.bp_labels(labels[f], lines[f], fl, R)
                    for name, t in (("lanes", lanes), ("gt_line", gt_line), ("horizon", horizon), ("valid_points", valid_points)):
                        assert np.array_equal(t.numpy(), mine[name]) and t.numpy().dtype == mine[name].dtype, (c, R, name)
                    rec["lanes_R%d" % R][c], rec["horizon_R%d" % R][c] = lanes.numpy(), horizon.numpy()
                    rec["valid_points"][c], rec["gt_line"][c] = valid_points.numpy(), gt_line.numpy()
                else:
                    params, idx, gt_line = item[2], item[3], item[4]
                    assert params.dtype == torch.float32 and gt_line.dtype == torch.int64
                    mine = loader_ref.bev_labels(labels[f], lines[f], fl)
                    assert params.numpy().tobytes() == mine["params"].tobytes() and np.array_equal(gt_line.numpy(), mine["gt_line"])
                    rec["params"][c], rec["gt_line"][c] = params.numpy(), gt_line.numpy()
                assert idx == f
                rec["idx"][c] = idx
                if is_valid:
                    rec["index"][c] = item[6]
                    assert item[6] == valid_positions.index(p)
        rec["label_json"], rec["line_json"] = np.array(rec["label_json"]), np.array(rec["line_json"])
        check_conditions(tree, rec)
        out.update({tree + "_" + k: v for k, v in rec.items()})
        out.update({tree + "_" + k: v for k, v in splits.items()})
    return out


def check_conditions(tree, rec):
    """Every situation the tests rely on occurs in the fixture."""
    flipped = (rec["draw"] > 0.5) & (rec["flip_on"] == 1) & (rec["is_valid"] == 0)
    train = rec["is_valid"] == 0
    assert np.any(flipped) and np.any(train & ~flipped & (rec["flip_on"] == 1))             # a flipped and an unflipped training sample
    assert np.any((rec["is_valid"] == 1) & (rec["draw"] > 0.5) & (rec["flip_on"] == 1))     # a validation sample that drew > 0.5
    assert np.any(train & (rec["draw"] > 0.5) & (rec["flip_on"] == 0))                      # flip_on false holds a drawn flip back
    lines = np.array([json.loads(s)["lines"][3:7] for s in rec["line_json"]])
    assert (lines == -1).any() and (lines == 1).any() and (lines == 0).any()                # values that clamp
    labels = [json.loads(s) for s in rec["label_json"]]
    if tree == "bp":
        S = np.array([len(l["h_samples"]) for l in labels])
        assert (S == 48).any() and (S == 56).any()
        raw = np.stack([loader_ref.pad_lanes(l["lanes"]) for l in labels])
        absent = (raw < 0).all(axis=2)
        assert absent.any() and absent.all(axis=1).any() and (absent.any(axis=1) & flipped).any()
        assert (raw[:, :, :8] >= 0).any() and (raw == 0).any()                              # 0 <= x in columns 0..7; x == 0
        assert (rec["valid_points"][:, :, :8] == 0).all() and rec["valid_points"].any()
        y = [np.where(r[:, :len(l["h_samples"])] >= 0, np.array(l["h_samples"])[None, :] / 2.5 - 32, np.inf).min(axis=1)
             for r, l in zip(raw, labels)]
        assert any(np.isfinite(v).all() and v.min() > 256 for v in y)                      # all four lanes present, all above resize
        hz = rec["horizon_R256"].sum(axis=1)
        assert (hz == 256).any() and ((hz > 0) & (hz < 256)).any() and len(set(hz.tolist())) > 5
        assert (rec["horizon_R16"].sum(axis=1) == 0).any()                                  # Python's negative slice, emptied
        assert (rec["gt_line"] == 0).any() and (rec["gt_line"] == 1).any()
    else:
        absent = np.array([[not any(p) for p in l["poly_params"]] for l in labels])
        assert (absent.any(axis=1) & flipped).any() and (absent.any(axis=1) & ~flipped).any()
        assert np.any(np.signbit(rec["params"]) & (rec["params"] == 0))                     # the (-0, -0, 1) of a flipped absent lane
        assert set(np.unique(rec["gt_line"]).tolist()) == {0, 1, 2}


if __name__ == "__main__":
    sys.exit(main())
