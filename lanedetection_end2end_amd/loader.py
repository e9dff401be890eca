"""Resident dataset and device-side loader: the mirror of both trees' ``get_loader``.

The whole decoded dataset -- uint8 frames, uint8 label maps and the parsed label tables -- is uploaded ONCE and stays in HBM; a
batch is an index vector.  ``ResidentDataset.batch(sel, flip)`` makes three launches: ``lf_label_batch_bp`` / ``lf_label_batch_bev``
(the label statements of ``LaneDataset.__getitem__``, BP/Dataloader/Load_Data_new.py:133-197, BEV/Dataloader/Load_Data_new.py:74,
86-111) and the two ``InputPipeline`` launches (the pixel statements), and returns the default-collated tuple of the reference's
DataLoader -- with no host read and no host -> device copy of batch data.  ``ResidentLoader`` draws the index batches with torch's own
samplers and the flips from numpy's global state in the reference's order, so a seeded run reproduces the reference's
``num_workers=0`` stream; an epoch's permutation and flip flags are the only upload, once per epoch.

    from lanedetection_end2end_amd.loader import get_loader_bp as get_loader      # the one-line edit of BP/main.py
    from lanedetection_end2end_amd.loader import get_loader_bev as get_loader     # ... of BEV/main.py

Deviations from the reference, all at construction time:
  * the assertion that both listings hold exactly 3626 (BP :95) / 2535 (BEV :51) files is not kept: any number of files is a dataset;
  * a BP label with fewer than 4 lanes is padded with absent lanes (the reference raises in ``np.hstack``);
  * a label with more than 56 heights, a lane row whose length differs from its ``h_samples``, a lane x that is no integer (the
    reference would keep the float; the device table is int32 like TuSimple's labels), ragged ``poly_params`` and a ``lines``
    list that is not 10 long raise ``ValueError`` when the labels are parsed, not at the first ``__getitem__`` that meets them;
  * a BEV label whose ``poly_params`` are JSON integers throughout is negated as an integer array by the reference, so its flipped
    zeros are +0; the fp64 table gives -0 there as for every other label (an all-integer label does not occur in fitted parameters);
  * ``json_file`` is not read by the BP tree (the reference loads it and never looks at it);
  * the flips of an epoch are all drawn at the first ``next()`` of its iterator (with the permutation), not one per ``__getitem__``:
    the same numbers in the same order as long as nothing else draws from ``np.random`` inside the epoch.
Multi-GPU: one ``ResidentDataset`` per rank holds the WHOLE pool; sharding the index stream is left to ``dp.epoch_batches`` in a loop
of one's own (``dataset.batch(sel, flip)`` takes any device index vector).
"""
import json
import math
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _lib
from .pipeline import InputPipeline

NUM_POINTS = 56         # BP :99
NUM_LINES = 10          # length of a label_new.json "lines" list
DECODE_THREADS = 16


# ----------------------------------------------------------------------------------------------------------------- label tables
def _line_table(line_labels, rows):
    out = np.zeros((len(rows), NUM_LINES), np.int8)
    for m, r in enumerate(rows):
        lst = line_labels[r]["lines"]
        if len(lst) != NUM_LINES:
            raise ValueError("label %d: a 'lines' list of %d entries (expected %d)" % (r, len(lst), NUM_LINES))
        out[m] = lst
    return out


def parse_bp_labels(lane_labels, line_labels, rows):
    """Label tables of the BP tree for the label-list entries ``rows`` (file number - 1 per pool row):
    lanes (M,4,56) int32 left-padded with -2 (BP :135-137), h_samples (M,56) fp64, h_count (M) int32, lines (M,10) int8."""
    M = len(rows)
    lanes = np.full((M, 4, NUM_POINTS), -2, np.int32)
    h_samples = np.zeros((M, NUM_POINTS), np.float64)
    h_count = np.zeros(M, np.int32)
    for m, r in enumerate(rows):
        lab = lane_labels[r]
        h = lab["h_samples"]
        S = len(h)
        if S > NUM_POINTS:
            raise ValueError("label %d: %d heights, more than %d" % (r, S, NUM_POINTS))
        if len(lab["lanes"]) > 4:
            raise ValueError("label %d: %d lanes, more than 4" % (r, len(lab["lanes"])))
        for l, lane in enumerate(lab["lanes"]):
            if len(lane) != S:
                raise ValueError("label %d: lane %d has %d points, h_samples has %d" % (r, l, len(lane), S))
            if S:
                x = np.asarray(lane, np.float64)
                if not np.array_equal(x, np.rint(x)) or np.abs(x).max() >= 2 ** 31:
                    raise ValueError("label %d: lane %d holds x values that are no int32 (the table is integer, as TuSimple's labels)" % (r, l))
                lanes[m, l, NUM_POINTS - S:] = x
        h_samples[m, :S] = h
        h_count[m] = S
    return dict(lanes=lanes, h_samples=h_samples, h_count=h_count, lines=_line_table(line_labels, rows))


def parse_bev_labels(param_labels, line_labels, rows):
    """Label tables of the BEV tree: params (M,4,3) fp64 (``poly_params``, BEV :74), lines (M,10) int8."""
    params = np.zeros((len(rows), 4, 3), np.float64)
    for m, r in enumerate(rows):
        p = param_labels[r]["poly_params"]
        if len(p) != 4 or any(len(q) != 3 for q in p):
            raise ValueError("label %d: poly_params is not 4 x 3: row lengths %s" % (r, [len(q) for q in p]))
        params[m] = p
    return dict(params=params, lines=_line_table(line_labels, rows))


def split_tables(file_numbers, valid_idx):
    """file_idx (M) int64, is_valid (M) uint8, valid_pos (M) int32 and the dataset's own ``valid_idx`` list: the positions the split
    produced mapped through ``target_idx[i] - 1`` (BP :97-98); membership and ``.index`` are on the file number - 1 (:168,194-195)."""
    file_idx = np.asarray(file_numbers, np.int64) - 1
    mapped = [int(file_idx[i]) for i in valid_idx]
    first = {}
    for pos, v in enumerate(mapped):
        first.setdefault(v, pos)
    valid_pos = np.array([first.get(int(v), -1) for v in file_idx], np.int32).reshape(-1)
    return file_idx, (valid_pos >= 0).astype(np.uint8), valid_pos, mapped


def _read_json_lines(path):
    with open(path) as fh:
        return [json.loads(line) for line in fh.readlines()]


# ------------------------------------------------------------------------------------------------------------------ the dataset
def _pool_fits(nbytes, device):
    free, total = torch.cuda.mem_get_info(device)
    if nbytes > free:
        raise _lib.LaneFitLibraryError("ResidentDataset: the decoded pool needs %d bytes, the device has %d bytes free (of %d)"
                                       % (nbytes, free, total))


def _upload_chunked(host, device, chunk_bytes=64 << 20):
    """A host uint8 array to a new device tensor through one pinned staging buffer, in chunks along axis 0."""
    host = np.ascontiguousarray(host)
    out = torch.empty(host.shape, dtype=torch.uint8, device=device)
    if host.shape[0] == 0:
        return out
    per = max(1, chunk_bytes // max(1, host[0].nbytes))
    stage = torch.empty((per,) + host.shape[1:], dtype=torch.uint8, pin_memory=True)
    done = torch.cuda.Event()
    for a in range(0, host.shape[0], per):
        b = min(a + per, host.shape[0])
        stage[:b - a].copy_(torch.from_numpy(host[a:b]))
        out[a:b].copy_(stage[:b - a], non_blocking=True)
        done.record()
        done.synchronize()              # the staging buffer is reused by the next chunk
    return out


class ResidentDataset:
    """``ResidentDataset(tree, resize, nclasses, frames_u8, labels_u8, file_numbers, tables, valid_idx=(), crop=640)``.

    frames_u8 (M,H,W,3) / labels_u8 (M,H,W) uint8 ON THE DEVICE, file_numbers (M) the integer stems of the files (the reference's
    ``target_idx``), tables the host dict of ``parse_bp_labels`` / ``parse_bev_labels`` for the same M rows, valid_idx the POSITIONS
    of the validation samples as the split produced them.  Use ``from_arrays`` / ``from_directory``."""

    def __init__(self, tree, resize, nclasses, frames_u8, labels_u8, file_numbers, tables, valid_idx=(), crop=640):
        assert tree in ("bev", "bp")
        if not (frames_u8.is_cuda and labels_u8.is_cuda):
            raise _lib.LaneFitLibraryError("ResidentDataset needs the decoded pools on the MI355X; there is no CPU path")
        M, H, W, _ = frames_u8.shape
        assert labels_u8.shape == (M, H, W) and len(file_numbers) == M and M > 0
        self.tree, self.resize, self.nclasses, self.M = tree, int(resize), nclasses, M
        self.device = frames_u8.device
        self.frames, self.labels = frames_u8.contiguous(), labels_u8.contiguous()
        self.pipeline = InputPipeline(resize, tree=tree, nclasses=nclasses, frame_hw=(H, W), crop=crop)
        file_idx, is_valid, valid_pos, self.valid_idx = split_tables(file_numbers, valid_idx)
        self.valid_rows = frozenset(int(m) for m in np.nonzero(is_valid)[0])
        host = dict(tables, file_idx=file_idx, is_valid=is_valid, valid_pos=valid_pos)
        for name, arr in host.items():
            assert arr.shape[0] == M, name
        self.tables = {k: torch.from_numpy(np.ascontiguousarray(v)).to(self.device) for k, v in host.items()}      # uploaded once
        self.flipped = None             # the effective flips of the last batch (N,) uint8
        self._bad = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._pending = None

    def __len__(self):
        return self.M

    # ------------------------------------------------------------------------------------------------------------ constructors
    @staticmethod
    def host_tables(tree, file_numbers, line_labels, lane_labels=None, param_labels=None):
        rows = [int(f) - 1 for f in file_numbers]
        if tree == "bp":
            return parse_bp_labels(lane_labels, line_labels, rows)
        return parse_bev_labels(param_labels, line_labels, rows)

    @classmethod
    def from_arrays(cls, tree, resize, frames_u8, labels_u8, file_numbers, line_labels, lane_labels=None, param_labels=None,
                    valid_idx=(), nclasses=2, crop=640, device="cuda"):
        """frames_u8 / labels_u8: uint8 tensors (any device) or numpy arrays; ``*_labels``: the parsed JSON lines of the label files,
        indexed by file number - 1 like the reference's lists (lane_labels: ``lanes`` + ``h_samples``, BP; param_labels:
        ``poly_params``, BEV; line_labels: ``lines``)."""
        tables = cls.host_tables(tree, file_numbers, line_labels, lane_labels, param_labels)
        device = torch.device(device)
        pools = []
        for pool in (frames_u8, labels_u8):
            if isinstance(pool, torch.Tensor) and pool.is_cuda:
                pools.append(pool)
                continue
            pool = pool.numpy() if isinstance(pool, torch.Tensor) else np.asarray(pool)
            assert pool.dtype == np.uint8
            _pool_fits(pool.nbytes, device)
            pools.append(_upload_chunked(pool, device))
        return cls(tree, resize, nclasses, pools[0], pools[1], file_numbers, tables, valid_idx, crop)

    @classmethod
    def from_directory(cls, image_dir, gt_dir, json_file, lanes_file=None, line_file="Labels/label_new.json", tree="bev", resize=256,
                       nclasses=2, valid_idx=(), crop=640, device="cuda", threads=DECODE_THREADS, decode_only=False):
        """The reference's own bookkeeping (BP :88-98, BEV :45-54): sorted listings, matching stems, ``target_idx = int(stem)``; every
        file decoded once with PIL (``convert('RGB')`` / ``convert('P')``, BP :118-121).  ``decode_only=True`` stops before the upload
        and returns the host dict (file_numbers, valid_idx, frames, labels, tables) -- no GPU is touched.  The whole decoded pool
        (M * H * W * 4 bytes, 13.4 GB for TuSimple) is held in pageable HOST memory until the chunked upload has finished; only the
        device side is checked (``mem_get_info``) before anything is allocated."""
        from PIL import Image
        images, maps = sorted(os.listdir(image_dir)), sorted(os.listdir(gt_dir))
        if len(images) != len(maps):
            raise ValueError("%d images in %s, %d label maps in %s" % (len(images), image_dir, len(maps), gt_dir))
        stems = [name.partition(".")[0] for name in images]          # up to the first dot, as the reference cuts it (BP :97,115)
        for name, stem, other in zip(images, stems, maps):
            if other.partition(".")[0] != stem:
                raise ValueError("image %s and label map %s do not match" % (name, other))
        file_numbers = list(map(int, stems))
        line_labels = _read_json_lines(line_file)
        if tree == "bp":
            tables = parse_bp_labels(_read_json_lines(lanes_file), line_labels, [f - 1 for f in file_numbers])
        else:
            tables = parse_bev_labels(_read_json_lines(json_file), line_labels, [f - 1 for f in file_numbers])
        M = len(images)
        if M == 0:
            raise ValueError("no images in " + image_dir)

        def decode(name_mode):
            with open(name_mode[0], "rb") as fh:
                return np.asarray(Image.open(fh).convert(name_mode[1]))

        with Image.open(os.path.join(image_dir, images[0])) as first:      # the header only
            W, H = first.size
        if not decode_only:
            device = torch.device(device)
            _pool_fits(M * H * W * 4, device)
        frames, labels = np.empty((M, H, W, 3), np.uint8), np.empty((M, H, W), np.uint8)
        jobs = [(os.path.join(image_dir, n), "RGB") for n in images] + [(os.path.join(gt_dir, n), "P") for n in maps]
        workers = max(1, min(int(threads), DECODE_THREADS, len(jobs)))
        with ThreadPoolExecutor(max_workers=workers) as pool:
            for k, arr in enumerate(pool.map(decode, jobs)):
                dst = frames[k] if k < M else labels[k - M]
                if arr.shape != dst.shape:
                    raise ValueError("%s is %s, the first frame is %d x %d" % (jobs[k][0], arr.shape, H, W))
                dst[...] = arr
        if decode_only:
            return dict(file_numbers=file_numbers, valid_idx=split_tables(file_numbers, valid_idx)[3], frames=frames, labels=labels,
                        tables=tables)
        return cls(tree, resize, nclasses, _upload_chunked(frames, device), _upload_chunked(labels, device), file_numbers, tables,
                   valid_idx, crop)

    # ------------------------------------------------------------------------------------------------------------------ batches
    def flush(self):
        """Raise now if the previous batch held an index outside the pool (counted on the device, read one call late)."""
        pend, self._pending = self._pending, None
        if pend is not None and int(pend.get()[0]):
            n = int(pend.get()[0])
            self._bad.zero_()
            self.pipeline._pending = None                           # the pixel kernels counted the same indices
            if self.pipeline._bad is not None:
                self.pipeline._bad.zero_()
            raise IndexError("ResidentDataset: %d index value(s) outside the pool of %d samples" % (n, self.M))
        self.pipeline.flush()

    def label_batch(self, sel, flip=None):
        """The ONE label launch of a batch -> dict of device tensors: ``idx``, ``index``, ``flipped`` (the effective flips) and, BP,
        ``lanes`` / ``valid_points`` / ``horizon`` / ``gt_line``; BEV, ``params`` / ``gt_line``.  ``sel`` / ``flip`` as in ``batch``."""
        lib, T, dev = _lib.load(), self.tables, self.device
        if not sel.is_cuda or (flip is not None and not flip.is_cuda):
            raise _lib.LaneFitLibraryError("ResidentDataset.batch needs sel and flip on the MI355X; there is no CPU path")
        sel = sel.to(dtype=torch.int64).contiguous()
        fl = None if flip is None else flip.to(dtype=torch.uint8).contiguous()
        N, R = sel.numel(), self.resize
        assert N > 0 and (fl is None or fl.numel() == N)
        out = dict(idx=torch.empty(N, dtype=torch.int64, device=dev), index=torch.empty(N, dtype=torch.int64, device=dev),
                   flipped=torch.empty(N, dtype=torch.uint8, device=dev))
        P = _lib.ptr
        if self.tree == "bp":
            out.update(valid_points=torch.empty(N, 4, NUM_POINTS, dtype=torch.float64, device=dev),
                       lanes=torch.empty(N, 4, NUM_POINTS, dtype=torch.float64, device=dev),
                       horizon=torch.empty(N, R, dtype=torch.float32, device=dev),
                       gt_line=torch.empty(N, 4, dtype=torch.float32, device=dev))
            _lib.check(lib.lf_label_batch_bp(P(T["lanes"]), P(T["h_samples"]), P(T["h_count"]), P(T["lines"]), P(T["file_idx"]),
                                             P(T["is_valid"]), P(T["valid_pos"]), self.M, P(sel), P(fl), N, R, P(out["valid_points"]),
                                             P(out["lanes"]), P(out["horizon"]), P(out["gt_line"]), P(out["idx"]), P(out["index"]),
                                             P(out["flipped"]), P(self._bad), _lib.stream()), "lf_label_batch_bp")
        else:
            out.update(params=torch.empty(N, 4, 3, dtype=torch.float32, device=dev),
                       gt_line=torch.empty(N, 4, dtype=torch.int64, device=dev))
            _lib.check(lib.lf_label_batch_bev(P(T["params"]), P(T["lines"]), P(T["file_idx"]), P(T["is_valid"]), P(T["valid_pos"]),
                                              self.M, P(sel), P(fl), N, P(out["params"]), P(out["gt_line"]), P(out["idx"]),
                                              P(out["index"]), P(out["flipped"]), P(self._bad), _lib.stream()), "lf_label_batch_bev")
        return sel, out

    def batch(self, sel, flip=None, valid=False):
        """The reference's collated batch for pool rows ``sel`` (N,) int64 and drawn flips ``flip`` (N,) bool / uint8, both on the
        device.  BP: (image, gt, lanes, idx, gt_line, horizon, valid_points); BEV: (image, gt, params, idx, gt_line, horizon);
        ``valid=True`` (a batch of validation samples) adds ``index`` where the reference has it.  One label launch, then the two
        pipeline launches with its ``flipped`` output, so pixels and labels cannot disagree."""
        self.flush()
        sel, lab = self.label_batch(sel, flip)
        self._pending = _lib.DeferredRead(self._bad)
        self.flipped = lab["flipped"]
        image, gt, bev_horizon = self.pipeline(self.frames, self.labels, flip=self.flipped, index=sel)
        index = (lab["index"],) if valid else ()
        if self.tree == "bp":
            return (image, gt, lab["lanes"], lab["idx"], lab["gt_line"], lab["horizon"]) + index + (lab["valid_points"],)
        return (image, gt, lab["params"], lab["idx"], lab["gt_line"], bev_horizon) + index


# ------------------------------------------------------------------------------------------------------------------- the loader
class ResidentLoader:
    """``ResidentLoader(dataset, indices, batch_size, flip_on, drop_last=False, shuffle=True)``: iterable over the batches of one
    epoch, ``len()`` = batches per epoch.

    The index batches are those of ``DataLoader(ds, batch_size=..., sampler=SubsetRandomSampler(indices), num_workers=0)`` under the
    same ``torch.manual_seed`` (``shuffle=False``: the BP tree's ``SequentialIndicesSampler``): torch's own sampler objects, the
    default generator consumed at ``DataLoader``'s moments -- the base-seed draw when ``iter(loader)`` is called, the permutation
    at the first ``next()``.  One ``np.random.uniform(0.0, 1.0)`` per sample in batch order from numpy's global state, all of an
    epoch's at that first ``next()``, for validation samples and with ``flip_on`` false too (the reference evaluates the draw before ``and
    self.flip_on``).  ``dataset`` needs ``batch(sel, flip[, valid=True])`` and ``device``; ``valid_rows`` (a set of pool rows) marks
    the validation samples."""

    def __init__(self, dataset, indices, batch_size, flip_on, drop_last=False, shuffle=True):
        self.dataset, self.indices, self.batch_size = dataset, [int(i) for i in indices], int(batch_size)
        self.flip_on, self.drop_last, self.shuffle = bool(flip_on), bool(drop_last), bool(shuffle)
        sampler = (torch.utils.data.SubsetRandomSampler(self.indices) if self.shuffle
                   else torch.utils.data.SequentialSampler(self.indices))
        self._sequential = not self.shuffle
        self.batch_sampler = torch.utils.data.BatchSampler(sampler, self.batch_size, self.drop_last)
        valid_rows = getattr(dataset, "valid_rows", frozenset())
        inside = [i in valid_rows for i in self.indices]
        if any(inside) and not all(inside):
            raise ValueError("ResidentLoader: training and validation samples in one loader (their batch tuples differ)")
        self.valid = bool(inside) and all(inside)

    def __len__(self):
        return len(self.batch_sampler)

    def _to_device(self, host_array):
        device = torch.device(getattr(self.dataset, "device", "cpu"))
        t = torch.from_numpy(host_array)
        if device.type != "cuda":
            return t, None
        pinned = t.pin_memory()                                       # as optim._upload: no stall of the stream
        return pinned.to(device, non_blocking=True), pinned

    def __iter__(self):
        # DataLoader.__iter__ -> _BaseDataLoaderIter.__init__ draws the workers' base seed from the default generator NOW ...
        torch.empty((), dtype=torch.int64).random_()
        return self._epoch()

    def _epoch(self):
        # ... and the first next() starts the sampler: torch.randperm inside SubsetRandomSampler.__iter__
        if self._sequential:
            batches = [[self.indices[k] for k in b] for b in self.batch_sampler]      # SequentialSampler yields positions
        else:
            batches = [list(b) for b in self.batch_sampler]
        sizes = [len(b) for b in batches]
        total = sum(sizes)
        draws = np.array([np.random.uniform(0.0, 1.0) for _ in range(total)], np.float64)      # BP :167, BEV :87
        flips = ((draws > 0.5) & self.flip_on).astype(np.uint8)
        perm = np.array([i for b in batches for i in b], np.int64)
        if total == 0:
            return
        perm_dev, keep_a = self._to_device(perm)                      # ONE upload per epoch, a few bytes per sample
        flip_dev, keep_b = self._to_device(flips)
        start = 0
        for n in sizes:
            sel, fl = perm_dev[start:start + n], flip_dev[start:start + n]
            start += n
            yield self.dataset.batch(sel, fl, valid=True) if self.valid else self.dataset.batch(sel, fl)
        del keep_a, keep_b


# ------------------------------------------------------------------------------------------------------------------ get_loader
def split_indices(num_train, shuffle, split_percentage=0.2, whole_batches=None):
    """The train / validation split both ``get_loader`` functions make (BEV :298-306, BP :260-266) -> (train_idx, valid_idx) as lists
    of ints: positions 0 .. num_train - 1, permuted by numpy's global generator seeded with ``num_train`` when ``shuffle`` is the
    bool True, the first ``floor(split_percentage * num_train)`` of them for validation.  ``whole_batches=B`` (the BEV tree) cuts
    both lists to a multiple of B; the BP tree leaves that to ``drop_last``."""
    order = np.arange(num_train)
    if isinstance(shuffle, bool) and shuffle:
        np.random.seed(num_train)
        np.random.shuffle(order)
    n_valid = int(math.floor(split_percentage * num_train))
    parts = [order[n_valid:], order[:n_valid]]
    if whole_batches:
        parts = [part[:len(part) - len(part) % whole_batches] for part in parts]
    return [int(i) for i in parts[0]], [int(i) for i in parts[1]]


def get_loader_bev(num_train, json_file, image_dir, gt_dir, flip_on, batch_size, shuffle, num_workers, end_to_end, resize,
                   split_percentage=0.2, line_file="Labels/label_new.json", device="cuda"):
    """BEV/Dataloader/Load_Data_new.py:293-326 ``get_loader`` on a resident dataset -> (train_loader, valid_loader, valid_idx).
    ``num_workers`` and ``end_to_end`` are accepted and unused (there are no workers; the dataset never reads ``end_to_end``)."""
    train_idx, valid_idx = split_indices(num_train, shuffle, split_percentage, whole_batches=batch_size)
    dataset = ResidentDataset.from_directory(image_dir, gt_dir, json_file, None, line_file, tree="bev", resize=resize, nclasses=2,
                                             valid_idx=valid_idx, device=device)
    return (ResidentLoader(dataset, train_idx, batch_size, flip_on), ResidentLoader(dataset, valid_idx, batch_size, flip_on),
            valid_idx)


def get_loader_bp(num_train, json_file, lanes_file, image_dir, gt_dir, flip_on, batch_size, val_batch_size, shuffle, num_workers,
                  end_to_end, resize, nclasses, split_percentage=0.2, line_file="Labels/label_new.json", device="cuda"):
    """BP/Dataloader/Load_Data_new.py:255-290 ``get_loader`` on a resident dataset -> (train_loader, valid_loader, valid_idx): a
    SubsetRandomSampler over the training indices, the validation indices in sequence, ``drop_last=True`` on both."""
    train_idx, valid_idx = split_indices(num_train, shuffle, split_percentage)
    dataset = ResidentDataset.from_directory(image_dir, gt_dir, json_file, lanes_file, line_file, tree="bp", resize=resize,
                                             nclasses=nclasses, valid_idx=valid_idx, device=device)
    return (ResidentLoader(dataset, train_idx, batch_size, flip_on, drop_last=True),
            ResidentLoader(dataset, valid_idx, val_batch_size, flip_on, drop_last=True, shuffle=False), valid_idx)
