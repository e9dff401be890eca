"""CPU: the resident loader's host side (lanedetection_end2end_amd/loader.py) and the numpy restatement of the label statements
(tests/loader_ref.py) against tests/golden/loader.npz -- recorded from the real ``LaneDataset.__getitem__`` of both trees by
tools/gen_golden_loader.py.  Everything is exact, so every comparison is ``==`` on the bits."""
import ast
import json
import os

import numpy as np
import pytest
import torch

import loader_ref
from conftest import GOLDEN, ROOT


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "loader.npz"), allow_pickle=False)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------------------------ restatement
def test_restatement_reproduces_the_reference_bp(golden):
    g = golden
    C = len(g["bp_draw"])
    assert C >= 50
    for c in range(C):
        lab, line = json.loads(str(g["bp_label_json"][c])), json.loads(str(g["bp_line_json"][c]))
        fl = loader_ref.effective_flip(g["bp_draw"][c], g["bp_flip_on"][c], g["bp_is_valid"][c])
        for R in (256, 16):
            mine = loader_ref.bp_labels(lab, line, fl, R)
            assert same_bits(mine["lanes"], g["bp_lanes_R%d" % R][c]), (c, R)
            assert same_bits(mine["horizon"], g["bp_horizon_R%d" % R][c]), (c, R)
            assert same_bits(mine["valid_points"], g["bp_valid_points"][c]), c
            assert same_bits(mine["gt_line"], g["bp_gt_line"][c]), c
        assert g["bp_tuple_len"][c] == 7 + g["bp_is_valid"][c] and g["bp_idx"][c] == g["bp_file_number"][c] - 1


def test_restatement_reproduces_the_reference_bev(golden):
    g = golden
    for c in range(len(g["bev_draw"])):
        lab, line = json.loads(str(g["bev_label_json"][c])), json.loads(str(g["bev_line_json"][c]))
        fl = loader_ref.effective_flip(g["bev_draw"][c], g["bev_flip_on"][c], g["bev_is_valid"][c])
        mine = loader_ref.bev_labels(lab, line, fl)
        assert same_bits(mine["params"], g["bev_params"][c]), c          # (bits: the -0 of a flipped absent lane counts)
        assert same_bits(mine["gt_line"], g["bev_gt_line"][c]), c
        assert g["bev_tuple_len"][c] == 6 + g["bev_is_valid"][c] and g["bev_idx"][c] == g["bev_file_number"][c] - 1


@pytest.mark.parametrize("tree", ["bp", "bev"])
def test_split_tables_reproduce_idx_and_index(golden, tree):
    """``split_tables`` on the golden's listing: the file-number mapping of ``valid_idx``, membership and ``.index``."""
    from lanedetection_end2end_amd import loader
    count = {"bp": 3626, "bev": 2535}[tree]
    target_idx = sorted(range(1, count + 1), key=str)           # the lexicographic listing of 1.png .. count.png
    file_idx, is_valid, valid_pos, mapped = loader.split_tables(target_idx, [int(v) for v in golden[tree + "_valid_positions"]])
    pos = golden[tree + "_position"]
    assert np.array_equal(file_idx[pos], golden[tree + "_idx"]) and np.array_equal(is_valid[pos], golden[tree + "_is_valid"])
    assert np.array_equal(valid_pos[pos], golden[tree + "_index"]) and is_valid.sum() == len(mapped) == 15
    assert file_idx.dtype == np.int64 and is_valid.dtype == np.uint8 and valid_pos.dtype == np.int32


def test_golden_holds_the_situations_the_tests_rely_on(golden):
    g = golden
    for tree in ("bp", "bev"):
        flipped = (g[tree + "_draw"] > 0.5) & (g[tree + "_flip_on"] == 1) & (g[tree + "_is_valid"] == 0)
        assert flipped.any() and ((g[tree + "_is_valid"] == 0) & ~flipped).any()
        assert ((g[tree + "_is_valid"] == 1) & (g[tree + "_draw"] > 0.5)).any()
    S = np.array([len(json.loads(str(s))["h_samples"]) for s in g["bp_label_json"]])
    assert (S == 48).any() and (S == 56).any()
    assert os.path.getsize(os.path.join(GOLDEN, "loader.npz")) < 256 * 1024


# ------------------------------------------------------------------------------------------------------------ sampler and flips
class StubDataset:
    """Host-only stand-in: records the ``batch(sel, flip)`` calls."""
    device = "cpu"

    def __init__(self, valid_rows=()):
        self.valid_rows = frozenset(valid_rows)
        self.calls = []

    def batch(self, sel, flip=None, valid=False):
        self.calls.append((sel.tolist(), None if flip is None else flip.tolist(), valid))
        return sel, flip


class IndexDataset(torch.utils.data.Dataset):
    def __len__(self):
        return 10000

    def __getitem__(self, i):
        return i


@pytest.mark.parametrize("seed", range(5))
@pytest.mark.parametrize("indices,batch_size", [(list(range(3, 43)), 8), ([5, 900, 17, 3, 44, 2, 71, 8, 19, 23, 6], 4)])
def test_index_batches_are_the_dataloaders(seed, indices, batch_size):
    from lanedetection_end2end_amd.loader import ResidentLoader
    from torch.utils.data import DataLoader, SubsetRandomSampler
    torch.manual_seed(seed)
    ref_loader = DataLoader(IndexDataset(), batch_size=batch_size, sampler=SubsetRandomSampler(indices), num_workers=0)
    ref = [[b.tolist() for b in ref_loader] for _ in range(2)]              # two epochs on one generator
    after = torch.rand(1)
    stub = StubDataset()
    mine = ResidentLoader(stub, indices, batch_size, flip_on=True)
    assert len(mine) == len(ref_loader) == -(-len(indices) // batch_size)
    torch.manual_seed(seed)
    np.random.seed(seed)
    for epoch in range(2):
        stub.calls.clear()
        assert len(list(mine)) == len(ref[epoch])
        assert [c[0] for c in stub.calls] == ref[epoch]
        assert sorted(i for c in stub.calls for i in c[0]) == sorted(indices)
        if epoch == 0:
            flips = [f for c in stub.calls for f in c[1]]
    assert torch.equal(torch.rand(1), after)                                  # the default generator was consumed alike
    np.random.seed(seed)
    assert flips == (np.random.uniform(size=len(indices)) > 0.5).astype(np.uint8).tolist() and 0 < sum(flips) < len(flips)
    assert not any(c[2] for c in stub.calls)


def test_flip_draws_are_made_for_validation_and_with_flip_off():
    """The reference evaluates ``np.random.uniform(0.0, 1.0) > 0.5`` before ``and self.flip_on``, for every sample."""
    from lanedetection_end2end_amd.loader import ResidentLoader
    stub = StubDataset(valid_rows=range(8))
    np.random.seed(3)
    list(ResidentLoader(stub, list(range(8)), 4, flip_on=False))
    assert [c[1] for c in stub.calls] == [[0] * 4, [0] * 4] and all(c[2] for c in stub.calls)
    follow = np.random.uniform()
    np.random.seed(3)
    np.random.uniform(size=8)
    assert follow == np.random.uniform()
    with pytest.raises(ValueError):
        ResidentLoader(stub, [7, 8], 2, flip_on=True)                          # a training and a validation sample in one loader


def test_sequential_loader_and_drop_last():
    from lanedetection_end2end_amd.loader import ResidentLoader
    stub = StubDataset()
    mine = ResidentLoader(stub, [9, 4, 7, 1, 3], 2, flip_on=True, drop_last=True, shuffle=False)
    assert len(mine) == 2 and len(list(mine)) == 2
    assert [c[0] for c in stub.calls] == [[9, 4], [7, 1]]


# ------------------------------------------------------------------------------------------------------------------------ split
@pytest.mark.parametrize("num_train", [10, 37])
@pytest.mark.parametrize("shuffle", [True, False])
def test_get_loader_split_is_the_references(golden, monkeypatch, num_train, shuffle):
    """Against the split the REAL ``get_loader`` of each tree made (recorded by tools/gen_golden_loader.py: the samplers' index lists,
    the returned ``valid_idx``, the batches per epoch; batch 4, BP validation batch 2)."""
    from lanedetection_end2end_amd import loader
    made = []

    def fake_from_directory(cls, *args, **kwargs):
        made.append(kwargs)
        return StubDataset(valid_rows=kwargs["valid_idx"])

    monkeypatch.setattr(loader.ResidentDataset, "from_directory", classmethod(fake_from_directory))

    def want(tree, what):
        return golden["%s_split_n%d_s%d_%s" % (tree, num_train, shuffle, what)].tolist()

    np.random.seed(12345)                                   # whatever state the caller is in, the split seeds itself
    tl, vl, vi = loader.get_loader_bev(num_train, "params.json", "img", "gt", True, 4, shuffle, 8, True, 64)
    assert tl.indices == want("bev", "train") and vl.indices == want("bev", "valid") and vi == want("bev", "returned")
    assert [len(tl), len(vl)] == want("bev", "batches") and made[-1]["valid_idx"] == vi
    assert made[-1]["tree"] == "bev" and made[-1]["resize"] == 64 and all(type(i) is int for i in vi + tl.indices)
    tl, vl, vi = loader.get_loader_bp(num_train, "params.json", "lanes.json", "img", "gt", True, 4, 2, shuffle, 8, True, 64, 4)
    assert tl.indices == want("bp", "train") and vl.indices == want("bp", "valid") and vi == want("bp", "returned")
    assert [len(tl), len(vl)] == want("bp", "batches") and made[-1]["valid_idx"] == vi
    assert made[-1]["tree"] == "bp" and made[-1]["nclasses"] == 4
    vl.dataset.calls.clear()
    list(vl)                                                # the BP validation loader: in sequence, the short last batch dropped
    assert [i for c in vl.dataset.calls for i in c[0]] == vi[:len(vi) // 2 * 2] and all(c[2] for c in vl.dataset.calls)
    # hand-computed: 20 % of 10 unshuffled is [0, 1]; BEV cuts 8 / 2 samples to whole batches of 4, BP keeps them for drop_last
    if num_train == 10 and not shuffle:
        assert want("bev", "returned") == [] and want("bev", "train") == list(range(2, 10)) and want("bev", "batches") == [2, 0]
        assert want("bp", "returned") == [0, 1] and want("bp", "train") == list(range(2, 10)) and want("bp", "batches") == [2, 1]
    if num_train == 37:
        assert len(want("bev", "returned")) == 4 and len(want("bev", "train")) == 28 and len(want("bp", "returned")) == 7
        assert (sorted(want("bp", "train") + want("bp", "returned")) == list(range(37)))
        assert (want("bp", "returned") == list(range(7))) == (not shuffle)


def test_generator_draws_at_the_dataloaders_moments():
    """``iter()`` on two loaders before either is consumed: the base-seed draws happen at ``iter()``, the permutations at the
    first ``next()``, as with two DataLoaders."""
    from lanedetection_end2end_amd.loader import ResidentLoader
    from torch.utils.data import DataLoader, SubsetRandomSampler
    first, second = list(range(10, 30)), list(range(40, 52))
    torch.manual_seed(9)
    a = iter(DataLoader(IndexDataset(), batch_size=4, sampler=SubsetRandomSampler(first), num_workers=0))
    b = iter(DataLoader(IndexDataset(), batch_size=4, sampler=SubsetRandomSampler(second), num_workers=0))
    want_b, want_a = [t.tolist() for t in b], [t.tolist() for t in a]
    stub_a, stub_b = StubDataset(), StubDataset()
    torch.manual_seed(9)
    a, b = iter(ResidentLoader(stub_a, first, 4, True)), iter(ResidentLoader(stub_b, second, 4, True))
    list(b), list(a)
    assert [c[0] for c in stub_a.calls] == want_a and [c[0] for c in stub_b.calls] == want_b


# ------------------------------------------------------------------------------------------------------------ parse-time errors
def test_parse_time_errors():
    from lanedetection_end2end_amd import loader
    lines = [dict(lines=[-1, -1, 1, 0, 0, 0, 0, 1, -1, -1])]
    ok = dict(lanes=[[-2] * 48] * 4, h_samples=list(range(240, 720, 10)))
    t = loader.parse_bp_labels([ok], lines, [0])
    assert t["lanes"].shape == (1, 4, 56) and t["lanes"].dtype == np.int32 and t["h_count"][0] == 48
    assert t["h_samples"].dtype == np.float64 and t["lines"].dtype == np.int8
    with pytest.raises(ValueError, match="57 heights"):
        loader.parse_bp_labels([dict(lanes=[[-2] * 57] * 4, h_samples=list(range(57)))], lines, [0])
    with pytest.raises(ValueError, match="lane 2 has 47 points"):
        loader.parse_bp_labels([dict(lanes=[[-2] * 48, [-2] * 48, [-2] * 47, [-2] * 48], h_samples=ok["h_samples"])], lines, [0])
    with pytest.raises(ValueError, match="no int32"):           # the device table is integer: no silent truncation
        loader.parse_bp_labels([dict(lanes=[[-2] * 47 + [640.5]] + [[-2] * 48] * 3, h_samples=ok["h_samples"])], lines, [0])
    whole = loader.parse_bp_labels([dict(lanes=[[-2.0] * 47 + [640.0]] + [[-2] * 48] * 3, h_samples=ok["h_samples"])], lines, [0])
    assert whole["lanes"][0, 0, 55] == 640 and whole["lanes"].dtype == np.int32
    with pytest.raises(ValueError, match="poly_params"):
        loader.parse_bev_labels([dict(poly_params=[[0, 0, 0], [0, 0], [0, 0, 0], [0, 0, 0]])], lines, [0])
    with pytest.raises(ValueError, match="poly_params"):
        loader.parse_bev_labels([dict(poly_params=[[0, 0, 0]] * 3)], lines, [0])
    with pytest.raises(ValueError, match="lines"):
        loader.parse_bp_labels([ok], [dict(lines=[0] * 8)], [0])
    # fewer than 4 lanes: padded with absent lanes (documented deviation; the reference raises in np.hstack)
    three = loader.parse_bp_labels([dict(lanes=[[5] * 48] * 3, h_samples=ok["h_samples"])], lines, [0])
    assert (three["lanes"][0, :3, 8:] == 5).all() and (three["lanes"][0, 3] == -2).all() and (three["lanes"][0, :, :8] == -2).all()


def test_tables_carry_the_labels(golden):
    """The parsed tables hold what the kernel's statements need: the padded lanes and the label's own height count."""
    from lanedetection_end2end_amd import loader
    labs = [json.loads(str(s)) for s in golden["bp_label_json"]]
    lines = [json.loads(str(s)) for s in golden["bp_line_json"]]
    t = loader.parse_bp_labels(labs, lines, list(range(len(labs))))
    for m, lab in enumerate(labs):
        assert np.array_equal(t["lanes"][m], loader_ref.pad_lanes(lab["lanes"])) and t["h_count"][m] == len(lab["h_samples"])
        assert np.array_equal(t["h_samples"][m, :t["h_count"][m]], np.array(lab["h_samples"], np.float64))
        assert t["lines"][m].tolist() == lines[m]["lines"]


# ------------------------------------------------------------------------------------------------------------- directory listing
def test_from_directory_listing(tmp_path):
    from PIL import Image
    from lanedetection_end2end_amd.loader import ResidentDataset
    rng = np.random.default_rng(0)
    img_dir, gt_dir = tmp_path / "img", tmp_path / "gt"
    img_dir.mkdir(), gt_dir.mkdir()
    frames, maps = {}, {}
    for number in (1, 2, 10, 7):
        frames[number] = rng.integers(0, 256, (6, 8, 3), dtype=np.uint8)
        maps[number] = rng.integers(0, 5, (6, 8), dtype=np.uint8)
        Image.fromarray(frames[number]).save(str(img_dir / ("%d.png" % number)))
        im = Image.frombytes("P", (8, 6), maps[number].tobytes())
        im.putpalette([v for i in range(256) for v in (i, i, i)])
        im.save(str(gt_dir / ("%d.png" % number)))
    lines = tmp_path / "label_new.json"
    lines.write_text("".join(json.dumps(dict(lines=[k % 3 - 1] * 10)) + "\n" for k in range(10)))
    params = tmp_path / "Curve_parameters.json"
    params.write_text("".join(json.dumps(dict(poly_params=[[0.0, 0.5, float(k)]] * 4)) + "\n" for k in range(10)))
    lanes = tmp_path / "lanes_ordered.json"
    lanes.write_text("".join(json.dumps(dict(lanes=[[k + 1] * 48] * 4, h_samples=list(range(240, 720, 10)))) + "\n" for k in range(10)))
    got = ResidentDataset.from_directory(str(img_dir), str(gt_dir), str(params), None, str(lines), tree="bev", valid_idx=[1, 3],
                                         decode_only=True, threads=64)
    assert got["file_numbers"] == [1, 10, 2, 7]                 # sorted listing, lexicographic like the reference's
    assert got["valid_idx"] == [9, 6]                           # positions mapped through target_idx[i] - 1
    for row, number in enumerate(got["file_numbers"]):
        assert np.array_equal(got["frames"][row], frames[number]) and np.array_equal(got["labels"][row], maps[number])
        assert got["tables"]["params"][row, 0, 2] == number - 1 and got["tables"]["lines"][row, 0] == (number - 1) % 3 - 1
    assert got["frames"].dtype == np.uint8 and got["frames"].shape == (4, 6, 8, 3) and got["labels"].shape == (4, 6, 8)
    bp = ResidentDataset.from_directory(str(img_dir), str(gt_dir), str(params), str(lanes), str(lines), tree="bp", decode_only=True)
    assert [int(v) for v in bp["tables"]["lanes"][:, 0, 55]] == [1, 10, 2, 7] and bp["valid_idx"] == []
    # mismatching stems / counts raise
    os.rename(str(gt_dir / "7.png"), str(gt_dir / "8.png"))
    with pytest.raises(ValueError, match="do not match"):
        ResidentDataset.from_directory(str(img_dir), str(gt_dir), str(params), None, str(lines), tree="bev", decode_only=True)
    os.remove(str(gt_dir / "8.png"))
    with pytest.raises(ValueError, match="4 images"):
        ResidentDataset.from_directory(str(img_dir), str(gt_dir), str(params), None, str(lines), tree="bev", decode_only=True)


# ---------------------------------------------------------------------------------------------------------------------- surface
def test_loader_imports_and_surface():
    path = os.path.join(ROOT, "lanedetection_end2end_amd", "loader.py")
    tree = ast.parse(open(path).read())
    names = []
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            names += [a.name for a in node.names]
        elif isinstance(node, ast.ImportFrom):
            names.append(("." * node.level) + (node.module or ""))
    assert names and not any(n.split(".")[0] in ("oracle", "torchvision", "cv2", "Dataloader", "Networks") or "_refpath" in n
                             for n in names), names
    import inspect
    from lanedetection_end2end_amd import _lib, loader
    assert list(inspect.signature(loader.get_loader_bev).parameters)[:11] == [
        "num_train", "json_file", "image_dir", "gt_dir", "flip_on", "batch_size", "shuffle", "num_workers", "end_to_end", "resize",
        "split_percentage"]
    assert list(inspect.signature(loader.get_loader_bp).parameters)[:14] == [
        "num_train", "json_file", "lanes_file", "image_dir", "gt_dir", "flip_on", "batch_size", "val_batch_size", "shuffle",
        "num_workers", "end_to_end", "resize", "nclasses", "split_percentage"]
    lib = _lib.load()
    assert hasattr(lib, "lf_label_batch_bp") and hasattr(lib, "lf_label_batch_bev") and lib.lf_abi_version() == 5
    header = open(os.path.join(ROOT, "include", "lanefit.h")).read()
    assert "lf_label_batch_bp" in header and "lf_label_batch_bev" in header and "#define LF_ABI_VERSION 5" in header
    assert "lanedetection_end2end_amd.loader import get_loader_bp as get_loader" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
