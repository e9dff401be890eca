"""``Dataloader.Load_Data_new`` of the BEV tree: ``write_lsq_results`` (BEV/Dataloader/Load_Data_new.py:334-420) with the
reference's signature, decoding on the device (``ProjectionsBEV.decode_lanes``, ``lf_lane_decode_bev``).

The data loading itself (``get_loader``, ``LaneDataset``, ``get_homography``, ``load_valid_set_file*``, ...) is not replaced.  This
package precedes the reference's ``Dataloader`` on ``sys.path`` under tools/run_reference_main.py, so with LANEFIT_REFERENCE_ROOT
set the reference's file is loaded under a private module name and every public name this module does not define is re-exported
from it; without the variable only ``write_lsq_results`` exists here."""
import json

import torch

from lanedetection_end2end_amd import _lib
from lanedetection_end2end_amd._refpath import load_reference_module as _load_reference_module
from lanedetection_end2end_amd.clas import MAX_LANES, LaneLabels, ProjectionsBEV

__all__ = ["write_lsq_results"]


def write_lsq_results(src_file, dst_file, nclasses, all_branches_ready, horizon_on, resize, no_ortho, calc_intersection=False,
                      draw_image=False, path_test_set='../../../', test_phase=False):
    """Computes json file with point coordinates for every lane: every line of ``src_file`` -- a label with the model's ``params``,
    ``line_id`` and ``horizon_est`` -- is written to ``dst_file`` with all its keys, ``lanes`` replaced by ``nclasses`` rows of
    decoded x coordinates and ``run_time`` set to 20.  The file is parsed once and decoded in one launch and one read per distinct
    number of sample heights (one in a TuSimple file).  Not provided (``NotImplementedError``): ``calc_intersection`` (the
    reference calls a function no file defines), ``draw_image`` (it draws on the frames on disk) and ``test_phase``."""
    for name, value in (("calc_intersection", calc_intersection), ("draw_image", draw_image), ("test_phase", test_phase)):
        if value:
            raise NotImplementedError("lanefit write_lsq_results does not provide %s=True" % name)
    lines = [json.loads(line) for line in open(src_file).readlines()]
    groups = {}
    for i, line in enumerate(lines):
        params, _, _ = line["params"], line["line_id"], line["horizon_est"]            # (KeyError as in the reference)
        if any(len(p) > 3 for p in params):
            raise ValueError("too many values to unpack (expected 3): a lane of label %d has more than three coefficients" % i)
        if len(params) > min(nclasses, MAX_LANES):
            raise IndexError("label %d has %d lanes of params for %d rows" % (i, len(params), min(nclasses, MAX_LANES)))
        groups.setdefault((len(line["h_samples"]), len(params), len(line["horizon_est"])), []).append(i)
    if lines and not torch.cuda.is_available():
        raise _lib.LaneFitLibraryError("lanefit write_lsq_results decodes on the MI355X; there is no CPU path")
    decoded = [None] * len(lines)
    proj = ProjectionsBEV(_Options(resize, nclasses))
    for (S, L, R), members in groups.items():
        rows = [lines[i] for i in members]
        if L == 0:
            for i in members:
                decoded[i] = [[-2] * S for _ in range(nclasses)]
            continue
        dev = torch.device("cuda", torch.cuda.current_device())
        beta = torch.tensor([[[0.] * (3 - len(p)) + list(p) for p in l["params"]] for l in rows], dtype=torch.float64).to(dev)
        line_id = torch.tensor([l["line_id"] for l in rows], dtype=torch.int32).to(dev)
        horizon = torch.tensor([l["horizon_est"] for l in rows], dtype=torch.float32).reshape(len(rows), R).to(dev)
        lanes, _ = proj.decode_lanes([beta[:, j, :, None] for j in range(L)], LaneLabels(rows), line_pred=line_id, horizon_pred=horizon,
                                     all_branches_ready=all_branches_ready, horizon_on=horizon_on, no_ortho=no_ortho)
        for i, rows_i in zip(members, lanes.cpu().tolist()):
            decoded[i] = rows_i
    with open(dst_file, 'w') as jsonFile:
        for line, lanes in zip(lines, decoded):
            json_line = line
            json_line["run_time"] = 20
            json_line["lanes"] = lanes
            json.dump(json_line, jsonFile)
            jsonFile.write('\n')


class _Options:
    def __init__(self, resize, nclasses):
        self.resize, self.nclasses = resize, nclasses


_reference = _load_reference_module("Birds_Eye_View_Loss", "Dataloader/Load_Data_new.py", "_lanefit_reference_bev_Load_Data_new")
if _reference is not None:
    for _name in dir(_reference):
        if not _name.startswith("_") and _name not in globals():
            globals()[_name] = getattr(_reference, _name)
            __all__.append(_name)
