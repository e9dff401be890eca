"""``Networks.LSQ_layer`` of the BP tree (BP/Networks/LSQ_layer.py): same public names."""
import torch

from lanedetection_end2end_amd import geometry, ops
from lanedetection_end2end_amd.clas import Classification  # noqa: F401
from lanedetection_end2end_amd.fit import WeightedLeastSquares
from lanedetection_end2end_amd.geometry import get_homography  # noqa: F401
from lanedetection_end2end_amd.lsq import BPNet as Net, activation_layer  # noqa: F401


def ProjectiveGridGenerator(size, theta, no_cuda):
    """(N, H*W, 2) pixel-coordinate grid -- BP/Networks/LSQ_layer.py:50-68.  One gradient-free matrix for the whole batch gives
    the host-made grid; a per-image theta or one that requires a gradient runs ``lf_theta_grid`` and is differentiable."""
    N, C, H, W = size
    grid = geometry.constant_grid(theta, H, W, False, no_cuda)
    if grid is None:
        return ops.theta_grid(theta, H, W, False)
    return grid[1].unsqueeze(0).expand(N, -1, -1)


class Weighted_least_squares(WeightedLeastSquares):
    """BP flavour: y = 255 - grid_y, orders 0..3, fp64 betas (BP/Networks/LSQ_layer.py:72-154)."""
    y_offset = 255.0
    max_order = 3
    out_dtype = torch.float64
    cholesky_drops_reg = True    # the --use_cholesky branch is GELS.apply(Y0, W*x): no regulariser (BP/Networks/LSQ_layer.py:112-119, gels.py)
