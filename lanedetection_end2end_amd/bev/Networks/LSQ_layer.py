"""``Networks.LSQ_layer`` of the BEV tree (BEV/Networks/LSQ_layer.py): same public names."""
import torch
import torch.nn as nn

from lanedetection_end2end_amd import geometry, ops
from lanedetection_end2end_amd.clas import ClassificationBEV as Classification  # noqa: F401  (four 3-way line heads, :198-205)
from lanedetection_end2end_amd.fit import WeightedLeastSquares
from lanedetection_end2end_amd.lsq import BEVNet as Net, activation_layer  # noqa: F401


def Init_Projective_transform(nclasses, batch_size, resize):
    """(size, M, M_inv) with M expanded to (batch,3,3) fp32 -- LSQ_layer.py:17-32."""
    size = torch.Size([batch_size, nclasses, resize, 2 * resize])
    M, M_inv = geometry.bev_homography()
    ex = lambda m: torch.from_numpy(m).unsqueeze(0).expand(batch_size, 3, 3).float()
    return size, ex(M), ex(M_inv)


class ProjectiveGridGenerator(nn.Module):
    """forward(theta) -> (N, H*W, 2) grid (LSQ_layer.py:66-87), for the theta it is called with.

    One gradient-free matrix for the whole batch -- the reference's own use -- gives the grid made on the host with the
    reference's fp32 ops, kept until a different matrix arrives.  A theta that differs per image or requires a gradient runs
    ``lf_theta_grid`` on the device; its backward carries the grid's gradient to theta."""

    def __init__(self, size, theta, no_cuda=False):
        super().__init__()
        self.N, self.C, self.H, self.W = size
        self.no_cuda = no_cuda
        self._cache = None          # (theta[0] the grid was made from, grid)

    def forward(self, theta):
        grid = geometry.constant_grid(theta, self.H, self.W, True, self.no_cuda, self._cache)
        if grid is None:
            return ops.theta_grid(theta, self.H, self.W, True)
        self._cache = grid
        return grid[1].unsqueeze(0).expand(self.N, -1, -1)


class Weighted_least_squares(WeightedLeastSquares):
    """BEV flavour: y = 1 - grid_y, orders 0..2, fp32 betas (LSQ_layer.py:90-167)."""
    y_offset = 1.0
    max_order = 2
    out_dtype = torch.float32
