"""lanedetection_end2end_amd -- MI355X-native hot path of LaneDetection_End2End.

ERFNet backbone -> differentiable weighted-least-squares lane fit -> area / back-projection /
segmentation losses, forward and backward, as hand-written HIP kernels for gfx950 behind the C ABI
of include/lanefit.h.  ``bev`` and ``bp`` mirror the reference's two source trees module by module
so that its own main.py can import them unchanged.
"""
from . import _lib  # noqa: F401

__all__ = ["bev", "bp", "fit", "losses", "erfnet", "lsq", "geometry", "ops", "use_inference_engine"]


def use_inference_engine(module, on=True):
    """Set ``inference_engine`` on every lanefit ERFNet and every ``--clas`` head inside ``module`` (the module itself, or e.g. the
    LSQ ``Net`` with its ``.net``, ``.line_classification`` and ``.horizon_estimation``): their eval-mode forwards under
    ``torch.no_grad()`` / ``torch.inference_mode()`` then run the forward-only engine -- the whole network (``lf_erfnet_infer``),
    block-level calls (``lf_erfnet_infer_range``) and the heads' trunk (``lf_convchain_infer``).  Returns ``module``."""
    from .clas import Classification
    from .erfnet import Net
    for m in module.modules():
        if isinstance(m, (Net, Classification)):
            m.inference_engine = bool(on)
    return module
