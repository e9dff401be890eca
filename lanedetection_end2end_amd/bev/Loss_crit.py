"""``Loss_crit`` of the BEV tree (BEV/Loss_crit.py): same public names."""
from lanedetection_end2end_amd.losses import Area_Loss, CrossEntropyLoss2d, MSE_Loss, polynomial  # noqa: F401
from lanedetection_end2end_amd.losses import define_loss_crit_bev as define_loss_crit  # noqa: F401
from lanedetection_end2end_amd.losses import StepCriterion, StepLoss  # noqa: F401  (the whole step's criterion as one launch)
from lanedetection_end2end_amd.losses import SegStepCriterion, SegStepLoss  # noqa: F401  (the segmentation-mode step in one pass over the logits)
