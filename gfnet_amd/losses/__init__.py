"""The reference's training objective (losses/robust_loss.py) on this package's HIP kernels."""
from .robust_loss import RobustLosses, get_gt_warp_homography  # noqa: F401
