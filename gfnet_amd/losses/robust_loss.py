"""losses/robust_loss.py of the reference: `get_gt_warp_homography` and `RobustLosses`, on csrc/robust_loss.hip.

The module takes what `GFNet.forward` / `forward_pyramids` return in training mode and a batch with `H_s2t`, `im_A` and `im_B`, as
trainer/train.py:29-33 hands them over.  One forward launch pair and one backward launch per scale, no host synchronisation: the
ground-truth warp is recomputed per cell and never stored.  What the reference sends to wandb (:75, :89) is left in
`RobustLosses.last_losses` instead, as 0-dim device tensors under the reference's key names.  There is no CPU path.
"""
import torch
import torch.nn as nn

from .. import _lib, ops


def _extent(img, what):
    if not hasattr(img, "shape") or len(img.shape) != 4:
        raise ValueError(f"{what} must be a (B,C,H,W) image batch (only its height is read)")
    return int(img.shape[2]) - 1


def get_gt_warp_homography(H_s2t, img_src, img_tgt, H, W, im_A_coords=None, normalized=True, return_x1_n=False):
    """robust_loss.py:9-42: the ground-truth warp of an H x W grid of cells of img_src into img_tgt under the homographies H_s2t
    (B,3,3).  Returns (x2_n, prob), or (x1_n, x2_n, prob) with return_x1_n, or (x2, prob) in pixels when not normalized; x2_n / x2 /
    x1_n are (B,H,W,2), prob (B,H,W).  As in the reference the image HEIGHT scales both axes."""
    out, prob, x1n = ops.gt_warp_homography(H_s2t, int(H), int(W), _extent(img_src, "img_src"), _extent(img_tgt, "img_tgt"),
                                            im_A_coords=im_A_coords, normalized=normalized, return_x1_n=normalized and return_x1_n)
    if normalized and return_x1_n:
        return x1n, out, prob
    return out, prob


class RobustLosses(nn.Module):
    """robust_loss.py:44-128 with the same constructor and defaults.  `depth_interpolation_mode` is stored and, as in the reference,
    never read."""

    def __init__(self, ce_weight=0.01, local_dist=None, local_largest_scale=8, depth_interpolation_mode="bilinear", alpha=1., c=1e-3,
                 iteration_base=0.85):
        super().__init__()
        self.ce_weight = ce_weight
        self.local_dist = local_dist
        self.local_largest_scale = local_largest_scale
        self.depth_interpolation_mode = depth_interpolation_mode
        self.alpha = alpha
        self.c = c
        self.iteration_base = iteration_base
        self.last_losses = {}

    def forward(self, corresps, batch):
        scales, maps, names, grid = [], [], [], None
        for key, per_itr in corresps.items():
            gm = key == "gm"                                      # the global matcher's output counts as scale 16 (:110-111)
            scale = 16 if gm else int(key)
            itrs = sorted(per_itr.keys())
            n = len(itrs)
            if n > _lib.RL_MAX_ITR:
                raise ValueError(f"RobustLosses: scale {key} has {n} iterations, at most {_lib.RL_MAX_ITR} are supported")
            if itrs != list(range(1, n + 1)):
                raise ValueError(f"RobustLosses: scale {key}: iterations must be numbered 1..n, got {itrs}")
            flows = [per_itr[k]["flow"] for k in itrs]
            certs = [per_itr[k]["certainty"] for k in itrs]
            grid = tuple(flows[0].shape[-2:])
            for k, (f, ct) in enumerate(zip(flows, certs)):
                if f.dim() != 4 or ct.dim() != 4 or f.shape[1] != 2 or ct.shape[1] != 1 or f.shape[0] != ct.shape[0] \
                        or tuple(f.shape[-2:]) != grid or tuple(ct.shape[-2:]) != grid:
                    raise ValueError(f"RobustLosses: scale {key}, iteration {k + 1}: flow {tuple(f.shape)} and certainty {tuple(ct.shape)} "
                                     f"must be (B,2,h,w) and (B,1,h,w) on the scale's {grid} grid")
            narrowed = (not gm) and self.local_largest_scale >= scale
            thresh = 0.0
            if narrowed:
                if not scales:
                    raise ValueError(f"RobustLosses: scale {key} comes first but local_largest_scale = {self.local_largest_scale} narrows "
                                     "its mask by the previous scale's end-point error, which does not exist")
                if self.local_dist is None or scale not in self.local_dist:
                    raise ValueError(f"RobustLosses: local_largest_scale = {self.local_largest_scale} narrows scale {scale}, "
                                     "local_dist has no entry for it")
                thresh = (2 / 448) * (self.local_dist[scale] * scale)                                   # :120
            a = self.alpha[scale] if isinstance(self.alpha, dict) else self.alpha                       # :68
            scales.append({"n": n, "a": float(a), "cs": float(self.c * scale), "pck": 0.5 * (2 / (448. / scale)),   # :69, :73-74
                           "narrowed": narrowed, "prev_thresh": float(thresh)})
            maps += flows + certs
            names.append(("gm" if gm else "delta", scale))
        if not scales:
            raise ValueError("RobustLosses: corresps is empty")
        _lib.require_gpu(batch["H_s2t"], *maps)
        loss, stats = ops.robust_loss(scales, batch["H_s2t"], _extent(batch["im_A"], "batch['im_A']"), _extent(batch["im_B"], "batch['im_B']"),
                                      self.ce_weight, self.iteration_base, maps)
        self.last_losses = {}
        for i, (mode, scale) in enumerate(names):
            self.last_losses[f"{mode}_certainty_loss_{scale}"] = stats[i, _lib.RL_STAT_CE]
            self.last_losses[f"{mode}_regression_loss_{scale}"] = stats[i, _lib.RL_STAT_REG]
            self.last_losses[f"train_pck_05_scale_{scale}"] = stats[i, _lib.RL_STAT_PCK]
        return loss
