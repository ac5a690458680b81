"""The online pair synthesis of the reference's HomographyDataset (datasets/homography_dataset_large_size.py:148-228), batched on the
device: `PairSynthesizer` is the train branch (:168-185) -- after `initial_transforms`, or with a `PhotometricAugment`
(datasets/photometric.py) from the decoded uint8 pixels on -- and `val_pair` the val branch's H rescale and warped image (:203-207).
File lists, image decoding and the offline `glunet` branch's masks are out of scope."""
import random

import torch

from .. import ops
from .generate_random_H_large_size import draw_random_h, pre_resize


class PairSynthesizer:
    """Two lists of (3,h,w) images in [0,1] (host or device; what the reference's `initial_transforms` leaves) -> the batch dict a
    training step consumes, {"im_A", "im_B", "H_s2t"}, on the device: im_A is the imgs0 image under its random homography, im_B the
    imgs1 image under its own (the plain centre crop with bi=False), H_s2t (B,3,3) float32 maps im_A pixels to im_B pixels.

    input_resolution: int or (h, w); crop_size = int(input_resolution[0] / (1 - ratio)) (:175) and deform_area = int(crop_size *
    ratio) (generate_random_H_large_size.py:57), with one ratio drawn from deformation_ratio per call (the reference draws one per
    sample; its default list has one entry).  An image that does not hold the crop is first resized as :45-48 resize it.  The
    random integers come from `generator` (None: torch's global generator) in the reference's order.

    photometric: None, or a PhotometricAugment; the two lists then hold decoded (h,w,3) uint8 images, which it augments first, in
    the order imgs0[0], imgs1[0], imgs0[1], ... in which __getitem__ (:168) passes them through `initial_transforms`."""

    def __init__(self, input_resolution, deformation_ratio=(0.3,), bi=True, normalize=True, generator=None, return_warped=False,
                 device="cuda", photometric=None):
        res = (int(input_resolution),) * 2 if isinstance(input_resolution, int) else tuple(int(v) for v in input_resolution)
        if len(res) != 2 or min(res) < 2:
            raise ValueError(f"PairSynthesizer: input_resolution must be an int or an (h, w) pair, got {input_resolution!r}")
        self.input_resolution, self.deformation_ratio = res, [float(r) for r in deformation_ratio]
        if not self.deformation_ratio or not all(0.0 < r < 1.0 for r in self.deformation_ratio):
            raise ValueError(f"PairSynthesizer: deformation ratios must lie in (0, 1), got {deformation_ratio!r}")
        self.bi, self.normalize, self.generator, self.return_warped = bool(bi), bool(normalize), generator, bool(return_warped)
        self.device, self.photometric = torch.device(device), photometric

    def __call__(self, imgs0, imgs1):
        if len(imgs0) != len(imgs1) or not len(imgs0):
            raise ValueError(f"PairSynthesizer: {len(imgs0)} and {len(imgs1)} images")
        if self.photometric is not None:                                                            # :168
            both = self.photometric([t for pair in zip(imgs0, imgs1) for t in pair])
            imgs0, imgs1 = both[0::2], both[1::2]
        ratio = float(random.sample(self.deformation_ratio, 1)[0])                                  # :174
        crop_size = int(self.input_resolution[0] / (1 - ratio))                                     # :175
        a = [pre_resize(t.to(self.device, torch.float32), crop_size) for t in imgs0]
        b = [pre_resize(t.to(self.device, torch.float32), crop_size) for t in imgs1]
        draws = draw_random_h(len(a), [t.shape[2] for t in a], [t.shape[1] for t in a], crop_size, int(crop_size * ratio), self.generator)
        out = ops.random_h_batch(a, b, draws, crop_size, self.input_resolution, ratio, self.bi, self.normalize, self.return_warped)
        batch = {"im_A": out["im_A"], "im_B": out["im_B"], "H_s2t": out["H_s2t"]}
        if self.return_warped:
            batch["warped_img1"] = out["warped_img1"]
        return batch


def val_pair(img0, img1, H, res):
    """The val branch for one pair of (3,h,w) images in [0,1] and the H_s2t of their files: both resized to res x res (bicubic on
    the tensor, not normalised), H_s2t rescaled as :203-205 -- diag(res / w1, res / h1, 1) H diag(res / w0, res / h0, 1)^-1, in
    float64 -- and warped_img1 = warp_perspective(img0, H_s2t^-1, (res, res)) (:207), i.e. pixel p reads img0 at H_s2t p.  Returns
    {"im_A": img1, "im_B": img0, "H_s2t" (3,3) float32, "warped_img1"} on the device."""
    dev = ops.require_gpu(img0, img1)
    res = int(res)
    (_, h0, w0), (_, h1, w1) = img0.shape, img1.shape
    unit = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    im0 = ops.resize_normalise(img0[None], (res, res), "bicubic", *unit)
    im1 = ops.resize_normalise(img1[None], (res, res), "bicubic", *unit)
    H64 = torch.as_tensor(H).to(device=dev, dtype=torch.float64).reshape(3, 3)
    left = torch.tensor([res / w1, res / h1, 1.0], dtype=torch.float64, device=dev)
    right = torch.tensor([res / w0, res / h0, 1.0], dtype=torch.float64, device=dev)
    H_s2t = (left[:, None] * H64) * (1.0 / right)[None, :]
    warped = ops._warp(im0, H_s2t[None].contiguous(), False, (res, res), what="val_pair")
    return {"im_A": im1[0], "im_B": im0[0], "H_s2t": H_s2t.float(), "warped_img1": warped[0]}
