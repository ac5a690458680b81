"""The reference's `initial_transforms` (train.py:74-79 online datasets, :88-93 glunet) on the device: Resize(640), ColorJitter,
RandomGrayscale, RandomGaussianBlur (datasets/homography_dataset_large_size.py:17-28) and ToTensor for a batch of decoded uint8 images.
`draw_photometric` makes the random draws on the host in the reference's order, `PhotometricAugment` is the batched transform
(ops.photo_augment, csrc/photometric.hip) and `reference_photometric` the same chain through Pillow on the CPU, the tests' oracle.
Pinned against Pillow (12.2.0), which is what torchvision's PIL backend executes; not against torchvision itself."""
import random

import numpy as np
import torch

from .. import ops


def _jitter_range(value, name, centre=1.0, bound=(0.0, float("inf")), clip_first_on_zero=True):
    """ColorJitter._check_input: a scalar v means [centre - v, centre + v] (the lower end clipped at 0 for the three factors), a pair
    is taken as it is; None, or a range that is only the centre, switches the op off."""
    if value is None:
        return None
    if isinstance(value, (int, float)):
        if value < 0:
            raise ValueError(f"{name}: a single number must be non negative, got {value}")
        value = [centre - float(value), centre + float(value)]
        if clip_first_on_zero:
            value[0] = max(value[0], 0.0)
    else:
        value = [float(value[0]), float(value[1])]
    if not bound[0] <= value[0] <= value[1] <= bound[1]:
        raise ValueError(f"{name}: values should be between {bound}, got {value}")
    return None if value[0] == value[1] == centre else (value[0], value[1])


def jitter_ranges(brightness, contrast, saturation, hue):
    return (_jitter_range(brightness, "brightness"), _jitter_range(contrast, "contrast"), _jitter_range(saturation, "saturation"),
            _jitter_range(hue, "hue", centre=0.0, bound=(-0.5, 0.5), clip_first_on_zero=False))


def draw_photometric(n, brightness=0.2, contrast=0.2, saturation=0.2, hue=0.2, grayscale_p=0.0, blur_p=0.5, blur_radius=(0.1, 2.0),
                     generator=None, rng=None):
    """The random draws of n images, image by image, as the reference's transforms make them: ColorJitter.get_params'
    torch.randperm(4), then torch.empty(1).uniform_(lo, hi) for each enabled op of brightness, contrast, saturation, hue in that
    order; RandomGrayscale's torch.rand(1) < grayscale_p when grayscale_p > 0; RandomGaussianBlur's random.random() < blur_p and,
    when that holds, random.uniform(*blur_radius).  The torch draws come from `generator` (None: the global one), the others from
    `rng`, a random.Random (None: the random module).  Returns a list of n dicts as ops.photo_augment takes them."""
    ranges = jitter_ranges(brightness, contrast, saturation, hue)
    rng = random if rng is None else rng
    params = []
    for _ in range(n):
        p = {"order": torch.randperm(4, generator=generator).tolist()}
        for name, r in zip(ops.PHOTO_OPS, ranges):
            p[name] = None if r is None else float(torch.empty(1).uniform_(r[0], r[1], generator=generator))
        p["grayscale"] = bool(torch.rand(1, generator=generator) < grayscale_p) if grayscale_p > 0 else False
        p["blur_radius"] = rng.uniform(blur_radius[0], blur_radius[1]) if rng.random() < blur_p else None
        params.append(p)
    return params


class PhotometricAugment:
    """A list of decoded (h,w,3) uint8 images (host or device), or one (N,h,w,3) tensor -> a list of (3,h',w') float32 device tensors
    in [0,1]: what the reference's `initial_transforms` leave.  For device images whose rows are dense or evenly strided the whole
    batch is one table upload and at most three launches, without a host synchronisation; a host image costs its own copy to the
    device first, any other view a copy of its own.  The defaults are the online datasets' preset (train.py:74-79); the glunet one (:88-93) is
    PhotometricAugment(resize=None, brightness=0.6, contrast=0.6, saturation=0.6, hue=0.2, grayscale_p=0.2)."""

    def __init__(self, resize=640, brightness=0.2, contrast=0.2, saturation=0.2, hue=0.2, grayscale_p=0.0, blur_p=0.5,
                 blur_radius=(0.1, 2.0), generator=None, rng=None, device="cuda"):
        jitter_ranges(brightness, contrast, saturation, hue)  # (refuses bad ranges here, not at the first batch)
        self.resize = None if resize is None else int(resize)
        self.jitter = dict(brightness=brightness, contrast=contrast, saturation=saturation, hue=hue)
        self.grayscale_p, self.blur_p, self.blur_radius = float(grayscale_p), float(blur_p), (float(blur_radius[0]), float(blur_radius[1]))
        self.generator, self.rng, self.device = generator, rng, torch.device(device)

    def draw(self, n):
        return draw_photometric(n, **self.jitter, grayscale_p=self.grayscale_p, blur_p=self.blur_p, blur_radius=self.blur_radius,
                                generator=self.generator, rng=self.rng)

    def __call__(self, images):
        images = list(images.unbind(0)) if isinstance(images, torch.Tensor) else list(images)
        images = [t.to(self.device) for t in images]
        return ops.photo_augment(images, self.draw(len(images)), out="float", resize=self.resize)


def reference_photometric(image_u8, params, resize=None):
    """One image through Pillow on the CPU, driven as torchvision's PIL backend drives it: image_u8 (h,w,3) uint8 (tensor or array),
    params one dict of draw_photometric, resize an int or None.  Returns the (h',w',3) uint8 array; ToTensor is `/ 255`."""
    from PIL import Image, ImageEnhance, ImageFilter

    arr = image_u8.cpu().numpy() if isinstance(image_u8, torch.Tensor) else np.asarray(image_u8)
    img = Image.fromarray(np.ascontiguousarray(arr, dtype=np.uint8))
    if resize is not None:
        h, w = ops.resize_output_size(img.size[1], img.size[0], int(resize))
        if (h, w) != (img.size[1], img.size[0]):
            img = img.resize((w, h), Image.BILINEAR)
    for op in params.get("order", (0, 1, 2, 3)):
        factor = params.get(ops.PHOTO_OPS[op])
        if factor is None:
            continue
        if op == 0:
            img = ImageEnhance.Brightness(img).enhance(factor)
        elif op == 1:
            img = ImageEnhance.Contrast(img).enhance(factor)
        elif op == 2:
            img = ImageEnhance.Color(img).enhance(factor)
        else:  # adjust_hue
            h, s, v = img.convert("HSV").split()
            np_h = np.array(h, dtype=np.uint8)
            np_h = ((np_h.astype(np.int32) + (int(factor * 255) & 255)) & 255).astype(np.uint8)
            img = Image.merge("HSV", (Image.fromarray(np_h), s, v)).convert("RGB")
    if params.get("grayscale"):
        grey = np.array(img.convert("L"), dtype=np.uint8)
        img = Image.fromarray(np.dstack([grey, grey, grey]))
    if params.get("blur_radius"):
        img = img.filter(ImageFilter.GaussianBlur(params["blur_radius"]))
    return np.array(img)
