"""Writes tests/golden/photometric_*.npz: small uint8 images, photometric parameters and what Pillow makes of them, through
gfnet_amd.datasets.reference_photometric (Image.resize, ImageEnhance, the HSV round trip, convert("L"), ImageFilter.GaussianBlur).
The GPU tests read these files, so that they need no Pillow.  Run: python tests/golden/make_golden_photometric.py  (needs Pillow;
the goldens in the tree were written with Pillow 12.2.0)."""
import itertools
import json
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

SIZES = ((70, 45), (41, 83), (5, 3), (1, 9))        # (h, w): 3 x 1 and 2 x 2 tiles of 32 rows x 64 columns with ragged edges; smaller
                                                    # than the blur's halo; a single row
BLEND_FACTORS = (0.4, 0.8, 1.0, 1.2, 1.6)
BLUR_RADII = (0.1, 0.7, 1.0, 1.5, 2.0)
HUE_FACTORS = (0.2, -0.2, 0.07, 0.5, -0.5)
RESIZE_INPUT, RESIZE_SIZES = (97, 131), (48, 64, 150, 97)
PALETTE = ((0, 0, 0), (255, 255, 255), (128, 128, 128), (255, 0, 0), (0, 255, 0), (0, 0, 255))


def make_image(h, w, seed):
    """Smooth colour, a block of uint8 noise, flat black / white / mid-grey blocks (max == min, S == 0) and saturated primaries."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([xx * 255 // max(w - 1, 1), yy * 255 // max(h - 1, 1), (xx + yy) * 255 // max(h + w - 2, 1)], -1).astype(np.uint8)
    if h < 8 or w < 8:                              # too small for blocks: the same content pixel by pixel
        flat = img.reshape(-1, 3)
        for k in range(len(flat)):
            if k % 9 < 6:
                flat[k] = PALETTE[k % 9]
            elif k % 9 < 8:
                flat[k] = rng.integers(0, 256, 3)
        return flat.reshape(h, w, 3)
    img[h // 4:h // 2, w // 4:] = rng.integers(0, 256, (h // 2 - h // 4, w - w // 4, 3))
    edges = np.linspace(0, w, len(PALETTE) + 1).astype(int)
    for k, colour in enumerate(PALETTE):
        img[2 * h // 3:, edges[k]:edges[k + 1]] = colour
    return img


def off():
    return {"order": [0, 1, 2, 3], "brightness": None, "contrast": None, "saturation": None, "hue": None, "grayscale": False,
            "blur_radius": None}


def stage_cases():
    """One op per case: name -> parameters"""
    cases = {"grey": dict(off(), grayscale=True), "none": off()}
    for op in ("brightness", "contrast", "saturation"):
        for f in BLEND_FACTORS:
            cases[f"{op}_{f}"] = dict(off(), **{op: f})
    for rho in BLUR_RADII:
        cases[f"blur_{rho}"] = dict(off(), blur_radius=rho)
    for f in HUE_FACTORS:
        cases[f"hue_{f}"] = dict(off(), hue=f)
    return cases


def chain_batches():
    """All six orders of brightness / contrast / saturation (hue off), each on a batch of the four images with different factors;
    within a batch the four (grey, blur) combinations, rotated so that every image meets several."""
    combos = [(False, None), (True, None), (False, 1.3), (True, 0.6)]
    batches = []
    for b, perm in enumerate(itertools.permutations((0, 1, 2))):
        batch = []
        for j in range(len(SIZES)):
            grey, rho = combos[(j + b) % 4]
            order = list(perm)
            order.insert((b + j) % 4, 3)            # the (disabled) hue slot moves about too
            batch.append({"order": order, "brightness": (0.45, 0.9, 1.15, 1.55)[(j + b) % 4], "contrast": (1.6, 0.5, 0.85, 1.2)[j],
                          "saturation": (0.3, 1.4, 1.0, 0.75)[(j + 2 * b) % 4], "hue": None, "grayscale": grey, "blur_radius": rho})
        batches.append(batch)
    return batches


def preset_batches():
    """The two presets of the reference's train.py under seeded draws, hue included: (name, resize, parameters)"""
    from gfnet_amd.datasets import draw_photometric

    gen, rng = torch.Generator().manual_seed(20), random.Random(21)
    online = draw_photometric(len(SIZES), generator=gen, rng=rng)
    glunet = draw_photometric(len(SIZES), 0.6, 0.6, 0.6, 0.2, grayscale_p=0.2, generator=gen, rng=rng)
    return (("online", 24, online), ("glunet", None, glunet))


def main():
    from gfnet_amd.datasets import reference_photometric

    images = [make_image(h, w, 100 + i) for i, (h, w) in enumerate(SIZES)]
    out = {f"image_{i}": im for i, im in enumerate(images)}
    cases = stage_cases()
    out["cases"] = np.array(json.dumps(cases))
    for name, p in cases.items():
        for i, im in enumerate(images):
            out[f"{name}/{i}"] = reference_photometric(im, p)
    np.savez_compressed(os.path.join(HERE, "photometric_stages.npz"), **out)

    out = {f"image_{i}": im for i, im in enumerate(images)}
    batches = chain_batches()
    out["batches"] = np.array(json.dumps(batches))
    for b, batch in enumerate(batches):
        for i, (im, p) in enumerate(zip(images, batch)):
            out[f"chain_{b}/{i}"] = reference_photometric(im, p)
    presets = preset_batches()
    out["presets"] = np.array(json.dumps([(name, size, batch) for name, size, batch in presets]))
    for name, size, batch in presets:
        for i, (im, p) in enumerate(zip(images, batch)):
            out[f"{name}/{i}"] = reference_photometric(im, p, size)
    np.savez_compressed(os.path.join(HERE, "photometric_chains.npz"), **out)

    big = make_image(*RESIZE_INPUT, 200)
    out = {"image": big, "sizes": np.array(RESIZE_SIZES)}
    for size in RESIZE_SIZES:
        out[f"resize_{size}"] = reference_photometric(big, off(), size)
    for i, im in enumerate(images):                 # every small shape, down and up
        out[f"small_{i}"] = reference_photometric(im, off(), 4)
        out[f"small_up_{i}"] = reference_photometric(im, off(), 12)
    np.savez_compressed(os.path.join(HERE, "photometric_resize.npz"), **out)
    for name in ("stages", "chains", "resize"):
        print(name, os.path.getsize(os.path.join(HERE, f"photometric_{name}.npz")), "bytes")


if __name__ == "__main__":
    main()
