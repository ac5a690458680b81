"""What make_golden_vit.py and the ViT tests share: the model and the inputs of fixture G16, and the parameters that both regenerate
from synth.py by seed instead of storing them.

Every value is a float32 product of lattice values and a constant, computed by numpy in float32: the same bits under any numpy
version.  None of the parameters keeps its initialiser's value (an initialised model has cls_token at 1e-6, LayerScale at exactly 1,
LayerNorm at (1, 0) and zero biases, all of which hide errors): cls_token, mask_token and the position table are of the tokens' own
size, LayerScale lies in [0.4, 1.1), LayerNorm weights in [0.6, 1.4) with biases in [-0.2, 0.2), Linear biases in [-0.1, 0.1)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import synth  # noqa: E402

# the small ViT of G16: a 5 x 5 native grid, two blocks, two heads of 64 (the head dim of ViT-L/14, so the HIP path takes it)
CONFIG = dict(img_size=70, patch_size=14, embed_dim=128, depth=2, num_heads=2, init_values=1.0, ffn_layer="mlp", block_chunks=0)
# (name, images, height, width): the native grid (interpolate_pos_encoding returns early) and two interpolated, non-square grids in
# both orders (4 x 6 and 6 x 4)
INPUTS = (("native", 2, 70, 70), ("wide", 2, 56, 84), ("tall", 1, 84, 56))
OUTPUTS = ("x_norm_patchtokens", "x_norm_clstoken")
# the model whose key -> shape list the fixture records (reference model/network.py:48-54)
LARGE = dict(img_size=518, patch_size=14, init_values=1.0, ffn_layer="mlp", block_chunks=0)
SEED = 1600


def values(key, shape, seed):
    """The float32 array of state-dict entry `key`."""
    u, n = synth.lattice_uniform, synth.lattice_normalish
    if len(shape) == 4 or (len(shape) == 2 and key.endswith(".weight")):  # patch convolution and Linear weights: unit-scale outputs
        return n(shape, seed) * np.float32(0.87 / np.sqrt(np.prod(shape[1:])))
    if key in ("cls_token", "mask_token"):
        return np.float32(0.5) * n(shape, seed)
    if key == "pos_embed":
        return np.float32(0.25) * n(shape, seed)
    if key.endswith(".gamma"):
        return np.float32(0.75) + np.float32(0.35) * u(shape, seed)
    if ".norm" in key or key.startswith("norm."):
        return (np.float32(1.0) + np.float32(0.4) * u(shape, seed)) if key.endswith(".weight") else np.float32(0.2) * u(shape, seed)
    return np.float32(0.1) * u(shape, seed)  # Linear and convolution biases


def state_dict(model, seed=SEED):
    """A state dict under `model`'s own keys and shapes with the fixture's values, in the order of the sorted keys."""
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    return {k: torch.from_numpy(np.ascontiguousarray(values(k, shapes[k], seed + 7 * i), dtype=np.float32))
            for i, k in enumerate(sorted(shapes))}


def fill(model, seed=SEED):
    """Overwrite every parameter of `model` in place; returns the sorted key list."""
    state = state_dict(model, seed)
    model.load_state_dict(state, strict=True)
    return sorted(state)


def inputs(name, seed=SEED):
    """The images (B, 3, H, W) of one fixture input, float32 in [-1, 1)."""
    idx, (_, B, H, W) = next((i, s) for i, s in enumerate(INPUTS) if s[0] == name)
    return torch.from_numpy(synth.lattice_uniform((B, 3, H, W), seed + 5000 + idx))
