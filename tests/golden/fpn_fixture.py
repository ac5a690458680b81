"""What make_golden_fpn.py and the FPN tests share: the shapes of fixture G15, and the parameters, BatchNorm buffers and inputs that
both regenerate from synth.py by seed instead of storing them.

Every value is a float32 product of lattice values and a power-free constant, computed by numpy in float32: the same bits under
any numpy version.  BatchNorm is made non-trivial on purpose (an identity BatchNorm would hide a wrong fold): running means in
[-0.5, 0.5), running variances in [0.25, 1.75), gamma in [0.4, 1.1) (below 1 more often than not), beta in [-0.1, 0.5)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import synth  # noqa: E402

FEAT_CHS = [8, 16, 32, 64]  # fine to coarse: the shipped encoder_cfg.feat_chs [64, 32, 16, 8] reversed, as network.py:62-63 passes it
# (name, images, height, width): both non-square, with odd sizes at stride 8 (5 x 7 and 3 x 9)
SHAPES = (("a", 2, 40, 56), ("b", 2, 24, 72))
MAPS = ("enc1", "enc2", "enc4", "enc8", "dec8", "dec4", "dec2", "dec1")  # conv01, conv11, conv21, merged conv31; out0 .. out3
# The maps at strides 4 and 8 are stored whole; at strides 2 and 1 every second row and column is stored, from these (row, column)
# phases -- all eight maps of both shapes in full are 930 KiB of float32, which does not compress, against the 400 KiB a fixture may
# take.  The two maps of a stride use opposite phases.
PHASE = {"enc1": (0, 0), "dec1": (1, 1), "enc2": (1, 0), "dec2": (0, 1)}
SEED = 1500


def stored(name, m):
    """The part of map `name` that the fixture holds."""
    if name in PHASE:
        return m[..., PHASE[name][0]::2, PHASE[name][1]::2]
    return m


def fill(modules, seed=SEED):
    """Overwrite every parameter and BatchNorm buffer of `modules` (a dict name -> module: encoder, decoder, merge_layer) in place, in
    the order of the sorted state-dict keys."""
    state = {f"{top}.{k}": v for top, m in modules.items() for k, v in m.state_dict().items()}
    with torch.no_grad():
        for i, key in enumerate(sorted(state)):
            t, s = state[key], seed + 7 * i
            if key.endswith("num_batches_tracked"):
                continue
            if t.dim() == 4:  # conv weight: unit-scale outputs on unit-scale inputs
                v = synth.lattice_normalish(tuple(t.shape), s) * np.float32(0.87 / np.sqrt(t.shape[1] * t.shape[2] * t.shape[3]))
            elif key.endswith("running_var"):
                v = np.float32(1.0) + np.float32(0.75) * synth.lattice_uniform(tuple(t.shape), s)
            elif key.endswith("running_mean"):
                v = np.float32(0.5) * synth.lattice_uniform(tuple(t.shape), s)
            elif key.endswith(".bn.weight") or key.endswith(".1.weight"):  # gamma
                v = np.float32(0.75) + np.float32(0.35) * synth.lattice_uniform(tuple(t.shape), s)
            else:  # beta and the conv biases
                v = np.float32(0.2) + np.float32(0.3) * synth.lattice_uniform(tuple(t.shape), s)
            t.copy_(torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(t.dtype))
    return sorted(state)


def inputs(shape_name, seed=SEED):
    """(images (B, 3, H, W), side map (B, 64, H/8, W/8)) of one fixture shape, float32."""
    idx, (_, B, H, W) = next((i, s) for i, s in enumerate(SHAPES) if s[0] == shape_name)
    images = synth.lattice_uniform((B, 3, H, W), seed + 5000 + idx)
    side = np.float32(0.5) * synth.lattice_normalish((B, FEAT_CHS[-1], H // 8, W // 8), seed + 6000 + idx)
    return torch.from_numpy(images), torch.from_numpy(side)
