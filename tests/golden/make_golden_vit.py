#!/usr/bin/env python3
"""Generate the DINOv2 fixture G16 by running the REFERENCE's own module (like make_golden_fpn.py, whose import stubs it uses):

    python tests/golden/make_golden_vit.py [/path/to/GFNet-checkout]      (default: $GFNET_REFERENCE, as make_golden.py)

G16 (g16_dinov2.npz): `DinoVisionTransformer` (model/transformer/dinov2.py:43-237) with vit_fixture.CONFIG and the block class
vit_large uses, `partial(Block, attn_class=MemEffAttention)` (dinov2.py:340), in eval mode on the three inputs of
vit_fixture.INPUTS.  Parameters and inputs come from vit_fixture.py by seed and are NOT stored.  Recorded, per input s and output o
(vit_fixture.OUTPUTS): `s/o` the reference's fp32 result of forward_features, and `s/o/fp32_vs_fp64`, the largest difference
between that fp32 run and the same module run in float64 -- the unit of the parity bound in tests/test_vit_cpu.py.  Recorded once:
`keys`, the sorted state-dict key list of the small model, and `large`, the key -> shape list (as JSON) of the reference's real
`vit_large(**vit_fixture.LARGE)`.  meta.json describes the G1..G9 run and is left alone.
"""
import json
import os
import sys
from functools import partial

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden  # noqa: E402
import vit_fixture  # noqa: E402
from make_golden import install_stubs, save, t2n  # noqa: E402


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else make_golden.REF
    install_stubs()
    sys.path.insert(0, ref)
    from model.transformer import vit_large
    from model.transformer.dinov2 import DinoVisionTransformer
    from model.transformer.layers import MemEffAttention
    from model.transformer.layers import NestedTensorBlock as Block

    model = DinoVisionTransformer(block_fn=partial(Block, attn_class=MemEffAttention), **vit_fixture.CONFIG)
    keys = vit_fixture.fill(model)
    model.train(False)
    large = vit_large(**vit_fixture.LARGE)  # (on the CPU: the reference's constructor calls .item(), which the meta device refuses)
    arrays = {"torch_version": np.array(torch.__version__), "keys": np.array(keys),
              "large": np.array(json.dumps({k: list(v.shape) for k, v in large.state_dict().items()}, sort_keys=True))}
    for name, *_ in vit_fixture.INPUTS:
        x = vit_fixture.inputs(name)
        with torch.no_grad():
            out32 = model.forward_features(x)
            out64 = model.double().forward_features(x.double())
            model.float()
        for o in vit_fixture.OUTPUTS:
            err = float((out32[o].double() - out64[o]).abs().max())
            arrays[f"{name}/{o}"] = t2n(out32[o].contiguous())
            arrays[f"{name}/{o}/fp32_vs_fp64"] = np.float64(err)
            print(f"{name}/{o}: {tuple(out32[o].shape)}  max |v| {float(out32[o].abs().max()):.3f}  fp32 vs float64 {err:.3e}")
    save("g16_dinov2", **arrays)


if __name__ == "__main__":
    main()
