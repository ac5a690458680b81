#!/usr/bin/env python3
"""Generate the cross-view decoder fixture G14 by running the REFERENCE's own module (like make_golden.py, whose import stubs it uses):

    python tests/golden/make_golden_decoder.py [/path/to/GFNet-checkout]      (default: $GFNET_REFERENCE, as make_golden.py)

G14 (g14_crossview_decoder.npz): `CrossVITDecoder_noself` (model/crossview_decoder_light.py:12-112) with the shipped decoder settings
at a small size -- d_model 32, two cross blocks, 8 heads, out dim 64 (head dim 8) -- on tokens of B = 2 pairs on a 6 x 5 grid.

The module's attention, `CrossFlashAttention2` (model/transformer/layers/attention.py:227-258), calls flash_attn_func, which is
absent here (the class then raises).  This file supplies the one missing name from its published definition, evaluated in float64:
out = softmax(q k^T * softmax_scale) v per batch and head on (B, N, H, D) tensors, returned in the input's dtype.  Everything else
-- projections, position encoding, LayerNorm, LayerScale, MLP, the block order -- is the reference's code.

Recorded: the conf (JSON), every parameter under the reference's name and both token inputs as float16 arrays (the values are drawn,
rounded to fp16 and THEN loaded into the module, so the arrays are exact), the module's two output maps run in fp32, and
`fp32_vs_fp64`: the largest difference between that fp32 run and the same module run in float64, which is the unit of the parity
bound in tests/test_cross_attn_cpu.py.  meta.json describes the G1..G9 run and is left alone.
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden  # noqa: E402
from make_golden import install_stubs, save, t2n  # noqa: E402

CONF = {
    "dino_cfg": {"d_model": 32,
                 "decoder_cfg": {"num_cross_attn": 2, "init_values": 1.0, "prev_values": 0.5, "nhead": 8, "attention_type": "FLASH2",
                                 "ffn_type": "ffn", "softmax_scale": "entropy_invariance", "train_avg_length": 1024,
                                 "self_cross_types": None, "post_norm": False, "pre_norm_query": True, "no_combine_norm": False}},
    "encoder_cfg": {"feat_chs": [64, 32, 16, 8]},
}
B, H, W = 2, 6, 5


def flash_attn_func(q, k, v, dropout_p=0.0, softmax_scale=None, causal=False):
    """flash-attn's documented function for dropout_p = 0, causal = False: (B, N, H, D) in, (B, N, H, D) out."""
    assert dropout_p == 0.0 and not causal
    scale = q.shape[-1] ** -0.5 if softmax_scale is None else softmax_scale
    s = torch.einsum("bihd,bjhd->bhij", q.double(), k.double()) * scale
    return torch.einsum("bhij,bjhd->bihd", torch.softmax(s, dim=-1), v.double()).to(q.dtype)


def fp16_values(t, generator, scale=1.0, mean=0.0):
    """Random values that float16 holds exactly, in t's shape and dtype."""
    return (mean + torch.randn(t.shape, generator=generator) * scale).half().to(t.dtype)


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else make_golden.REF
    install_stubs()
    sys.path.insert(0, ref)
    from model.transformer.layers import attention

    attention.flash_attn_func, attention.FLASH_AVAILABLE = flash_attn_func, True
    from model.crossview_decoder_light import CrossVITDecoder_noself

    g = torch.Generator().manual_seed(1414)
    dec = CrossVITDecoder_noself(conf=CONF, upsample=False)
    dec.train(False)
    with torch.no_grad():
        for name, p in dec.named_parameters():
            if name.endswith("gamma"):  # LayerScale: around its init value 1, not symmetric about 0
                p.copy_(fp16_values(p, g, 0.25, 1.0))
            elif ".norm" in name and name.endswith("weight"):
                p.copy_(fp16_values(p, g, 0.1, 1.0))
            elif name.endswith("bias"):
                p.copy_(fp16_values(p, g, 0.1))
            else:  # linear weights: unit-scale outputs on unit-scale inputs
                p.copy_(fp16_values(p, g, p.shape[1] ** -0.5))
    x = fp16_values(torch.empty(B, H * W, CONF["dino_cfg"]["d_model"]), g)
    y = fp16_values(torch.empty(B, H * W, CONF["dino_cfg"]["d_model"]), g)
    shape = (B, 3, H, W)
    with torch.no_grad():
        out32 = dec(x, y, vit_shape=shape)
        dec.pe.pe_dict.clear()  # (the cached encoding is fp32 in both runs, as the module computes it)
        out64 = dec.double()(x.double(), y.double(), vit_shape=shape)
    dec.float()
    err = max(float((a.double() - b).abs().max()) for a, b in zip(out32, out64))
    arrays = {"torch_version": np.array(torch.__version__), "conf": np.array(json.dumps(CONF)), "grid": np.array([B, H, W], dtype=np.int64),
              "x": t2n(x.half()), "y": t2n(y.half()), "out_x": t2n(out32[0].contiguous()), "out_y": t2n(out32[1].contiguous()),
              "fp32_vs_fp64": np.float64(err)}
    for name, p in dec.state_dict().items():
        assert torch.equal(p.half().float(), p), name
        arrays["param/" + name] = t2n(p.half())
    save("g14_crossview_decoder", **arrays)
    print(f"fp32 vs float64: {err:.3e}; max |out| {max(float(o.abs().max()) for o in out32):.3f}")


if __name__ == "__main__":
    main()
