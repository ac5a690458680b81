#!/usr/bin/env python3
"""Generate the FPN fixture G15 by running the REFERENCE's own modules (like make_golden_decoder.py, whose import stubs it uses):

    python tests/golden/make_golden_fpn.py [/path/to/GFNet-checkout]      (default: $GFNET_REFERENCE, as make_golden.py)

G15 (g15_fpn.npz): `FPNEncoder`, `FPNDecoder_concat` and `Swish` (model/FPN.py:5-69, 88-93) with the shipped channel counts, and
the merge layer exactly as the reference's constructor builds it and `extract_features` applies it (model/network.py:66, 182):

    conv01, conv11, conv21, conv31 = encoder(images)
    conv31 = conv31 + merge_layer(cat(conv31, side))
    out0 .. out3 = decoder(conv01, conv11, conv21, conv31)

in eval mode on two shapes (fpn_fixture.SHAPES).  Parameters, BatchNorm buffers and inputs come from fpn_fixture.py by seed and are
NOT stored.  Recorded, per shape s and map m (fpn_fixture.MAPS: the four merged encoder maps and the four decoder maps):
`s/m` the reference's fp32 map (at strides 1 and 2 every second row and column, see fpn_fixture.PHASE: the size limit),
`s/m/shape` its full shape, and `s/m/fp32_vs_fp64`, the largest difference over the WHOLE map between that fp32 run and the same
modules run in float64 -- the unit of the parity bounds in tests/test_fpn_cpu.py and tests/test_fpn_gpu.py.  `keys` is the sorted
state-dict key list under the names GFNet gives the three modules (encoder, decoder, merge_layer).  meta.json describes the G1..G9
run and is left alone.
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fpn_fixture  # noqa: E402
import make_golden  # noqa: E402
from make_golden import install_stubs, save, t2n  # noqa: E402


def run(mods, images, side):
    c0, c1, c2, c3 = mods["encoder"](images)
    c3 = c3 + mods["merge_layer"](torch.cat((c3, side), dim=1))  # network.py:182
    return dict(zip(fpn_fixture.MAPS, [c0, c1, c2, c3] + list(mods["decoder"](c0, c1, c2, c3))))


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else make_golden.REF
    install_stubs()
    sys.path.insert(0, ref)
    from model.FPN import FPNDecoder_concat, FPNEncoder, Swish

    chs = fpn_fixture.FEAT_CHS
    mods = {"encoder": FPNEncoder(feat_chs=chs), "decoder": FPNDecoder_concat(feat_chs=chs),
            "merge_layer": nn.Sequential(nn.Conv2d(2 * chs[-1], chs[-1], kernel_size=3, padding=1), nn.BatchNorm2d(chs[-1]), Swish())}  # network.py:66
    keys = fpn_fixture.fill(mods)
    for m in mods.values():
        m.train(False)
    arrays = {"torch_version": np.array(torch.__version__), "keys": np.array(keys), "feat_chs": np.array(chs, dtype=np.int64)}
    for name, *_ in fpn_fixture.SHAPES:
        images, side = fpn_fixture.inputs(name)
        with torch.no_grad():
            out32 = run(mods, images, side)
            for m in mods.values():
                m.double()
            out64 = run(mods, images.double(), side.double())
            for m in mods.values():
                m.float()
        for k in fpn_fixture.MAPS:
            err = float((out32[k].double() - out64[k]).abs().max())
            arrays[f"{name}/{k}"] = t2n(fpn_fixture.stored(k, out32[k]).contiguous())
            arrays[f"{name}/{k}/shape"] = np.array(out32[k].shape, dtype=np.int64)
            arrays[f"{name}/{k}/fp32_vs_fp64"] = np.float64(err)
            print(f"{name}/{k}: {tuple(out32[k].shape)}  max |v| {float(out32[k].abs().max()):.3f}  fp32 vs float64 {err:.3e}")
    save("g15_fpn", **arrays)


if __name__ == "__main__":
    main()
