#!/usr/bin/env python3
"""Generate the FPN training fixture G17 by running the REFERENCE's own modules in train() mode (like make_golden_fpn.py):

    python tests/golden/make_golden_fpn_train.py [/path/to/GFNet-checkout]      (default: $GFNET_REFERENCE, as make_golden.py)

G17 (g17_fpn_train.npz): `FPNEncoder`, `FPNDecoder_concat`, `Swish` and the merge layer as in G15, with fpn_fixture's parameters and
buffers, in train(True) on fixture shape "b": one forward on the batch's own statistics and one backward of

    loss = sum_k (map_k * w_k).sum() / sqrt(numel of one image's map_k)        w_k = synth.lattice_normalish(map_k.shape, 9000 + k)

over the eight maps of fpn_fixture.MAPS, in fp32 and in float64.  Recorded from the fp32 run: `map/<m>` the eight maps (through
fpn_fixture.stored), `buf/<key>` the 57 BatchNorm buffers after the step, `grad/<key>` the first 2048 elements of every parameter's
gradient and of `grad/images` and `grad/side`; and for each of them `<name>/e32`, the largest difference over the WHOLE tensor
between the fp32 and the float64 run: the unit of the bounds in tests/test_fpn_train_cpu.py and tests/test_fpn_train_gpu.py.  Data
only; parameters and inputs are regenerated from fpn_fixture.py by seed.
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fpn_fixture  # noqa: E402
import synth  # noqa: E402

SHAPE = "b"
GRAD_ELEMS = 2048  # (4096 would make the file 450 KiB)
MAX_BYTES = 400 * 1024


def train_step(mods, run, images, side):
    """One forward and backward of the three modules (already in train mode, on the device and in the dtype of `images`) through
    run(mods, images, side) -> the eight maps: every map, every buffer after the step and every gradient as float64 CPU tensors
    under map/, buf/ and grad/."""
    images, side = images.clone().requires_grad_(), side.clone().requires_grad_()
    maps = run(mods, images, side)
    loss = 0
    for k, name in enumerate(fpn_fixture.MAPS):
        w = torch.from_numpy(synth.lattice_normalish(tuple(maps[name].shape), 9000 + k)).to(device=images.device, dtype=images.dtype)
        loss = loss + (maps[name] * w).sum() / float(np.sqrt(maps[name][0].numel()))
    loss.backward()
    res = {f"map/{k}": v for k, v in maps.items()}
    res.update({f"buf/{top}.{k}": v for top, m in mods.items() for k, v in m.named_buffers()})
    res.update({f"grad/{top}.{k}": p.grad for top, m in mods.items() for k, p in m.named_parameters()})
    res.update({"grad/images": images.grad, "grad/side": side.grad})
    return {k: v.detach().cpu().double() for k, v in res.items()}


def stored(name, t):
    """The part of tensor `name` of train_step's result that the fixture holds."""
    if name.startswith("map/"):
        return fpn_fixture.stored(name[4:], t)
    if name.startswith("grad/"):
        return t.reshape(-1)[:GRAD_ELEMS]
    return t


def main():
    import make_golden
    from make_golden import install_stubs, save
    from make_golden_fpn import run

    ref = sys.argv[1] if len(sys.argv) > 1 else make_golden.REF
    install_stubs()
    sys.path.insert(0, ref)
    from model.FPN import FPNDecoder_concat, FPNEncoder, Swish

    chs = fpn_fixture.FEAT_CHS
    results = {}
    for dtype in (torch.float32, torch.float64):
        mods = {"encoder": FPNEncoder(feat_chs=chs), "decoder": FPNDecoder_concat(feat_chs=chs),
                "merge_layer": nn.Sequential(nn.Conv2d(2 * chs[-1], chs[-1], kernel_size=3, padding=1), nn.BatchNorm2d(chs[-1]), Swish())}
        fpn_fixture.fill(mods)
        for m in mods.values():
            m.to(dtype).train(True)
        images, side = (t.to(dtype) for t in fpn_fixture.inputs(SHAPE))
        results[dtype] = train_step(mods, run, images, side)
    r32, r64 = results[torch.float32], results[torch.float64]
    arrays = {"torch_version": np.array(torch.__version__), "names": np.array(sorted(r32))}
    for name in sorted(r32):
        e32 = float((r32[name] - r64[name]).abs().max())
        part = stored(name, r32[name]).contiguous().numpy()
        arrays[name] = part.astype(np.int64 if name.endswith("num_batches_tracked") else np.float32)
        arrays[name + "/e32"] = np.float64(e32)
        print(f"{name}: {tuple(r32[name].shape)}  max |v| {float(r32[name].abs().max()):.3e}  fp32 vs float64 {e32:.3e}")
    save("g17_fpn_train", **arrays)
    size = os.path.getsize(os.path.join(make_golden.OUT, "g17_fpn_train.npz"))
    assert size <= MAX_BYTES, f"g17_fpn_train.npz is {size} bytes, a fixture may take {MAX_BYTES}"


if __name__ == "__main__":
    main()
