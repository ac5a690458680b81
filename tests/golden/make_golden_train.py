#!/usr/bin/env python3
"""Generate the training fixture G12 by running the REFERENCE itself (like make_golden.py, whose import stubs it uses):

    python tests/golden/make_golden_train.py

G12 (g12_train_grads.npz): one training step of the reference's coarse-to-fine loop, GFNet.forward (model/network.py:203-283) with
`training` set, on toy refiners (ConvRefiner, :444-564) in train() mode with amp=False, a plain batch of 2.  The scale-16 map has
36 positions (not a multiple of 32) and 9 channels (not a multiple of the 2-channel k-step); scales 16 and 8 take two iterations,
so a flow update feeds the same refiner again.  A fixed random weighting of every (scale, iteration) flow and certainty is summed
and back-propagated.  Recorded: the inputs and state dicts, every flow and certainty, the gradients of both pyramids at every scale,
every refiner parameter's gradient and the refiners' buffers after the step (BatchNorm running statistics).  The torch version is recorded
inside (meta.json describes the G1..G9 run and is left alone).
"""
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, REF, install_stubs, save, t2n  # noqa: E402

SCALES = ("16", "8", "4", "2", "1")
FEAT_CH = (9, 9, 4, 3, 2)
DISP = (4, 4, 2, 2, 2)
RADIUS = (2, 2, 1, 1, 0)
SIDES = (6, 8, 12, 16, 24)         # feature map side per scale
NUM_GRID = (6, 6, 10, 14, 20)      # the scale-16 grid is its map (the flow comes from the global match)
NUM_ITR = (2, 2, 1, 1, 1)
HIDDEN_BLOCKS = 1
B = 2
IMAGE_HW = (80, 96)                # network input (H0, W0): only the displacement scaling reads it (network.py:262-263)


def g12_train_grads(network):
    torch.manual_seed(1212)
    GFNet = network.GFNet
    refiners = {}
    for i, s in enumerate(SCALES):
        K = (2 * RADIUS[i] + 1) ** 2 if RADIUS[i] > 0 else 0
        dim = 2 * FEAT_CH[i] + DISP[i] + K
        refiners[s] = network.ConvRefiner(dim, dim, 3, kernel_size=5, dw=True, hidden_blocks=HIDDEN_BLOCKS, displacement_emb="linear",
                                          displacement_emb_dim=DISP[i], local_corr_num=RADIUS[i], corr_in_other=RADIUS[i] > 0,
                                          amp=False, disable_local_corr_grad=True, bn_momentum=0.01).train()
    me = types.SimpleNamespace(conv_refiner=refiners, num_grid=list(NUM_GRID), num_itr=list(NUM_ITR), radius=list(RADIUS),
                               training=True)
    me.corr_volume = lambda a, b: GFNet.corr_volume(me, a, b)
    me.pos_embed = lambda v: GFNet.pos_embed(me, v)
    arrays = {"torch_version": np.array(torch.__version__), "feat_ch": np.array(FEAT_CH), "disp": np.array(DISP),
              "radius": np.array(RADIUS), "num_grid": np.array(NUM_GRID), "num_itr": np.array(NUM_ITR),
              "hidden_blocks": np.int64(HIDDEN_BLOCKS), "image_hw": np.array(IMAGE_HW)}
    for s in SCALES:
        for k, v in refiners[s].state_dict().items():
            arrays[f"sd.{s}.{k}"] = t2n(v).copy()   # (a view of the buffer would see the step's BatchNorm updates)
    pyr0 = {s: torch.randn(B, FEAT_CH[i], SIDES[i], SIDES[i]).requires_grad_() for i, s in enumerate(SCALES)}
    pyr1 = {s: torch.randn(B, FEAT_CH[i], SIDES[i], SIDES[i]).requires_grad_() for i, s in enumerate(SCALES)}
    me.extract_features = lambda x, upsample=False: (dict(pyr0), dict(pyr1))
    im = torch.zeros(B, 3, *IMAGE_HW)
    corresps = GFNet.forward(me, {"im_A": im, "im_B": im})
    loss = torch.zeros(())
    for i, s in enumerate(SCALES):
        arrays[f"pyr0.{s}"] = t2n(pyr0[s])
        arrays[f"pyr1.{s}"] = t2n(pyr1[s])
        for itr, d in corresps[s].items():
            wf = torch.randn(d["flow"].shape)
            wc = torch.randn(d["certainty"].shape)
            loss = loss + (wf * d["flow"]).sum() + (wc * d["certainty"]).sum()
            arrays[f"wflow.{s}.{itr}"] = t2n(wf)
            arrays[f"wcert.{s}.{itr}"] = t2n(wc)
            arrays[f"flow.{s}.{itr}"] = t2n(d["flow"])
            arrays[f"cert.{s}.{itr}"] = t2n(d["certainty"])
    loss.backward()
    arrays["loss"] = t2n(loss)
    for s in SCALES:
        arrays[f"grad0.{s}"] = t2n(pyr0[s].grad)
        arrays[f"grad1.{s}"] = t2n(pyr1[s].grad)
        for k, p in refiners[s].named_parameters():
            arrays[f"pgrad.{s}.{k}"] = t2n(p.grad)
        for k, v in refiners[s].named_buffers():
            arrays[f"buf_after.{s}.{k}"] = t2n(v)
    save("g12_train_grads", **arrays)


def main():
    torch.set_num_threads(4)
    install_stubs()
    sys.path.insert(0, REF)
    import model.network as network

    g12_train_grads(network)
    print(f"G12: {os.path.getsize(os.path.join(OUT, 'g12_train_grads.npz'))/1024:.1f} KiB")


if __name__ == "__main__":
    main()
