#!/usr/bin/env python3
"""Generate the loss fixture G13 by running the REFERENCE's RobustLosses on the CPU (like make_golden_train.py, whose helpers and
import stubs it shares through make_golden.py):

    python tests/golden/make_golden_loss.py

G13 (g13_robust_loss.npz): losses/robust_loss.py, RobustLosses.forward (:92-128) on a batch of 2 with G12's grids (6, 6, 10, 14, 20
for scales 16..1; two iterations at scales 16 and 8) and 96x96 images.  H_s2t: one mild perspective warp that sends about a third
of the cells outside the target, one near-identity.  Every flow is the ground-truth warp plus noise whose magnitude is log-uniform
from 0.1 * cs to 100 * cs of c = 1e-3 -- but from at least NOISE_FLOOR (see there), and up to three times the next scale's local_dist
threshold where that is more, so that the threshold is crossed; the certainties are random logits.  The same flows serve both
parameter sets; under c = 1e-4 they span up to 1000 cs.  Two parameter sets: "train", the one train.py:98-106 constructs, and "default", the constructor
defaults with alpha as a per-scale dict.  Recorded: the inputs, the loss, what the reference logs (through a recording `wandb`
stand-in) and the gradient of every flow and certainty.

Two third-party names the reference's module imports are absent here and are supplied by this file: `wandb` (only `log`, which
keeps the dicts it is given) and `kornia.geometry.linalg.transform_points`, written from kornia's documented rule: append 1, multiply
by the 3x3 matrix, divide by the last coordinate (by 1 where its magnitude is at most 1e-8).
"""
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, REF, install_stubs, save, t2n  # noqa: E402

SCALES = ("16", "8", "4", "2", "1")
GRIDS = (6, 6, 10, 14, 20)
NUM_ITR = (2, 2, 1, 1, 1)
B = 2
IMAGE = 96
LOCAL_DIST = {1: 4, 2: 4, 4: 8, 8: 8}
PARAMS = {
    "train": dict(ce_weight=0.01, local_dist=LOCAL_DIST, local_largest_scale=8, depth_interpolation_mode="bilinear", alpha=0.5, c=1e-4,
                  iteration_base=1),
    "default": dict(ce_weight=0.01, local_dist=LOCAL_DIST, local_largest_scale=8, depth_interpolation_mode="bilinear",
                    alpha={16: 0.5, 8: 0.65, 4: 0.8, 2: 1.0, 1: 1.5}, c=1e-3, iteration_base=0.85),
}
# The reference computes x2_n in float32: pixel coordinates near 100 carry an ulp of 7.6e-6, and through the matrix product, the
# division and the normalisation x2_n ends up to about 5e-7 off.  Where a flow's error is below cs the regression gradient passes that
# offset on at full weight, and with alpha < 1 its largest entry is only about 0.6 * cs: at cs = 1e-4 the reference's own rounding
# would be several times the 1e-3 gradient tolerance.  So no flow is closer to the ground truth than 2400 times that offset, and the
# default set's per-scale alpha grows towards the fine scales, where cs is smallest (alpha > 1: the gradient keeps growing with the
# error, so its largest entry is many cs).
NOISE_FLOOR = 1.2e-3
H_S2T = [[[1.111, 0.07, 15.01], [-0.06, 1.087, -11.49], [7e-4, -4e-4, 1.0]],
         [[1.001, 0.006, -0.19], [-0.004, 0.997, 0.29], [2e-5, 3e-5, 1.0]]]


def transform_points(trans_01, points_1):
    ones = torch.ones_like(points_1[..., :1])
    p = torch.cat((points_1, ones), dim=-1) @ trans_01.to(points_1.dtype).transpose(-1, -2)
    z = p[..., -1:]
    return p[..., :-1] / torch.where(z.abs() > 1e-8, z, torch.ones_like(z))


class WandbRecorder(types.ModuleType):
    def __init__(self):
        super().__init__("wandb")
        self.logged = []

    def log(self, values, step=None):
        self.logged.append(dict(values))


def g13_robust_loss(robust_loss, wandb):
    gen = torch.Generator().manual_seed(1313)
    H = torch.tensor(H_S2T, dtype=torch.float32)
    im = torch.zeros(B, 3, IMAGE, IMAGE)
    batch = {"H_s2t": H, "im_A": im, "im_B": im}
    arrays = {"torch_version": np.array(torch.__version__), "H_s2t": t2n(H), "image_hw": np.array((IMAGE, IMAGE)),
              "grids": np.array(GRIDS), "num_itr": np.array(NUM_ITR)}
    inputs = {}
    for i, s in enumerate(SCALES):
        g, scale = GRIDS[i], int(s)
        x2_n, prob = robust_loss.get_gt_warp_homography(H, im, im, H=g, W=g)
        if i == 0:
            arrays["outside_fraction"] = t2n(1 - prob.mean(dim=(1, 2)))
        # magnitudes from 0.1 * cs of c = 1e-3, but at least NOISE_FLOOR, up to 100 * cs and at least three times the next scale's threshold
        nxt = int(SCALES[i + 1]) if i + 1 < len(SCALES) else None
        lo = max(0.1 * 1e-3 * scale, NOISE_FLOOR)
        hi = max(100 * 1e-3 * scale, 3 * (2 / 448) * LOCAL_DIST[nxt] * nxt if nxt else 0.0)
        for k in range(1, NUM_ITR[i] + 1):
            mag = torch.exp(torch.rand(B, g, g, generator=gen) * np.log(hi / lo) + np.log(lo))
            ang = torch.rand(B, g, g, generator=gen) * (2 * np.pi)
            noise = torch.stack((mag * torch.cos(ang), mag * torch.sin(ang)), dim=1)
            inputs[(s, k)] = ((x2_n.permute(0, 3, 1, 2) + noise).contiguous(), torch.randn(B, 1, g, g, generator=gen) * 2)
            arrays[f"flow.{s}.{k}"] = t2n(inputs[(s, k)][0])
            arrays[f"cert.{s}.{k}"] = t2n(inputs[(s, k)][1])
    for name, kw in PARAMS.items():
        leaves = {key: (f.clone().requires_grad_(), c.clone().requires_grad_()) for key, (f, c) in inputs.items()}
        corresps = {s: {k: {"flow": leaves[(s, k)][0], "certainty": leaves[(s, k)][1]} for k in range(1, NUM_ITR[i] + 1)}
                    for i, s in enumerate(SCALES)}
        wandb.logged.clear()
        loss = robust_loss.RobustLosses(**kw)(corresps, batch)
        loss.backward()
        arrays[f"{name}.loss"] = t2n(loss)
        for d in wandb.logged:
            for key, v in d.items():
                arrays[f"{name}.log.{key}"] = t2n(v)
        for (s, k), (f, c) in leaves.items():
            arrays[f"{name}.gflow.{s}.{k}"] = t2n(f.grad)
            arrays[f"{name}.gcert.{s}.{k}"] = t2n(c.grad)
    save("g13_robust_loss", **arrays)


def main():
    torch.set_num_threads(4)
    install_stubs()
    import kornia

    kornia.geometry.linalg = types.SimpleNamespace(transform_points=transform_points)
    wandb = WandbRecorder()
    sys.modules["wandb"] = wandb
    sys.path.insert(0, REF)
    import losses.robust_loss as robust_loss

    g13_robust_loss(robust_loss, wandb)
    print(f"G13: {os.path.getsize(os.path.join(OUT, 'g13_robust_loss.npz'))/1024:.1f} KiB")


if __name__ == "__main__":
    main()
