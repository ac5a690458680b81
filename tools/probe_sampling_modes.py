"""Kernel-time probe of the sampling-mode kernels (csrc/local_corr_modes.hip, csrc/grid_modes.hip) on the bench's scale-4 shape
(448b32: 32 directions, c32, 112 x 112 maps, G 64, r 4), next to the bilinear kernels they stand beside:

    rocprofv3 --kernel-trace --stats -d OUT -- python tools/probe_sampling_modes.py [--reps N]

local correlation: nearest / bicubic (zeros padding) and bilinear + border on local_corr_mode_kernel, bilinear + zeros on the general
per-tap kernel (local_corr_mode_kernel, `_variant=1`) and on the product's tiled path; refiner input: ops.refiner_input with
sample_mode nearest / bicubic (refiner_input_mode_kernel + local_corr_mode_kernel) and bilinear (the product path)."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import synth  # noqa: E402
from gfnet_amd import ops  # noqa: E402
from gfnet_amd.utils.local_correlation import local_correlation  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    B, c, h, w, G, r = 32, 32, 112, 112, 64, 4
    f0 = torch.from_numpy(synth.lattice_normalish((B, c, G, G), 1)).cuda()
    f1 = torch.from_numpy(synth.lattice_normalish((B, c, h, w), 2)).cuda()
    x = torch.from_numpy(synth.lattice_normalish((B, c, h, w), 3)).cuda()
    flow = torch.from_numpy(synth.homography_flow(B, G, 4)).cuda()
    dw = torch.from_numpy(synth.lattice_normalish((32, 2, 1, 1), 5)).cuda()
    db = torch.from_numpy(synth.lattice_normalish((32,), 6)).cuda()
    calls = {
        "lc nearest/zeros": lambda: local_correlation((B, c, h, w), f0, f1, r, G, flow=flow, sample_mode="nearest"),
        "lc bicubic/zeros": lambda: local_correlation((B, c, h, w), f0, f1, r, G, flow=flow, sample_mode="bicubic"),
        "lc bilinear/border": lambda: local_correlation((B, c, h, w), f0, f1, r, G, flow=flow, padding_mode="border"),
        "lc bilinear/zeros general": lambda: local_correlation((B, c, h, w), f0, f1, r, G, flow=flow, _variant=1),
        "lc bilinear/zeros tiled": lambda: local_correlation((B, c, h, w), f0, f1, r, G, flow=flow),
        "refiner_input nearest": lambda: ops.refiner_input(G, x, f1, flow, dw, db, r, sample_mode="nearest"),
        "refiner_input bicubic": lambda: ops.refiner_input(G, x, f1, flow, dw, db, r, sample_mode="bicubic"),
        "refiner_input bilinear": lambda: ops.refiner_input(G, x, f1, flow, dw, db, r),
    }
    for name, fn in calls.items():
        fn()  # warm-up
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        print(f"{name:28s} {e0.elapsed_time(e1) * 1e3 / args.reps:9.1f} us/call (events, incl. launch gaps)", flush=True)
    out = local_correlation((B, c, h, w), f0, f1, r, G, flow=flow, sample_mode="bicubic")
    print("bicubic finite:", bool(torch.isfinite(out).all()), "mean |.|", float(out.abs().mean()), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
