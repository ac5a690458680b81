"""A training batch synthesised on the device, timed (GPU): python tools/time_pair_synth.py [--reps 15] [--warmup 3]

The 448 configuration (ratio 0.3: crop 640, deform_area 192, centre crop 448, no final resize), batch 8, sources 650 x 867 of white
noise already on the device, made two ways from the same draws:
  fused  gfnet_amd.datasets.PairSynthesizer: one parameter launch, one warp launch for the sixteen images with the Normalize fused.
  torch  the reference's chain (datasets/generate_random_H_large_size.py:38-85 and the Normalize of the dataset) restated per batch
         in float32 torch on the same device: torch.linalg.solve on the 8 x 8 systems, the 640 x 640 crops, F.grid_sample
         (align_corners=True) at 640 x 640, the centre crops, H_1t2t by torch.linalg.inv, the corner flow and the third solve, the
         Normalize.  No kornia, no per-sample loop: this is the reference's arithmetic at its best batched form, not its run time.
Both run in one process, alternating; every timed step is bracketed by device synchronisation; the figure is the median of --reps
steps after --warmup untimed ones, the spread their min .. max.  The last batch of both is then compared with the same chain in
float64 on the device (largest absolute difference of the normalised images and of H_s2t).  One JSON line, then markdown table rows
for DESIGN 4.5."""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gfnet_amd import ops  # noqa: E402
from gfnet_amd.datasets import PairSynthesizer, draw_random_h  # noqa: E402

RES, RATIO, BATCH, SRC = 448, 0.3, 8, (650, 867)


def solve_batch(src, dst):
    """kornia's get_perspective_transform, batched: (B,4,2) x 2 -> (B,3,3) in the inputs' dtype"""
    x, y, u, v = src[..., 0], src[..., 1], dst[..., 0], dst[..., 1]
    one, zero = torch.ones_like(x), torch.zeros_like(x)
    ax = torch.stack([x, y, one, zero, zero, zero, -x * u, -y * u], dim=-1)
    ay = torch.stack([zero, zero, zero, x, y, one, -x * v, -y * v], dim=-1)
    A = torch.stack([ax, ay], dim=2).reshape(-1, 8, 8)
    sol = torch.linalg.solve(A, torch.stack([u, v], dim=2).reshape(-1, 8))
    return torch.cat([sol, torch.ones_like(sol[:, :1])], dim=1).reshape(-1, 3, 3)


def transform_points(H, pts):
    ph = torch.cat([pts, torch.ones_like(pts[..., :1])], dim=-1) @ H.transpose(1, 2)
    z = ph[..., 2:]
    return ph[..., :2] * torch.where(z.abs() > 1e-8, 1.0 / z, torch.ones_like(z))


def warp_batch(img, H, size):
    """warp_perspective(align_corners=True) through F.grid_sample: img (B,C,h,w), H (B,3,3) source -> destination"""
    B, _, h, w = img.shape
    v, u = torch.meshgrid(torch.arange(size[0], device=img.device, dtype=img.dtype), torch.arange(size[1], device=img.device, dtype=img.dtype),
                          indexing="ij")
    p = transform_points(torch.linalg.inv(H), torch.stack([u.reshape(-1), v.reshape(-1)], dim=-1).expand(B, -1, 2))
    grid = torch.stack([p[..., 0] * (2 / (w - 1)) - 1, p[..., 1] * (2 / (h - 1)) - 1], dim=-1).reshape(B, size[0], size[1], 2)
    return F.grid_sample(img, grid, mode="bilinear", padding_mode="zeros", align_corners=True)


def torch_chain(imgs0, imgs1, draws, crop, deform, mean, std, dtype=torch.float32):
    d2, dev = deform // 2, imgs0[0].device
    mean, std = mean.to(dtype), std.to(dtype)
    d = draws.tolist()
    c0 = torch.stack([im[:, r[1]:r[1] + crop, r[0]:r[0] + crop] for im, r in zip(imgs0, d)]).to(dtype)
    c1 = torch.stack([im[:, r[1]:r[1] + crop, r[0]:r[0] + crop] for im, r in zip(imgs1, d)]).to(dtype)
    corners = draws[:, 2:].to(dev, dtype).reshape(-1, 2, 4, 2)
    tgt = torch.tensor([[d2, d2], [crop - d2 - 1, d2], [crop - d2 - 1, crop - d2 - 1], [d2, crop - d2 - 1]], dtype=dtype, device=dev)
    tgt = tgt.expand(len(d), 4, 2)
    H1, H2 = solve_batch(corners[:, 0], tgt), solve_batch(corners[:, 1], tgt)
    a = warp_batch(c0, H1, (crop, crop))[:, :, d2:crop - d2, d2:crop - d2]
    b = warp_batch(c1, H2, (crop, crop))[:, :, d2:crop - d2, d2:crop - d2]
    flow = transform_points(H2 @ torch.linalg.inv(H1), tgt) - tgt
    n = crop - 2 * d2
    src = torch.tensor([[0, 0], [n - 1, 0], [n - 1, n - 1], [0, n - 1]], dtype=dtype, device=dev).expand(len(d), 4, 2)
    H = solve_batch(src, src + flow)
    return {"im_A": (a - mean) / std, "im_B": (b - mean) / std, "H_s2t": H}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    gen = torch.Generator().manual_seed(0)
    imgs0 = [torch.rand((3,) + SRC, generator=gen).cuda() for _ in range(BATCH)]
    imgs1 = [torch.rand((3,) + SRC, generator=gen).cuda() for _ in range(BATCH)]
    crop = int(RES / (1 - RATIO))
    deform = int(crop * RATIO)
    mean = torch.tensor(ops.IMAGENET_MEAN, device="cuda")[None, :, None, None]
    std = torch.tensor(ops.IMAGENET_STD, device="cuda")[None, :, None, None]
    draw_gen = torch.Generator().manual_seed(1)
    synth = PairSynthesizer(RES, deformation_ratio=[RATIO], generator=draw_gen)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6, out

    t_fused, t_torch = [], []
    for k in range(args.warmup + args.reps):
        state = draw_gen.get_state()
        a, got = timed(lambda: synth(imgs0, imgs1))
        draw_gen.set_state(state)                                               # the same draws for the restated chain
        draws = draw_random_h(BATCH, SRC[1], SRC[0], crop, deform, generator=draw_gen)
        b, ref = timed(lambda: torch_chain(imgs0, imgs1, draws, crop, deform, mean, std))
        if k >= args.warmup:
            t_fused.append(a)
            t_torch.append(b)
    # the last batch of both paths against the same chain in float64 on the device (untimed)
    ref64 = torch_chain(imgs0, imgs1, draws, crop, deform, mean, std, torch.float64)
    worst = {name: {key: float((out[key].double() - ref64[key]).abs().max()) for key in ("im_A", "im_B", "H_s2t")}
             for name, out in (("fused", got), ("torch32", ref))}
    ops.kernel_events = {"warp_perspective": []}
    synth(imgs0, imgs1)
    torch.cuda.synchronize()
    warp_us = sum(e0.elapsed_time(e1) for e0, e1 in ops.kernel_events["warp_perspective"]) * 1e3
    ops.kernel_events = None
    out_bytes = 2 * BATCH * 3 * RES * RES * 4
    row = {"res": RES, "batch": BATCH, "source": list(SRC), "crop": crop, "reps": args.reps,
           "fused_us": statistics.median(t_fused), "fused_min": min(t_fused), "fused_max": max(t_fused),
           "torch_us": statistics.median(t_torch), "torch_min": min(t_torch), "torch_max": max(t_torch),
           "warp_launch_event_us": warp_us, "warp_output_bytes": out_bytes, "max_abs_difference_from_float64_chain": worst,
           "device": torch.cuda.get_device_name(0)}
    print(json.dumps(row), flush=True)
    print("| path | median per batch | min .. max | launches per batch |")
    print("|---|---|---|---|")
    print(f"| `PairSynthesizer` (draws on the host, one upload each of draws and source table) | {row['fused_us']:.0f} us | "
          f"{row['fused_min']:.0f} .. {row['fused_max']:.0f} us | 2 HIP launches |")
    print(f"| the same chain restated in float32 torch on the device | {row['torch_us']:.0f} us | {row['torch_min']:.0f} .. "
          f"{row['torch_max']:.0f} us | not counted |")


if __name__ == "__main__":
    main()
