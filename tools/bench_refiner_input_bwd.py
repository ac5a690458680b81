"""Cost of one refiner's input assembly in training, forward + backward, at the production shapes of a batch of 8 pairs
(gfnet_configs/basic.json): the differentiable HIP op (ops.refiner_input: inference's launch forward, gfn_refiner_input_bwd
backward) against the torch restatement it replaces for bilinear refiners (ConvRefiner._assemble_autograd: two F.grid_sample, a 1x1
conv, the stand-alone local correlation, torch.cat).  HIP events around `iters` forward + backward passes, the two paths alternating
`rounds` times in one process; peak memory is torch.cuda.max_memory_allocated over one pass, above what the inputs already hold.

    python tools/bench_refiner_input_bwd.py [--rounds 7] [--iters 20] [--out profiles/refiner_input_bwd.md]

--deterministic measures something else: the backward alone (ops.refiner_input_bwd, all five gradients, the local correlation's
feature0 gradient included), deterministic=False against deterministic=True -- dy as the fp32 atomic scatter against the 64-bit
fixed-point sum -- at the same three shapes, the two alternating `rounds` times, with the deterministic route's workspace in MB.

    python tools/bench_refiner_input_bwd.py --deterministic [--rounds 7] [--iters 20] [--out FILE]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gfnet_amd.model.network import _refiner_for  # noqa: E402

# (scale, C, map, G, r, Dd)
SHAPES = [("16", 64, 32, 32, 7, 64), ("4", 32, 112, 64, 4, 32), ("1", 8, 448, 256, 0, 8)]
B = 8


def inputs(C, hs, G, seed):
    gen = torch.Generator().manual_seed(seed)
    x, y = (torch.randn(B, C, hs, hs, generator=gen).cuda().requires_grad_(True) for _ in range(2))
    lin = torch.linspace(-1 + 1 / G, 1 - 1 / G, G)
    gy, gx = torch.meshgrid(lin, lin, indexing="ij")
    flow = torch.stack((gx, gy))[None].repeat(B, 1, 1, 1)
    flow = flow * 0.9 + 0.05 * torch.sin(3 * flow.flip(1)) + 0.5 / hs * torch.randn(B, 2, G, G, generator=gen)  # a smooth warp plus sub-pixel noise
    return x, y, flow.cuda().requires_grad_(True)


def one_pass(ref, path, G, x, y, flow, grad_d):
    for t in (x, y, flow, ref.disp_emb.weight, ref.disp_emb.bias):
        t.grad = None
    d, _ = ref._assemble_autograd(G, x, y, flow, 1.0) if path == "torch" else ref.assemble(G, x, y, flow, 1.0)
    d.backward(grad_d)


def deterministic_leg(a):
    from gfnet_amd import _lib, ops

    lines = ["| scale | C | map | G | r | plain bwd ms (median, min..max) | deterministic bwd ms (median, min..max) | det / plain | workspace MB |",
             "|---|---|---|---|---|---|---|---|---|"]
    for scale, C, hs, G, r, Dd in SHAPES:
        ref = _refiner_for(C, Dd, r).cuda().train()
        x, y, flow = (t.detach() for t in inputs(C, hs, G, 1))
        w = ref.disp_emb.weight.detach()
        grad_d = torch.randn(B, 2 * C + Dd + ((2 * r + 1) ** 2 if r else 0), G, G, device="cuda")
        run = lambda det: ops.refiner_input_bwd(grad_d, y, flow, w, r, 1.0, r > 0, deterministic=det)  # noqa: E731
        series = {False: [], True: []}
        for det in series:
            for _ in range(3):
                run(det)
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for det in series:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.iters):
                    run(det)
                e1.record()
                torch.cuda.synchronize()
                series[det].append(e0.elapsed_time(e1) / a.iters)
        fmt = lambda v: f"{statistics.median(v):.3f} ({min(v):.3f}..{max(v):.3f})"  # noqa: E731
        mp, md = statistics.median(series[False]), statistics.median(series[True])
        ws = int(_lib.lib().gfn_refiner_input_bwd_det_ws_bytes(B, C, hs, hs)) / 2 ** 20
        lines.append(f"| {scale} | {C} | {hs} | {G} | {r} | {fmt(series[False])} | {fmt(series[True])} | {md / mp:.2f}x | {ws:.1f} |")
        print(lines[-1], flush=True)
        print(f"  series plain {[round(v, 3) for v in series[False]]} deterministic {[round(v, 3) for v in series[True]]}", flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--deterministic", action="store_true", help="the backward alone, plain against deterministic dy")
    a = ap.parse_args()
    if a.deterministic:
        return deterministic_leg(a)
    lines = ["| scale | C | map | G | r | torch path ms (median, min..max) | HIP path ms (median, min..max) | speed-up | torch peak MB | HIP peak MB | dy atomic GB/s |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for scale, C, hs, G, r, Dd in SHAPES:
        ref = _refiner_for(C, Dd, r).cuda().train()
        x, y, flow = inputs(C, hs, G, 1)
        grad_d = torch.randn(B, 2 * C + Dd + ((2 * r + 1) ** 2 if r else 0), G, G, device="cuda")
        series, peak = {"torch": [], "hip": []}, {}
        for path in series:
            for _ in range(3):
                one_pass(ref, path, G, x, y, flow, grad_d)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            one_pass(ref, path, G, x, y, flow, grad_d)
            torch.cuda.synchronize()
            peak[path] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
        for _ in range(a.rounds):
            for path in series:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.iters):
                    one_pass(ref, path, G, x, y, flow, grad_d)
                e1.record()
                torch.cuda.synchronize()
                series[path].append(e0.elapsed_time(e1) / a.iters)
        fmt = lambda v: f"{statistics.median(v):.3f} ({min(v):.3f}..{max(v):.3f})"  # noqa: E731
        mt, mh = statistics.median(series["torch"]), statistics.median(series["hip"])
        atomic_bytes = B * C * G * G * 4 * 4  # four fp32 adds per cell and channel
        lines.append(f"| {scale} | {C} | {hs} | {G} | {r} | {fmt(series['torch'])} | {fmt(series['hip'])} | {mt / mh:.2f}x | "
                     f"{peak['torch']:.1f} | {peak['hip']:.1f} | {atomic_bytes / (mh * 1e-3) / 1e9:.0f} |")
        print(lines[-1], flush=True)
        print(f"  series torch {[round(v, 3) for v in series['torch']]} hip {[round(v, 3) for v in series['hip']]}", flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
