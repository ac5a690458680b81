"""Forward + backward time of one refiner's conv stack in train() (GPU): python tools/time_conv_train.py [--batch 8] [--reps 15] [--scales 16,8]

Six paths on the same ConvRefiner weights, the same concat tensor d and the same output weighting, at the five GFNet widths on the
grids bench.py's default 448 workload gives them (C, G = 417/32, 361/32, 177/64, 73/128, 24/256): `train_conv_impl = "hip"`
(csrc/conv_stack_train.hip, fp32) and "torch" (the nn modules on MIOpen, fp32, amp off), and in the reference's autocast class
"hip_amp" (csrc/conv_stack_train_half.hip, fp16 maps) and "torch_amp" (the nn modules under torch.autocast, amp on), and in the bf16
autocast class "hip_bf16" (csrc/conv_stack_train_bf16.hip, bf16 maps) and "torch_bf16" (the nn modules under bf16 autocast).  The runs
alternate in one process; every timed step is bracketed by device synchronisation; the figure is the median of --reps steps after
--warmup untimed ones, the spread their min .. max; <path>_peak_mib is the peak of torch's allocator over one more step of that path
alone (d, w and every path's parameters stay allocated throughout).  One JSON line per width, then a markdown table.  --scales picks widths, so
that a job can give every width a process and a time limit of its own; --paths picks paths."""
import argparse
import copy
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gfnet_amd.model.network import ConvRefiner  # noqa: E402

# (scale, feature channels, displacement dim, local-correlation radius, grid at 448)
WIDTHS = [("16", 64, 64, 7, 32), ("8", 64, 64, 6, 32), ("4", 32, 32, 4, 64), ("2", 16, 16, 2, 128), ("1", 8, 8, 0, 256)]


def step(ref, d, w):
    """one training step of the stack: forward, weighted sum, backward into d and every parameter"""
    d.grad = None
    ref.zero_grad(set_to_none=True)
    (ref.apply_stack(d) * w).sum().backward()


def timed(ref, d, w):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    step(ref, d, w)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


# path -> (train_conv_impl, amp, amp_dtype)
PATHS = {"hip": ("hip", False, torch.float16), "modules": ("torch", False, torch.float16), "hip_amp": ("hip_amp", True, torch.float16),
         "torch_amp": ("torch", True, torch.float16), "hip_bf16": ("hip_bf16", True, torch.bfloat16),
         "torch_bf16": ("torch", True, torch.bfloat16)}


def peak_mib(ref, d, w):
    """the allocator's peak over one step, above nothing: MiB"""
    d.grad = None
    ref.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    step(ref, d, w)
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scales", default=",".join(w[0] for w in WIDTHS), help="comma-separated subset of 16,8,4,2,1")
    ap.add_argument("--paths", default=",".join(PATHS), help="comma-separated subset of " + ",".join(PATHS))
    args = ap.parse_args()
    chosen, paths = args.scales.split(","), args.paths.split(",")
    unknown = [s for s in chosen if s not in [w[0] for w in WIDTHS]] + [p for p in paths if p not in PATHS]
    if unknown:
        ap.error(f"unknown scales or paths {unknown}")
    rows = []
    for scale, feat, disp, r, G in [w for w in WIDTHS if w[0] in chosen]:
        dim = 2 * feat + disp + ((2 * r + 1) ** 2 if r > 0 else 0)
        torch.manual_seed(0)
        base = ConvRefiner(dim, dim, 3, kernel_size=5, dw=True, hidden_blocks=8, displacement_emb="linear", displacement_emb_dim=disp,
                           local_corr_num=r, corr_in_other=r > 0, amp=False, bn_momentum=0.01).cuda().train()
        g = torch.Generator().manual_seed(1)
        d = torch.randn(args.batch, dim, G, G, generator=g).cuda().requires_grad_()
        w = torch.randn(args.batch, 3, G, G, generator=g).cuda()
        refs = {}
        for name in paths:
            refs[name] = copy.deepcopy(base)
            refs[name].train_conv_impl, refs[name].amp, refs[name].amp_dtype = PATHS[name]
            assert refs[name]._hip_train_stack_supported(d) == (name == "hip") and refs[name]._hip_amp_train_stack_supported(d) == (name == "hip_amp")
            assert refs[name]._hip_bf16_train_stack_supported(d) == (name == "hip_bf16")
        for _ in range(args.warmup):
            for ref in refs.values():
                step(ref, d, w)
        times = {name: [] for name in paths}
        for _ in range(args.reps):
            for name, ref in refs.items():
                times[name].append(timed(ref, d, w))
        row = {"scale": scale, "C": dim, "G": G, "batch": args.batch}
        for name, t in times.items():
            row.update({name + "_ms": statistics.median(t), name + "_min": min(t), name + "_max": max(t)})
        for name, ref in refs.items():
            for other in refs.values():
                other.zero_grad(set_to_none=True)
            row[name + "_peak_mib"] = peak_mib(ref, d, w)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del base, refs, d, w
        torch.cuda.empty_cache()
    print("| C | G | batch | " + " | ".join(f"{name} ms (min .. max), peak MiB" for name in paths) + " |")
    print("|---|---|---|" + "---|" * len(paths))
    for q in rows:
        print(f"| {q['C']} | {q['G']} | {q['batch']} | " +
              " | ".join(f"{q[n + '_ms']:.2f} ({q[n + '_min']:.2f} .. {q[n + '_max']:.2f}), {q[n + '_peak_mib']:.0f}" for n in paths) + " |")


if __name__ == "__main__":
    main()
