#!/usr/bin/env python3
"""Time the native DINOv2 ViT (gfnet_amd/model/dinov2.py) and its two kernels against the torch ops they replace, on the same data.

    python tools/time_vit.py --leg attn|seam|model [--dtype fp16|bf16] [--rounds 7] [--reps 5] [--out vit_timing.json]

  attn    ops.self_attention on the packed fp16 projection against F.scaled_dot_product_attention on the permuted tensors (what the
          reference's Attention.forward runs), B = 64, H = 16, N in 1025, 1601
  seam    ops.ls_add_layernorm (fused, in place) against torch's three ops (LayerScale multiply, residual add, LayerNorm) at
          64 x 1025 x 1024 in fp16
  model   vit_large forward_features with impl "hip" against impl "torch" in fp16, 64 x 3 x 448 x 448 and 16 x 3 x 560 x 560,
          random weights (no checkpoint is needed)

The two paths ALTERNATE round by round; a round is `reps` back-to-back calls between two device events; reported per path are the
median round and the spread (min .. max) over the rounds, in ms per call.  Every shape is warmed up on both paths first.  The
largest difference between the two paths' outputs is printed beside the times.  Run one leg per process.  Needs a GPU; nothing here
falls back.

--dtype bf16 runs all three legs in the bf16 class: tensors and models in bfloat16, ops.self_attention_bf16 for the attention, and
on the torch side the same torch ops on bfloat16 tensors.  The default, fp16, is what the text above describes."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gfnet_amd import ops  # noqa: E402
from gfnet_amd.model import dinov2  # noqa: E402


def time_pair(fn, rounds, reps):
    """fn(hip) timed on both paths, alternating: {"hip": [ms per call, one per round], "torch": [...]}."""
    out = {"hip": [], "torch": []}
    for hip in (True, False, True, False):  # warm-up: code objects, algorithm choice, allocator
        fn(hip)
    torch.cuda.synchronize()
    for _ in range(rounds):
        for path in ("hip", "torch"):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn(path == "hip")
            e1.record()
            e1.synchronize()
            out[path].append(e0.elapsed_time(e1) / reps)
    return out


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def row(name, t, diff, extra=""):
    h, c = summary(t["hip"]), summary(t["torch"])
    print(f"| {name} | {h['median_ms']:.3f} ({h['min_ms']:.3f} .. {h['max_ms']:.3f}) | {c['median_ms']:.3f} ({c['min_ms']:.3f} .. {c['max_ms']:.3f}) | "
          f"{c['median_ms'] / h['median_ms']:.2f} | {diff:.2e} |{extra}", flush=True)
    return {"hip": h, "torch": c, "max_abs_diff": diff}


DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}


def leg_attn(args, dev):
    B, H, D, res = 64, 16, 64, {}
    attn = ops.self_attention_bf16 if args.dtype == "bf16" else ops.self_attention
    print("| B x N x H | HIP | SDPA | SDPA / HIP | max diff | HIP TFLOP/s |\n|---|---|---|---|---|---|")
    for N in (1025, 1601):
        qkv = torch.randn(B, N, 3, H, D, device=dev, dtype=DTYPES[args.dtype])
        q, k, v = qkv.permute(2, 0, 3, 1, 4).unbind(0)

        def fn(hip):
            return attn(qkv, D ** -0.5) if hip else F.scaled_dot_product_attention(q, k, v, scale=D ** -0.5).transpose(1, 2)

        diff = float((fn(True).float() - fn(False).float()).abs().max())
        t = time_pair(fn, args.rounds, args.reps)
        flops = 4.0 * B * H * N * N * D
        res[str(N)] = row(f"{B} x {N} x {H}", t, diff, f" {flops / (statistics.median(t['hip']) * 1e-3) / 1e12:.1f} |")
    return res


def leg_seam(args, dev):
    rows, C = 64 * 1025, 1024
    dtype = DTYPES[args.dtype]
    x0, y = torch.randn(rows, C, device=dev, dtype=dtype), torch.randn(rows, C, device=dev, dtype=dtype)
    gamma, w, b = (torch.rand(C, device=dev, dtype=dtype) + 0.5 for _ in range(3))
    x = x0.clone()

    def fn(hip):
        if hip:
            return ops.ls_add_layernorm(x, y, gamma, w, b, 1e-6, inplace=True)
        xo = x0 + y * gamma
        return xo, F.layer_norm(xo, (C,), w, b, 1e-6)

    x.copy_(x0)
    diff = float((fn(True)[1].float() - fn(False)[1].float()).abs().max())
    print("| rows x C | HIP | torch (mul, add, LayerNorm) | torch / HIP | max diff of h | HIP GB/s |\n|---|---|---|---|---|---|")
    t = time_pair(fn, args.rounds, args.reps)
    moved = 4.0 * rows * C * 2  # x and y read, x and h written
    return {"seam": row(f"{rows} x {C}", t, diff, f" {moved / (statistics.median(t['hip']) * 1e-3) / 1e9:.0f} |")}


def leg_model(args, dev):
    torch.manual_seed(0)
    vit = dinov2.vit_large().to(dev, DTYPES[args.dtype]).train(False)
    res = {}
    print("| images | impl hip | impl torch | torch / hip | max diff of patch tokens |\n|---|---|---|---|---|")
    for B, size in ((64, 448), (16, 560)):
        x = torch.rand(B, 3, size, size, device=dev, dtype=DTYPES[args.dtype]) * 2 - 1

        def fn(hip):
            vit.impl = "hip" if hip else "torch"
            return vit.forward_features(x)["x_norm_patchtokens"]

        diff = float((fn(True).float() - fn(False).float()).abs().max())
        res[f"{B}x{size}"] = row(f"{B} x 3 x {size} x {size}", time_pair(fn, args.rounds, args.reps), diff)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--leg", choices=("attn", "seam", "model"), required=True)
    ap.add_argument("--dtype", choices=tuple(DTYPES), default="fp16", help="the 16-bit class all tensors and models are built in")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="write the numbers as JSON here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_vit.py needs a GPU")
    dev = torch.device("cuda")
    print(f"{args.leg}{'' if args.dtype == 'fp16' else ' in ' + args.dtype} on {torch.cuda.get_device_name(0)}: ms per call, median (min .. max) of {args.rounds} rounds of {args.reps}")
    with torch.no_grad():
        result = {"device": torch.cuda.get_device_name(0), "leg": args.leg, "dtype": args.dtype, "rounds": args.rounds, "reps": args.reps,
                  "rows": {"attn": leg_attn, "seam": leg_seam, "model": leg_model}[args.leg](args, dev)}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
