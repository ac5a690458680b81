#!/usr/bin/env python3
"""Time forward plus backward of the whole cross-view decoder in train(): blocks trained in HIP against the torch blocks (GPU).

    python tools/time_decoder_train.py [--rounds 7] [--reps 3] [--pairs 16] [--out profiles/decoder_train.md]

CrossViewDecoder (gfnet_amd/model/crossview_decoder.py) at d_model 1024, width 64, 8 heads, 4 blocks, under fp16 autocast in
train(), on `pairs` image pairs (2 * pairs directions) of N = 1024 (the 448 pass) and N = 1600 (the 560 pass) fp16 ViT tokens:
train_block_impl="hip" (per block ops.decoder_qkv_train, ops.cross_attention, ops.decoder_post_train and their backward kernels)
against train_block_impl="torch" (the same attention launches between torch's LayerNorm, Linear, GELU and element-wise ops and their
autograd), one set of weights.  A step is the forward, sum(map_x * G) + sum(map_y * G) and its backward to every parameter.

The two paths ALTERNATE round by round; a round is `reps` back-to-back steps between two device events; reported per path are the
median round and the spread (min .. max) over the rounds, in ms per step.  Both are warmed up first.  Then, outside the timed
rounds: the peak allocated memory of one step above what is allocated before it, the per-kernel share of a HIP step from
ops.kernel_events, and the number of device kernels one step launches on each path, counted by torch.profiler.  Prints a markdown
report, also written to --out."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gfnet_amd import ops  # noqa: E402
from gfnet_amd.model.crossview_decoder import CrossViewDecoder  # noqa: E402
from tools.time_decoder import CONF, fmt, launches  # noqa: E402

KERNELS = ("decoder_qkv", "cross_attn_fwd", "decoder_post", "decoder_post_bwd", "cross_attn_bwd", "decoder_qkv_bwd")


def time_pair(fn, rounds, reps):
    out = {"hip": [], "torch": []}
    for impl in ("hip", "torch", "hip", "torch"):  # warm-up: code objects, GEMM algorithm choice, allocator
        fn(impl)
    torch.cuda.synchronize()
    for _ in range(rounds):
        for impl in ("hip", "torch"):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn(impl)
            e1.record()
            e1.synchronize()
            out[impl].append(e0.elapsed_time(e1) / reps)
    return out


def peak_mib(fn, impl):
    """Peak allocated memory of one step above what was allocated before it, MiB."""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn(impl)
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def kernel_share(fn, reps):
    ops.kernel_events = {n: [] for n in KERNELS}
    try:
        for _ in range(reps):
            fn("hip")
        torch.cuda.synchronize()
        return {n: sum(a.elapsed_time(b) for a, b in ev) / reps for n, ev in ops.kernel_events.items()}
    finally:
        ops.kernel_events = None


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=16)
    ap.add_argument("--no-launch-count", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_decoder_train.py needs a GPU")
    dev = torch.device("cuda")
    torch.manual_seed(0)
    decs = {"torch": CrossViewDecoder(CONF, attn_impl="hip", train_block_impl="torch").to(dev).train()}
    decs["hip"] = CrossViewDecoder(CONF, attn_impl="hip", train_block_impl="hip").to(dev).train()
    decs["hip"].load_state_dict(decs["torch"].state_dict())
    lines = [f"Cross-view decoder forward + backward on {torch.cuda.get_device_name(0)}: d_model 1024, 4 blocks, {args.pairs} pairs "
             f"({2 * args.pairs} directions), fp16 autocast, train(); ms per step, median (min .. max) of {args.rounds} alternating rounds "
             f"of {args.reps}.", "",
             "| N | train_block_impl=\"hip\" | train_block_impl=\"torch\" | torch / hip | torch's spread | peak MiB, hip | torch | "
             "kernels per step, hip | torch |",
             "|---|---|---|---|---|---|---|---|---|"]
    shares = []
    for N, grid in ((1024, (32, 32)), (1600, (40, 40))):
        x, y = (torch.randn(args.pairs, N, 1024, device=dev).half() for _ in range(2))
        G = torch.randn(args.pairs, 64, *grid, device=dev)
        shape = (args.pairs, 3) + grid

        def fn(impl):
            dec = decs[impl]
            for p in dec.parameters():
                p.grad = None
            with torch.autocast(device_type="cuda", dtype=torch.float16):
                mx, my = dec(x, y, vit_shape=shape)
            ((mx * G).sum() + (my * G).sum()).backward()

        with torch.autocast(device_type="cuda", dtype=torch.float16):
            assert decs["hip"]._train_fused(x, y) and not decs["torch"]._train_fused(x, y)
        t = time_pair(fn, args.rounds, args.reps)
        mem = peak_mib(fn, "hip"), peak_mib(fn, "torch")
        share = kernel_share(fn, args.reps)
        counts = (None, None) if args.no_launch_count else (launches(fn, "hip"), launches(fn, "torch"))
        mh, mt = statistics.median(t["hip"]), statistics.median(t["torch"])
        lines.append(f"| {N} | {fmt(t['hip'])} | {fmt(t['torch'])} | {mt / mh:.2f} | {max(t['torch']) - min(t['torch']):.3f} | {mem[0]:.0f} | "
                     f"{mem[1]:.0f} | {counts[0] or 'n/a'} | {counts[1] or 'n/a'} |")
        shares.append((N, mh, share))
    lines += ["", "Inside a HIP step (device events around each op, 4 of each per step; the rest is the entry projection and its backward, the "
              "position encoding, the concatenation, the loss and launch gaps):", "",
              "| N | " + " | ".join(KERNELS) + " | rest |", "|---|" + "---|" * (len(KERNELS) + 1)]
    for N, total, share in shares:
        rest = total - sum(share.values())
        lines.append(f"| {N} | " + " | ".join(f"{share[n]:.3f} ms ({100 * share[n] / total:.0f} %)" for n in KERNELS)
                     + f" | {rest:.3f} ms ({100 * rest / total:.0f} %) |")
    report = "\n".join(lines) + "\n"
    print(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(report)


if __name__ == "__main__":
    main()
