#!/usr/bin/env python3
"""Time forward plus backward of the whole cross-view decoder in train(): blocks trained in HIP against the torch blocks (GPU).

    python tools/time_decoder_train.py [--rounds 7] [--reps 3] [--pairs 16] [--amp both] [--out profiles/decoder_train.md]

CrossViewDecoder (gfnet_amd/model/crossview_decoder.py) at d_model 1024, width 64, 8 heads, 4 blocks, under autocast in train(), on
`pairs` image pairs (2 * pairs directions) of N = 1024 (the 448 pass) and N = 1600 (the 560 pass) ViT tokens in the autocast dtype
(--amp fp16, bf16 or both, the default: a bf16 row stands under its fp16 row with its ratio to it):
train_block_impl="hip" (per block ops.decoder_qkv_train, ops.cross_attention, ops.decoder_post_train and their backward kernels)
against train_block_impl="torch" (the same attention launches between torch's LayerNorm, Linear, GELU and element-wise ops and their
autograd), one set of weights.  A step is the forward, sum(map_x * G) + sum(map_y * G) and its backward to every parameter.

The paths ALTERNATE round by round; a round is `reps` back-to-back steps between two device events; reported per path are the
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
from tools.time_decoder import AMP, CONF, fmt, launches, time_paths  # noqa: E402

KERNELS = ("decoder_qkv", "cross_attn_fwd", "decoder_post", "decoder_post_bwd", "cross_attn_bwd", "decoder_qkv_bwd")


def peak_mib(fn):
    """Peak allocated memory of one step above what was allocated before it, MiB."""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def kernel_share(fn, reps):
    ops.kernel_events = {n: [] for n in KERNELS}
    try:
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return {n: sum(a.elapsed_time(b) for a, b in ev) / reps for n, ev in ops.kernel_events.items()}
    finally:
        ops.kernel_events = None


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=16)
    ap.add_argument("--amp", choices=("fp16", "bf16", "both"), default="both")
    ap.add_argument("--no-launch-count", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    amps = ("fp16", "bf16") if args.amp == "both" else (args.amp,)
    if not torch.cuda.is_available():
        sys.exit("time_decoder_train.py needs a GPU")
    dev = torch.device("cuda")
    torch.manual_seed(0)
    decs = {"torch": CrossViewDecoder(CONF, attn_impl="hip", train_block_impl="torch").to(dev).train()}
    decs["hip"] = CrossViewDecoder(CONF, attn_impl="hip", train_block_impl="hip").to(dev).train()
    decs["hip"].load_state_dict(decs["torch"].state_dict())
    lines = [f"Cross-view decoder forward + backward on {torch.cuda.get_device_name(0)}: d_model 1024, 4 blocks, {args.pairs} pairs "
             f"({2 * args.pairs} directions), autocast, train(); ms per step, median (min .. max) of {args.rounds} alternating rounds "
             f"of {args.reps}.", "",
             "| N | autocast | train_block_impl=\"hip\" | train_block_impl=\"torch\" | torch / hip | hip / hip fp16 | torch's spread | "
             "peak MiB, hip | torch | kernels per step, hip | torch |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    shares = []
    for N, grid in ((1024, (32, 32)), (1600, (40, 40))):
        tokens = [torch.randn(args.pairs, N, 1024, device=dev) for _ in range(2)]
        G = torch.randn(args.pairs, 64, *grid, device=dev)
        shape = (args.pairs, 3) + grid

        def path(impl, amp):  # (the tokens are converted once, outside what is timed: the ViT hands them over in this dtype)
            x, y = (t.to(AMP[amp]) for t in tokens)
            dec = decs[impl]

            def step():
                for p in dec.parameters():
                    p.grad = None
                with torch.autocast(device_type="cuda", dtype=AMP[amp]):
                    mx, my = dec(x, y, vit_shape=shape)
                ((mx * G).sum() + (my * G).sum()).backward()
            with torch.autocast(device_type="cuda", dtype=AMP[amp]):
                assert dec._train_fused(x, y) == (impl == "hip")
            return step

        fns = {(impl, amp): path(impl, amp) for amp in amps for impl in ("hip", "torch")}
        t = time_paths(fns, args.rounds, args.reps)
        for amp in amps:
            mem = peak_mib(fns["hip", amp]), peak_mib(fns["torch", amp])
            share = kernel_share(fns["hip", amp], args.reps)
            counts = (None, None) if args.no_launch_count else (launches(fns["hip", amp]), launches(fns["torch", amp]))
            th, tt = t["hip", amp], t["torch", amp]
            mh, mt = statistics.median(th), statistics.median(tt)
            vs16 = f"{mh / statistics.median(t['hip', 'fp16']):.2f}" if "fp16" in amps else "n/a"
            lines.append(f"| {N} | {amp} | {fmt(th)} | {fmt(tt)} | {mt / mh:.2f} | {vs16} | {max(tt) - min(tt):.3f} | {mem[0]:.0f} | "
                         f"{mem[1]:.0f} | {counts[0] or 'n/a'} | {counts[1] or 'n/a'} |")
            shares.append((f"{N} {amp}", mh, share))
    lines += ["", "Inside a HIP step (device events around each op, 4 of each per step; the rest is the entry projection and its backward, the "
              "position encoding, the concatenation, the loss and launch gaps):", "",
              "| N, autocast | " + " | ".join(KERNELS) + " | rest |", "|---|" + "---|" * (len(KERNELS) + 1)]
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
