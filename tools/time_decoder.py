#!/usr/bin/env python3
"""Time the whole cross-view decoder forward with fused blocks against the torch blocks, on the same data (GPU).

    python tools/time_decoder.py [--rounds 7] [--reps 5] [--pairs 32] [--out profiles/decoder_blocks.md]

CrossViewDecoder (gfnet_amd/model/crossview_decoder.py) at d_model 1024, width 64, 8 heads, 4 blocks, under fp16 autocast in
eval(), on `pairs` image pairs (2 * pairs directions) of N = 1024 (the 448 pass) and N = 1600 (the 560 pass) fp16 ViT tokens:
block_impl="hip" (three launches per block: ops.decoder_qkv, ops.cross_attention, ops.decoder_post) against block_impl="torch"
(the same attention launch between torch's LayerNorm, Linear, GELU and element-wise ops), one set of weights.

The two paths ALTERNATE round by round; a round is `reps` back-to-back forwards between two device events; reported per path are
the median round and the spread (min .. max) over the rounds, in ms per forward.  Both are warmed up first.  Then, outside the timed
rounds: the per-kernel share of a fused forward from ops.kernel_events (device events around each launch), and the number of device
kernels one forward launches on each path, counted by torch.profiler.  Prints a markdown report, also written to --out."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gfnet_amd import ops  # noqa: E402
from gfnet_amd.model.crossview_decoder import CrossViewDecoder  # noqa: E402

CONF = {"dino_cfg": {"d_model": 1024, "decoder_cfg": {"num_cross_attn": 4, "init_values": 1.0, "nhead": 8, "attention_type": "FLASH2",
                                                     "ffn_type": "ffn", "softmax_scale": "entropy_invariance", "train_avg_length": 1024}},
        "encoder_cfg": {"feat_chs": [64, 64, 32, 16, 8]}}
KERNELS = ("decoder_qkv", "cross_attn_fwd", "decoder_post")


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


def kernel_share(fn, reps):
    """ms per forward inside each of the fused path's three kernels."""
    ops.kernel_events = {n: [] for n in KERNELS}
    try:
        for _ in range(reps):
            fn("hip")
        torch.cuda.synchronize()
        return {n: sum(a.elapsed_time(b) for a, b in ev) / reps for n, ev in ops.kernel_events.items()}
    finally:
        ops.kernel_events = None


def launches(fn, impl):
    """Device kernels launched by one forward, or None where the profiler is not available."""
    try:
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn(impl)
            torch.cuda.synchronize()
        kernels = [e for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")]
        return len(kernels) or None
    except Exception as e:  # noqa: BLE001 (a report without this column is still a report)
        print(f"(launch count not available: {type(e).__name__}: {e})", file=sys.stderr)
        return None


def fmt(ms):
    return f"{statistics.median(ms):.3f} ({min(ms):.3f} .. {max(ms):.3f})"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=32)
    ap.add_argument("--no-launch-count", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_decoder.py needs a GPU")
    dev = torch.device("cuda")
    torch.manual_seed(0)
    decs = {"torch": CrossViewDecoder(CONF, attn_impl="hip", block_impl="torch").to(dev).train(False)}
    decs["hip"] = CrossViewDecoder(CONF, attn_impl="hip", block_impl="hip").to(dev).train(False)
    decs["hip"].load_state_dict(decs["torch"].state_dict())
    lines = [f"Cross-view decoder forward on {torch.cuda.get_device_name(0)}: d_model 1024, 4 blocks, {args.pairs} pairs "
             f"({2 * args.pairs} directions), fp16 autocast, eval(); ms per forward, median (min .. max) of {args.rounds} alternating rounds "
             f"of {args.reps}.", "",
             "| N | block_impl=\"hip\" | block_impl=\"torch\" | torch / hip | torch's spread | max diff of the maps | kernels per forward, hip | torch |",
             "|---|---|---|---|---|---|---|---|"]
    shares = []
    with torch.no_grad():
        for N, grid in ((1024, (32, 32)), (1600, (40, 40))):
            x, y = (torch.randn(args.pairs, N, 1024, device=dev).half() for _ in range(2))
            shape = (args.pairs, 3) + grid

            def fn(impl):
                with torch.autocast(device_type="cuda", dtype=torch.float16):
                    return decs[impl](x, y, vit_shape=shape)

            with torch.autocast(device_type="cuda", dtype=torch.float16):
                assert decs["hip"]._fused(x, y) and not decs["torch"]._fused(x, y)
            diff = max(float((a - b).abs().max()) for a, b in zip(fn("hip"), fn("torch")))
            t = time_pair(fn, args.rounds, args.reps)
            share = kernel_share(fn, args.reps)
            counts = (None, None) if args.no_launch_count else (launches(fn, "hip"), launches(fn, "torch"))
            mh, mt = statistics.median(t["hip"]), statistics.median(t["torch"])
            lines.append(f"| {N} | {fmt(t['hip'])} | {fmt(t['torch'])} | {mt / mh:.2f} | {max(t['torch']) - min(t['torch']):.3f} | {diff:.2e} | "
                         f"{counts[0] or 'n/a'} | {counts[1] or 'n/a'} |")
            shares.append((N, mh, share))
    lines += ["", "Inside a fused forward (device events around each launch, 4 launches of each per forward; the rest is the entry projection, "
              "the position encoding, the concatenation and launch gaps):", "",
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
