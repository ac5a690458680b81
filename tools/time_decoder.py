#!/usr/bin/env python3
"""Time the whole cross-view decoder forward with fused blocks against the torch blocks, on the same data (GPU).

    python tools/time_decoder.py [--rounds 7] [--reps 5] [--pairs 32] [--amp both] [--out profiles/decoder_blocks.md]

CrossViewDecoder (gfnet_amd/model/crossview_decoder.py) at d_model 1024, width 64, 8 heads, 4 blocks, under autocast in eval(), on
`pairs` image pairs (2 * pairs directions) of N = 1024 (the 448 pass) and N = 1600 (the 560 pass) ViT tokens in the autocast dtype:
block_impl="hip" (three launches per block: ops.decoder_qkv, ops.cross_attention, ops.decoder_post) against block_impl="torch"
(the same attention launch between torch's LayerNorm, Linear, GELU and element-wise ops), one set of weights.  --amp fp16, bf16 or
both (the default): the autocast classes timed; with both, a bf16 row stands under its fp16 row with its ratio to it, and the bf16
class takes ops.cross_attention_bf16 and the bf16 block kernels.

The paths ALTERNATE round by round; a round is `reps` back-to-back forwards between two device events; reported per path are
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


AMP = {"fp16": torch.float16, "bf16": torch.bfloat16}


def time_paths(fns, rounds, reps):
    """fns: name -> callable; every path once per round, in turn; name -> ms per call of every round."""
    out = {k: [] for k in fns}
    for _ in range(2):  # warm-up: code objects, GEMM algorithm choice, allocator
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            e1.synchronize()
            out[k].append(e0.elapsed_time(e1) / reps)
    return out


def kernel_share(fn, reps):
    """ms per forward inside each of the fused path's three kernels."""
    ops.kernel_events = {n: [] for n in KERNELS}
    try:
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return {n: sum(a.elapsed_time(b) for a, b in ev) / reps for n, ev in ops.kernel_events.items()}
    finally:
        ops.kernel_events = None


def launches(fn, *args):
    """Device kernels launched by one call fn(*args), or None where the profiler is not available."""
    try:
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn(*args)
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
    ap.add_argument("--amp", choices=("fp16", "bf16", "both"), default="both")
    ap.add_argument("--no-launch-count", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    amps = ("fp16", "bf16") if args.amp == "both" else (args.amp,)
    if not torch.cuda.is_available():
        sys.exit("time_decoder.py needs a GPU")
    dev = torch.device("cuda")
    torch.manual_seed(0)
    decs = {"torch": CrossViewDecoder(CONF, attn_impl="hip", block_impl="torch").to(dev).train(False)}
    decs["hip"] = CrossViewDecoder(CONF, attn_impl="hip", block_impl="hip").to(dev).train(False)
    decs["hip"].load_state_dict(decs["torch"].state_dict())
    lines = [f"Cross-view decoder forward on {torch.cuda.get_device_name(0)}: d_model 1024, 4 blocks, {args.pairs} pairs "
             f"({2 * args.pairs} directions), autocast, eval(); ms per forward, median (min .. max) of {args.rounds} alternating rounds "
             f"of {args.reps}.", "",
             "| N | autocast | block_impl=\"hip\" | block_impl=\"torch\" | torch / hip | hip / hip fp16 | torch's spread | max diff of the maps | "
             "kernels per forward, hip | torch |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    shares = []
    with torch.no_grad():
        for N, grid in ((1024, (32, 32)), (1600, (40, 40))):
            tokens = [torch.randn(args.pairs, N, 1024, device=dev) for _ in range(2)]
            shape = (args.pairs, 3) + grid

            def path(impl, amp):  # (the tokens are converted once, outside what is timed: the ViT hands them over in this dtype)
                x, y = (t.to(AMP[amp]) for t in tokens)

                def run():
                    with torch.autocast(device_type="cuda", dtype=AMP[amp]):
                        return decs[impl](x, y, vit_shape=shape)
                return run

            for amp in amps:
                x, y = (t.to(AMP[amp]) for t in tokens)
                with torch.autocast(device_type="cuda", dtype=AMP[amp]):
                    assert decs["hip"]._fused(x, y) and not decs["torch"]._fused(x, y)
            fns = {(impl, amp): path(impl, amp) for amp in amps for impl in ("hip", "torch")}
            t = time_paths(fns, args.rounds, args.reps)
            for amp in amps:
                diff = max(float((a - b).abs().max()) for a, b in zip(fns["hip", amp](), fns["torch", amp]()))
                share = kernel_share(fns["hip", amp], args.reps)
                counts = (None, None) if args.no_launch_count else (launches(fns["hip", amp]), launches(fns["torch", amp]))
                th, tt = t["hip", amp], t["torch", amp]
                mh, mt = statistics.median(th), statistics.median(tt)
                vs16 = f"{mh / statistics.median(t['hip', 'fp16']):.2f}" if "fp16" in amps else "n/a"
                lines.append(f"| {N} | {amp} | {fmt(th)} | {fmt(tt)} | {mt / mh:.2f} | {vs16} | {max(tt) - min(tt):.3f} | {diff:.2e} | "
                             f"{counts[0] or 'n/a'} | {counts[1] or 'n/a'} |")
                shares.append((f"{N} {amp}", mh, share))
    lines += ["", "Inside a fused forward (device events around each launch, 4 launches of each per forward; the rest is the entry projection, "
              "the position encoding, the concatenation and launch gaps):", "",
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
