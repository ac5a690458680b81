"""The decoder's attention core at the workload's shapes, timed (GPU): python tools/probe_cross_attn.py [--reps 20] [--warmup 5] [--out FILE.md]

ops.cross_attention (csrc/cross_attn.hip) against F.scaled_dot_product_attention on the same tensors -- the only alternative a user
has without flash-attn -- at 2B = 64 directions, N = 1024 (the 448 pass) and 1600 (the 560 pass), 8 heads of dim 8, fp16: forward,
and forward + backward.  SDPA takes (B, H, N, D), so its timed call includes the transposes from and to the (B, N, H, D) layout the
decoder's projections produce, as a user's replacement would.

Both run in one process, alternating per repetition; every timed call is bracketed by device events after --warmup untimed calls
of each; the figure is the median of --reps calls, the spread their min .. max.  Outputs are compared first (same inputs) and the
largest difference printed.  Prints one JSON line and a markdown table (also written to --out)."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gfnet_amd import ops  # noqa: E402


def sdpa(q, k, v, scale):
    return F.scaled_dot_product_attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2), scale=scale).transpose(1, 2)


def timed(fn, reps_events):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    reps_events.append((e0, e1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    rows, result = [], {"device": torch.cuda.get_device_name(0), "batch": args.batch, "reps": args.reps, "cases": []}
    for N in (1024, 1600):
        g = torch.Generator(device="cuda").manual_seed(N)
        q, k, v, dout = (torch.randn(args.batch, N, 8, 8, device="cuda", dtype=torch.float16, generator=g) for _ in range(4))
        scale = 8 ** -0.5 * (torch.log(torch.tensor(float(N))) / torch.log(torch.tensor(1024.0))).item()
        diff = float((ops.cross_attention(q, k, v, scale).float() - sdpa(q, k, v, scale).float()).abs().max())

        def fwd(attend):
            with torch.no_grad():
                attend(q, k, v, scale)

        def fwd_bwd(attend):
            a, b, c = (t.detach().requires_grad_() for t in (q, k, v))
            attend(a, b, c, scale).backward(dout)

        for what, step in (("forward", fwd), ("forward+backward", fwd_bwd)):
            events = {"hip": [], "sdpa": []}
            for i in range(args.warmup + args.reps):
                for name, attend in (("hip", ops.cross_attention), ("sdpa", sdpa)):
                    timed(lambda: step(attend), events[name] if i >= args.warmup else [])
            torch.cuda.synchronize()
            ms = {name: sorted(a.elapsed_time(b) for a, b in ev) for name, ev in events.items()}
            med = {name: statistics.median(t) for name, t in ms.items()}
            # useful work: 4 N^2 D flops per (batch, head) forward (QK^T and PV), 2.5x that again for the backward's five products
            flops = 4 * N * N * 8 * args.batch * 8 * (1 if what == "forward" else 3.5)
            result["cases"].append({"N": N, "what": what, "hip_ms": med["hip"], "hip_min": ms["hip"][0], "hip_max": ms["hip"][-1],
                                    "sdpa_ms": med["sdpa"], "sdpa_min": ms["sdpa"][0], "sdpa_max": ms["sdpa"][-1],
                                    "hip_tflops": flops / med["hip"] / 1e9, "max_abs_diff_fwd": diff})
            rows.append(f"| {N} | {what} | {med['hip']:.3f} ({ms['hip'][0]:.3f} .. {ms['hip'][-1]:.3f}) | "
                        f"{med['sdpa']:.3f} ({ms['sdpa'][0]:.3f} .. {ms['sdpa'][-1]:.3f}) | {med['sdpa'] / med['hip']:.2f} | "
                        f"{flops / med['hip'] / 1e9:.1f} |")
    print(json.dumps(result))
    table = "\n".join(["| N | pass | cross_attn.hip ms: median (min .. max) | SDPA ms: median (min .. max) | SDPA / HIP | HIP TFLOP/s |",
                       "|---|---|---|---|---|---|"] + rows)
    print(table)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(table + "\n\n" + json.dumps(result) + "\n")


if __name__ == "__main__":
    main()
