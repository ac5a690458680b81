#!/usr/bin/env python3
"""Time the native FPN pyramid (gfnet_amd/model/fpn.py): its HIP path, one fused launch per layer, against its own torch path -- the
library convolutions plus separate BatchNorm, activation, interpolate, cat and add launches that a checkout's FPN runs -- on the same
parameters and inputs.

    python tools/time_fpn.py [--images 64] [--sizes 448 560] [--rounds 7] [--reps 5] [--precision fp32|fp16|tf32] [--out fpn_timing.json]

Per size: every layer on its real input (the maps of one torch-path forward), then the whole pyramid (encoder, merge layer, decoder).
The two paths ALTERNATE round by round; a round is `reps` back-to-back calls between two device events; reported per path are the
median round and the spread (min .. max) over the rounds, in ms per call.  Every shape is warmed up on both paths first (the library
picks its algorithms then).  The largest difference between the two paths' outputs at the timed size is printed beside the times.
--precision fp16 adds two legs to the same alternation: "half", the HIP path in its fp16 class (conv_precision "fp16": fp16 maps, the
matrix core, csrc/fpn_conv_half.hip) on fp16 inputs, and "torch_amp", the torch path under torch.autocast(dtype=float16) on the same
fp16 inputs.  The fp32 HIP leg is the comparator of the fp16 class: the table gives fp32 HIP / half and torch_amp / half per layer and
for the whole pyramid, and for the whole pyramid the gap between the two medians beside the larger min .. max spread of the two legs.
--precision tf32 adds one leg to the alternation: "tf32", the HIP path in the reference's TF32 class (conv_precision "tf32": fp32 maps,
split-bf16 operands on the matrix core, csrc/fpn_conv_tf32.hip) on the same fp32 inputs; the table gives fp32 HIP / tf32 and torch /
tf32 per layer and for the whole pyramid.
Needs a GPU; nothing here falls back."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gfnet_amd.model import fpn  # noqa: E402

FEAT_CHS = [8, 16, 32, 64]
ENCODER = ("conv00", "conv01", "downsample1", "conv10", "conv11", "downsample2", "conv20", "conv21", "downsample3", "conv30", "conv31")


def build(device):
    torch.manual_seed(0)
    mods = {"encoder": fpn.FPNEncoder(FEAT_CHS), "decoder": fpn.FPNDecoder_concat(FEAT_CHS), "merge_layer": fpn.merge_layer(FEAT_CHS[-1])}
    with torch.no_grad():
        for m in mods.values():
            for name, b in m.named_buffers():  # non-trivial statistics: an identity BatchNorm is not what a checkpoint holds
                if name.endswith("running_mean"):
                    b.uniform_(-0.5, 0.5)
                elif name.endswith("running_var"):
                    b.uniform_(0.25, 1.75)
            m.to(device).train(False)
    return mods


PATHS = {"fp32": ("hip", "torch"), "fp16": ("half", "hip", "torch", "torch_amp"), "tf32": ("tf32", "hip", "torch")}
HIP_LEGS = ("hip", "half", "tf32")
PRECISION_OF = {"half": "fp16", "tf32": "tf32"}  # conv_precision of a leg; every other leg is "fp32"


def on_path(path, hip_call, torch_call):
    """One call on a leg: hip_call(half, tf32) for "hip" / "half" / "tf32", torch_call() for "torch", and under fp16 autocast for
    "torch_amp"."""
    if path in HIP_LEGS:
        return hip_call(path == "half", path == "tf32")
    with torch.autocast("cuda", dtype=torch.float16, enabled=path == "torch_amp"):
        return torch_call()


def layer_calls(mods):
    """[(name, inputs(ctx) -> tuple, call(path, *inputs) -> map, key under which the map goes into ctx)] in forward order."""
    enc, dec, merge = mods["encoder"], mods["decoder"], mods["merge_layer"]
    calls, prev = [], "image"
    for name in ENCODER:
        calls.append((name, (prev,), (lambda layer: lambda path, x: on_path(path, lambda half, tf32: layer.run(x, True, half=half, tf32=tf32),
                                                                            lambda: layer.run(x, False)))(getattr(enc, name)), name))
        prev = name

    def run_merge(path, c3, side):
        merge.conv_impl = "hip" if path in HIP_LEGS else "torch"
        merge.conv_precision = PRECISION_OF.get(path, "fp32")
        return on_path(path, lambda half, tf32: merge(c3, side), lambda: merge(c3, side))

    def head(seq):
        return lambda path, x: on_path(path, lambda half, tf32: fpn._hip_layer(*fpn._head(seq), x, half=half, tf32=tf32), lambda: seq(x))

    def inner(seq):
        def run(path, intra, skip):
            return on_path(path, lambda half, tf32: fpn._hip_layer(*fpn._head(seq), intra, x1=skip, up0=True, residual=skip, half=half, tf32=tf32),
                           lambda: skip + seq(torch.cat((fpn._up2(intra), skip), dim=1)))
        return run

    calls.append(("merge_layer", ("conv31", "side"), run_merge, "merged"))
    calls.append(("out0", ("merged",), head(dec.out0), "out0"))
    calls.append(("inner1", ("merged", "conv21"), inner(dec.inner1), "intra1"))
    calls.append(("out1", ("intra1",), head(dec.out1), "out1"))
    calls.append(("inner2", ("intra1", "conv11"), inner(dec.inner2), "intra2"))
    calls.append(("out2", ("intra2",), head(dec.out2), "out2"))
    calls.append(("inner3", ("intra2", "conv01"), inner(dec.inner3), "intra3"))
    calls.append(("out3", ("intra3",), head(dec.out3), "out3"))
    return calls


def pyramid(mods, path, image, side):
    for m in mods.values():
        m.conv_impl = "hip" if path in HIP_LEGS else "torch"
        m.conv_precision = PRECISION_OF.get(path, "fp32")

    def run():
        c0, c1, c2, c3 = mods["encoder"](image)
        return mods["decoder"](c0, c1, c2, mods["merge_layer"](c3, side))
    return on_path(path, lambda half, tf32: run(), run)


def time_pair(fn, rounds, reps, paths=PATHS["fp32"]):
    """fn(path) timed on every leg, alternating round by round: {leg: [ms per call, one per round]}."""
    out = {path: [] for path in paths}
    for path in paths + paths:  # warm-up: code objects, algorithm choice, allocator
        fn(path)
    torch.cuda.synchronize()
    for _ in range(rounds):
        for path in paths:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn(path)
            e1.record()
            e1.synchronize()
            out[path].append(e0.elapsed_time(e1) / reps)
    return out


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--images", type=int, default=64, help="images per call (a 32-pair batch is 64)")
    ap.add_argument("--sizes", type=int, nargs="+", default=[448, 560])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--precision", choices=sorted(PATHS), default="fp32", help="fp16: add the fp16 class and torch's fp16 autocast as legs; tf32: add the TF32 class as a leg")
    ap.add_argument("--out", default=None, help="write the numbers as JSON here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_fpn.py needs a GPU")
    dev = torch.device("cuda")
    mods = build(dev)
    calls = layer_calls(mods)
    paths, fp16 = PATHS[args.precision], args.precision == "fp16"
    result = {"device": torch.cuda.get_device_name(0), "images": args.images, "rounds": args.rounds, "reps": args.reps,
              "precision": args.precision, "sizes": {}}
    with torch.no_grad():
        for size in args.sizes:
            g = torch.Generator(device=dev).manual_seed(size)
            ctx = {"image": torch.rand((args.images, 3, size, size), device=dev, generator=g) * 2 - 1,
                   "side": torch.randn((args.images, FEAT_CHS[-1], size // 8, size // 8), device=dev, generator=g) * 0.5}
            ctx16 = {k: v.half() for k, v in ctx.items()}  # the fp16 legs' inputs: the maps of one forward of the fp16 class
            rows, worst = {}, 0.0
            for name, keys, call, key in calls:
                inputs = tuple(ctx[k] for k in keys)
                ctx[key] = call("torch", *inputs)
                diff = float((call("hip", *inputs) - ctx[key]).abs().max())
                worst = max(worst, diff)
                if fp16:
                    inputs16 = tuple(ctx16[k] for k in keys)
                    ctx16[key] = call("half", *inputs16)
                t = time_pair(lambda path: call(path, *(inputs16 if path in ("half", "torch_amp") else inputs)), args.rounds, args.reps, paths)
                rows[name] = dict({path: summary(t[path]) for path in paths}, max_abs_diff=diff, shape=list(ctx[key].shape))
                if fp16:
                    rows[name]["half_max_abs_diff"] = float((ctx16[key].float() - ctx[key]).abs().max())
                if "tf32" in paths:
                    rows[name]["tf32_max_abs_diff"] = float((call("tf32", *inputs) - ctx[key]).abs().max())
            t = time_pair(lambda path: pyramid(mods, path, ctx["image"], ctx["side"]), args.rounds, args.reps, paths)
            total = {path: summary(t[path]) for path in paths}
            result["sizes"][str(size)] = {"layers": rows, "total": total, "max_abs_diff": worst}
            print(f"\n{args.images} images of {size} x {size} on {result['device']}: ms per call, median (min .. max) of {args.rounds} rounds of {args.reps}")
            print("| layer | output | HIP | torch | torch / HIP |\n|---|---|---|---|---|")
            for name, r in list(rows.items()) + [("whole pyramid", dict(total, shape=[]))]:
                h, c = r["hip"], r["torch"]
                print(f"| {name} | {'x'.join(str(v) for v in r['shape'][1:])} | {h['median_ms']:.3f} ({h['min_ms']:.3f} .. {h['max_ms']:.3f}) | "
                      f"{c['median_ms']:.3f} ({c['min_ms']:.3f} .. {c['max_ms']:.3f}) | {c['median_ms'] / h['median_ms']:.2f} |")
            print(f"largest difference between the two paths over all layers: {worst:.3e}")
            if fp16:
                print("\n| layer | half (fp16 class) | fp32 HIP | torch fp16 autocast | fp32 HIP / half | autocast / half |\n|---|---|---|---|---|---|")
                for name, r in list(rows.items()) + [("whole pyramid", total)]:
                    cells = [f"{r[p]['median_ms']:.3f} ({r[p]['min_ms']:.3f} .. {r[p]['max_ms']:.3f})" for p in ("half", "hip", "torch_amp")]
                    print(f"| {name} | {' | '.join(cells)} | {r['hip']['median_ms'] / r['half']['median_ms']:.2f} | "
                          f"{r['torch_amp']['median_ms'] / r['half']['median_ms']:.2f} |")
                gap = total["hip"]["median_ms"] - total["half"]["median_ms"]
                spread = max(total[p]["max_ms"] - total[p]["min_ms"] for p in ("hip", "half"))
                result["sizes"][str(size)]["gate"] = {"gap_ms": gap, "spread_ms": spread, "met": gap > spread}
                print(f"whole pyramid: fp32 HIP median - half median = {gap:.3f} ms, larger min .. max spread of the two legs {spread:.3f} ms: "
                      f"the fp16 class is {'faster beyond the spread' if gap > spread else 'NOT faster beyond the spread'}")
                print(f"largest |half - torch fp32| over all layers: {max(r['half_max_abs_diff'] for r in rows.values()):.3e}")
            if "tf32" in paths:
                print("\n| layer | tf32 class | fp32 HIP | torch | fp32 HIP / tf32 | torch / tf32 |\n|---|---|---|---|---|---|")
                for name, r in list(rows.items()) + [("whole pyramid", total)]:
                    cells = [f"{r[p]['median_ms']:.3f} ({r[p]['min_ms']:.3f} .. {r[p]['max_ms']:.3f})" for p in ("tf32", "hip", "torch")]
                    print(f"| {name} | {' | '.join(cells)} | {r['hip']['median_ms'] / r['tf32']['median_ms']:.2f} | "
                          f"{r['torch']['median_ms'] / r['tf32']['median_ms']:.2f} |")
                print(f"largest |tf32 - torch fp32| over all layers: {max(r['tf32_max_abs_diff'] for r in rows.values()):.3e}")
            del ctx, ctx16
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
