#!/usr/bin/env python3
"""Time the native FPN pyramid (gfnet_amd/model/fpn.py): its HIP path, one fused launch per layer, against its own torch path -- the
library convolutions plus separate BatchNorm, activation, interpolate, cat and add launches that a checkout's FPN runs -- on the same
parameters and inputs.

    python tools/time_fpn.py [--images 64] [--sizes 448 560] [--rounds 7] [--reps 5] [--out fpn_timing.json]

Per size: every layer on its real input (the maps of one torch-path forward), then the whole pyramid (encoder, merge layer, decoder).
The two paths ALTERNATE round by round; a round is `reps` back-to-back calls between two device events; reported per path are the
median round and the spread (min .. max) over the rounds, in ms per call.  Every shape is warmed up on both paths first (the library
picks its algorithms then).  The largest difference between the two paths' outputs at the timed size is printed beside the times.
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


def layer_calls(mods):
    """[(name, inputs(ctx) -> tuple, call(hip, *inputs) -> map, key under which the map goes into ctx)] in forward order."""
    enc, dec, merge = mods["encoder"], mods["decoder"], mods["merge_layer"]
    calls, prev = [], "image"
    for name in ENCODER:
        calls.append((name, (prev,), (lambda layer: lambda hip, x: layer.run(x, hip))(getattr(enc, name)), name))
        prev = name

    def run_merge(hip, c3, side):
        merge.conv_impl = "hip" if hip else "torch"
        return merge(c3, side)

    def head(seq):
        return lambda hip, x: fpn._hip_layer(*fpn._head(seq), x) if hip else seq(x)

    def inner(seq):
        def run(hip, intra, skip):
            if hip:
                return fpn._hip_layer(*fpn._head(seq), intra, x1=skip, up0=True, residual=skip)
            return skip + seq(torch.cat((fpn._up2(intra), skip), dim=1))
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


def pyramid(mods, hip, image, side):
    for m in mods.values():
        m.conv_impl = "hip" if hip else "torch"
    c0, c1, c2, c3 = mods["encoder"](image)
    return mods["decoder"](c0, c1, c2, mods["merge_layer"](c3, side))


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


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--images", type=int, default=64, help="images per call (a 32-pair batch is 64)")
    ap.add_argument("--sizes", type=int, nargs="+", default=[448, 560])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="write the numbers as JSON here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_fpn.py needs a GPU")
    dev = torch.device("cuda")
    mods = build(dev)
    calls = layer_calls(mods)
    result = {"device": torch.cuda.get_device_name(0), "images": args.images, "rounds": args.rounds, "reps": args.reps, "sizes": {}}
    with torch.no_grad():
        for size in args.sizes:
            g = torch.Generator(device=dev).manual_seed(size)
            ctx = {"image": torch.rand((args.images, 3, size, size), device=dev, generator=g) * 2 - 1,
                   "side": torch.randn((args.images, FEAT_CHS[-1], size // 8, size // 8), device=dev, generator=g) * 0.5}
            rows, worst = {}, 0.0
            for name, keys, call, key in calls:
                inputs = tuple(ctx[k] for k in keys)
                ctx[key] = call(False, *inputs)
                diff = float((call(True, *inputs) - ctx[key]).abs().max())
                worst = max(worst, diff)
                t = time_pair(lambda hip: call(hip, *inputs), args.rounds, args.reps)
                rows[name] = {"hip": summary(t["hip"]), "torch": summary(t["torch"]), "max_abs_diff": diff,
                              "shape": list(ctx[key].shape)}
            t = time_pair(lambda hip: pyramid(mods, hip, ctx["image"], ctx["side"]), args.rounds, args.reps)
            total = {"hip": summary(t["hip"]), "torch": summary(t["torch"])}
            result["sizes"][str(size)] = {"layers": rows, "total": total, "max_abs_diff": worst}
            print(f"\n{args.images} images of {size} x {size} on {result['device']}: ms per call, median (min .. max) of {args.rounds} rounds of {args.reps}")
            print("| layer | output | HIP | torch | torch / HIP |\n|---|---|---|---|---|")
            for name, r in list(rows.items()) + [("whole pyramid", dict(total, shape=[]))]:
                h, c = r["hip"], r["torch"]
                print(f"| {name} | {'x'.join(str(v) for v in r['shape'][1:])} | {h['median_ms']:.3f} ({h['min_ms']:.3f} .. {h['max_ms']:.3f}) | "
                      f"{c['median_ms']:.3f} ({c['min_ms']:.3f} .. {c['max_ms']:.3f}) | {c['median_ms'] / h['median_ms']:.2f} |")
            print(f"largest difference between the two paths over all layers: {worst:.3e}")
            del ctx
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
