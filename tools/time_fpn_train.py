#!/usr/bin/env python3
"""Time the native FPN in TRAINING mode (gfnet_amd/model/fpn.py under train()): forward + backward with train_conv_impl "hip"
(csrc/fpn_conv_train.hip: one op per layer, one saved map per layer) and "hip_fused" (the same with the decoder's 2x upsample inside
the inner1..3 ops: no doubled map) against the module's own torch path on the same commit (F.conv2d, BatchNorm2d on batch statistics,
the activation, F.interpolate, torch.cat and autograd), same parameters and inputs.

    python tools/time_fpn_train.py [--images 16] [--sizes 448] [--rounds 7] [--reps 3] [--precision fp32|tf32] [--out fpn_train_timing.json]

Per size: every layer forward + backward on its real input (the maps of one torch-path forward) with a fixed output gradient, then
the three modules forward + backward, and for those the peak of torch.cuda.max_memory_allocated above what is allocated before the
step.  The paths ALTERNATE round by round ("hip_fused" is timed for inner1..3, the only layers it changes, and for the three
modules); a round is `reps` back-to-back calls between two device events; reported per path are the median round and the spread
(min .. max) over the rounds, in ms per call.  Every shape is warmed up on every path first.
--precision tf32 (the default, fp32, changes nothing) adds the legs "hip_tf32" and "hip_fused_tf32" to the same alternation: the two HIP
paths with conv_precision "tf32" (the forward convolution and the stride-1 input gradient with split-bf16 operands on the matrix core,
csrc/fpn_conv_tf32.hip), and prints them beside the fp32 HIP legs and torch.
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
    for m in mods.values():
        m.to(device).train(True)
    return mods


def layer_calls(mods):
    """[(name, input keys, call(path, *inputs) -> map, parameters, key under which the map goes into ctx)] in forward order; path is
    "torch", "hip" or "hip_fused", the last two also with the suffix "_tf32" for the TF32 class."""
    enc, dec, merge = mods["encoder"], mods["decoder"], mods["merge_layer"]
    calls, prev = [], "image"
    for name in ENCODER:
        layer = getattr(enc, name)
        calls.append((name, (prev,), (lambda layer: lambda path, x: layer.run(x, False, path != "torch", tf32=path.endswith("_tf32")))(layer), list(layer.parameters()), name))
        prev = name

    def run_merge(path, c3, side):
        if path != "torch":
            return fpn._hip_train_layer(*fpn._head(merge), c3, x1=side, residual=c3, tf32=path.endswith("_tf32"))
        return c3 + torch.nn.Sequential.forward(merge, torch.cat((c3, side), dim=1))

    def head(seq):
        return lambda path, x: fpn._hip_train_layer(*fpn._head(seq), x, tf32=path.endswith("_tf32")) if path != "torch" else seq(x)

    def inner(seq):
        def run(path, intra, skip):
            tf32 = path.endswith("_tf32")
            if path.startswith("hip_fused"):
                return fpn._hip_train_layer(*fpn._head(seq), intra, x1=skip, residual=skip, up0=True, tf32=tf32)
            if path.startswith("hip"):
                return fpn._hip_train_layer(*fpn._head(seq), fpn._up2(intra), x1=skip, residual=skip, tf32=tf32)
            return skip + seq(torch.cat((fpn._up2(intra), skip), dim=1))
        return run

    calls.append(("merge_layer", ("conv31", "side"), run_merge, list(merge.parameters()), "merged"))
    calls.append(("out0", ("merged",), head(dec.out0), list(dec.out0.parameters()), "out0"))
    calls.append(("inner1", ("merged", "conv21"), inner(dec.inner1), list(dec.inner1.parameters()), "intra1"))
    calls.append(("out1", ("intra1",), head(dec.out1), list(dec.out1.parameters()), "out1"))
    calls.append(("inner2", ("intra1", "conv11"), inner(dec.inner2), list(dec.inner2.parameters()), "intra2"))
    calls.append(("out2", ("intra2",), head(dec.out2), list(dec.out2.parameters()), "out2"))
    calls.append(("inner3", ("intra2", "conv01"), inner(dec.inner3), list(dec.inner3.parameters()), "intra3"))
    calls.append(("out3", ("intra3",), head(dec.out3), list(dec.out3.parameters()), "out3"))
    return calls


def pyramid_step(mods, path, image, side, gys):
    """The three modules forward and backward: gradients of sum_k (out_k * gy_k).sum() for every parameter and the side map."""
    for m in mods.values():
        m.train_conv_impl = path[:-5] if path.endswith("_tf32") else path
        m.conv_precision = "tf32" if path.endswith("_tf32") else "fp32"
    c0, c1, c2, c3 = mods["encoder"](image)
    outs = mods["decoder"](c0, c1, c2, mods["merge_layer"](c3, side))
    params = [p for m in mods.values() for p in m.parameters()]
    return torch.autograd.grad(outs, [side] + params, gys)


def time_paths(fn, paths, rounds, reps):
    """fn(path) timed on every path, alternating: {path: [ms per call, one per round]}."""
    out = {path: [] for path in paths}
    for path in paths * 2:  # warm-up: code objects, algorithm choice, allocator
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


def peak_bytes(fn):
    """The peak of allocated device memory during fn() above what is allocated before it."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--images", type=int, default=16, help="images per call (an 8-pair batch is 16)")
    ap.add_argument("--sizes", type=int, nargs="+", default=[448])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--precision", choices=("fp32", "tf32"), default="fp32", help="tf32: add the HIP paths in the TF32 class as legs")
    ap.add_argument("--out", default=None, help="write the numbers as JSON here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_fpn_train.py needs a GPU")
    tf32 = args.precision == "tf32"
    dev = torch.device("cuda")
    mods = build(dev)
    calls = layer_calls(mods)
    result = {"device": torch.cuda.get_device_name(0), "images": args.images, "rounds": args.rounds, "reps": args.reps, "precision": args.precision,
              "sizes": {}}
    for size in args.sizes:
        g = torch.Generator(device=dev).manual_seed(size)
        ctx = {"image": torch.rand((args.images, 3, size, size), device=dev, generator=g) * 2 - 1,
               "side": (torch.randn((args.images, FEAT_CHS[-1], size // 8, size // 8), device=dev, generator=g) * 0.5).requires_grad_()}
        rows, worst = {}, 0.0
        for name, keys, call, params, key in calls:
            inputs = tuple(ctx[k] for k in keys)
            paths = ("hip", "hip_fused", "torch") if name.startswith("inner") else ("hip", "torch")
            if tf32:
                paths = tuple(p + "_tf32" for p in paths[:-1]) + paths
            with torch.no_grad():
                ref = call("torch", *inputs)
                diff = max(float((call(path, *inputs) - ref).abs().max()) for path in paths[:-1])
            ctx[key] = ref.detach().requires_grad_()
            worst = max(worst, diff)
            gy = torch.randn(ref.shape, device=dev, generator=g)
            wanted = [t for t in inputs if t.requires_grad] + params

            def step(path, call=call, inputs=inputs, gy=gy, wanted=wanted):
                return torch.autograd.grad(call(path, *inputs), wanted, gy)

            t = time_paths(step, paths, args.rounds, args.reps)
            rows[name] = {**{path: summary(t[path]) for path in paths}, "max_abs_diff": diff, "shape": list(ref.shape)}
            del ref, gy
        side = ctx["side"]
        image = ctx["image"]
        shapes = [ctx[k].shape for k in ("out0", "out1", "out2", "out3")]
        del ctx
        gys = [torch.randn(s, device=dev, generator=g) for s in shapes]
        paths = ("hip_tf32", "hip_fused_tf32") * tf32 + ("hip", "hip_fused", "torch")
        t = time_paths(lambda path: pyramid_step(mods, path, image, side, gys), paths, args.rounds, args.reps)
        total = {path: summary(t[path]) for path in paths}
        memory = {path: peak_bytes(lambda: pyramid_step(mods, path, image, side, gys)) for path in paths}
        result["sizes"][str(size)] = {"layers": rows, "total": total, "peak_bytes": memory, "max_abs_diff": worst}
        print(f"\n{args.images} images of {size} x {size} on {result['device']}, forward + backward: ms per call, median (min .. max) of "
              f"{args.rounds} rounds of {args.reps}")
        print("| layer | output | HIP | HIP fused | torch | torch / HIP | torch / HIP fused |\n|---|---|---|---|---|---|---|")

        def cell(r):
            return f"{r['median_ms']:.3f} ({r['min_ms']:.3f} .. {r['max_ms']:.3f})" if r else ""

        for name, r in list(rows.items()) + [("three modules", dict(total, shape=[]))]:
            h, f, c = r["hip"], r.get("hip_fused"), r["torch"]
            print(f"| {name} | {'x'.join(str(v) for v in r['shape'][1:])} | {cell(h)} | {cell(f)} | {cell(c)} | "
                  f"{c['median_ms'] / h['median_ms']:.2f} | {c['median_ms'] / f['median_ms']:.2f} |" if f else
                  f"| {name} | {'x'.join(str(v) for v in r['shape'][1:])} | {cell(h)} | | {cell(c)} | {c['median_ms'] / h['median_ms']:.2f} | |")
        print(f"peak memory of one step above the resident tensors: HIP {memory['hip'] / 2 ** 20:.0f} MiB, HIP fused "
              f"{memory['hip_fused'] / 2 ** 20:.0f} MiB, torch {memory['torch'] / 2 ** 20:.0f} MiB")
        print(f"largest difference between the two paths' layer outputs: {worst:.3e}")
        if tf32:
            print("\n| layer | HIP tf32 | HIP fused tf32 | HIP | HIP fused | torch | HIP / HIP tf32 | HIP fused / HIP fused tf32 | torch / HIP tf32 | "
                  "torch / HIP fused tf32 |\n|---|---|---|---|---|---|---|---|---|---|")
            for name, r in list(rows.items()) + [("three modules", total)]:
                ratio = lambda a, b: f"{r[a]['median_ms'] / r[b]['median_ms']:.2f}" if a in r and b in r else ""
                print(f"| {name} | {cell(r['hip_tf32'])} | {cell(r.get('hip_fused_tf32'))} | {cell(r['hip'])} | {cell(r.get('hip_fused'))} | "
                      f"{cell(r['torch'])} | {ratio('hip', 'hip_tf32')} | {ratio('hip_fused', 'hip_fused_tf32')} | {ratio('torch', 'hip_tf32')} | "
                      f"{ratio('torch', 'hip_fused_tf32')} |")
            print(f"peak memory of one step: HIP tf32 {memory['hip_tf32'] / 2 ** 20:.0f} MiB, HIP fused tf32 {memory['hip_fused_tf32'] / 2 ** 20:.0f} MiB")
        del gys, image, side
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
