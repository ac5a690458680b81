"""The photometric augmentation of one batch, timed (GPU): python tools/bench_photometric.py [--reps 30] [--warmup 5] [--cpu-images 4] [--cpu-reps 5]

One batch of 16 decoded uint8 images of 853 x 1137 (white noise, already on the device) under the online preset of the reference's
train.py:74-79: Resize(640) -> 640 x 853, ColorJitter(0.2, 0.2, 0.2, 0.2), a blur on every second image.  The parameters are drawn
once (seeded) so that every repetition does the same work; the draws and the table upload are inside the timed call, as they are in
`PhotometricAugment.__call__`.
  device  ops.photo_augment(images, params, resize=640): device events around the call on the launch stream, after --warmup untimed
          calls; the figure is the median of --reps, the spread their min .. max.  The three launches are then timed one by one with
          events of their own, and counted.
  cpu     the same chain through Pillow (`reference_photometric`, i.e. Image.resize, ImageEnhance, the HSV round trip, GaussianBlur)
          on ONE core, for the first --cpu-images images of the batch, scaled to 16: a host clock around each of --cpu-reps passes
          after one warm-up pass, median and min .. max; only where Pillow is installed.  The outputs of
          those images are compared with the device's (values that differ, of all).
One JSON line; bytes are what the algorithm has to move (uint8 source read, uint8 intermediate written and read, float planes
written), from the shapes."""
import argparse
import json
import os
import random
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gfnet_amd import ops  # noqa: E402
from gfnet_amd.datasets import draw_photometric, reference_photometric  # noqa: E402

BATCH, SRC, SIZE = 16, (853, 1137), 640


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cpu-images", type=int, default=4)
    ap.add_argument("--cpu-reps", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_photometric needs a GPU"
    gen = torch.Generator().manual_seed(0)
    images = [torch.randint(0, 256, SRC + (3,), generator=gen, dtype=torch.uint8).cuda() for _ in range(BATCH)]
    params = draw_photometric(BATCH, generator=torch.Generator().manual_seed(1), rng=random.Random(2))
    for i, p in enumerate(params):                                              # blur on exactly half of the batch
        p["blur_radius"] = None if i % 2 else 0.1 + 1.9 * i / (BATCH - 2)
    oh, ow = ops.resize_output_size(*SRC, SIZE)

    times = []
    for k in range(args.warmup + args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        out = ops.photo_augment(images, params, resize=SIZE)
        e1.record()
        torch.cuda.synchronize()
        if k >= args.warmup:
            times.append(e0.elapsed_time(e1) * 1e3)
    names = ("photo_resize", "photo_stats", "photo_jitter_blur")
    per = {n: [] for n in names}
    for _ in range(args.reps):
        ops.kernel_events = {n: [] for n in names}
        ops.photo_augment(images, params, resize=SIZE)
        torch.cuda.synchronize()
        for n in names:
            per[n].append(sum(a.elapsed_time(b) for a, b in ops.kernel_events[n]) * 1e3)
        launches = sum(len(v) for v in ops.kernel_events.values())
    ops.kernel_events = None
    row = {"batch": BATCH, "source": list(SRC), "output": [oh, ow], "reps": args.reps, "device": torch.cuda.get_device_name(0),
           "device_us": statistics.median(times), "device_min": min(times), "device_max": max(times),
           "launches_per_batch": launches, "uploads_per_batch": 1,
           "launch_us": {n: statistics.median(v) for n, v in per.items()},
           "bytes": {"source_read": BATCH * 3 * SRC[0] * SRC[1], "resized_written": BATCH * 3 * oh * ow,
                     "resized_read_stats_and_jitter": 2 * BATCH * 3 * oh * ow, "float_written": BATCH * 12 * oh * ow}}
    try:
        import PIL
    except ImportError:
        row["cpu_us"] = None
    else:
        torch.set_num_threads(1)
        n = min(args.cpu_images, BATCH)
        host = [t.cpu().numpy() for t in images[:n]]
        cpu = []
        for k in range(1 + args.cpu_reps):                                      # one warm-up pass, then the timed ones
            t0 = time.perf_counter()
            ref = [reference_photometric(im, p, SIZE) for im, p in zip(host, params)]
            if k:
                cpu.append((time.perf_counter() - t0) * 1e6 * BATCH / n)
        row["cpu_us"], row["cpu_min"], row["cpu_max"] = statistics.median(cpu), min(cpu), max(cpu)
        row["cpu_images_timed"], row["cpu_reps"], row["pillow"] = n, args.cpu_reps, PIL.__version__
        u8 = ops.photo_augment(images[:n], params[:n], out="uint8", resize=SIZE)
        row["values_differing_from_pillow"] = int(sum((torch.from_numpy(r).cuda() != g).sum() for r, g in zip(ref, u8)))
        row["values_compared"] = int(sum(r.size for r in ref))
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
