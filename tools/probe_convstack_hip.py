"""Timing probe (GPU): refiner conv stacks on the bench shapes -- HIP (csrc/conv_stack.hip) per kernel.
PROBE_VARIANTS=0,2 (default): gfn_conv_block_fwd variants on fp32 maps, the stack and its first block.
PROBE_PRECISIONS=amp,bf16 (instead): the 16-bit map classes (csrc/conv_stack_half.hip, csrc/conv_stack_bf16.hip) through
ConvRefiner.conv_precision, alternating PROBE_ROUNDS (3) times in one process; per shape the median over PROBE_ITERS (20) timed
stacks of each round, and at the end bf16 / amp per shape and over the step from the medians of the rounds."""
import os, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gfnet_amd import ops
from gfnet_amd.model.network import _refiner_for

shapes448 = [("16", 64, 64, 7, 32), ("8", 64, 64, 6, 32), ("4", 32, 32, 4, 64), ("2", 16, 16, 2, 128), ("1", 8, 8, 0, 256)]
shapes560 = [("8", 64, 64, 6, 40), ("4", 32, 32, 4, 80), ("2", 16, 16, 2, 160), ("1", 8, 8, 0, 320)]
B = int(os.environ.get("PROBE_B", 64))


def timeit(fn, n=3):
    for _ in range(2): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


for variant in [int(v) for v in os.environ.get("PROBE_VARIANTS", "" if os.environ.get("PROBE_PRECISIONS") else "0,2").split(",") if v]:
    total = 0.0
    for name, shapes in (("448", shapes448), ("560", shapes560)):
        for (s, feat, disp, r, G) in shapes:
            ref = _refiner_for(feat, disp, r).cuda().eval()
            C = ref.block1[0].in_channels
            d = torch.randn(B, C, G, G, device="cuda")
            with torch.no_grad():
                ms = timeit(lambda: ref.conv_stack(d, variant=variant))
                fold, _ = ref.folded_stack()
                y = torch.empty_like(d)
                t = torch.empty_like(d)
                ms_blk = timeit(lambda: ops.conv_block(d, fold[0][0], C, out=y, variant=variant, t_scratch=t))
            total += ms
            byts = B * C * G * G * 4
            fl = 2.0 * B * C * C * G * G
            print(f"variant={variant} pass {name} scale {s}: C={C} G={G}: stack {ms:.2f} ms | block {ms_blk*1e3:.0f} us "
                  f"({fl/ms_blk/1e9:.1f} TFLOP/s, {2*byts/ms_blk/1e9:.2f} TB/s x+y)", flush=True)
    print(f"variant={variant}: HIP conv stacks total per step ({B} directions, 448+560): {total:.1f} ms", flush=True)


def medians(fn, iters):
    """median device time in ms of one call, each call between its own pair of events"""
    for _ in range(3): fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for e0, e1 in ev:
        e0.record(); fn(); e1.record()
    torch.cuda.synchronize()
    return sorted(e0.elapsed_time(e1) for e0, e1 in ev)[iters // 2]


precisions = [p for p in os.environ.get("PROBE_PRECISIONS", "").split(",") if p]
if precisions:
    rounds, iters = int(os.environ.get("PROBE_ROUNDS", 3)), int(os.environ.get("PROBE_ITERS", 20))
    cases = []
    for name, shapes in (("448", shapes448), ("560", shapes560)):
        for (s, feat, disp, r, G) in shapes:
            ref = _refiner_for(feat, disp, r).cuda().eval()
            C = ref.block1[0].in_channels
            cases.append((f"pass {name} scale {s}: C={C} G={G}", ref, torch.randn(B, C, G, G, device="cuda")))
    ms = {p: [[] for _ in cases] for p in precisions}
    with torch.no_grad():
        for rnd in range(rounds):
            for p in precisions:
                for i, (label, ref, d) in enumerate(cases):
                    ref.conv_precision = p
                    ms[p][i].append(medians(lambda: ref.conv_stack(d), iters))
                print(f"round {rnd} {p}: " + " ".join(f"{v[-1]:.3f}" for v in ms[p]) + f" | step {sum(v[-1] for v in ms[p]):.2f} ms", flush=True)
    med = {p: [sorted(v)[len(v) // 2] for v in ms[p]] for p in precisions}
    for i, (label, _, _) in enumerate(cases):
        print(f"{label}: " + " ".join(f"{p} {med[p][i]:.3f} ms" for p in precisions) +
              (f" | {precisions[-1]}/{precisions[0]} {med[precisions[-1]][i] / med[precisions[0]][i]:.3f}" if len(precisions) > 1 else ""), flush=True)
    print(f"nine-block stacks per step ({B} directions, 448+560): " + " ".join(f"{p} {sum(med[p]):.2f} ms" for p in precisions) +
          (f" | {precisions[-1]}/{precisions[0]} {sum(med[precisions[-1]]) / sum(med[precisions[0]]):.3f}" if len(precisions) > 1 else ""), flush=True)
