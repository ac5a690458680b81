"""What follows backward() in a training step, timed (GPU): python tools/time_train_step.py [--reps 15] [--warmup 3]

The parameters of the five refiners of the default 448 workload (the widths of gfnet_amd._synthetic, built as GFNet builds them) with
random gradients, stepped two ways:
  torch  the sequence of the reference's trainer/train.py:30-41 on torch's own pieces: GradScaler.unscale_, the two norms per tensor of
         log_param_statistics with its norm of norms and two .item() calls,
         clip_grad_norm_, GradScaler.step(AdamW), GradScaler.update(), the read of the scale and its floor, and the zero_grad of :30
         (timed at the end of the step it follows, as the fused step zeroes the gradients it has read).  No wandb.
  fused  gfnet_amd.trainer.FusedAdamWStep.step(): three launches, no host synchronisation.
Both run in one process, alternating; every timed step is bracketed by device synchronisation and gets fresh scaled gradients first
(untimed); the figure is the median of --reps steps after --warmup untimed ones, the spread their min .. max.  One JSON line, then a
markdown table row for DESIGN 4.4."""
import argparse
import copy
import json
import os
import statistics
import sys
import time

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gfnet_amd._synthetic import DISP, FEAT, RADIUS, SCALES  # noqa: E402
from gfnet_amd.model.network import _refiner_for  # noqa: E402
from gfnet_amd.trainer import FusedAdamWStep  # noqa: E402


def torch_sequence(named, params, optimizer, scaler, max_norm):
    """What trainer/train.py:34-41 and the next step's :30 do after the backward has written the scaled gradients, on the same torch
    calls: one 2-norm per parameter and per gradient, a norm of each stack, three reads of a device scalar on the host."""
    scaler.unscale_(optimizer)
    with_grad = [(name, p) for name, p in named if p.grad is not None]
    p_norm = torch.stack([p.norm(p=2) for _, p in with_grad]).norm(p=2)
    per_tensor = torch.stack([torch.norm(p.grad.detach(), 2) for _, p in with_grad])
    flagged = torch.isinf(per_tensor) | torch.isnan(per_tensor)
    g_norm = torch.norm(per_tensor, 2)
    if torch.any(flagged):                                                       # a host read, as the reference's `if` is
        print("non-finite gradients:", [name for (name, _), f in zip(with_grad, flagged) if f])
    logged = {"grad_norm": g_norm.item(), "param_norm": p_norm.item()}
    torch.nn.utils.clip_grad_norm_(params, max_norm)
    scaler.step(optimizer)
    scaler.update()
    logged["grad_scale"] = scaler._scale.item()
    if bool(scaler._scale < 1.0):                                                # the floor of the scale, with its own host read
        scaler._scale.fill_(1.0)
    optimizer.zero_grad()
    return logged


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    torch.manual_seed(0)
    fused_net = nn.ModuleDict({s: _refiner_for(FEAT[s], DISP[s], RADIUS[i]) for i, s in enumerate(SCALES)}).cuda().train()
    torch_net = copy.deepcopy(fused_net)
    lr, wd, max_norm, scale = 1e-4, 0.01, 0.01, 65536.0
    fused_named, torch_named = list(fused_net.named_parameters()), list(torch_net.named_parameters())
    fused_params, torch_params = [p for _, p in fused_named], [p for _, p in torch_named]
    stepper = FusedAdamWStep(fused_net.named_parameters(), lr=lr, weight_decay=wd, max_norm=max_norm, init_scale=scale)
    optimizer = torch.optim.AdamW(torch_params, lr=lr, weight_decay=wd)
    scaler = torch.amp.GradScaler("cuda", init_scale=scale)
    scaler.scale(torch.zeros((), device="cuda"))                                 # creates the scale tensor, as the first scaled loss would
    gen = torch.Generator(device="cuda").manual_seed(1)
    for p in fused_params:
        p.grad = torch.zeros_like(p)

    def fresh_gradients():
        grads = [torch.randn(p.shape, generator=gen, device="cuda") * (1e-3 * scale) for p in fused_params]
        for p, q, g in zip(fused_params, torch_params, grads):
            p.grad.copy_(g)
            q.grad = g.clone()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6

    def run_torch():
        torch_sequence(torch_named, torch_params, optimizer, scaler, max_norm)

    t_fused, t_torch = [], []
    for k in range(args.warmup + args.reps):
        fresh_gradients()
        a = timed(stepper.step)
        b = timed(run_torch)
        if k >= args.warmup:
            t_fused.append(a)
            t_torch.append(b)
    worst = max(float((p.detach() - q.detach()).abs().max()) for p, q in zip(fused_params, torch_params))
    row = {"tensors": len(fused_params), "elements": sum(p.numel() for p in fused_params), "reps": args.reps,
           "fused_us": statistics.median(t_fused), "fused_min": min(t_fused), "fused_max": max(t_fused),
           "torch_us": statistics.median(t_torch), "torch_min": min(t_torch), "torch_max": max(t_torch),
           "max_param_difference": worst, "device": torch.cuda.get_device_name(0)}
    print(json.dumps(row), flush=True)
    print("| parameter tensors | elements | `FusedAdamWStep.step()` us (min .. max) | torch sequence us (min .. max) | torch / fused |")
    print("|---|---|---|---|---|")
    print(f"| {row['tensors']} | {row['elements']} | {row['fused_us']:.0f} ({row['fused_min']:.0f} .. {row['fused_max']:.0f}) | "
          f"{row['torch_us']:.0f} ({row['torch_min']:.0f} .. {row['torch_max']:.0f}) | {row['torch_us'] / row['fused_us']:.1f} |")


if __name__ == "__main__":
    main()
