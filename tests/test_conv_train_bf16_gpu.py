"""GPU: the refiner conv block in the bf16 autocast training class (ops.conv_block_train_bf16, csrc/conv_stack_train_bf16.hip) and
ConvRefiner's `train_conv_impl = "hip_bf16"` stack.

Oracle: float64 on the CPU on the rounded operands (x, dw_w, pw_w, gy rounded to bf16) with no rounding inside --
reference_bf16_block(mode="exact") of test_conv_train_bf16_cpu.py, whose docstring states the bound; the calibration is the same
restatement in the modules' own class (mode="autocast"), never the code under test.

ReLU mask: a pre-ReLU value within a bf16 ulp of zero flips a mask bit and moves whole reductions, so in this class no seed keeps
every cell away from zero.  Oracle and calibration therefore take the device's mask, which the host recomputes from the returned u,
mean and invstd with the kernels' own fp32 expressions (numpy, one rounding per operation); separately the device mask may differ
from the true float64 mask only at cells with |pre64| <= 2^-7 (1 + |u64|) |alpha64|, and such cells are at most 1.5 % of a case.

Measured on an MI355X (worst ratio to the bound over the eight cases, per tensor kind): see DESIGN.md section 4.2."""
import copy
import functools

import numpy as np
import pytest
import torch

from conftest import load_golden
from test_conv_train_bf16_cpu import (MASK_BAND_SHARE, PARAMS, block_ratios, bound_ratio, mask_band, reference_bf16_block,
                                      reference_bf16_chain)
from test_conv_train_gpu import CASES, EPS, LEAVES, MOMENTUM, float64_stack, make_inputs, make_refiner

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


def on_gpu(inp):
    return {k: (v.cuda() if v is not None else None) for k, v in inp.items()}


def device_mask(u, mean, invstd, gamma, beta):
    """relu's mask as both kernels form it: alpha = gamma * invstd, beta' = beta - mean * alpha, u * alpha + beta' > 0, in fp32"""
    assert u.dtype == BF16
    u = u.detach().float().cpu().numpy()                 # numpy has no bf16; widening is exact
    mean, invstd, gamma, beta = (v.detach().cpu().numpy() for v in (mean, invstd, gamma, beta))
    assert all(v.dtype == np.float32 for v in (u, mean, invstd, gamma, beta))
    alpha = gamma * invstd
    betap = beta - mean * alpha
    pre = u * alpha[None, :, None, None] + betap[None, :, None, None]
    return torch.from_numpy(pre > 0)


def run_hip(inp, need=LEAVES, momentum=MOMENTUM, gy_scale=1.0):
    """ops.conv_block_train_bf16 forward + backward on the GPU; `need`: the leaves that require grad"""
    from gfnet_amd import ops

    t = on_gpu(inp)
    for k in need:
        if t[k] is not None:
            t[k].requires_grad_()
    nbt = torch.tensor(3, device="cuda")
    versions = (t["rm"]._version, t["rv"]._version)
    y = ops.conv_block_train_bf16(t["x"], t["dw_w"], t["dw_b"], t["bn_w"], t["bn_b"], t["rm"], t["rv"], nbt, momentum, EPS, t["pw_w"], t["pw_b"])
    saved = [s.dtype for s in y.grad_fn.saved_tensors[:4]] if y.grad_fn is not None else None
    if y.requires_grad:
        (y.float() * (t["gy"] * gy_scale)).sum().backward()
    torch.cuda.synchronize()
    return {"y": y.detach().cpu(), "rm": t["rm"].cpu(), "rv": t["rv"].cpu(), "nbt": int(nbt), "saved": saved,
            "bumped": t["rm"]._version > versions[0] and t["rv"]._version > versions[1],
            "grads": {k: (t[k].grad.cpu() if t[k] is not None and t[k].grad is not None else None) for k in LEAVES}}


def forward_mask(inp, x=None):
    """the forward op alone on fresh copies of the buffers: (y, mask of the device)"""
    from gfnet_amd import ops

    t = on_gpu(inp)
    y, u, mean, invstd = ops.conv_block_train_bf16_fwd(t["x"] if x is None else x, t["dw_w"].reshape(-1, 25), t["dw_b"], t["bn_w"], t["bn_b"],
                                                       t["rm"], t["rv"], MOMENTUM, EPS, t["pw_w"].flatten(1), t["pw_b"])
    assert y.dtype == u.dtype == BF16 and mean.dtype == invstd.dtype == torch.float32
    return y, device_mask(u, mean, invstd, t["bn_w"], t["bn_b"])


@functools.lru_cache(maxsize=None)
def case(name):
    inp = make_inputs(*CASES[name])
    got = run_hip(inp)
    y, mask = forward_mask(inp)
    assert torch.equal(y.cpu(), got["y"])
    true64 = reference_bf16_block(inp, mode="exact")
    exact, ref = (reference_bf16_block(inp, mask=mask, mode=m) for m in ("exact", "autocast"))
    return inp, got, mask, true64, exact, ref


@pytest.mark.parametrize("name", list(CASES))
def test_block_stays_inside_the_bound_of_the_bf16_class(name):
    inp, got, _, _, exact, ref = case(name)
    assert got["y"].dtype == BF16 and got["nbt"] == 4 and got["bumped"]
    for k in LEAVES:
        if inp[k] is None:
            assert got["grads"][k] is None
        else:
            assert got["grads"][k] is not None and got["grads"][k].dtype == torch.float32 and torch.isfinite(got["grads"][k]).all(), k
    ratios = block_ratios(got, ref, exact)
    print(f"BF16_RATIO {name}: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert torch.isfinite(got["y"]).all() and max(ratios.values()) <= 1.0, ratios


@pytest.mark.parametrize("name", list(CASES))
def test_device_mask_differs_from_float64_only_next_to_zero(name):
    _, _, mask, true64, _, _ = case(name)
    near = mask_band(true64)
    flipped = mask != (true64["pre"] > 0)
    share = float(near.double().mean())
    print(f"BF16_MASK {name}: {int(flipped.sum())} of {mask.numel()} cells flipped, {int((flipped & ~near).sum())} outside the band, band share {share:.5f}")
    assert not (flipped & ~near).any()
    assert share <= MASK_BAND_SHARE


def test_two_block_chain_reads_fp32_then_bf16():
    """block 1 reads the fp32 map, block 2 block 1's bf16 y; each block's device mask; the bound on y, d.grad and the fourteen
    parameter gradients"""
    from gfnet_amd import ops

    blocks = [make_inputs(*CASES["g_not_4k_batch3"]), make_inputs(3, 37, 10, True, 5)]
    x, gy = blocks[0]["x"], blocks[1]["gy"]
    y1, m1 = forward_mask(blocks[0])
    _, m2 = forward_mask(blocks[1], x=y1)
    t = [on_gpu(b) for b in blocks]
    for b in t:
        for k in PARAMS:
            b[k].requires_grad_()
    d = x.cuda().requires_grad_()
    h = d
    for b in t:
        h = ops.conv_block_train_bf16(h, b["dw_w"], b["dw_b"], b["bn_w"], b["bn_b"], b["rm"], b["rv"], None, MOMENTUM, EPS, b["pw_w"], b["pw_b"])
    assert h.dtype == BF16 and torch.equal(h.grad_fn.saved_tensors[0], y1)       # block 2 saved its bf16 input
    (h.float() * gy.cuda()).sum().backward()
    exact, ref = (reference_bf16_chain(blocks, x, gy, masks=[m1, m2], mode=m) for m in ("exact", "autocast"))
    ratios = {"y": bound_ratio(h.detach().cpu(), ref["y"], exact["y"]), "dx": bound_ratio(d.grad.cpu(), ref["grads"]["x"], exact["grads"]["x"])}
    assert d.grad.dtype == torch.float32
    for i, b in enumerate(t):
        for k in PARAMS:
            assert b[k].grad.dtype == torch.float32
            ratios[f"d{k}.{i}"] = bound_ratio(b[k].grad.cpu(), ref["grads"][(i, k)], exact["grads"][(i, k)])
    print("BF16_RATIO chain: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert max(ratios.values()) <= 1.0, ratios


def test_saved_maps_are_bf16_and_a_first_blocks_gx_is_fp32():
    from gfnet_amd import ops

    inp, got, _, _, _, _ = case("odd_c")
    assert got["saved"] == [torch.float32, BF16, torch.float32, torch.float32]           # x as it came, u, mean, invstd
    t = on_gpu(inp)
    args = (t["dw_w"].reshape(-1, 25), t["dw_b"], t["bn_w"], t["bn_b"], t["rm"], t["rv"], MOMENTUM, EPS, t["pw_w"].flatten(1), t["pw_b"])
    for x in (t["x"], t["x"].bfloat16()):
        y, u, mean, invstd = ops.conv_block_train_bf16_fwd(x, *args)
        gx = ops.conv_block_train_bf16_bwd(t["gy"].bfloat16(), x, u, mean, invstd, args[0], t["bn_w"], t["bn_b"], args[8])[0]
        assert y.dtype == u.dtype == BF16 and gx.dtype == x.dtype
    hidden = run_hip({**inp, "x": inp["x"].bfloat16()})
    assert hidden["saved"][0] == BF16 and hidden["grads"]["x"].dtype == BF16
    # the fp32 map is rounded on load: the same block on x.bfloat16() gives the same bits, and its gx is the fp32 one rounded once
    assert torch.equal(hidden["y"], got["y"]) and torch.equal(hidden["grads"]["x"], got["grads"]["x"].bfloat16())
    for k in PARAMS:
        assert torch.equal(hidden["grads"][k], got["grads"][k]), k


def test_need_mask_each_gradient_alone_equals_the_joint_run():
    inp, joint = case("g_not_4k_batch3")[:2]
    for k in LEAVES:
        alone = run_hip(inp, need=(k,))
        assert torch.equal(alone["y"], joint["y"])
        for j in LEAVES:
            if j == k:
                assert torch.equal(alone["grads"][j], joint["grads"][j]), f"d{j} alone differs from the joint run"
            else:
                assert alone["grads"][j] is None
    frozen_x = run_hip(inp, need=LEAVES[1:])
    assert frozen_x["grads"]["x"] is None
    for j in LEAVES[1:]:
        assert torch.equal(frozen_x["grads"][j], joint["grads"][j]), f"d{j} changes when x needs no gradient"


def test_two_runs_are_bit_identical():
    inp, first = case("edge_tiles")[:2]
    second = run_hip(inp)
    for k in ("y", "rm", "rv"):
        assert torch.equal(first[k], second[k]), k
    for k in LEAVES:
        assert torch.equal(first["grads"][k], second["grads"][k]), f"d{k}"


def test_no_grad_still_uses_batch_statistics_and_updates_the_buffers():
    inp, got = case("below_a_tile")[:2]
    with torch.no_grad():
        quiet = run_hip(inp)
    for k in ("y", "rm", "rv"):
        assert torch.equal(quiet[k], got[k])
    assert quiet["nbt"] == 4 and quiet["bumped"] and all(g is None for g in quiet["grads"].values())


def test_a_gradient_scaled_by_2_to_the_20_is_the_unscaled_one_times_2_to_the_20():
    """The backward is linear in gy, and a power of two commutes with every rounding while nothing under- or overflows: bf16 has
    fp32's exponent range, so gy * 2^20 gives every gradient times 2^20 bit for bit and y unchanged.  (The fp16 class cannot pass
    this: its own test asserts the overflow.)"""
    inp, got = case("narrow")[:2]
    big = run_hip(inp, gy_scale=2.0 ** 20)
    assert torch.equal(big["y"], got["y"])
    for k in LEAVES:
        g, want = big["grads"][k], got["grads"][k] * 2.0 ** 20
        assert torch.isfinite(g).all() and (k == "dw_b" or g.abs().max() > 0), f"d{k}"     # d dw_b: analytically zero
        assert torch.equal(g, want), f"d{k}: {int((g != want).sum())} of {g.numel()} values differ from 2^20 x the unscaled run"


def test_bad_arguments_raise_value_errors():
    from gfnet_amd import ops

    inp = on_gpu(make_inputs(1, 7, 5, True, 0))
    nbt = torch.tensor(0, device="cuda")

    def call(**kw):
        t = {**inp, **kw}
        return ops.conv_block_train_bf16(t["x"], t["dw_w"], t["dw_b"], t["bn_w"], t["bn_b"], t["rm"], t["rv"], nbt, t.get("momentum", 0.1), EPS,
                                         t["pw_w"], t["pw_b"])

    for kw in {"fp16 map": dict(x=inp["x"].half()), "fp64 map": dict(x=inp["x"].double()), "bf16 taps": dict(dw_w=inp["dw_w"].bfloat16()),
               "fp16 1x1 weights": dict(pw_w=inp["pw_w"].half()), "bf16 bn_weight": dict(bn_w=inp["bn_w"].bfloat16()),
               "non-square grid": dict(x=inp["x"][..., :4]), "one value per channel": dict(x=inp["x"][:, :, :1, :1]),
               "bn_weight of another width": dict(bn_w=inp["bn_w"][:5]), "no momentum": dict(momentum=None)}.values():
        with pytest.raises(ValueError):
            call(**kw)
    assert int(nbt) == 0
    assert call().dtype == BF16 and int(nbt) == 1                      # the same call without a bad argument runs


# ---- the stack in ConvRefiner ------------------------------------------------------------------------------------------------------
def bf16_refiner(feat, disp, r):
    ref, dim = make_refiner(feat, disp, r)
    ref.amp, ref.amp_dtype = True, BF16
    return ref.train(), dim


def hand_chain(ref, d):
    from gfnet_amd import ops

    h = d
    for conv, norm, _, pw in [ref.block1] + list(ref.hidden_blocks):
        h = ops.conv_block_train_bf16(h, conv.weight, conv.bias, norm.weight, norm.bias, norm.running_mean, norm.running_var,
                                      norm.num_batches_tracked, norm.momentum, norm.eps, pw.weight, pw.bias)
    assert h.dtype == BF16
    return ref.out_conv(h.float())


def stack_step(ref, d, w, stack=None):
    d = d.clone().requires_grad_()
    out = ref.apply_stack(d) if stack is None else stack(ref, d)
    (out * w).sum().backward()
    return out.detach(), d.grad


@pytest.mark.parametrize("feat,disp,r,G,B", [(8, 8, 0, 24, 2), (16, 16, 2, 12, 1)])
def test_refiner_stack_runs_nine_bf16_blocks_and_equals_the_hand_written_chain(feat, disp, r, G, B, monkeypatch):
    from gfnet_amd import ops

    # out_conv stays an nn.Conv2d on both sides: ask torch for its deterministic weight-gradient kernels, or two runs of the same
    # module differ in the last bits and torch.equal on out_conv.weight.grad would compare the library with itself
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    ref, dim = bf16_refiner(feat, disp, r)
    g = torch.Generator().manual_seed(7)
    d, w = torch.randn(B, dim, G, G, generator=g).cuda(), torch.randn(B, 3, G, G, generator=g).cuda()
    gold = copy.deepcopy(ref).cpu().double()
    by_torch, by_hand = copy.deepcopy(ref), copy.deepcopy(ref)
    ref.train_conv_impl = "hip_bf16"
    ref.conv_precision = "amp"                       # an eval-mode setting: not consulted
    assert ref._hip_bf16_train_stack_supported(d) and not ref._hip_amp_train_stack_supported(d)
    assert not ref._hip_train_stack_supported(d) and not ref._hip_stack_supported() and not by_torch._hip_bf16_train_stack_supported(d)
    calls, orig = [], ops.conv_block_train_bf16
    monkeypatch.setattr(ops, "conv_block_train_bf16", lambda *a, **k: (calls.append(a[0].dtype), orig(*a, **k))[1])
    monkeypatch.setattr(ops, "conv_block_train", lambda *a, **k: pytest.fail("the bf16 stack must not reach ops.conv_block_train"))
    monkeypatch.setattr(ops, "conv_block_train_amp", lambda *a, **k: pytest.fail("the bf16 stack must not reach ops.conv_block_train_amp"))
    out, dgrad = stack_step(ref, d, w)
    assert calls == [torch.float32] + [BF16] * 8, "all nine blocks on ops.conv_block_train_bf16, bf16 maps between them"
    monkeypatch.setattr(ops, "conv_block_train_bf16", orig)
    hand_out, hand_dgrad = stack_step(by_hand, d, w, stack=hand_chain)
    assert out.dtype == torch.float32 and torch.equal(out, hand_out) and torch.equal(dgrad, hand_dgrad)
    for (k, p), (_, q) in zip(ref.named_parameters(), by_hand.named_parameters()):
        if not k.startswith("disp_emb"):
            assert p.grad is not None and p.grad.dtype == torch.float32 and torch.equal(p.grad, q.grad), k
    for (k, a), (_, b) in zip(ref.named_buffers(), by_hand.named_buffers()):
        assert torch.equal(a, b), k
    # accuracy of the output against the float64 modules, calibrated by the modules under bf16 autocast on this device
    want = stack_step(gold, d.cpu().double(), w.cpu().double(), stack=float64_stack)[0]
    torch_out = stack_step(by_torch, d, w)[0]
    l2 = lambda a: float((a.cpu().double() - want).norm() / want.norm())
    print(f"BF16_STACK C={dim} G={G}: rel L2 error hip_bf16 {l2(out):.3e}, modules under bf16 autocast {l2(torch_out):.3e}")
    assert torch.isfinite(out).all() and l2(out) <= 2.0 * l2(torch_out)


@pytest.mark.parametrize("what", ["amp_off", "fp16", "eval", "groupnorm"])
def test_refiners_outside_the_class_keep_the_modules(what, monkeypatch):
    import torch.nn as nn
    from gfnet_amd import ops

    kw = {"groupnorm": dict(norm_type=functools.partial(nn.GroupNorm, 4))}.get(what, {})
    ref, dim = make_refiner(8, 8, 0, **kw)
    ref.train()
    ref.amp = what != "amp_off"
    ref.amp_dtype = torch.float16 if what == "fp16" else BF16
    if what == "eval":
        ref.eval()
    plain = copy.deepcopy(ref)
    ref.train_conv_impl = "hip_bf16"
    d = torch.randn(2, dim, 12, 12, generator=torch.Generator().manual_seed(3)).cuda()
    assert not ref._hip_bf16_train_stack_supported(d) and not ref._hip_amp_train_stack_supported(d)
    for op in ("conv_block_train_bf16", "conv_block_train_amp"):
        monkeypatch.setattr(ops, op, lambda *a, **k: pytest.fail("the fallback must not reach ops.conv_block_train_bf16 / _amp"))
    with torch.no_grad():
        got, want = ref.apply_stack(d), plain.apply_stack(d)
    assert torch.equal(got, want)


# ---- a training step -----------------------------------------------------------------------------------------------------------------
def test_training_steps_without_a_loss_scale_on_hip_bf16_refiners():
    """trainer.train_step with FusedAdamWStep on the G12 model, every refiner amp=True, amp_dtype=bfloat16 on "hip_bf16", the scale
    fixed at 1: two steps find no overflow and move the parameters; a stepper whose scale is 2^20 -- far past what fp16 maps hold --
    finds none either and moves them too"""
    import torch.nn as nn
    from gfnet_amd import ops
    from gfnet_amd.trainer import FusedAdamWStep, train_step
    from test_train_cpu import SCALES, g12_pyramids
    from test_train_gpu import g12_model

    g = load_golden("g12_train_grads")
    torch.manual_seed(0)
    model = g12_model(g)
    for ref in model.conv_refiner.values():
        ref.amp, ref.amp_dtype, ref.train_conv_impl = True, BF16, "hip_bf16"
    pyr0, pyr1 = g12_pyramids(g, "cuda")
    hw = tuple(int(v) for v in g["image_hw"])
    weights = {(s, itr, kind): torch.from_numpy(g[f"w{kind}.{s}.{itr}"]).cuda() for s in SCALES for itr in range(1, int(g["num_itr"][SCALES.index(s)]) + 1)
               for kind in ("flow", "cert")}

    class Wrapped(nn.Module):
        def __init__(self, net):
            super().__init__()
            self.net = net

        def forward(self, batch):
            return self.net.forward_pyramids(batch["pyr0"], batch["pyr1"], hw)

    def objective(out, batch):
        loss = torch.zeros((), device="cuda")
        for s in SCALES:
            for itr, d in out[s].items():
                loss = loss + (weights[(s, itr, "flow")] * d["flow"]).sum() + (weights[(s, itr, "cert")] * d["certainty"]).sum()
        return loss

    batch = {"pyr0": {s: t.detach() for s, t in pyr0.items()}, "pyr1": {s: t.detach() for s, t in pyr1.items()}}
    calls, orig = [], ops.conv_block_train_bf16
    ops.conv_block_train_bf16 = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
    try:
        stepper = FusedAdamWStep(model.named_parameters(), lr=1e-3, max_norm=0.01, init_scale=1., growth_factor=1., backoff_factor=1.)
        stack = [p for n, p in model.named_parameters() if "disp_emb" not in n]
        for step in range(2):
            before = [p.detach().clone() for p in stack]
            res = train_step(batch, Wrapped(model), objective, stepper)
            assert float(stepper.last_stats["found_inf"]) == 0.0 and stepper.nonfinite_names() == [], f"step {step}"
            assert float(stepper.last_stats["grad_scale"]) == 1.0 and torch.isfinite(res["train_loss"]).item()
            assert all(not torch.equal(a, p.detach()) for a, p in zip(before, stack)), f"step {step}: a parameter did not move"
        blocks = 1 + int(g["hidden_blocks"])
        assert len(calls) == 2 * blocks * sum(int(v) for v in g["num_itr"]), "a refiner call did not take the bf16 stack"
        hot = FusedAdamWStep(model.named_parameters(), lr=1e-3, max_norm=0.01, init_scale=2. ** 20, growth_factor=1., backoff_factor=1.)
        before = [p.detach().clone() for p in stack]
        train_step(batch, Wrapped(model), objective, hot)
        assert float(hot.last_stats["found_inf"]) == 0.0 and float(hot.last_stats["grad_scale"]) == 2. ** 20 and hot.nonfinite_names() == []
        assert all(not torch.equal(a, p.detach()) for a, p in zip(before, stack)), "a parameter did not move under the 2^20 scale"
        assert len(calls) == 3 * blocks * sum(int(v) for v in g["num_itr"])
    finally:
        ops.conv_block_train_bf16 = orig
