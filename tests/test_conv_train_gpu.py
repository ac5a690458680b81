"""GPU: one refiner conv block in training mode (ops.conv_block_train, csrc/conv_stack_train.hip) and ConvRefiner's
`train_conv_impl = "hip"` stack.  The reference is the block written with F.conv2d / F.batch_norm(training=True) / F.relu / F.conv2d
in float64 on the same fp32 inputs (model/network.py:471-487, 560-563), torch autograd for the gradients.

A pre-ReLU value that rounds across zero flips a mask bit and moves whole reductions, so every block case asserts -- on the float64
reference -- that no pre-ReLU value lies within RELU_MARGIN of zero; the seeds below were searched on the CPU for that, and no cell
is left out of any comparison."""
import copy
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import load_golden
from test_train_cpu import SCALES, compare_to_g12, g12_pyramids, g12_refiners, weighted_loss

pytestmark = pytest.mark.gpu

RELU_MARGIN = 1e-5
MOMENTUM, EPS = 0.1, 1e-5
# name: (B, C, G, depthwise bias, seed)
CASES = {
    "narrow": (2, 24, 16, True, 1),
    "odd_c": (1, 73, 12, True, 1),
    "g_not_4k_batch3": (3, 37, 10, True, 2),
    "below_a_tile": (1, 7, 5, True, 1),
    "five_row_tiles": (1, 150, 8, True, 1),
    "widest_k": (1, 417, 8, True, 1),
    "edge_tiles": (2, 16, 36, True, 3),
    "no_dw_bias": (2, 24, 16, False, 2),
}
LEAVES = ("x", "dw_w", "dw_b", "bn_w", "bn_b", "pw_w", "pw_b")


def make_inputs(B, C, G, bias, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    return {"x": r(B, C, G, G), "dw_w": 0.2 * r(C, 1, 5, 5), "dw_b": 0.1 * r(C) if bias else None, "bn_w": 1 + 0.1 * r(C),
            "bn_b": 0.1 * r(C), "rm": 0.1 * r(C), "rv": 0.5 + torch.rand(C, generator=g), "pw_w": r(C, C, 1, 1) / C ** 0.5,
            "pw_b": 0.1 * r(C), "gy": r(B, C, G, G)}


def reference(inp, momentum=MOMENTUM):
    """float64 on the CPU: y, the updated buffers, the pre-ReLU map, the batch variance and the gradients of sum(y * gy)"""
    t = {k: v.double().requires_grad_() for k, v in inp.items() if k in LEAVES and v is not None}
    C = inp["x"].shape[1]
    rm, rv = inp["rm"].double().clone(), inp["rv"].double().clone()
    u = F.conv2d(t["x"], t["dw_w"], t.get("dw_b"), padding=2, groups=C)
    pre = F.batch_norm(u, rm, rv, t["bn_w"], t["bn_b"], training=True, momentum=momentum, eps=EPS)
    y = F.conv2d(F.relu(pre), t["pw_w"], t["pw_b"])
    names = [k for k in LEAVES if k in t]
    grads = dict(zip(names, torch.autograd.grad(y, [t[k] for k in names], inp["gy"].double())))
    return {"y": y.detach(), "rm": rm, "rv": rv, "pre": pre.detach(), "var": u.detach().var(dim=(0, 2, 3), unbiased=False), "grads": grads}


def run_hip(inp, need=LEAVES, momentum=MOMENTUM):
    """ops.conv_block_train forward + backward on the GPU; `need`: the leaves that require grad"""
    from gfnet_amd import ops

    t = {k: (v.cuda() if v is not None else None) for k, v in inp.items()}
    for k in need:
        if t[k] is not None:
            t[k].requires_grad_()
    nbt = torch.tensor(3, device="cuda")
    versions = (t["rm"]._version, t["rv"]._version)
    y = ops.conv_block_train(t["x"], t["dw_w"], t["dw_b"], t["bn_w"], t["bn_b"], t["rm"], t["rv"], nbt, momentum, EPS, t["pw_w"], t["pw_b"])
    if y.requires_grad:
        y.backward(t["gy"])
    torch.cuda.synchronize()
    return {"y": y.detach().cpu(), "rm": t["rm"].cpu(), "rv": t["rv"].cpu(), "nbt": int(nbt),
            "bumped": t["rm"]._version > versions[0] and t["rv"]._version > versions[1],
            "grads": {k: (t[k].grad.cpu() if t[k] is not None and t[k].grad is not None else None) for k in LEAVES}}


@functools.lru_cache(maxsize=None)
def case(name):
    inp = make_inputs(*CASES[name])
    return inp, reference(inp), run_hip(inp)


def assert_relu_margin(ref):
    m = float(ref["pre"].abs().min())
    assert m >= RELU_MARGIN, f"a pre-ReLU value lies {m:.2e} from zero: pick another seed for this case"


def assert_outputs_close(name, got, want, tol):
    err = (got.double() - want).abs()
    ratio = float((err / (tol * want.abs().clamp(min=1.0))).max())
    print(f"{name}: max err {float(err.max()):.3e}, {ratio:.3f} x the tolerance")
    assert torch.isfinite(got).all() and ratio <= 1.0, f"{name}: err {float(err.max()):.3e}, {ratio:.2f} x the tolerance"


def assert_grad_close(name, got, want, tol):
    err = float((got.double() - want).abs().max())
    bound = tol * max(1.0, float(want.abs().max()))
    print(f"{name}: max err {err:.3e}, bound {bound:.3e}")
    assert got.shape == want.shape and torch.isfinite(got).all() and err <= bound, f"{name}: err {err:.3e} > {bound:.3e}"


@pytest.mark.parametrize("name", list(CASES))
def test_forward_matches_float64_and_updates_the_buffers(name):
    """y and the new running statistics within 1e-5 * max(1, |want|) (the per-block bound of test_conv_stack_gpu.py)"""
    _, ref, got = case(name)
    assert_relu_margin(ref)
    for k in ("y", "rm", "rv"):
        assert_outputs_close(f"{name} {k}", got[k], ref[k], 1e-5)
    assert got["nbt"] == 4 and got["bumped"]


@pytest.mark.parametrize("name", list(CASES))
def test_backward_matches_float64_autograd(name):
    """every gradient within 1e-4 * max(1, max|ref|) of its tensor (the bound of test_refiner_input_bwd_gpu.py); dw_b's gradient
    is analytically zero -- BatchNorm removes the mean -- and the floor of 1 covers it"""
    inp, ref, got = case(name)
    assert_relu_margin(ref)
    for k in LEAVES:
        if inp[k] is None:
            assert got["grads"][k] is None
            continue
        assert got["grads"][k] is not None, f"{name}: no gradient for {k}"
        assert_grad_close(f"{name} d{k}", got["grads"][k], ref["grads"][k], 1e-4)


@pytest.mark.parametrize("name", ["narrow", "odd_c", "g_not_4k_batch3", "five_row_tiles", "widest_k", "edge_tiles", "no_dw_bias"])
def test_forward_is_the_eval_block_on_the_batch_statistics_bit_for_bit(name):
    """The training forward and the eval-mode block (csrc/conv_stack.hip) share their depthwise arithmetic and their 1x1 tile
    (csrc/pw_gemm_tile.h): with alpha = gamma * invstd and beta' = beta - mean * alpha formed as bn_affine forms them -- float32,
    one rounding per operation -- and packed for the eval block, the two-pass kernels and, where G % 4 == 0, the fused kernel
    give the training forward's y bit for bit."""
    from gfnet_amd import ops

    _, C, G, _, _ = CASES[name]
    t = {k: (v.cuda() if v is not None else None) for k, v in make_inputs(*CASES[name]).items()}
    y, _, mean, invstd = ops.conv_block_train_fwd(t["x"], t["dw_w"], t["dw_b"], t["bn_w"], t["bn_b"], t["rm"].clone(), t["rv"].clone(),
                                                  MOMENTUM, EPS, t["pw_w"], t["pw_b"])
    gamma, beta, mean, invstd = (v.cpu().numpy() for v in (t["bn_w"], t["bn_b"], mean, invstd))
    assert all(v.dtype == np.float32 for v in (gamma, beta, mean, invstd))
    alpha = gamma * invstd
    betap = beta - mean * alpha
    packed = ops.conv_block_pack(t["dw_w"], t["dw_b"], torch.from_numpy(alpha).cuda(), torch.from_numpy(betap).cuda(), t["pw_w"], t["pw_b"])
    assert torch.equal(y, ops.conv_block(t["x"], packed, C, variant=1)), "two-pass eval block"
    if G % 4 == 0:
        assert torch.equal(y, ops.conv_block(t["x"], packed, C, variant=0)), "fused eval block"


def cancellation_inputs():
    """channel 0 of u is 30 + 0.1 * noise: |mean| / std = 300 (its taps are the identity, no bias, so u = x there)"""
    inp = make_inputs(2, 24, 16, True, 1)
    inp["x"][:, 0] = 30 + 0.1 * inp["x"][:, 0]
    inp["dw_w"][0] = 0
    inp["dw_w"][0, 0, 2, 2] = 1
    inp["dw_b"][0] = 0
    return inp


def test_statistics_survive_cancellation():
    """|var - want| <= 1e-3 * want on the channel with |mean| / std = 300, and y within 1e-4 * max(1, |want|).  With momentum = 1 the
    new running_var is the batch's unbiased variance, which is how the variance is read back.
    Observed on the CPU for these inputs (|mean| / std = 296): torch's own fp32 F.batch_norm has a variance error of 5e-8 x want and
    a y error of 0.06 x the bound -- inside both; E[u^2] - E[u]^2 from fp32 sums has a variance error of 1.2e-2 x want with torch's
    pairwise sums and 5.9e-2 x want summed cell after cell -- outside.  The kernels' u * alpha + beta' with exact statistics has a
    y error of 0.13 x the bound.  So the bounds separate a shifted / merged reduction from the plain one."""
    inp = cancellation_inputs()
    ref, got = reference(inp, momentum=1.0), run_hip(inp, momentum=1.0)
    assert_relu_margin(ref)
    n = inp["x"].numel() // inp["x"].shape[1]
    u0 = inp["x"][:, 0].double()
    assert 250 <= float(u0.mean().abs() / u0.std()) <= 350
    want = float(ref["var"][0])
    var = float(got["rv"][0].double()) * (n - 1) / n
    print(f"cancellation: var {var:.9e}, want {want:.9e}, rel err {abs(var - want) / want:.3e}")
    assert abs(var - want) <= 1e-3 * want
    assert_outputs_close("cancellation y", got["y"], ref["y"], 1e-4)


def test_need_mask_each_gradient_alone_equals_the_joint_run():
    inp, _, joint = case("g_not_4k_batch3")
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
    inp, _, first = case("edge_tiles")
    second = run_hip(inp)
    for k in ("y", "rm", "rv"):
        assert torch.equal(first[k], second[k]), k
    for k in LEAVES:
        assert torch.equal(first["grads"][k], second["grads"][k]), f"d{k}"


def test_no_grad_still_uses_batch_statistics_and_updates_the_buffers():
    inp, ref, got = case("below_a_tile")
    with torch.no_grad():
        quiet = run_hip(inp)
    for k in ("y", "rm", "rv"):
        assert torch.equal(quiet[k], got[k])
    assert quiet["nbt"] == 4 and quiet["bumped"] and all(g is None for g in quiet["grads"].values())


def test_bad_arguments_raise_value_errors():
    from gfnet_amd import ops

    inp = {k: (v.cuda() if v is not None else None) for k, v in make_inputs(1, 7, 5, True, 0).items()}
    nbt = torch.tensor(0, device="cuda")

    def call(**kw):
        t = {**inp, **kw}
        return ops.conv_block_train(t["x"], t["dw_w"], t["dw_b"], t["bn_w"], t["bn_b"], t["rm"], t["rv"], nbt, t.get("momentum", 0.1), EPS,
                                    t["pw_w"], t["pw_b"])

    for kw in {"non-square grid": dict(x=inp["x"][..., :4]), "bn_weight of another width": dict(bn_w=inp["bn_w"][:5]),
                     "fp16 taps": dict(dw_w=inp["dw_w"].half()), "fp64 1x1 weights": dict(pw_w=inp["pw_w"].double()),
                     "running_var of another width": dict(rv=inp["rv"][:3]), "no momentum": dict(momentum=None)}.values():
        with pytest.raises(ValueError):
            call(**kw)
    assert int(nbt) == 0


# ---- the stack in ConvRefiner ------------------------------------------------------------------------------------------------------
def make_refiner(feat, disp, r, **kw):
    from gfnet_amd.model.network import ConvRefiner

    dim = 2 * feat + disp + ((2 * r + 1) ** 2 if r > 0 else 0)
    torch.manual_seed(feat + r)
    kw = {"bn_momentum": 0.1, **kw}
    ref = ConvRefiner(dim, dim, 3, kernel_size=5, dw=True, hidden_blocks=8, displacement_emb="linear", displacement_emb_dim=disp,
                      local_corr_num=r, corr_in_other=r > 0, amp=False, **kw)
    with torch.no_grad():  # statistics and affine parameters away from their initial 0 / 1
        for m in ref.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.1)
                m.running_var.uniform_(0.5, 1.5)
                m.weight.normal_(1, 0.1)
                m.bias.normal_(0, 0.1)
    return ref.cuda(), dim


def float64_stack(ref, d):
    """the modules themselves, network.py:560-563 without its `.float()`, which would round the float64 reference's map to fp32"""
    return ref.out_conv(ref.hidden_blocks(ref.block1(d)))


def train_step(ref, d, w, stack=None):
    """one forward + backward of the stack on a copy of d; returns (out, d.grad)"""
    d = d.clone().requires_grad_()
    out = ref.apply_stack(d) if stack is None else stack(ref, d)
    (out * w).sum().backward()
    return out.detach(), d.grad


@pytest.mark.parametrize("feat,disp,r,G,B", [(8, 8, 0, 24, 2), (16, 16, 2, 12, 1)])
def test_refiner_stack_in_train_mode_matches_the_float64_modules(feat, disp, r, G, B):
    """train_conv_impl "hip" and "torch" against the float64 modules: outputs and buffers within 1e-4 * max(1, |want|), every
    parameter gradient and d.grad within 1e-3 * max(1, max|want|) -- the bounds of the G12 GPU test; then eval() re-folds."""
    ref, dim = make_refiner(feat, disp, r)
    assert ref.train_conv_impl == "torch"
    g = torch.Generator().manual_seed(7)
    d, w = torch.randn(B, dim, G, G, generator=g).cuda(), torch.randn(B, 3, G, G, generator=g).cuda()
    ref.eval()
    with torch.no_grad():
        eval_before = ref.apply_stack(d).clone()   # fills folded_stack()'s cache with the old statistics
    ref.train()
    gold = copy.deepcopy(ref).cpu().double()
    by_torch = copy.deepcopy(ref)
    ref.train_conv_impl = "hip"
    assert ref._hip_train_stack_supported(d) and not ref._hip_stack_supported()
    want_out, want_dgrad = train_step(gold, d.cpu().double(), w.cpu().double(), stack=float64_stack)
    for name, model in (("hip", ref), ("torch", by_torch)):
        out, dgrad = train_step(model, d, w)
        assert_outputs_close(f"{name} out", out.cpu(), want_out, 1e-4)
        for (k, buf), (_, wb) in zip(model.named_buffers(), gold.named_buffers()):
            assert_outputs_close(f"{name} {k}", buf.detach().cpu(), wb.double(), 1e-4)
        assert_grad_close(f"{name} d.grad", dgrad.cpu(), want_dgrad, 1e-3)
        for (k, p), (_, wp) in zip(model.named_parameters(), gold.named_parameters()):
            if k.startswith("disp_emb"):
                continue   # not part of the stack
            assert p.grad is not None, f"{name}: no gradient for {k}"
            assert_grad_close(f"{name} d{k}", p.grad.cpu(), wp.grad, 1e-3)
    ref.eval()
    gold.eval()
    with torch.no_grad():
        eval_after = ref.apply_stack(d)
        want_eval = float64_stack(gold, d.cpu().double())
    assert_outputs_close("eval after the step", eval_after.cpu(), want_eval, 1e-4)
    assert float((eval_after - eval_before).abs().max()) > 1e-3, "eval() still runs on the statistics from before the step"


def test_g12_training_step_with_every_refiner_on_the_hip_stack():
    """test_train_gpu.py's G12 case with train_conv_impl = "hip" everywhere: same tolerances, same check on the loss"""
    from gfnet_amd import ops
    from gfnet_amd.model.network import GFNet

    g = load_golden("g12_train_grads")
    torch.manual_seed(0)
    refiners = g12_refiners(g, "cuda")
    for ref in refiners.values():
        ref.train_conv_impl = "hip"
    conf = {"matcher": {"num_grid": [int(v) for v in g["num_grid"]], "radius": [int(v) for v in g["radius"]],
                        "num_itr": [int(v) for v in g["num_itr"]]}}
    model = GFNet(conf, conv_refiner=nn.ModuleDict(refiners)).cuda().train()
    calls, orig = [], ops.conv_block_train
    ops.conv_block_train = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
    try:
        pyr0, pyr1 = g12_pyramids(g, "cuda")
        corresps = model.forward_pyramids(pyr0, pyr1, tuple(int(v) for v in g["image_hw"]))
    finally:
        ops.conv_block_train = orig
    blocks = 1 + int(g["hidden_blocks"])
    assert len(calls) == blocks * sum(int(v) for v in g["num_itr"]), "a refiner call did not take the HIP stack"
    loss = weighted_loss(g, corresps)
    loss.backward()
    torch.cuda.synchronize()
    assert abs(loss.item() - float(g["loss"])) <= 1e-4 * max(1.0, abs(float(g["loss"])))
    worst = compare_to_g12(g, corresps, pyr0, pyr1, {s: model.conv_refiner[s] for s in SCALES}, 1e-4, 1e-3)
    print(f"G12 on the HIP training stack: worst err / tol {worst}")


@pytest.mark.parametrize("what", ["amp", "groupnorm", "momentum_none"])
def test_unsupported_refiners_fall_back_to_the_modules(what, monkeypatch):
    from gfnet_amd import ops

    kw = {"groupnorm": dict(norm_type=functools.partial(nn.GroupNorm, 4)), "momentum_none": dict(bn_momentum=None)}.get(what, {})
    ref, dim = make_refiner(8, 8, 0, **kw)
    ref.train()
    if what == "amp":
        ref.conv_precision = "amp"
    plain = copy.deepcopy(ref)
    ref.train_conv_impl = "hip"
    d = torch.randn(2, dim, 12, 12, generator=torch.Generator().manual_seed(3)).cuda()
    assert not ref._hip_train_stack_supported(d)

    def refuse(*a, **k):
        raise AssertionError("the fallback must not reach ops.conv_block_train")

    monkeypatch.setattr(ops, "conv_block_train", refuse)
    with torch.no_grad():
        got, want = ref.apply_stack(d), plain.apply_stack(d)
    assert torch.equal(got, want)
    for (k, a), (_, b) in zip(ref.named_buffers(), plain.named_buffers()):
        assert torch.equal(a, b), k
