"""The FPN decoder's 2x upsample inside the training op on the GPU (ops.conv2d_bn_act_train(..., up0=True), csrc/fpn_conv_train.hip;
train_conv_impl = "hip_fused"): x0 is the coarse map, the doubled map is never written, and gx0 comes back at the coarse shape.

The definition is tests/test_fpn_train_gpu.py's with x0 replaced by F.interpolate(x0, scale_factor=2, mode="bilinear",
align_corners=False) inside the differentiated expression, in float64; the unit of every bound is that file's e32 (the same
definition in fp32 by torch on the CPU against float64), the bound 4 x e32, with that file's floor (one fp32 rounding of the tensor's
largest magnitude) for the per-channel vectors and on the tiny maps.  The conv-bias gradient is asserted to be exact zeros.

Shapes: inner1..3 on a coarse 7 x 11 map (odd sizes: both clamps; the 64-, 32- and 16-channel x0); inner3 and inner1 on 36 x 68 ->
72 x 136 (three chunks per reduction, 45 weight-gradient tiles, and for inner1 five groups of staged input channels); coarse 1 x 1
and 1 x 3 (every tap clamped); the general convolution kernel (Cout = 5, K = 5) and a layer without x1.

Largest ratios measured (MI355X; also in DESIGN 4.8): as ops 2.51 (inner3; inner1 1.76, inner2 1.13), across a tile boundary 1.83
(inner3) and 1.58 (inner1), tiny maps 2.61 (1 x 1) and 2.04 (1 x 3), general_up 1.73, up_alone 1.90; the three modules against
float64 1.85 (shape a) and 2.60 (b), against their torch path 2.44 and 2.75, against g17_fpn_train.npz 3.30; the one-step loss
0.67592597 (hip_fused) against 0.67588842 (torch), 3.8e-5 apart."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fpn_fixture
import synth
from conftest import load_golden
from gfnet_amd import ops
from make_golden_fpn_train import SHAPE
from test_fpn_cpu import run_modules
from test_fpn_gpu import GENERAL, LAYERS
from test_fpn_train_gpu import (E2E_CONF, EPS, MOMENTUM, NAMES, VECTORS, act_fn, build, compare_modules, compare_to_golden, module_on_gpu,
                                module_reference, one_training_step)

pytestmark = pytest.mark.gpu

# the layers that upsample x0, and one without x1 (K, stride, C0, C1, Cout, up0, residual, act)
CONFIGS = {**{k: v for k, v in {**LAYERS, **GENERAL}.items() if v[5]}, "up_alone": (3, 1, 5, 0, 8, True, None, "leaky_relu")}
assert sorted(CONFIGS) == ["general_up", "inner1", "inner2", "inner3", "up_alone"]


def up2(x):
    return F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)


def definition(t, act):
    """test_fpn_train_gpu.definition at stride 1 with x0 -> up2(x0) inside the differentiated expression: everything the op returns and
    every gradient of sum(out * lw), gx0 at the coarse shape, in the dtype of the tensors of `t` (fresh leaves)."""
    leaf = {k: (None if v is None else v.clone().requires_grad_(k in ("x0", "x1", "w", "cb", "g", "b", "res"))) for k, v in t.items()}
    x = up2(leaf["x0"]) if leaf["x1"] is None else torch.cat((up2(leaf["x0"]), leaf["x1"]), dim=1)
    u = F.conv2d(x, leaf["w"], padding=leaf["w"].shape[-1] // 2)
    rm, rv = leaf["rm"], leaf["rv"]
    y = F.batch_norm(u if leaf["cb"] is None else u + leaf["cb"].view(1, -1, 1, 1), rm, rv, leaf["g"], leaf["b"], True, MOMENTUM, EPS)
    out = act_fn(y, act)
    if leaf["res"] is not None:
        out = out + leaf["res"]
    wanted = [k for k in ("x0", "x1", "res", "w", "g", "b", "cb") if leaf[k] is not None]
    grads = dict(zip(wanted, torch.autograd.grad((out * leaf["lw"]).sum(), [leaf[k] for k in wanted])))
    ud = u.detach()
    return {"out": out.detach(), "u": ud, "mean": ud.mean((0, 2, 3)), "invstd": (ud.var((0, 2, 3), unbiased=False) + EPS).rsqrt(),
            "running_mean": rm, "running_var": rv, "gx0": grads["x0"], "gx1": grads.get("x1"), "g_residual": grads.get("res"),
            "d_weight": grads["w"], "d_bn_w": grads["g"], "d_bn_b": grads["b"]}


@functools.lru_cache(maxsize=None)
def case(name, B, h, w):
    """Inputs of layer `name` with a coarse x0 of (B, C0, h, w) and everything else at (2h, 2w), the float64 results and every
    tensor's e32.  Computed once, never modified.  The residual is a tensor of its own (a copy of x1), so that its gradient is told
    apart; the swish layers have a conv bias."""
    K, stride, C0, C1, Cout, up0, res, act = CONFIGS[name]
    assert up0 and stride == 1 and res in ("x1", None)
    seed = 5300 + 17 * sorted(CONFIGS).index(name)

    def lat(shape, s, uniform=False):
        return torch.from_numpy((synth.lattice_uniform if uniform else synth.lattice_normalish)(shape, seed + s))

    t = {"x0": lat((B, C0, h, w), 0), "x1": lat((B, C1, 2 * h, 2 * w), 1) if C1 else None,
         "w": lat((Cout, C0 + C1, K, K), 2) * np.float32(0.87 / np.sqrt((C0 + C1) * K * K)),
         "cb": np.float32(0.3) * lat((Cout,), 3, True) if act == "swish" else None,
         "g": np.float32(0.9) + np.float32(0.5) * lat((Cout,), 4, True), "b": np.float32(0.4) * lat((Cout,), 5, True),
         "rm": np.float32(0.5) * lat((Cout,), 6, True), "rv": np.float32(1.0) + np.float32(0.75) * lat((Cout,), 7, True),
         "lw": lat((B, Cout, 2 * h, 2 * w), 8)}
    t["res"] = None if res is None else t["x1"].clone()
    ref = definition({k: (None if v is None else v.double()) for k, v in t.items()}, act)
    r32 = definition(t, act)
    e32 = {k: (None if ref[k] is None else float((r32[k].double() - ref[k]).abs().max())) for k in NAMES}
    assert tuple(ref["out"].shape) == (B, Cout, 2 * h, 2 * w) and tuple(ref["gx0"].shape) == (B, C0, h, w)
    return t, ref, e32


def run_op(name, t, residual="own", requires=("x0", "x1", "w", "g", "b", "res", "cb")):
    """The op with up0=True and its backward on the GPU: the same dict as `definition`, plus d_conv_bias.  residual: "own" (a leaf of
    its own) or "alias" (the very tensor x1)."""
    K, stride, C0, C1, Cout, _, res, act = CONFIGS[name]
    d = {k: (None if v is None else v.cuda().requires_grad_(k in requires)) for k, v in t.items()}
    if residual == "alias" and res is not None:
        d["res"] = d[res]
    nbt = torch.zeros((), dtype=torch.long, device="cuda")
    out = ops.conv2d_bn_act_train(d["x0"], d["w"], d["cb"], d["g"], d["b"], d["rm"], d["rv"], nbt, MOMENTUM, EPS, x1=d["x1"],
                                  residual=d["res"], stride=1, act=act, slope=0.1, up0=True)
    assert int(nbt) == 1
    got = {"out": out.detach(), "running_mean": d["rm"], "running_var": d["rv"]}
    if out.requires_grad:
        (out * d["lw"]).sum().backward()
        got.update(gx0=d["x0"].grad, gx1=None if d["x1"] is None else d["x1"].grad, d_weight=d["w"].grad, d_bn_w=d["g"].grad,
                   d_bn_b=d["b"].grad, g_residual=None if d["res"] is None else d["res"].grad,
                   d_conv_bias=None if d["cb"] is None else d["cb"].grad)
    return got


def saved(name, t):
    """(u, mean, invstd) of the forward, from the thin wrapper."""
    act = CONFIGS[name][7]
    d = {k: (None if v is None else v.cuda()) for k, v in t.items()}
    out, u, mean, invstd = ops.conv2d_bn_act_train_fwd(d["x0"], d["w"], d["cb"], d["g"], d["b"], d["rm"], d["rv"], MOMENTUM, EPS, x1=d["x1"],
                                                       residual=d["res"], stride=1, act=act, slope=0.1, up0=True)
    return d, out, u, mean, invstd


def check_case(name, B, h, w, floor=False):
    t, ref, e32 = case(name, B, h, w)
    got = run_op(name, t)
    _, out, u, mean, invstd = saved(name, t)
    assert torch.equal(out, got["out"])  # the wrapper and the autograd function run the same launches
    got.update(u=u, mean=mean, invstd=invstd)
    worst, failed = 0.0, []
    for k in NAMES:
        if ref[k] is None:
            assert got.get(k) is None, k
            continue
        if k == "g_residual":  # gy itself
            assert torch.equal(got[k].cpu().double(), ref[k]), k
            continue
        unit = e32[k]
        if floor or k in VECTORS:
            unit = max(unit, 2.0 ** -24 * float(ref[k].abs().max()))
        assert unit > 0.0, (name, k)
        assert got[k].shape == ref[k].shape and got[k].dtype == torch.float32, k
        err = float((got[k].detach().cpu().double() - ref[k]).abs().max())
        worst = max(worst, err / unit)
        print(f"{name} up0 {B}x{h}x{w}: {k}: max err {err:.3e}, unit {unit:.3e}, ratio {err / unit:.2f}")
        if err > 4 * unit:
            failed.append((name, k, err, unit))
    print(f"{name} up0 {B}x{h}x{w}: largest ratio {worst:.2f}")
    assert not failed, failed
    if t["cb"] is not None:
        assert got["d_conv_bias"] is not None and not bool(got["d_conv_bias"].any()), "the conv bias's gradient is exactly zero"


@pytest.mark.parametrize("name", ["inner1", "inner2", "inner3"])
def test_every_upsampling_layer_as_an_op(name):
    """B = 2, coarse 7 x 11 -> 14 x 22."""
    check_case(name, 2, 7, 11)


@pytest.mark.parametrize("name", ["inner3", "inner1"])
def test_across_a_tile_boundary(name):
    """B = 1, coarse 36 x 68 -> 72 x 136."""
    check_case(name, 1, 36, 68)


@pytest.mark.parametrize("h,w", [(1, 1), (1, 3)])
def test_tiny_maps(h, w):
    """B = 3, coarse 1 x 1 -> 2 x 2 and 1 x 3 -> 2 x 6: every tap of the upsample and of its transpose is clamped."""
    check_case("inner3", 3, h, w, floor=True)


@pytest.mark.parametrize("name", ["general_up", "up_alone"])
def test_general_kernel_and_a_layer_without_x1(name):
    """general_up: Cout = 5 and K = 5, off the 8-channel tile kernel in the forward and in the input gradient of x1 (5 channels; that
    of x0, 3 channels, too).  up_alone: x1 = None."""
    check_case(name, 2, 7, 11)


def test_op_checks_its_up0_arguments():
    x, w, s = torch.zeros(1, 3, 4, 4, device="cuda"), torch.zeros(8, 5, 3, 3, device="cuda"), torch.ones(8, device="cuda")
    x1 = torch.zeros(1, 2, 8, 8, device="cuda")
    with pytest.raises(ValueError, match=r"x1 must be \(1, C1, 8, 8\)"):
        ops.conv2d_bn_act_train(x, w, None, s, s, s.clone(), s.clone(), None, 0.1, 1e-5, x1=torch.zeros(1, 2, 4, 4, device="cuda"), up0=True)
    with pytest.raises(ValueError, match="residual must have the output's shape"):
        ops.conv2d_bn_act_train(x, w, None, s, s, s.clone(), s.clone(), None, 0.1, 1e-5, x1=x1, residual=torch.zeros(1, 8, 4, 4, device="cuda"),
                                up0=True)
    u = torch.zeros(1, 8, 4, 4, device="cuda")
    for call in (lambda: ops.conv2d_bn_act_train(x, w, None, s, s, s.clone(), s.clone(), None, 0.1, 1e-5, x1=x1, stride=2, up0=True),
                 lambda: ops.conv2d_bn_act_train_fwd(x, w, None, s, s, s.clone(), s.clone(), 0.1, 1e-5, x1=x1, stride=2, up0=True),
                 lambda: ops.conv2d_bn_act_train_bwd(u, x, w, s, s, u, s, s, x1=x1, stride=2, up0=True)):
        with pytest.raises(ValueError, match="up0 needs stride 1"):
            call()


def bwd(name, d, u, mean, invstd, need, buffers=None):
    act = CONFIGS[name][7]
    return ops.conv2d_bn_act_train_bwd(d["lw"], d["x0"], d["w"], d["g"], d["b"], u, mean, invstd, x1=d["x1"], stride=1, act=act, slope=0.1,
                                       need=need, buffers=buffers, up0=True)


@pytest.mark.parametrize("name", ["inner2", "up_alone"])
def test_need_mask(name):
    """Inputs without requires_grad: neither the gradient of the doubled map nor its transpose is launched -- a poisoned coarse gx0
    buffer handed to the backward comes back untouched -- and each single need bit gives the bits of the full call."""
    t, _, _ = case(name, 2, 7, 11)
    d, _, u, mean, invstd = saved(name, t)
    full = bwd(name, d, u, mean, invstd, (True, True, True))
    assert full[0].shape == d["x0"].shape
    poison = {"gx0": torch.full_like(d["x0"], 7.25), "gx1": None if d["x1"] is None else torch.full_like(d["x1"], 7.25)}
    partial = bwd(name, d, u, mean, invstd, (False, True, True), buffers=dict(poison))
    assert partial[0] is None and partial[1] is None
    assert bool((poison["gx0"] == 7.25).all()) and (poison["gx1"] is None or bool((poison["gx1"] == 7.25).all()))
    assert torch.equal(partial[2], full[2]) and torch.equal(partial[3], full[3]) and torch.equal(partial[4], full[4])
    only_x, only_w, only_bn = (bwd(name, d, u, mean, invstd, tuple(i == j for j in range(3))) for i in range(3))
    assert torch.equal(only_x[0], full[0]) and (full[1] is None or torch.equal(only_x[1], full[1])) and only_x[2] is None and only_x[3] is None
    assert torch.equal(only_w[2], full[2]) and only_w[0] is None and only_w[3] is None
    assert torch.equal(only_bn[3], full[3]) and torch.equal(only_bn[4], full[4]) and only_bn[0] is None and only_bn[2] is None
    assert all(g is None for g in bwd(name, d, u, mean, invstd, (False, False, False)))
    with pytest.raises(ValueError, match="buffer gx0"):  # the doubled shape is not gx0's
        bwd(name, d, u, mean, invstd, (True, True, True), buffers={"gx0": torch.zeros(2, d["x0"].shape[1], 14, 22, device="cuda")})
    frozen = run_op(name, t, requires=("w", "g", "b"))
    everything = run_op(name, t)
    assert frozen["gx0"] is None and torch.equal(frozen["d_weight"], everything["d_weight"]) and torch.equal(frozen["d_bn_w"], everything["d_bn_w"])


@pytest.mark.parametrize("name,shape", [("inner1", (2, 7, 11)), ("inner3", (1, 36, 68)), ("general_up", (2, 7, 11))])
def test_identical_calls_give_identical_bits(name, shape):
    t, _, _ = case(name, *shape)
    a, b = run_op(name, t), run_op(name, t)
    assert {"out", "running_mean", "running_var", "gx0", "gx1", "d_weight", "d_bn_w", "d_bn_b", "g_residual", "d_conv_bias"} == set(a)
    for k, v in a.items():
        assert (v is None and b[k] is None) or torch.equal(v, b[k]), k


def test_both_directions_read_the_inference_kernels_doubled_map_bit_for_bit():
    """ops.conv2d_bn_act's up0 staging, written out by a 1 x 1 identity convolution, is the doubled map x0'.  The plain training op
    on x0' and the up0 op on x0 give the same u (the forward interpolates while it stages) and the same weight gradient (the
    backward interpolates from its LDS copy of the coarse footprint; both calls cut this layer's 5 input channels into one group,
    so their sums run in the same order), and gx0 is the transposed upsample of the plain op's gx0."""
    name = "up_alone"
    K, _, C0, _, _, _, _, act = CONFIGS[name]
    t, _, _ = case(name, 2, 7, 11)
    d, _, u, mean, invstd = saved(name, t)
    eye = torch.eye(C0, device="cuda").view(C0, C0, 1, 1).contiguous()
    doubled = ops.conv2d_bn_act(d["x0"], eye, torch.ones(C0, device="cuda"), torch.zeros(C0, device="cuda"), up0=True)
    assert tuple(doubled.shape) == (2, C0, 14, 22)
    _, u_plain, mean_plain, invstd_plain = ops.conv2d_bn_act_train_fwd(doubled, d["w"], None, d["g"], d["b"], d["rm"].clone(), d["rv"].clone(),
                                                                       MOMENTUM, EPS, act=act, slope=0.1)
    assert torch.equal(u, u_plain) and torch.equal(mean, mean_plain) and torch.equal(invstd, invstd_plain)
    fused = bwd(name, d, u, mean, invstd, (True, True, True))
    plain = ops.conv2d_bn_act_train_bwd(d["lw"], doubled, d["w"], d["g"], d["b"], u_plain, mean_plain, invstd_plain, act=act, slope=0.1)
    assert torch.equal(fused[2], plain[2])
    x = d["x0"].double().requires_grad_()
    (want,) = torch.autograd.grad(up2(x), x, plain[0].double())
    # 16 exact products (the weights are multiples of 1/16) whose magnitudes sum to at most 4 max|g|, and under 20 fp32 roundings
    assert float((fused[0].double() - want).abs().max()) <= 20 * 2.0 ** -24 * 4 * float(plain[0].abs().max())


def test_residual_may_alias_x1():
    """residual IS x1: the same bits as with a copy, and its gradient arrives summed on the aliased leaf."""
    t, _, _ = case("inner1", 2, 7, 11)
    own, aliased = run_op("inner1", t), run_op("inner1", t, residual="alias")
    for k in ("out", "running_mean", "running_var", "d_weight", "d_bn_w", "d_bn_b", "gx0"):
        assert torch.equal(own[k], aliased[k]), k
    assert torch.equal(aliased["gx1"], own["gx1"] + own["g_residual"])


def test_train_under_no_grad():
    """Buffers move, num_batches_tracked goes up by one (run_op asserts it), out equals the grad-mode call bit for bit, nothing is
    differentiable."""
    t, _, _ = case("inner2", 2, 7, 11)
    graded = run_op("inner2", t)
    with torch.no_grad():
        plain = run_op("inner2", t)
    assert "gx0" not in plain and torch.equal(plain["out"], graded["out"])
    for k in ("running_mean", "running_var"):
        assert torch.equal(plain[k], graded[k]) and not torch.equal(plain[k].cpu(), t["rm" if k == "running_mean" else "rv"])


# ---- the three modules ---------------------------------------------------------------------------------------------------------------
def test_autograd_keeps_no_doubled_map():
    """Under saved_tensors_hooks a decoder forward with "hip_fused" saves no tensor of the shape of a doubled map (B, C0, 2h, 2w) of any
    innerN; the same check under "hip" finds all three."""
    chs, B, h, w = fpn_fixture.FEAT_CHS, 2, 3, 5
    maps = [torch.from_numpy(synth.lattice_normalish((B, c, h << (3 - i), w << (3 - i)), 7700 + i)).cuda().requires_grad_() for i, c in enumerate(chs)]
    doubled = {(B, chs[3], 2 * h, 2 * w), (B, chs[2], 4 * h, 4 * w), (B, chs[1], 8 * h, 8 * w)}  # in front of inner1, inner2, inner3
    assert not doubled & {tuple(m.shape) for m in maps}
    found = {}
    for impl in ("hip_fused", "hip"):
        dec = build(torch.float32, "cuda", impl)["decoder"]
        shapes = []
        with torch.autograd.graph.saved_tensors_hooks(lambda t: (shapes.append(tuple(t.shape)), t)[1], lambda t: t):
            outs = dec(*maps)
        assert all(o.requires_grad for o in outs) and shapes
        found[impl] = doubled & set(shapes)
    assert found["hip_fused"] == set() and found["hip"] == doubled


@pytest.mark.parametrize("shape_name", [s[0] for s in fpn_fixture.SHAPES])
def test_whole_module_with_hip_fused_against_float64(shape_name):
    ref, e32 = module_reference(shape_name)
    got = module_on_gpu(shape_name, "hip_fused")
    compare_modules(f"{shape_name} hip_fused vs float64", got, ref, e32)
    for k, v in got.items():
        if k.startswith("grad/") and k.endswith(".0.bias"):
            assert not bool(v.any()), k  # exact zeros


@pytest.mark.parametrize("shape_name", [s[0] for s in fpn_fixture.SHAPES])
def test_hip_fused_against_the_modules_own_torch_path(shape_name):
    _, e32 = module_reference(shape_name)
    compare_modules(f"{shape_name} hip_fused vs torch", module_on_gpu(shape_name, "hip_fused"), module_on_gpu(shape_name, "torch"), e32)


def test_hip_fused_against_the_reference_modules_own_step():
    compare_to_golden("hip_fused vs the reference's modules", module_on_gpu(SHAPE, "hip_fused"), load_golden("g17_fpn_train"))


def test_module_calls_the_op_19_times_three_of_them_with_up0(monkeypatch):
    calls = []
    orig = ops.conv2d_bn_act_train
    monkeypatch.setattr(ops, "conv2d_bn_act_train", lambda *a, **k: (calls.append(bool(k.get("up0"))), orig(*a, **k))[1])
    mods = build(torch.float32, "cuda", "hip_fused")
    images, side = (t.cuda() for t in fpn_fixture.inputs("b"))
    out = run_modules(mods, images, side)
    assert len(calls) == 19 and sum(calls) == 3 and all(v.requires_grad for v in out.values())
    del calls[:]
    for m in mods.values():
        m.train_conv_impl = "hip"  # "hip" keeps its meaning: F.interpolate in front of the op, no up0
    run_modules(mods, images, side)
    assert len(calls) == 19 and sum(calls) == 0
    del calls[:]
    for m in mods.values():
        m.train_conv_impl = "hip_fused"
        m.train(False)
    with torch.no_grad():
        run_modules(mods, images, side)  # eval() takes the inference launches
    assert not calls


def fused_training_step():
    """test_fpn_train_gpu.one_training_step with fpn_train_impl = "hip_fused" (that function pins the call count of the impl it is
    given to "hip"'s): the same seed, parameters, batch, objective and stepper."""
    from gfnet_amd.model.network import GFNet
    from gfnet_amd.reference_backbone import ReferenceBackbone
    from gfnet_amd.trainer import FusedAdamWStep, train_step as trainer_step
    from test_fpn_gpu import StubVit

    images = torch.from_numpy(synth.lattice_uniform((4, 3, 448, 448), 78)).cuda()
    batch = {"im_A": images[:2], "im_B": images[2:]}

    def objective(out, _):
        loss = torch.zeros((), device="cuda")
        for scale in out.values():
            for d in scale.values():
                loss = loss + d["flow"].float().square().mean() + d["certainty"].float().square().mean()
        return loss

    calls, orig = [], ops.conv2d_bn_act_train
    ops.conv2d_bn_act_train = lambda *a, **k: (calls.append(bool(k.get("up0"))), orig(*a, **k))[1]
    flags = (torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark)
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False  # as that function: the rest of the model's library convolutions
    try:
        torch.manual_seed(0)
        bb = ReferenceBackbone(E2E_CONF, vit=StubVit(), decoder="hip", fpn="hip", fpn_train_impl="hip_fused").cuda()
        fpn_fixture.fill({"encoder": bb.encoder, "decoder": bb.decoder, "merge_layer": bb.merge_layer})
        model = GFNet(E2E_CONF, backbone=bb).cuda()
        model.train()
        stepper = FusedAdamWStep([p for p in model.parameters() if p.requires_grad], lr=1e-4, init_scale=1.0, zero_grads=False)
        res = trainer_step(batch, model, objective, stepper)
    finally:
        ops.conv2d_bn_act_train = orig
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = flags
    for top in (bb.encoder, bb.decoder, bb.merge_layer):
        for k, p in top.named_parameters():
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
            assert k.endswith("0.bias") or float(p.grad.abs().max()) > 0.0, k
    assert len(calls) == 19 and sum(calls) == 3, "the FPN did not take the path it was asked for"
    return float(res["train_loss"])


def test_one_training_step_end_to_end():
    """One trainer.train_step on 2 pairs of 448 x 448 with E2E_CONF and fpn_train_impl = "hip_fused": every FPN parameter gets a finite
    gradient, and the loss is within 1e-4 max(1, |loss|) of the fpn_train_impl = "torch" run (the project's whole-model tolerance)."""
    fused, ref = fused_training_step(), one_training_step("torch")
    print(f"one training step: loss {fused:.9e} (hip_fused) vs {ref:.9e} (torch)")
    assert np.isfinite(fused) and abs(fused - ref) <= 1e-4 * max(1.0, abs(ref))
