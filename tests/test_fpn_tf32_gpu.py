"""The TF32 class of the native FPN on the GPU (csrc/fpn_conv_tf32.hip; ops.conv2d_bn_act_tf32, precision="tf32" of the training op,
conv_precision / fpn_precision "tf32"): a census that pins the arithmetic, the eval op against the class's oracle within the bound
derived in tests/test_fpn_tf32_cpu.py, the training op -- every output of test_fpn_train_gpu.NAMES -- against the float64
definition with the class's products where the class runs, the three modules in eval() and train() against float64 and against the
reference's own maps and step, and the whole model.

Which product of the training op is the class's (include/gfnet_hip.h): the forward convolution where Cout is a multiple of 8; the
input gradient of x0 (x1) under stride 1 where C0 (C1) is a multiple of 8; the weight gradient under stride 1 without up0, P on
(x, gu).  Everything else -- the stride-2 input gradient, the weight gradient under stride 2 and under up0, launches whose output
channels are no multiple of 8 -- is exact fp32 in the library and the exact product in the oracle.

Largest ratios measured (MI355X): see DESIGN 4.8."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fpn_fixture
import synth
import test_fpn_train_gpu as tg
import test_fpn_train_up_gpu as tu
from conftest import load_golden
from gfnet_amd import ops
from gfnet_amd.model import fpn
from make_golden_fpn_train import SHAPE, stored, train_step
from test_fpn_cpu import build_modules, run_modules
from test_fpn_gpu import LAYERS, StubVit
from test_fpn_half_cpu import CONF, CONFIGS, EDGE, shape_of
from test_fpn_tf32_cpu import E16, split, tf32_case

pytestmark = pytest.mark.gpu

MOMENTUM, EPS = tg.MOMENTUM, tg.EPS


# ---- census ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [8, 32])
def test_census_identity_weight_returns_hi_plus_lo_bit_for_bit(C):
    """A 1 x 1 identity weight (8 -> 8: the 16-wide instruction, 32 -> 32: the 32-wide one), scale 1, shift 0 on generic 24-bit
    inputs: 1 = 1 + 0 in the split, so every output is x_hi 1 + x_hi 0 + x_lo 1 = float32(hi + lo), for the eval op and for the
    training op's u -- and that is NOT the input, which is what the fp32 kernel would return."""
    # (the lattice values of synth have few significant bits and split exactly: scaled by 1 / 3 they fill all 24)
    x = torch.from_numpy(synth.lattice_normalish((2, C, 13, 19), 71 + C) * np.float32(1.0 / 3.0))
    hi, lo = split(x)
    want = hi + lo
    assert torch.equal(want.double(), hi.double() + lo.double()) and int((want != x).sum()) > x.numel() // 2
    eye = torch.eye(C).view(C, C, 1, 1).contiguous().cuda()
    one, zero = torch.ones(C, device="cuda"), torch.zeros(C, device="cuda")
    out = ops.conv2d_bn_act_tf32(x.cuda(), eye, one, zero)
    assert out.dtype == torch.float32 and torch.equal(out.cpu(), want) and not torch.equal(out.cpu(), x)
    assert torch.equal(ops.conv2d_bn_act(x.cuda(), eye, one, zero).cpu(), x)  # the fp32 class returns the input
    _, u, _, _ = ops.conv2d_bn_act_train_fwd(x.cuda(), eye, None, one, zero, zero.clone(), one.clone(), MOMENTUM, EPS, precision="tf32")
    assert torch.equal(u.cpu(), want)
    _, u32, _, _ = ops.conv2d_bn_act_train_fwd(x.cuda(), eye, None, one, zero, zero.clone(), one.clone(), MOMENTUM, EPS)
    assert torch.equal(u32.cpu(), x)
    # An inf in the input comes out inf and nothing becomes NaN.  Under an identity weight every arithmetic, fp32 included, multiplies
    # the inf by the other channels' zeros; so this part takes a dense weight of 1 + 2^-9 = (hi 1, lo 2^-9), both halves positive: inf
    # hi + inf lo + 0 hi = inf in every output channel of that pixel.  Without the guard lo = bf16(inf - inf) is NaN.
    xi = x.clone()
    xi[0, 1, 3, 4] = float("inf")
    xi[1, C - 1, 5, 6] = -float("inf")
    dense = torch.full((C, C, 1, 1), 1.0 + 2.0 ** -9, device="cuda")
    for outi in (ops.conv2d_bn_act_tf32(xi.cuda(), dense, one, zero).cpu(),
                 ops.conv2d_bn_act_train_fwd(xi.cuda(), dense, None, one, zero, zero.clone(), one.clone(), MOMENTUM, EPS, precision="tf32")[1].cpu()):
        assert not bool(torch.isnan(outi).any())
        assert bool((outi[0, :, 3, 4] == float("inf")).all()) and bool((outi[1, :, 5, 6] == -float("inf")).all())
        assert int(torch.isinf(outi).sum()) == 2 * C
        assert torch.equal(outi[:, :, :3], ops.conv2d_bn_act_tf32(x.cuda(), dense, one, zero).cpu()[:, :, :3])  # the other pixels as without it


# ---- the eval op -----------------------------------------------------------------------------------------------------------------------
def run_op(name, args):
    K, stride, C0, C1, Cout, up0, res, act = CONFIGS[name]
    x0, x1, w, scale, shift, _ = (None if t is None else t.cuda() for t in args)
    residual = {"x0": x0, "x1": x1, None: None}[res]
    return ops.conv2d_bn_act_tf32(x0, w, scale, shift, x1=x1, up0=up0, residual=residual, stride=stride, act=act, slope=0.1)


def check_case(name, B, Ho, Wo):
    args, ref, bound, exact, class_bound = tf32_case(name, B, Ho, Wo)
    out = run_op(name, args)
    assert out.shape == ref.shape and out.dtype == torch.float32
    got = out.cpu().double()
    assert bool(torch.isfinite(got).all())
    ratio = float(((got - ref).abs() / bound).max())
    L = 1.1 if CONFIGS[name][7] == "swish" else 1.0
    away = float(((got - exact).abs() / (L * class_bound + bound)).max())  # the class's distance from exact arithmetic
    print(f"{name} {B}x{Ho}x{Wo}: worst error / bound {ratio:.3f} (max err {float((got - ref).abs().max()):.3e}); "
          f"|out - exact| / (3 2^-16 S + bound) {away:.3f}")
    assert ratio <= 1.0, (name, ratio)
    assert away <= 1.0, (name, away)
    return out


@pytest.mark.parametrize("name", list(LAYERS))
def test_every_layer_of_the_fpn_as_an_op(name):
    """B = 2, output 13 x 19 (the up0 layers: 14 x 22 from a 7 x 11 map; stride 2: from 25 x 37)."""
    check_case(name, *shape_of(name))


@pytest.mark.parametrize("name", ["conv00", "conv01", "conv10", "out3", "inner3", "downsample1", "downsample2", "downsample3", "conv30",
                                  "merge_layer", "inner1", "out0"])
def test_every_kernel_variant_across_tile_boundaries(name):
    """B = 1, output 72 x 136: more than one 16 x 32 tile in both directions with a tail in each; every K, both strides, up0 and x1,
    the 16-wide instruction (Cout 8 and 16) and the 32-wide one (Cout 32 and 64)."""
    check_case(name, 1, 72, 136)


@pytest.mark.parametrize("name", list(EDGE))
def test_edge_channel_counts(name):
    """Cout 24 and 40 (padding inside a 16- or 32-wide instruction), Cin 3, 5 and 13 (a channel group that ends mid-unit) at a 9 x 35
    output (up0: 10 x 36)."""
    up0 = EDGE[name][5]
    check_case(name, 2, 10 if up0 else 9, 36 if up0 else 35)


@pytest.mark.parametrize("name", ["conv00", "conv01", "downsample1", "conv10", "out3", "downsample3", "conv30", "out0", "edge_k7_cout40"])
def test_tiny_maps(name):
    """1 x 1, 1 x 2 and 2 x 3 outputs with every K on both instructions: maps smaller than the kernel, most taps padding."""
    for Ho, Wo in ((1, 1), (1, 2), (2, 3)):
        check_case(name, 3, Ho, Wo)


@pytest.mark.parametrize("name", ["conv01", "inner2", "merge_layer", "downsample2"])
def test_identical_calls_give_identical_bits(name):
    args = tf32_case(name, 2, 14, 22)[0]
    assert torch.equal(run_op(name, args), run_op(name, args))


@pytest.mark.parametrize("name", ["inner1", "merge_layer", "edge_cin13_cout8"])
def test_residual_may_alias_an_input(name):
    """residual IS x1 (x0 for the merge layer) in run_op; a copy of it gives the same bits."""
    K, stride, C0, C1, Cout, up0, res, act = CONFIGS[name]
    args = tf32_case(name, 2, 14, 22)[0]
    x0, x1, w, scale, shift, _ = (None if t is None else t.cuda() for t in args)
    aliased = run_op(name, args)
    copied = ops.conv2d_bn_act_tf32(x0, w, scale, shift, x1=x1, up0=up0, residual=(x0 if res == "x0" else x1).clone(), stride=stride, act=act)
    assert torch.equal(aliased, copied)


def test_op_refuses_what_it_cannot_run():
    x, w, s = torch.zeros(1, 3, 8, 8, device="cuda"), torch.zeros(8, 3, 3, 3, device="cuda"), torch.zeros(8, device="cuda")
    with pytest.raises(TypeError, match="float32"):
        ops.conv2d_bn_act_tf32(x.half(), w, s, s)
    with pytest.raises(ValueError, match="channels"):
        ops.conv2d_bn_act_tf32(x, w, s, s, x1=x)
    with pytest.raises(Exception, match="kernel size 2"):
        ops.conv2d_bn_act_tf32(x, torch.zeros(8, 3, 2, 2, device="cuda"), s, s)
    with pytest.raises(Exception, match="multiple of 8"):
        ops.conv2d_bn_act_tf32(x, torch.zeros(12, 3, 3, 3, device="cuda"), torch.zeros(12, device="cuda"), torch.zeros(12, device="cuda"))
    layer = fpn.Conv2d(3, 12, 3, padding=1, conv_precision="tf32").cuda().train(False)  # the module runs such a layer on the fp32 op
    ref = fpn.Conv2d(3, 12, 3, padding=1).cuda().train(False)
    ref.load_state_dict(layer.state_dict())
    xr = torch.from_numpy(synth.lattice_normalish((1, 3, 8, 8), 3)).cuda()
    with torch.no_grad():
        assert torch.equal(layer(xr), ref(xr))


# ---- the training op -------------------------------------------------------------------------------------------------------------------
def halves(t):
    """The split of float32(t), in t's dtype (float64 for the oracle, fp32 for the unit)."""
    hi, lo = split(t.float())
    return hi.to(t.dtype), lo.to(t.dtype)


def three(op, a, b):
    """The class's product of a bilinear op: hi hi + hi lo + lo hi (= op(a~, b~) - op(a_lo, b_lo))."""
    (ah, al), (bh, bl) = halves(a), halves(b)
    return op(ah, bh) + op(ah, bl) + op(al, bh)


class ClassConv(torch.autograd.Function):
    """u = conv(x, w) with the class's product wherever the library runs the class (route: fwd, gx0, gx1, w), the exact one elsewhere."""

    @staticmethod
    def forward(ctx, x, w, stride, C0, route):
        ctx.save_for_backward(x, w)
        ctx.meta = (stride, C0, route)
        op = lambda a, b: F.conv2d(a, b, stride=stride, padding=w.shape[-1] // 2)
        return three(op, x, w) if route["fwd"] else op(x, w)

    @staticmethod
    def backward(ctx, gu):
        x, w = ctx.saved_tensors
        stride, C0, route = ctx.meta
        pad = w.shape[-1] // 2
        inp = lambda g, ww: torch.nn.grad.conv2d_input(x.shape, ww, g, stride=stride, padding=pad)
        wg = lambda xx, g: torch.nn.grad.conv2d_weight(xx, w.shape, g, stride=stride, padding=pad)
        gx = inp(gu, w)
        if route["gx0"] or route["gx1"]:
            gc = three(inp, gu, w)
            gx = torch.cat((gc[:, :C0] if route["gx0"] else gx[:, :C0], gc[:, C0:] if route["gx1"] else gx[:, C0:]), dim=1)
        return gx, (three(wg, x, gu) if route["w"] else wg(x, gu)), None, None, None


def routes(C0, C1, Cout, stride, up0):
    return {"fwd": Cout % 8 == 0, "gx0": stride == 1 and C0 % 8 == 0, "gx1": stride == 1 and C1 > 0 and C1 % 8 == 0,
            "w": stride == 1 and not up0}


def definition(t, stride, act, up0=False):
    """test_fpn_train_gpu.definition (with up0: test_fpn_train_up_gpu.definition) with ClassConv for F.conv2d."""
    leaf = {k: (None if v is None else v.clone().requires_grad_(k in ("x0", "x1", "w", "cb", "g", "b", "res"))) for k, v in t.items()}
    x0 = tu.up2(leaf["x0"]) if up0 else leaf["x0"]
    x = x0 if leaf["x1"] is None else torch.cat((x0, leaf["x1"]), dim=1)
    C0, C1, Cout = x0.shape[1], x.shape[1] - x0.shape[1], leaf["w"].shape[0]
    u = ClassConv.apply(x, leaf["w"], stride, C0, routes(C0, C1, Cout, stride, up0))
    rm, rv = leaf["rm"], leaf["rv"]
    y = F.batch_norm(u if leaf["cb"] is None else u + leaf["cb"].view(1, -1, 1, 1), rm, rv, leaf["g"], leaf["b"], True, MOMENTUM, EPS)
    out = tg.act_fn(y, act)
    if leaf["res"] is not None:
        out = out + leaf["res"]
    wanted = [k for k in ("x0", "x1", "res", "w", "g", "b", "cb") if leaf[k] is not None]
    grads = dict(zip(wanted, torch.autograd.grad((out * leaf["lw"]).sum(), [leaf[k] for k in wanted])))
    ud = u.detach()
    return {"out": out.detach(), "u": ud, "mean": ud.mean((0, 2, 3)), "invstd": (ud.var((0, 2, 3), unbiased=False) + EPS).rsqrt(),
            "running_mean": rm, "running_var": rv, "gx0": grads["x0"], "gx1": grads.get("x1"), "g_residual": grads.get("res"),
            "d_weight": grads["w"], "d_bn_w": grads["g"], "d_bn_b": grads["b"]}


@functools.lru_cache(maxsize=None)
def class_case(name, B, Ho, Wo, up0=False):
    """The inputs of test_fpn_train_gpu.case (up0: of test_fpn_train_up_gpu.case, Ho x Wo the coarse size), the class's float64 results,
    every tensor's e32 -- the same definition in fp32 on the CPU against it -- and what the fp32 class's case gives for u: the exact u,
    its e32 and 3 2^-16 conv64(|x|, |w|)."""
    t, exact, exact_e32 = tu.case(name, B, Ho, Wo) if up0 else tg.case(name, B, Ho, Wo)
    stride, act = (tu.CONFIGS if up0 else tg.CONFIGS)[name][1], (tu.CONFIGS if up0 else tg.CONFIGS)[name][7]
    ref = definition({k: (None if v is None else v.double()) for k, v in t.items()}, stride, act, up0)
    r32 = definition(t, stride, act, up0)
    e32 = {k: (None if ref[k] is None else float((r32[k].double() - ref[k]).abs().max())) for k in tg.NAMES}
    x0 = tu.up2(t["x0"].double()) if up0 else t["x0"].double()
    x = x0 if t["x1"] is None else torch.cat((x0, t["x1"].double()), 1)
    S = F.conv2d(x.abs(), t["w"].double().abs(), stride=stride, padding=t["w"].shape[-1] // 2)
    return t, ref, e32, exact["u"], exact_e32["u"], 3 * E16 * S


def run_train_op(name, t, up0=False, precision="tf32", requires=("x0", "x1", "w", "g", "b", "res", "cb")):
    K, stride, C0, C1, Cout, _, res, act = (tu.CONFIGS if up0 else tg.CONFIGS)[name]
    d = {k: (None if v is None else v.cuda().requires_grad_(k in requires)) for k, v in t.items()}
    nbt = torch.zeros((), dtype=torch.long, device="cuda")
    out = ops.conv2d_bn_act_train(d["x0"], d["w"], d["cb"], d["g"], d["b"], d["rm"], d["rv"], nbt, MOMENTUM, EPS, x1=d["x1"],
                                  residual=d["res"], stride=stride, act=act, slope=0.1, up0=up0, precision=precision)
    assert int(nbt) == 1
    got = {"out": out.detach(), "running_mean": d["rm"], "running_var": d["rv"]}
    if out.requires_grad:
        (out * d["lw"]).sum().backward()
        got.update(gx0=d["x0"].grad, gx1=None if d["x1"] is None else d["x1"].grad, d_weight=d["w"].grad, d_bn_w=d["g"].grad,
                   d_bn_b=d["b"].grad, g_residual=None if d["res"] is None else d["res"].grad,
                   d_conv_bias=None if d["cb"] is None else d["cb"].grad)
    return got


def saved(name, t, up0=False, precision="tf32"):
    K, stride, C0, C1, Cout, _, res, act = (tu.CONFIGS if up0 else tg.CONFIGS)[name]
    d = {k: (None if v is None else v.cuda()) for k, v in t.items()}
    out, u, mean, invstd = ops.conv2d_bn_act_train_fwd(d["x0"], d["w"], d["cb"], d["g"], d["b"], d["rm"], d["rv"], MOMENTUM, EPS, x1=d["x1"],
                                                       residual=d["res"], stride=stride, act=act, slope=0.1, up0=up0, precision=precision)
    return d, out, u, mean, invstd


def check_train_case(name, B, Ho, Wo, floor=False, up0=False):
    t, ref, e32, u_exact, u_e32, class_bound = class_case(name, B, Ho, Wo, up0)
    got = run_train_op(name, t, up0)
    _, out, u, mean, invstd = saved(name, t, up0)
    assert torch.equal(out, got["out"])  # the wrapper and the autograd function run the same launches
    got.update(u=u, mean=mean, invstd=invstd)
    worst, failed = 0.0, []
    for k in tg.NAMES:
        if ref[k] is None:
            assert got.get(k) is None, k
            continue
        if k == "g_residual":  # gy itself
            assert torch.equal(got[k].cpu().double(), ref[k]), k
            continue
        unit = e32[k]
        if floor or k in tg.VECTORS:
            unit = max(unit, 2.0 ** -24 * float(ref[k].abs().max()))
        assert unit > 0.0, (name, k)
        assert got[k].shape == ref[k].shape and got[k].dtype == torch.float32, k
        err = float((got[k].detach().cpu().double() - ref[k]).abs().max())
        worst = max(worst, err / unit)
        print(f"{name} {B}x{Ho}x{Wo} {k}: max err {err:.3e}, unit {unit:.3e}, ratio {err / unit:.2f}")
        if err > 4 * unit:
            failed.append((k, err, unit))
    if floor:
        u_e32 = max(u_e32, 2.0 ** -24 * float(u_exact.abs().max()))
    away = float(((u.cpu().double() - u_exact).abs() / (class_bound + 4 * u_e32)).max())
    print(f"{name} {B}x{Ho}x{Wo}: largest ratio {worst:.2f}; |u - exact u| / (3 2^-16 S + 4 e32) {away:.3f}")
    assert not failed, (name, failed)
    assert away <= 1.0, (name, away)
    if t["cb"] is not None:
        assert got["d_conv_bias"] is not None and not bool(got["d_conv_bias"].any()), "the conv bias's gradient is exactly zero"
    return got


@pytest.mark.parametrize("name", list(tg.CONFIGS))
def test_training_op_every_layer(name):
    """B = 2, output 13 x 19 (stride 2: from 25 x 37); the up0 layers take a pre-doubled 14 x 22 x0."""
    up0 = tg.CONFIGS[name][5]
    check_train_case(name, 2, 14 if up0 else 13, 22 if up0 else 19)


@pytest.mark.parametrize("name", ["conv00", "conv01", "downsample1", "downsample3", "conv30", "merge_layer", "inner3", "out3", "general_s2"])
def test_training_op_across_a_tile_boundary(name):
    check_train_case(name, 1, 72, 136)


@pytest.mark.parametrize("name", ["conv00", "downsample1", "out3", "general_k7", "inner3"])
def test_training_op_tiny_maps(name):
    check_train_case(name, 3, 2, 3, floor=True)


@pytest.mark.parametrize("name", ["inner1", "inner3", "general_up"])
def test_training_op_with_the_upsample_inside(name):
    """up0=True against the float64 definition with the upsample inside (coarse 7 x 11), and for inner1 against the doubled-map route:
    the plain tf32 op on the doubled map -- written out by the fp32 inference kernel's identity convolution -- gives the same u, mean,
    invstd, gx1 and BatchNorm gradients bit for bit, and gx0 is that route's gx0 through the transposed upsample."""
    got = check_train_case(name, 2, 7, 11, up0=True)
    if name != "inner1":
        return
    K, _, C0, C1, Cout, _, res, act = tu.CONFIGS[name]
    t = class_case(name, 2, 7, 11, True)[0]
    d, _, u, mean, invstd = saved(name, t, True)
    eye = torch.eye(C0, device="cuda").view(C0, C0, 1, 1).contiguous()
    doubled = ops.conv2d_bn_act(d["x0"], eye, torch.ones(C0, device="cuda"), torch.zeros(C0, device="cuda"), up0=True)
    _, u_p, mean_p, invstd_p = ops.conv2d_bn_act_train_fwd(doubled, d["w"], d["cb"], d["g"], d["b"], d["rm"].clone(), d["rv"].clone(), MOMENTUM, EPS,
                                                           x1=d["x1"], residual=d["res"], act=act, slope=0.1, precision="tf32")
    assert torch.equal(u, u_p) and torch.equal(mean, mean_p) and torch.equal(invstd, invstd_p)
    kw = dict(x1=d["x1"], act=act, slope=0.1, precision="tf32")
    fused = ops.conv2d_bn_act_train_bwd(d["lw"], d["x0"], d["w"], d["g"], d["b"], u, mean, invstd, up0=True, **kw)
    plain = ops.conv2d_bn_act_train_bwd(d["lw"], doubled, d["w"], d["g"], d["b"], u_p, mean_p, invstd_p, **kw)
    assert torch.equal(fused[1], plain[1]) and torch.equal(fused[3], plain[3]) and torch.equal(fused[4], plain[4])
    assert torch.equal(fused[0], got["gx0"]) and torch.equal(fused[2], got["d_weight"])
    x = d["x0"].double().requires_grad_()
    (want,) = torch.autograd.grad(tu.up2(x), x, plain[0].double())
    assert float((fused[0].double() - want).abs().max()) <= 20 * 2.0 ** -24 * 4 * float(plain[0].abs().max())


@pytest.mark.parametrize("name", ["conv00", "conv01", "conv30", "merge_layer", "out1", "general_k7", "downsample2", "inner2"])
def test_census_of_the_weight_gradient(name):
    """The same saved u, mean and invstd (the fp32 forward's) handed to the backward of both classes with need = weight only: gu is then
    the same map bit for bit, and d_weight differs in bits exactly where the class has its own weight gradient -- stride 1 without up0.
    A silent fall-back to the fp32 kernel there, or the class's kernel under stride 2 or up0, fails.  Where it differs it stays within
    the class's distance: 3 2^-16 sum |x| |gu| per weight, plus 4 x the fp32 kernel's own e32."""
    up0 = name == "inner2"  # (that one through the up0 entry on the coarse map; the other up0 layers of tg.CONFIGS get a doubled x0)
    t, _, e32 = (tu.case(name, 2, 7, 11) if up0 else tg.case(name, 2, 13, 19))
    K, stride, C0, C1, Cout, _, res, act = (tu.CONFIGS if up0 else tg.CONFIGS)[name]
    d, _, u, mean, invstd = saved(name, t, up0, precision="fp32")
    dw = {prec: ops.conv2d_bn_act_train_bwd(d["lw"], d["x0"], d["w"], d["g"], d["b"], u, mean, invstd, x1=d["x1"], stride=stride, act=act,
                                            slope=0.1, need=(False, True, False), up0=up0, precision=prec)[2] for prec in ("fp32", "tf32")}
    if stride == 1 and not up0:
        assert not torch.equal(dw["tf32"], dw["fp32"]), name
        x = d["x0"] if d["x1"] is None else torch.cat((d["x0"], d["x1"]), 1)
        # |gu| <= what the fp32 op's own input gradient of ones would need; bound it by the exact weight gradient of |x| against |gu|
        # recovered from the fp32 result's definition: d_weight = wg(x, gu), so use torch's own gu through autograd on the saved u
        uu = u.double().requires_grad_()
        y = F.batch_norm(uu, None, None, d["g"].double(), d["b"].double(), True, 0.0, EPS)
        (gu,) = torch.autograd.grad((tg.act_fn(y, act) * d["lw"].double()).sum(), uu)
        S = torch.nn.grad.conv2d_weight(x.double().abs(), d["w"].shape, gu.abs(), stride=1, padding=K // 2)
        diff = (dw["tf32"].double() - dw["fp32"].double()).abs()
        ratio = float((diff / (3 * E16 * S + 8 * e32["d_weight"])).max())
        print(f"{name}: |d_weight tf32 - fp32| / (3 2^-16 S + 8 e32) {ratio:.3f}")
        assert ratio <= 1.0, (name, ratio)
    else:
        assert torch.equal(dw["tf32"], dw["fp32"]), name


@pytest.mark.parametrize("name", ["conv01", "downsample2", "merge_layer"])
def test_training_op_need_mask(name):
    t = class_case(name, 2, 13, 19)[0]
    d, _, u, mean, invstd = saved(name, t)
    K, stride, C0, C1, Cout, _, res, act = tg.CONFIGS[name]

    def bwd(need, buffers=None):
        return ops.conv2d_bn_act_train_bwd(d["lw"], d["x0"], d["w"], d["g"], d["b"], u, mean, invstd, x1=d["x1"], stride=stride, act=act,
                                           slope=0.1, need=need, buffers=buffers, precision="tf32")

    full = bwd((True, True, True))
    poison = {"gx0": torch.full_like(d["x0"], 7.25), "gx1": None if d["x1"] is None else torch.full_like(d["x1"], 7.25)}
    partial = bwd((False, True, True), buffers=dict(poison))
    assert partial[0] is None and partial[1] is None
    assert bool((poison["gx0"] == 7.25).all()) and (poison["gx1"] is None or bool((poison["gx1"] == 7.25).all()))
    assert torch.equal(partial[2], full[2]) and torch.equal(partial[3], full[3]) and torch.equal(partial[4], full[4])
    only_x, only_w, only_bn = (bwd(tuple(i == j for j in range(3))) for i in range(3))
    assert torch.equal(only_x[0], full[0]) and (full[1] is None or torch.equal(only_x[1], full[1])) and only_x[2] is None and only_x[3] is None
    assert torch.equal(only_w[2], full[2]) and only_w[0] is None and only_w[3] is None
    assert torch.equal(only_bn[3], full[3]) and torch.equal(only_bn[4], full[4]) and only_bn[0] is None and only_bn[2] is None
    assert all(g is None for g in bwd((False, False, False)))
    frozen = run_train_op(name, t, requires=("w", "g", "b"))
    everything = run_train_op(name, t)
    assert frozen["gx0"] is None and torch.equal(frozen["d_weight"], everything["d_weight"]) and torch.equal(frozen["d_bn_w"], everything["d_bn_w"])


@pytest.mark.parametrize("name", ["conv01", "downsample2", "merge_layer", "inner2"])
def test_training_op_identical_calls_give_identical_bits_and_buffers_move_as_under_fp32(name):
    t = class_case(name, 2, 14, 22)[0]
    a, b = run_train_op(name, t), run_train_op(name, t)
    for k, v in a.items():
        assert (v is None and b[k] is None) or torch.equal(v, b[k]), k
    # the running buffers move as under "fp32": torch's momentum update of the class's OWN statistics, as the forward returns them
    # (mean, and var = 1 / invstd^2 - eps), with the conv bias in the mean and the unbiased variance; num_batches_tracked is asserted
    # in run_train_op.  Tolerance: the stored value rounds once (2^-24), the returned mean once, the returned invstd once, which var
    # takes twice: 2^-23 of the largest running mean, 2^-22 of the largest running variance
    f = run_train_op(name, t, precision="fp32")
    assert not torch.equal(a["out"], f["out"])  # another arithmetic ran
    d, _, u, mean, invstd = saved(name, t)
    n = u.numel() // u.shape[1]
    cb = 0.0 if t["cb"] is None else t["cb"].double()
    want_rm = (1 - MOMENTUM) * t["rm"].double() + MOMENTUM * (mean.cpu().double() + cb)
    want_rv = (1 - MOMENTUM) * t["rv"].double() + MOMENTUM * (invstd.cpu().double() ** -2 - EPS) * n / (n - 1)
    assert torch.equal(d["rm"], a["running_mean"]) and torch.equal(d["rv"], a["running_var"])
    assert float((a["running_mean"].cpu().double() - want_rm).abs().max()) <= 2.0 ** -23 * float(want_rm.abs().max())
    assert float((a["running_var"].cpu().double() - want_rv).abs().max()) <= 2.0 ** -22 * float(want_rv.abs().max())
    assert not torch.equal(a["running_mean"].cpu(), t["rm"]) and not torch.equal(a["running_var"].cpu(), t["rv"])


# ---- the three modules -----------------------------------------------------------------------------------------------------------------
class _EmulConv(torch.autograd.Function):
    """F.conv2d with every operand of every product, in both directions, replaced by hi + lo: the class without its dropped term."""

    @staticmethod
    def forward(ctx, x, w, bias, stride, padding):
        ctx.save_for_backward(x, w)
        ctx.meta = (stride, padding, bias is not None)
        til = lambda t: sum(halves(t))
        return _conv2d(til(x), til(w), bias, stride, padding)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        stride, padding, has_bias = ctx.meta
        til = lambda t: sum(halves(t))
        gx = torch.nn.grad.conv2d_input(x.shape, til(w), til(g), stride=stride, padding=padding)
        gw = torch.nn.grad.conv2d_weight(til(x), w.shape, til(g), stride=stride, padding=padding)
        return gx, gw, (g.sum((0, 2, 3)) if has_bias else None), None, None


_conv2d = F.conv2d


class emulation:
    """Within it torch.nn.functional.conv2d is _EmulConv (the FPN uses no dilation and no groups)."""

    def __enter__(self):
        F.conv2d = lambda x, w, bias=None, stride=1, padding=0, dilation=1, groups=1: _EmulConv.apply(x, w, bias, stride, padding)

    def __exit__(self, *exc):
        F.conv2d = _conv2d


def eval_modules(dtype, device, precision="fp32", conv_impl="hip"):
    mods, _ = build_modules(conv_impl)
    for m in mods.values():
        m.to(device=device, dtype=dtype)
        m.conv_precision = precision
    return mods


@functools.lru_cache(maxsize=None)
def eval_reference(shape_name):
    """(float64 maps, per map the unit: the larger of e32 and the emulation's error, per map the emulation's error alone)."""
    images, side = fpn_fixture.inputs(shape_name)
    with torch.no_grad():
        ref = run_modules(eval_modules(torch.float64, "cpu"), images.double(), side.double())
        r32 = run_modules(eval_modules(torch.float32, "cpu"), images, side)
        with emulation():
            emu = run_modules(eval_modules(torch.float64, "cpu"), images.double(), side.double())
    e_emu = {k: float((emu[k] - ref[k]).abs().max()) for k in ref}
    return ref, {k: max(float((r32[k].double() - ref[k]).abs().max()), e_emu[k]) for k in ref}, e_emu


@functools.lru_cache(maxsize=None)
def eval_on_gpu(shape_name):
    images, side = (t.cuda() for t in fpn_fixture.inputs(shape_name))
    with torch.no_grad():
        return run_modules(eval_modules(torch.float32, "cuda", "tf32"), images, side)


@pytest.mark.parametrize("shape_name", [s[0] for s in fpn_fixture.SHAPES])
def test_modules_in_eval_against_float64_and_the_reference_modules_maps(shape_name):
    ref, unit, e_emu = eval_reference(shape_name)
    got = eval_on_gpu(shape_name)
    g = load_golden("g15_fpn")
    for k in fpn_fixture.MAPS:
        assert got[k].dtype == torch.float32 and got[k].shape == ref[k].shape
        err = float((got[k].cpu().double() - ref[k]).abs().max())
        want, g32 = g[f"{shape_name}/{k}"], float(g[f"{shape_name}/{k}/fp32_vs_fp64"])
        gerr = float(np.abs(fpn_fixture.stored(k, got[k]).cpu().numpy().astype(np.float64) - want).max())
        gunit = max(g32, e_emu[k])
        print(f"{shape_name}/{k}: vs float64 {err:.3e} (unit {unit[k]:.3e}, ratio {err / unit[k]:.2f}); vs the reference's map {gerr:.3e} "
              f"(unit {gunit:.3e}, ratio {gerr / gunit:.2f})")
        assert err <= 4 * unit[k] and gerr <= 4 * gunit, (shape_name, k)
    fp32 = run_modules(eval_modules(torch.float32, "cuda"), *(t.cuda() for t in fpn_fixture.inputs(shape_name)))
    assert not any(torch.equal(fp32[k], got[k]) for k in fpn_fixture.MAPS)  # the class ran


def train_modules(dtype, device, train_conv_impl, precision="fp32"):
    mods = tg.build(dtype, device, train_conv_impl)
    for m in mods.values():
        m.conv_precision = precision
    return mods


@functools.lru_cache(maxsize=None)
def train_reference(shape_name):
    ref, e32 = tg.module_reference(shape_name)
    images, side = (t.double() for t in fpn_fixture.inputs(shape_name))
    with emulation():
        emu = train_step(train_modules(torch.float64, "cpu", "torch"), run_modules, images, side)
    e_emu = {k: float((emu[k] - ref[k]).abs().max()) for k in ref}
    return ref, {k: max(e32[k], e_emu[k]) for k in ref}, e_emu


@functools.lru_cache(maxsize=None)
def train_on_gpu(shape_name, impl):
    images, side = (t.cuda() for t in fpn_fixture.inputs(shape_name))
    return train_step(train_modules(torch.float32, "cuda", impl, "tf32"), run_modules, images, side)


@pytest.mark.parametrize("impl", ["hip", "hip_fused"])
@pytest.mark.parametrize("shape_name", [s[0] for s in fpn_fixture.SHAPES])
def test_modules_in_training_mode_against_float64(shape_name, impl):
    ref, unit, _ = train_reference(shape_name)
    got = train_on_gpu(shape_name, impl)
    tg.compare_modules(f"{shape_name} tf32 {impl} vs float64", got, ref, unit)
    for k, v in got.items():
        if k.startswith("grad/") and k.endswith(".0.bias"):
            assert not bool(v.any()), k  # exact zeros
    plain = tg.module_on_gpu(shape_name, "hip")
    assert not torch.equal(plain["map/dec1"], got["map/dec1"])  # the class ran


@pytest.mark.parametrize("impl", ["hip", "hip_fused"])
def test_modules_in_training_mode_against_the_reference_modules_own_step(impl):
    """tests/golden/g17_fpn_train.npz with test_fpn_train_gpu.compare_to_golden's rules; the unit is the larger of the recorded e32 and
    the emulation's error on the stored part."""
    g = load_golden("g17_fpn_train")
    got = train_on_gpu(SHAPE, impl)
    ref, _, _ = train_reference(SHAPE)
    images, side = (t.double() for t in fpn_fixture.inputs(SHAPE))
    names = [str(n) for n in g["names"]]
    assert sorted(got) == names
    with emulation():
        emu = train_step(train_modules(torch.float64, "cpu", "torch"), run_modules, images, side)
    worst, failed = 0.0, []
    for k in names:
        want, have = torch.from_numpy(g[k]).double(), stored(k, got[k])
        assert have.shape == want.shape, k
        if k.endswith("num_batches_tracked"):
            assert torch.equal(have, want)
            continue
        if k.startswith("grad/") and k.endswith(".0.bias"):
            assert not bool(have.any()), k
            continue
        unit = max(float(g[k + "/e32"]), float((stored(k, emu[k]) - stored(k, ref[k])).abs().max()))
        if got[k].dim() <= 1:
            unit = max(unit, 2.0 ** -24 * float(want.abs().max()))
        err = float((have - want).abs().max())
        worst = max(worst, err / unit)
        if err > 4 * unit:
            failed.append((k, err, unit))
    print(f"tf32 {impl} vs the reference's modules: largest ratio {worst:.2f}")
    assert not failed, failed


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
def test_one_training_step_end_to_end():
    """test_fpn_train_gpu.one_training_step's recipe with fpn_precision="tf32": the loss is finite, every FPN parameter gets a finite
    gradient, and every one of the FPN's 19 calls of the training op asked for the class."""
    from gfnet_amd.model.network import GFNet
    from gfnet_amd.reference_backbone import ReferenceBackbone
    from gfnet_amd.trainer import FusedAdamWStep, train_step as trainer_step

    images = torch.from_numpy(synth.lattice_uniform((4, 3, 448, 448), 78)).cuda()
    batch = {"im_A": images[:2], "im_B": images[2:]}

    def objective(out, _):
        loss = torch.zeros((), device="cuda")
        for scale in out.values():
            for d in scale.values():
                loss = loss + d["flow"].float().square().mean() + d["certainty"].float().square().mean()
        return loss

    calls, orig = [], ops.conv2d_bn_act_train
    ops.conv2d_bn_act_train = lambda *a, **k: (calls.append(k.get("precision")), orig(*a, **k))[1]
    try:
        torch.manual_seed(0)
        bb = ReferenceBackbone(tg.E2E_CONF, vit=StubVit(), decoder="hip", fpn="hip", fpn_train_impl="hip_fused", fpn_precision="tf32").cuda()
        fpn_fixture.fill({"encoder": bb.encoder, "decoder": bb.decoder, "merge_layer": bb.merge_layer})
        model = GFNet(tg.E2E_CONF, backbone=bb).cuda()
        model.train()
        stepper = FusedAdamWStep([p for p in model.parameters() if p.requires_grad], lr=1e-4, init_scale=1.0, zero_grads=False)
        res = trainer_step(batch, model, objective, stepper)
    finally:
        ops.conv2d_bn_act_train = orig
    for top in (bb.encoder, bb.decoder, bb.merge_layer):
        for k, p in top.named_parameters():
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
            assert k.endswith("0.bias") or float(p.grad.abs().max()) > 0.0, k
    assert calls == ["tf32"] * 19
    loss = float(res["train_loss"])
    print(f"one training step with fpn_precision='tf32': loss {loss:.9e}")
    assert np.isfinite(loss)


def test_backbone_hands_fp32_pyramids_to_the_matcher():
    from gfnet_amd.model.network import GFNet
    from gfnet_amd.reference_backbone import ReferenceBackbone

    torch.manual_seed(0)
    bb = ReferenceBackbone(CONF, vit=StubVit(), decoder="hip", fpn="hip", fpn_precision="tf32").cuda()
    fpn_fixture.fill({"encoder": bb.encoder, "decoder": bb.decoder, "merge_layer": bb.merge_layer})
    bb.train(False)
    images = torch.from_numpy(synth.lattice_uniform((2, 3, 448, 448), 77)).cuda()
    calls, orig = [], ops.conv2d_bn_act_tf32
    ops.conv2d_bn_act_tf32 = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
    try:
        with torch.no_grad():
            pa, pb = bb(images)
    finally:
        ops.conv2d_bn_act_tf32 = orig
    assert len(calls) == 19
    want = {"16": (1, 64, 32, 32), "8": (1, 64, 56, 56), "4": (1, 32, 112, 112), "2": (1, 16, 224, 224), "1": (1, 8, 448, 448)}
    for p in (pa, pb):
        assert {k: tuple(v.shape) for k, v in p.items()} == want
        assert all(v.dtype == torch.float32 and v.is_contiguous() and bool(torch.isfinite(v).all()) for v in p.values())
    model = GFNet(CONF, backbone=bb, upsample_preds=False).cuda()
    model.train(False)
    with torch.no_grad():
        warp, cert = model.match_batch(images[:1] * 0.5 + 0.5, images[1:] * 0.5 + 0.5)
    assert bool(torch.isfinite(warp).all()) and bool(torch.isfinite(cert).all())
