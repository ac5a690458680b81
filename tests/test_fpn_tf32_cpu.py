"""The TF32 class of the native FPN (csrc/fpn_conv_tf32.hip, conv_precision / fpn_precision "tf32", precision="tf32" of the training
op) as far as it goes without a GPU: the class's oracle in torch and its derived per-value forward bound (shared with
tests/test_fpn_tf32_gpu.py), the properties of the split, and the wiring.

The class (include/gfnet_hip.h): an fp32 operand v is split into hi = bf16(v) to nearest even and lo = bf16(v - hi), lo = 0 where
hi is not finite; a product a b is a_hi b_hi + a_hi b_lo + a_lo b_hi, each exact in fp32, summed in fp32; a_lo b_lo is dropped.
With a~ = a_hi + a_lo that is a~ b~ - a_lo b_lo, so for any bilinear `op` (the convolution, and both of its gradients)

    P(a, b) = op64(a~, b~) - op64(a_lo, b_lo)

is the class's result with exact sums: the ORACLE.  Properties checked here on the tests' own data: (a) hi + lo is an fp32 number,
(b) |v - (hi + lo)| <= 2^-16 |v|, (c) |P - exact| <= 3 2^-16 op64(|a|, |b|).

The forward bound on |result - oracle| per output value, derived as tests/test_fpn_half_cpu.py derives the fp16 class's with two
changes -- no element rounding at the store (the maps are fp32), and three products per term in the fp32 accumulation.  n = (C0 +
C1) K^2 terms, S = sum |w| |x| over them, S0 its part over the x0' channels, pre = conv * scale + shift, act = activation(pre),
out = act + residual, L the activation's Lipschitz constant (1, or 1.1 for swish):

    L * ( 3 n 2^-24 |scale| S                          fp32 accumulation of 3 n exact products, any order
        + (2^-16 + 8 2^-24) |scale| S0   with up0 )     the interpolated operand is rounded into the class: the oracle takes the exact
                                                         2x interpolation as a~ (and the split of its fp32 rounding for a_lo), the
                                                         kernel interpolates in fp32 (five roundings) and splits what it got
    + L 2^-24 |pre|                                     the fmaf of scale and shift rounds once
    + 8 2^-24 |act|                                     the activation in fp32
    + 2^-24 |out|                                       the residual add
"""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fpn_fixture
import synth
from gfnet_amd import _lib, ops
from gfnet_amd.model import fpn
from test_fpn_cpu import build_modules, run_modules
from test_fpn_half_cpu import CONF, CONFIGS, StubVit, activation, shape_of
from test_fpn_gpu import LAYERS

E24, E16 = 2.0 ** -24, 2.0 ** -16


def split(v):
    """(hi, lo) of an fp32 tensor, as fp32 tensors that hold bf16 values."""
    assert v.dtype == torch.float32
    hi = v.to(torch.bfloat16).float()  # to nearest even
    lo = torch.where(torch.isfinite(hi), v - hi, torch.zeros_like(v)).to(torch.bfloat16).float()
    return hi, lo


def tilde(v):
    """(a~, a_lo) in float64."""
    hi, lo = split(v)
    return hi.double() + lo.double(), lo.double()


def P(op, a, b):
    """The class's product for a bilinear op on float64 tensors, a and b fp32: op(a~, b~) - op(a_lo, b_lo)."""
    (at, al), (bt, bl) = tilde(a), tilde(b)
    return op(at, bt) - op(al, bl)


def conv_op(stride, K):
    return lambda x, w: F.conv2d(x, w, stride=stride, padding=K // 2)


def oracle_and_bound(x0, x1, w, scale, shift, residual, stride, up0, act):
    """(the class's oracle in float64, the bound of the module docstring, exact float64 result, 3 2^-16 |scale| S).  fp32 tensors."""
    K, C0 = w.shape[-1], x0.shape[1]
    op = conv_op(stride, K)
    d = lambda t: None if t is None else t.double()
    if up0:
        x0e = F.interpolate(x0.double(), scale_factor=2, mode="bilinear", align_corners=False)  # float64: exact to 2^-53
        x0t, x0l = x0e, split(x0e.float())[1].double()
    else:
        x0e = x0.double()
        x0t, x0l = tilde(x0)
    if x1 is None:
        xe, xt, xl = x0e, x0t, x0l
    else:
        x1t, x1l = tilde(x1)
        xe, xt, xl = torch.cat((x0e, x1.double()), 1), torch.cat((x0t, x1t), 1), torch.cat((x0l, x1l), 1)
    wt, wl = tilde(w)
    n = xe.shape[1] * K * K
    sc, sh = scale.double().view(1, -1, 1, 1), shift.double().view(1, -1, 1, 1)
    conv = op(xt, wt) - op(xl, wl)
    pre = conv * sc + sh
    actv = activation(pre, act)
    out = actv if residual is None else actv + d(residual)
    S = op(xe.abs(), w.double().abs())
    S0 = op(x0e.abs(), w.double()[:, :C0].abs())
    L = 1.1 if act == "swish" else 1.0
    bound = (L * (3 * n * E24 * sc.abs() * S + ((E16 + 8 * E24) * sc.abs() * S0 if up0 else 0.0)) + L * E24 * pre.abs() + 8 * E24 * actv.abs()
             + E24 * out.abs())
    exact = activation(op(xe, w.double()) * sc + sh, act)
    exact = exact if residual is None else exact + d(residual)
    return out, bound, exact, 3 * E16 * sc.abs() * S


@functools.lru_cache(maxsize=None)
def tf32_case(name, B, Ho, Wo):
    """fp32 inputs of layer `name` for an output of (B, Cout, Ho, Wo) -- test_fpn_half_cpu.half_case's recipe and seeds, not rounded --
    with the oracle and the bound.  Computed once, never modified."""
    K, stride, C0, C1, Cout, up0, res, act = CONFIGS[name]
    seed = 300 + 11 * sorted(CONFIGS).index(name)
    H, W = (Ho, Wo) if stride == 1 else (2 * Ho - 1, 2 * Wo - 1)  # odd inputs under stride 2
    x0 = torch.from_numpy(synth.lattice_normalish((B, C0, H // 2, W // 2) if up0 else (B, C0, H, W), seed))
    x1 = torch.from_numpy(synth.lattice_normalish((B, C1, H, W), seed + 1)) if C1 else None
    w = torch.from_numpy(synth.lattice_normalish((Cout, C0 + C1, K, K), seed + 2) * np.float32(0.87 / np.sqrt((C0 + C1) * K * K)))
    scale = torch.from_numpy(np.float32(0.9) + np.float32(0.5) * synth.lattice_uniform((Cout,), seed + 3))
    shift = torch.from_numpy(np.float32(0.4) * synth.lattice_uniform((Cout,), seed + 4))
    residual = {"x0": x0, "x1": x1, None: None}[res]
    ref, bound, exact, class_bound = oracle_and_bound(x0, x1, w, scale, shift, residual, stride, up0, act)
    assert tuple(ref.shape) == (B, Cout, Ho, Wo), (name, tuple(ref.shape))
    return (x0, x1, w, scale, shift, residual), ref, bound, exact, class_bound


def emulate_fp32(x0, x1, w, scale, shift, residual, stride, up0, act):
    """The class evaluated in fp32 by torch: three F.conv2d calls on the split operands, summed, and the epilogue in fp32."""
    if up0:
        x0 = F.interpolate(x0, scale_factor=2, mode="bilinear", align_corners=False)
    x = x0 if x1 is None else torch.cat((x0, x1), dim=1)
    (xh, xl), (wh, wl) = split(x), split(w)
    op = conv_op(stride, w.shape[-1])
    y = op(xh, wh) + op(xh, wl) + op(xl, wh)
    y = activation(y * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1), act)
    return y if residual is None else y + residual


def test_split_is_two_bf16_halves_of_16_significant_bits_and_keeps_an_inf():
    """(a), (b) and the non-finite guard, on every operand the forward tests use and on hostile exponents."""
    tensors = []
    for name in LAYERS:
        args = tf32_case(name, *shape_of(name))[0]
        tensors += [t for t in args[:3] if t is not None]
    tensors.append(torch.from_numpy(synth.lattice_normalish((4096,), 5)) * torch.tensor([1e-30, 1e-3, 1.0, 3e38 / 8]).repeat(1024))
    for v in tensors:
        hi, lo = split(v)
        assert torch.equal(hi.to(torch.bfloat16).float(), hi) and torch.equal(lo.to(torch.bfloat16).float(), lo)  # bf16 values
        s = hi.double() + lo.double()
        assert torch.equal(s.float().double(), s)                                    # (a) hi + lo is an fp32 number
        assert bool(((v.double() - s).abs() <= E16 * v.double().abs()).all())         # (b)
        assert bool((lo.abs() <= 2.0 ** -8 * hi.abs()).all())
    assert float(max(((v.double() - sum(split(v)).double()).abs() / v.double().abs().clamp_min(1e-300)).max() for v in tensors)) > 2.0 ** -19
    big = torch.tensor([float("inf"), -float("inf"), 3.4e38, -3.4e38, float("nan"), 1.0])
    hi, lo = split(big)  # 3.4e38 rounds to inf in bf16: lo must be 0 there, not -inf
    assert torch.equal(hi[:4], torch.tensor([float("inf"), -float("inf"), float("inf"), -float("inf")]))
    assert not bool(lo.any()) or float(lo[5]) == 0.0
    assert torch.equal(lo[:5], torch.zeros(5)) and bool(torch.isnan(hi[4]))
    assert torch.equal((hi + lo)[:4], hi[:4])  # an inf stays an inf


@pytest.mark.parametrize("name", list(LAYERS))
def test_class_product_is_within_three_roundings_of_exact_and_fp32_evaluation_within_the_forward_bound(name):
    """(c): |P - exact| <= 3 2^-16 conv64(|a|, |b|) on the raw convolution of every layer (the up0 layers on the doubled map), and
    (d): the class evaluated in fp32 by torch stays inside the forward bound the GPU is held to, so a failure there is the kernel's."""
    K, stride, C0, C1, Cout, up0, res, act = CONFIGS[name]
    args, ref, bound, exact, class_bound = tf32_case(name, *shape_of(name))
    x0, x1, w = args[:3]
    if up0:
        x0 = F.interpolate(x0, scale_factor=2, mode="bilinear", align_corners=False)
    x = x0 if x1 is None else torch.cat((x0, x1), 1)
    op = conv_op(stride, K)
    p, ex, S = P(op, x, w), op(x.double(), w.double()), op(x.double().abs(), w.double().abs())
    ratio_c = float(((p - ex).abs() / (3 * E16 * S)).max())
    got = emulate_fp32(*args, stride, up0, act)
    assert got.dtype == torch.float32 and got.shape == ref.shape
    ratio_d = float(((got.double() - ref).abs() / bound).max())
    print(f"{name}: |P - exact| / (3 2^-16 S) {ratio_c:.3f} (= {3 * ratio_c:.2f} 2^-16); fp32 evaluation worst error / bound {ratio_d:.3f}")
    assert 0.0 < ratio_c <= 1.0, (name, ratio_c)
    assert float(bound.min()) > 0 and ratio_d <= 1.0, (name, ratio_d)


def test_class_sits_between_fp32_and_tf32_operand_rounding():
    """The issue's table on conv20 (32 -> 32, 3 x 3): largest error against float64 of fp32, of the class and of TF32's operand
    rounding (10 explicit mantissa bits, to nearest even)."""
    args, ref, bound, exact, _ = tf32_case("conv20", *shape_of("conv20"))
    x, _, w = args[:3]
    op = conv_op(1, 3)
    ex = op(x.double(), w.double())

    def tf32_round(v):
        i = v.view(torch.int32)
        return ((i + 0xFFF + ((i >> 13) & 1)) & ~0x1FFF).view(torch.float32)

    e_fp32 = float((op(x, w).double() - ex).abs().max())
    e_class = float((P(op, x, w) - ex).abs().max())
    e_tf32 = float((op(tf32_round(x).double(), tf32_round(w).double()) - ex).abs().max())
    print(f"conv20: fp32 {e_fp32:.2e}  class {e_class:.2e}  tf32 operands {e_tf32:.2e}")
    assert e_fp32 < e_class < e_tf32 / 20


def test_abi_declares_the_entry_points_and_refuses_bad_arguments_before_any_launch():
    vp, i, f, d, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_int64
    P_ = _lib.PROTOTYPES
    assert P_["gfn_conv2d_bn_act_tf32_fwd"] == (i, [vp, i, i, vp, i, vp, vp, vp, vp, vp, i, i, i, i, i, i, i, f, vp, i64, vp])
    assert P_["gfn_conv2d_bn_act_tf32_ws_bytes"] == (i64, [i] * 4)
    assert P_["gfn_conv2d_bn_act_train_tf32_ws_bytes"] == P_["gfn_conv2d_up_bn_act_train_ws_bytes"] == (i64, [i] * 10)
    assert P_["gfn_conv2d_bn_act_train_tf32_fwd"] == P_["gfn_conv2d_up_bn_act_train_fwd"]
    assert P_["gfn_conv2d_bn_act_train_tf32_bwd"] == P_["gfn_conv2d_up_bn_act_train_bwd"]
    names = {"gfn_conv2d_bn_act_tf32_fwd", "gfn_conv2d_bn_act_train_tf32_fwd", "gfn_conv2d_bn_act_train_tf32_bwd"}
    sizes = {"gfn_conv2d_bn_act_tf32_ws_bytes", "gfn_conv2d_bn_act_train_tf32_ws_bytes"}
    assert names <= _lib.STATUS_FUNCS and not (sizes & _lib.STATUS_FUNCS) and (names | sizes) <= set(_lib.exported_symbols())
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p(ctypes.addressof(buf))

    def call(x0=p, C0=3, up0=0, x1=None, C1=0, weight=p, scale=p, shift=p, residual=None, out=p, B=1, H=8, W=8, Cout=8, K=3, stride=1,
             act=1, ws=p, ws_bytes=1 << 30):
        return L.gfn_conv2d_bn_act_tf32_fwd(x0, C0, up0, x1, C1, weight, scale, shift, residual, out, B, H, W, Cout, K, stride, act, 0.1,
                                            ws, ws_bytes, None)

    bad = [(dict(x0=None), "null"), (dict(weight=None), "null"), (dict(out=None), "null"), (dict(C1=4), "null"),
           (dict(Cout=12), "multiple of 8"), (dict(Cout=3), "multiple of 8"), (dict(K=4), "kernel size 4"), (dict(stride=3), "stride 3"),
           (dict(act=3), "act 3"), (dict(up0=1, H=7), "even"), (dict(C0=1, H=32768, W=16384), "2^31"), (dict(Cout=264), "Cout"),
           (dict(C0=0), "C0"), (dict(H=0), "H=0")]
    for kwargs, text in bad:
        assert call(**kwargs) == _lib.ERR_INVALID_ARG, kwargs
        assert text in L.gfn_last_error().decode(), (kwargs, L.gfn_last_error().decode())
    assert call(ws=None) == _lib.ERR_SCRATCH and call(ws_bytes=64) == _lib.ERR_SCRATCH and "workspace" in L.gfn_last_error().decode()
    assert call(B=0) == _lib.OK and call(B=0, x0=None, out=None, ws=None) == 0
    # the packed weight: hi and lo, (CoutP, CG, UP, 8) bf16 each, in conv2d_pack_half's shape
    for Cout, Cin, K in ((8, 3, 7), (40, 13, 3), (64, 128, 3), (16, 24, 5)):
        assert L.gfn_conv2d_bn_act_tf32_ws_bytes(Cin, 0, Cout, K) == 2 * ops.conv2d_pack_half(torch.zeros(Cout, Cin, K, K)).numel() * 2
    assert L.gfn_conv2d_bn_act_tf32_ws_bytes(3, 0, 12, 3) == 0 and L.gfn_conv2d_bn_act_tf32_ws_bytes(3, 0, 8, 4) == 0
    # training: the fp32 entries' workspace plus the largest packed weight of the launches; the same refusals, the same messages
    for up0 in (0, 1):
        for backward in (0, 1):
            a = (16, up0, 8, 2, 24, 40, 32, 3, 1, backward)
            extra = L.gfn_conv2d_bn_act_train_tf32_ws_bytes(*a) - L.gfn_conv2d_up_bn_act_train_ws_bytes(*a)
            assert extra == L.gfn_conv2d_bn_act_tf32_ws_bytes(16, 8, 32, 3) > 0
    assert L.gfn_conv2d_bn_act_train_tf32_ws_bytes(16, 1, 8, 2, 24, 40, 32, 3, 2, 1) == 0  # up0 under stride 2
    args = [p, 3, 0, None, 0] + [p] * 11 + [1, 1, 1, 8, 3, 1, 0, 0.1, 0.1, 1e-5, p, 1 << 30, None]
    assert L.gfn_conv2d_bn_act_train_tf32_fwd(*args) == _lib.ERR_INVALID_ARG
    assert "gfn_conv2d_bn_act_train_tf32_fwd: batch statistics need more than one value" in L.gfn_last_error().decode()
    args[16:19] = [2, 7, 8]
    args[2] = 1
    assert L.gfn_conv2d_bn_act_train_tf32_fwd(*args) == _lib.ERR_INVALID_ARG and "even" in L.gfn_last_error().decode()


def test_ops_refuse_cpu_tensors_and_unknown_precisions():
    x, w, s = torch.zeros(1, 3, 8, 8), torch.zeros(8, 3, 3, 3), torch.ones(8)
    with pytest.raises(_lib.GfnError, match="no CPU path"):
        ops.conv2d_bn_act_tf32(x, w, s, s)
    with pytest.raises(ValueError, match="act"):
        ops.conv2d_bn_act_tf32(x, w, s, s, act="relu")
    assert ops.CONV_TRAIN_PRECISIONS == ("fp32", "tf32")
    for bad in ("fp16", "bf16", None):
        with pytest.raises(ValueError, match="precision"):
            ops.conv2d_bn_act_train(x, w, None, s, s, s.clone(), s.clone(), None, 0.1, 1e-5, precision=bad)
        with pytest.raises(ValueError, match="precision"):
            ops.conv2d_bn_act_train_fwd(x, w, None, s, s, s.clone(), s.clone(), 0.1, 1e-5, precision=bad)
        with pytest.raises(ValueError, match="precision"):
            ops.conv2d_bn_act_train_bwd(torch.zeros(1, 8, 8, 8), x, w, s, s, torch.zeros(1, 8, 8, 8), s, s, precision=bad)
    with pytest.raises(_lib.GfnError, match="no CPU path"):
        ops.conv2d_bn_act_train(x, w, None, s, s, s.clone(), s.clone(), None, 0.1, 1e-5, precision="tf32")


def test_conv_precision_tf32_is_accepted_and_cpu_tensors_keep_the_fp32_torch_path():
    chs = fpn_fixture.FEAT_CHS
    assert fpn.ALL_CONV_PRECISIONS == ("fp32", "fp16", "tf32") and fpn.CONV_PRECISIONS == ("fp32", "fp16")
    for make in (lambda **kw: fpn.FPNEncoder(chs, **kw), lambda **kw: fpn.FPNDecoder_concat(chs, **kw), lambda **kw: fpn.merge_layer(64, **kw),
                 lambda **kw: fpn.Conv2d(3, 8, 3, padding=1, **kw)):
        assert make().conv_precision == "fp32" and make(conv_precision="tf32").conv_precision == "tf32"  # fp32 stays the default
    enc = fpn.FPNEncoder(chs, conv_precision="tf32")
    assert all(m.conv_precision == "tf32" for m in enc.modules() if isinstance(m, fpn.Conv2d))
    # on the CPU "tf32" is the fp32 torch path, bit for bit what "fp32" gives, in eval() and in train()
    for training in (False, True):
        outs = []
        for precision in ("fp32", "tf32"):
            mods, _ = build_modules()
            for m in mods.values():
                m.conv_precision, m.train_conv_impl = precision, "hip_fused"
                m.train(training)
            with torch.no_grad():
                outs.append(run_modules(mods, *fpn_fixture.inputs("b")))
        assert all(outs[1][k].dtype == torch.float32 and torch.equal(outs[0][k], outs[1][k]) for k in outs[0])


@pytest.mark.parametrize("precision", ["fp32", "tf32"])
def test_which_op_each_mode_calls(monkeypatch, precision):
    """With every tensor claiming to be on the GPU (there is none here) and the ops replaced by recorders: eval() runs conv2d_bn_act_tf32 for
    every layer under "tf32" and conv2d_bn_act under "fp32"; train() passes precision to conv2d_bn_act_train under "hip" and
    "hip_fused"; a layer whose Cout is no multiple of 8 runs the fp32 op in eval()."""
    calls = []

    def fake(kind):
        def f(x0, weight, *a, x1=None, up0=False, stride=1, **k):
            calls.append((kind, k.get("precision"), bool(up0)))
            H, W = (2 * x0.shape[2], 2 * x0.shape[3]) if up0 else x0.shape[2:]
            return torch.zeros(x0.shape[0], weight.shape[0], (H + stride - 1) // stride, (W + stride - 1) // stride)
        return f

    for kind in ("conv2d_bn_act", "conv2d_bn_act_tf32", "conv2d_bn_act_half", "conv2d_bn_act_train"):
        monkeypatch.setattr(ops, kind, fake(kind))
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True), raising=False)  # the modules ask nothing else of a device
    mods, _ = build_modules()
    images, side = fpn_fixture.inputs("b")
    for m in mods.values():
        m.conv_precision = precision
    with torch.no_grad():
        run_modules(mods, images, side)
        assert calls == [("conv2d_bn_act_tf32" if precision == "tf32" else "conv2d_bn_act", None, up) for _, _, up in calls] and len(calls) == 19
        assert sum(up for _, _, up in calls) == 3
        for impl, ups in (("hip", 0), ("hip_fused", 3)):
            del calls[:]
            for m in mods.values():
                m.train_conv_impl = impl
                m.train(True)
            run_modules(mods, images, side)
            assert calls == [("conv2d_bn_act_train", precision, up) for _, _, up in calls] and len(calls) == 19
            assert sum(up for _, _, up in calls) == ups
        del calls[:]
        odd = fpn.Conv2d(3, 12, 3, padding=1, conv_precision=precision).train(False)
        odd(images)
        assert calls == [("conv2d_bn_act", None, False)]  # Cout 12: the fp32 op, silently
        odd.train_conv_impl = "hip"
        odd.train(True)
        odd(images)
        assert calls[1] == ("conv2d_bn_act_train", precision, False)  # (the library routes its convolutions to the fp32 kernels)
        del calls[:]
        for m in mods.values():
            m.conv_precision = "fp16"  # "fp16" still does not touch train()
        run_modules(mods, images, side)
        assert calls == [("conv2d_bn_act_train", "fp32", up) for _, _, up in calls] and len(calls) == 19


def test_fpn_precision_tf32_of_the_backbone():
    from gfnet_amd.reference_backbone import ReferenceBackbone, reference_backbone

    for make in (ReferenceBackbone, reference_backbone):
        with pytest.raises(ValueError, match="fpn_precision"):  # the checkout's modules have no such class
            make(CONF, vit=StubVit(), decoder="hip", fpn="checkout", fpn_precision="tf32")
    bb = ReferenceBackbone(CONF, vit=StubVit(), decoder="hip", fpn="hip", fpn_precision="tf32", fpn_train_impl="hip_fused")
    assert bb.fpn_precision == bb.encoder.conv_precision == bb.decoder.conv_precision == bb.merge_layer.conv_precision == "tf32"
    assert bb.encoder.conv00.conv_precision == "tf32" and bb.encoder.conv_impl == "hip" and bb.decoder.train_conv_impl == "hip_fused"
