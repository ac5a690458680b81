"""The fp16 class of the native FPN (csrc/fpn_conv_half.hip, conv_precision="fp16") as far as it goes without a GPU: the class's
oracle and its derived per-value bound (shared with tests/test_fpn_half_gpu.py), a float64 emulation of the class that must stay
inside that bound, the packed weight layout, the C ABI's refusals and the wiring of conv_precision / fpn_precision.

The oracle is float64 on the ROUNDED operands: the fp16 maps, the fp16-rounded weight, the exact 2x interpolation of the coarse
fp16 values, the exact epilogue.  The bound on |result - oracle|, per output value, every term from the class's contract
(include/gfnet_hip.h) and none fitted to a measurement -- n = (C0 + C1) K^2 terms, S = sum |w| |x| over them, S0 its part over the
x0' channels, pre = conv * scale + shift, act = activation(pre), out = act + residual, L the activation's Lipschitz constant (1 for
none and leaky ReLU, 1.1 for swish: its slope peaks at 1.0998):

    L * ( n 2^-24 |scale| S                 fp32 accumulation of exact products, any order
        + 2^-11 |scale| S0   with up0 )      the interpolated operand is rounded to fp16
    + L 2^-24 |pre|                          the fmaf of scale and shift rounds once
    + 8 2^-24 |act|                          the activation in fp32: expf to 2 ulp, 1 + e, the division, the product; leaky ReLU one
    + 2^-24 |out|                            the residual add
    + 2^-11 |out|                            the one rounding at the store
"""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import synth
from gfnet_amd import _lib, ops
from gfnet_amd.model import fpn
from test_fpn_cpu import _child, build_modules
from test_fpn_gpu import LAYERS

# name: (K, stride, C0, C1, Cout, up0, residual, act) as in test_fpn_gpu.LAYERS.  Outside the FPN: Cout 24 (two 16-wide column tiles,
# the second half padding) and 40 (two 32-wide ones, 24 columns padding); Cin 3, 5 and 13 (the last channel group ends mid-unit),
# with x0 / x1 meeting inside one channel group
EDGE = {
    "edge_cin3_cout24": (3, 2, 3, 0, 24, False, None, "leaky_relu"), "edge_cin5_cout40": (1, 1, 5, 0, 40, False, None, "swish"),
    "edge_cin13_cout8": (5, 1, 5, 8, 8, False, "x1", "leaky_relu"), "edge_cin13_up_cout40": (3, 1, 5, 8, 40, True, None, "swish"),
    "edge_k7_cout40": (7, 1, 3, 0, 40, False, None, None),
}
CONFIGS = {**LAYERS, **EDGE}
E24, E11 = 2.0 ** -24, 2.0 ** -11


def activation(y, act):
    if act == "leaky_relu":
        return F.leaky_relu(y, 0.1)
    return y * torch.sigmoid(y) if act == "swish" else y


def oracle_and_bound(x0, x1, w, scale, shift, residual, stride, up0, act):
    """(float64 result on the rounded operands, the bound of the module docstring, that bound without its store term).  x0, x1,
    residual, w: fp16 tensors; scale, shift: fp32."""
    x0, x1, w, scale, shift, residual = (None if t is None else t.double() for t in (x0, x1, w, scale, shift, residual))
    if up0:
        x0 = F.interpolate(x0, scale_factor=2, mode="bilinear", align_corners=False)  # float64: exact to 2^-53
    x = x0 if x1 is None else torch.cat((x0, x1), dim=1)
    K, C0 = w.shape[-1], x0.shape[1]
    n = x.shape[1] * K * K
    sc = scale.view(1, -1, 1, 1)
    pre = F.conv2d(x, w, stride=stride, padding=K // 2) * sc + shift.view(1, -1, 1, 1)
    actv = activation(pre, act)
    out = actv if residual is None else actv + residual
    S = F.conv2d(x.abs(), w.abs(), stride=stride, padding=K // 2)
    S0 = F.conv2d(x0.abs(), w[:, :C0].abs(), stride=stride, padding=K // 2)
    L = 1.1 if act == "swish" else 1.0
    before_store = (L * (n * E24 * sc.abs() * S + (E11 * sc.abs() * S0 if up0 else 0.0)) + L * E24 * pre.abs() + 8 * E24 * actv.abs()
                    + E24 * out.abs())
    return out, before_store + E11 * out.abs(), before_store


@functools.lru_cache(maxsize=None)
def half_case(name, B, Ho, Wo, scale_by=1.0):
    """fp16 inputs of layer `name` for an output of (B, Cout, Ho, Wo) -- test_fpn_gpu.case's recipe, rounded -- with the fp32 weight,
    the oracle and the bound.  Computed once, never modified."""
    K, stride, C0, C1, Cout, up0, res, act = CONFIGS[name]
    seed = 300 + 11 * sorted(CONFIGS).index(name)
    H, W = (Ho, Wo) if stride == 1 else (2 * Ho - 1, 2 * Wo - 1)  # odd inputs under stride 2
    x0 = torch.from_numpy(synth.lattice_normalish((B, C0, H // 2, W // 2) if up0 else (B, C0, H, W), seed)).half()
    x1 = torch.from_numpy(synth.lattice_normalish((B, C1, H, W), seed + 1)).half() if C1 else None
    w = torch.from_numpy(synth.lattice_normalish((Cout, C0 + C1, K, K), seed + 2) * np.float32(0.87 / np.sqrt((C0 + C1) * K * K)))
    scale = torch.from_numpy((np.float32(0.9) + np.float32(0.5) * synth.lattice_uniform((Cout,), seed + 3)) * np.float32(scale_by))
    shift = torch.from_numpy(np.float32(0.4) * synth.lattice_uniform((Cout,), seed + 4))
    residual = {"x0": x0, "x1": x1, None: None}[res]
    ref, bound, before_store = oracle_and_bound(x0, x1, w.half(), scale, shift, residual, stride, up0, act)
    assert tuple(ref.shape) == (B, Cout, Ho, Wo), (name, tuple(ref.shape))
    return (x0, x1, w, scale, shift, residual), ref, bound, before_store


def emulate(x0, x1, w, scale, shift, residual, stride, up0, act):
    """The class in float64: operands and result rounded to fp16 (the interpolated operand from an fp32 interpolation, as the
    kernel forms it), sums and epilogue exact."""
    if up0:
        x0 = F.interpolate(x0.float(), scale_factor=2, mode="bilinear", align_corners=False).half()
    x = x0 if x1 is None else torch.cat((x0, x1), dim=1)
    y = F.conv2d(x.double(), w.half().double(), stride=stride, padding=w.shape[-1] // 2)
    y = activation(y * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1), act)
    return (y if residual is None else y + residual.double()).half()


def shape_of(name):
    up0 = CONFIGS[name][5]
    return (2, 14, 22) if up0 else (2, 13, 19)


@pytest.mark.parametrize("name", list(LAYERS))
def test_emulation_of_the_class_stays_inside_the_derived_bound(name):
    """All 19 layers at B = 2 with a 13 x 19 output (up0: 14 x 22 from 7 x 11; stride 2: from 25 x 37): the roundings the class makes
    by contract -- operands, the interpolated operand, the result -- fit the bound with exact sums, so a failure on the GPU is the
    kernel's and not the bound's."""
    args, ref, bound, _ = half_case(name, *shape_of(name))
    K, stride, _, _, _, up0, _, act = CONFIGS[name]
    got = emulate(*args, stride, up0, act)
    assert got.dtype == torch.float16 and got.shape == ref.shape
    ratio = float(((got.double() - ref).abs() / bound).max())
    print(f"{name}: emulation worst error / bound {ratio:.3f}")
    assert float(bound.min()) > 0 and ratio <= 1.0, (name, ratio)


@pytest.mark.parametrize("Cout,Cin,K", [(8, 3, 7), (8, 5, 3), (40, 5, 1), (40, 13, 3), (16, 24, 5), (64, 128, 3)])
def test_packed_layout_against_a_literal_loop(Cout, Cin, K):
    w = torch.from_numpy(synth.lattice_normalish((Cout, Cin, K, K), 40 + Cout + Cin + K))
    packed = ops.conv2d_pack_half(w)
    CG, UP, CP = (Cin + 7) // 8, (K * K + 3) // 4 * 4, (Cout + 15) // 16 * 16 if Cout < 32 else (Cout + 31) // 32 * 32
    assert packed.dtype == torch.float16 and packed.is_contiguous() and tuple(packed.shape) == (CP, CG, UP, 8)
    want = np.zeros((CP, CG, UP, 8), dtype=np.float16)
    wh = w.numpy().astype(np.float16)  # numpy rounds to nearest even as well
    for co in range(Cout):
        for ci in range(Cin):
            for ky in range(K):
                for kx in range(K):
                    want[co, ci // 8, ky * K + kx, ci % 8] = wh[co, ci, ky, kx]
    np.testing.assert_array_equal(packed.numpy(), want)
    assert np.count_nonzero(want) == np.count_nonzero(wh)  # everything else is padding, and zero
    with pytest.raises(ValueError, match="Cout,Cin,K,K"):
        ops.conv2d_pack_half(torch.zeros(8, 3, 3, 5))


def test_abi_declares_the_entry_point_and_refuses_bad_arguments_before_any_launch():
    """Argument errors return before any HIP call, so this runs without a GPU; the dummy pointers are never read."""
    vp, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    name = "gfn_conv2d_bn_act_half_fwd"
    assert _lib.PROTOTYPES[name] == (i, [vp, i, i, vp, i, vp, vp, vp, vp, vp, i, i, i, i, i, i, i, f, vp])
    assert name in _lib.STATUS_FUNCS and name in _lib.exported_symbols()
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p(ctypes.addressof(buf))

    def call(x0=p, C0=3, up0=0, x1=None, C1=0, weight=p, scale=p, shift=p, residual=None, out=p, B=1, H=8, W=8, Cout=8, K=3, stride=1,
             act=1):
        return L.gfn_conv2d_bn_act_half_fwd(x0, C0, up0, x1, C1, weight, scale, shift, residual, out, B, H, W, Cout, K, stride, act, 0.1,
                                            None)

    bad = [(dict(x0=None), "null"), (dict(weight=None), "null"), (dict(scale=None), "null"), (dict(shift=None), "null"),
           (dict(out=None), "null"), (dict(C1=4), "null"),                    # x1 missing although C1 > 0
           (dict(Cout=12), "multiple of 8"), (dict(Cout=3), "multiple of 8"),  # no general kernel in this class
           (dict(K=4), "kernel size 4"), (dict(K=2), "kernel size 2"), (dict(K=9), "kernel size 9"),
           (dict(stride=3), "stride 3"), (dict(stride=0), "stride 0"), (dict(act=3), "act 3"), (dict(act=-1), "act -1"),
           (dict(up0=1, H=7), "even"), (dict(up0=1, W=9), "even"),
           (dict(C0=1, H=32768, W=32768), "2^31"),                           # x0 of exactly 2^31 bytes per image in fp16
           (dict(C0=1, Cout=256, H=2048, W=2048), "2^31"),                   # the output map
           (dict(C1=64, x1=p, H=4096, W=4096), "2^31"),                      # x1
           (dict(Cout=0), "Cout"), (dict(Cout=264), "Cout"), (dict(C0=0), "C0"), (dict(H=0), "H=0")]
    for kwargs, text in bad:
        assert call(**kwargs) == _lib.ERR_INVALID_ARG == -1, kwargs
        assert text in L.gfn_last_error().decode(), (kwargs, L.gfn_last_error().decode())
    assert call(B=0) == _lib.OK == 0
    assert call(B=0, x0=None, out=None) == 0  # an empty batch reads nothing
    with pytest.raises(_lib.GfnError, match=name + " failed"):
        _lib.checked().gfn_conv2d_bn_act_half_fwd(p, 3, 0, None, 0, p, p, p, None, p, 1, 8, 8, 12, 3, 1, 0, 0.1, None)


def test_op_refuses_cpu_tensors_and_wrong_arguments():
    x, w, s = torch.zeros(1, 3, 8, 8).half(), torch.zeros(8, 3, 3, 3), torch.zeros(8)
    with pytest.raises(_lib.GfnError, match="no CPU path"):
        ops.conv2d_bn_act_half(x, w, s, s)
    with pytest.raises(ValueError, match="act"):
        ops.conv2d_bn_act_half(x, w, s, s, act="relu")


def test_conv_precision_is_validated_and_cpu_tensors_keep_the_fp32_torch_path():
    import fpn_fixture

    chs = fpn_fixture.FEAT_CHS
    assert fpn.CONV_PRECISIONS == ("fp32", "fp16")
    for make in (lambda **kw: fpn.FPNEncoder(chs, **kw), lambda **kw: fpn.FPNDecoder_concat(chs, **kw), lambda **kw: fpn.merge_layer(64, **kw),
                 lambda **kw: fpn.Conv2d(3, 8, 3, padding=1, **kw)):
        assert make().conv_precision == "fp32" and make(conv_precision="fp16").conv_precision == "fp16"  # fp32 stays the default
        with pytest.raises(ValueError, match="conv_precision"):
            make(conv_precision="bf16")
    enc = fpn.FPNEncoder(chs, conv_precision="fp16")
    assert all(m.conv_precision == "fp16" for m in enc.modules() if isinstance(m, fpn.Conv2d))
    # on the CPU "fp16" is the fp32 torch path, bit for bit what "fp32" gives
    mods, _ = build_modules()
    images, side = fpn_fixture.inputs("b")
    with torch.no_grad():
        want = mods["decoder"](*mods["encoder"](images)[:3], mods["merge_layer"](mods["encoder"](images)[3], side))
        for m in mods.values():
            m.conv_precision = "fp16"
        c0, c1, c2, c3 = mods["encoder"](images)
        got = mods["decoder"](c0, c1, c2, mods["merge_layer"](c3, side))
    assert all(g.dtype == torch.float32 and torch.equal(g, v) for g, v in zip(got, want))
    mods["encoder"].conv_precision = "fp8"  # a value set after construction is checked where it is used
    with pytest.raises(ValueError, match="conv_precision"):
        mods["encoder"](images)


class StubVit(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.embed = torch.nn.Conv2d(3, 32, 14, stride=14)

    def forward_features(self, x):
        return {"x_norm_patchtokens": self.embed(x).flatten(2).transpose(1, 2)}


CONF = {"dino_cfg": {"d_model": 32,
                     "decoder_cfg": {"num_cross_attn": 2, "init_values": 1.0, "prev_values": 0.5, "nhead": 8, "attention_type": "FLASH2",
                                     "ffn_type": "ffn", "softmax_scale": "entropy_invariance", "train_avg_length": 1024,
                                     "self_cross_types": None, "post_norm": False, "pre_norm_query": True, "no_combine_norm": False}},
        "encoder_cfg": {"feat_chs": [64, 32, 16, 8]},
        "matcher": {"num_grid": [32, 32, 64, 128, 256], "radius": [7, 6, 4, 2, 0], "displacement_dim": [64, 64, 32, 16, 8],
                    "num_itr": [1, 1, 1, 1, 1]}}


def test_fpn_precision_of_the_backbone():
    from gfnet_amd.reference_backbone import ReferenceBackbone, reference_backbone

    for make in (ReferenceBackbone, reference_backbone):
        with pytest.raises(ValueError, match="fpn_precision"):
            make(CONF, vit=StubVit(), decoder="hip", fpn="hip", fpn_precision="bf16")
        with pytest.raises(ValueError, match="fpn_precision"):  # the checkout's modules have no such class
            make(CONF, vit=StubVit(), decoder="hip", fpn="checkout", fpn_precision="fp16")
    bb = ReferenceBackbone(CONF, vit=StubVit(), decoder="hip", fpn="hip", fpn_precision="fp16")
    assert bb.encoder.conv_precision == bb.decoder.conv_precision == bb.merge_layer.conv_precision == "fp16"
    assert bb.encoder.conv00.conv_precision == "fp16" and bb.encoder.conv_impl == "hip"
    bb = ReferenceBackbone(CONF, vit=StubVit(), decoder="hip", fpn="hip")
    assert bb.fpn_precision == bb.encoder.conv_precision == bb.decoder.conv_precision == bb.merge_layer.conv_precision == "fp32"


def test_wiring_environment_switch_on_the_reference_constructor_path(tmp_path):
    env = {"GFNET_COMPAT_BACKBONE": "reference", "GFNET_COMPAT_DECODER": "hip", "GFNET_COMPAT_FPN": "hip"}
    _child("""
    import gfnet_amd.reference_backbone as rb
    rb._build_vit = lambda w: vit
    from model.network import GFNet
    bb = GFNet(conf=conf).backbone
    assert bb.fpn_precision == bb.encoder.conv_precision == bb.decoder.conv_precision == bb.merge_layer.conv_precision == "fp16"
    print("ok")
    """, tmp_path, env=dict(env, GFNET_COMPAT_FPN_PRECISION="fp16"))
    _child("""
    import gfnet_amd.reference_backbone as rb
    rb._build_vit = lambda w: vit
    from model.network import GFNet
    bb = GFNet(conf=conf).backbone
    assert bb.fpn_precision == bb.encoder.conv_precision == "fp32"  # unset: fp32, as before
    try:
        os.environ["GFNET_COMPAT_FPN_PRECISION"] = "fp16"
        os.environ["GFNET_COMPAT_FPN"] = ""
        GFNet(conf=conf)
    except ValueError as e:
        assert "fpn_precision" in str(e)
    else:
        raise AssertionError("fp16 with the checkout's FPN must be refused")
    print("ok")
    """, tmp_path, env=dict(env, GFNET_COMPAT_FPN_PRECISION=""))
