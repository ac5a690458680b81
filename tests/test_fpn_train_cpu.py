"""The FPN's training mode as far as it goes without a GPU: the module's torch training path against the reference's own modules in
train() (tests/golden/g17_fpn_train.npz, made by tests/golden/make_golden_fpn_train.py), the C ABI's three entry points are bound and
refuse bad arguments before any launch, the train_conv_impl switch of the modules and the fpn_train_impl keyword of the backbone, and
the ops' refusal of CPU tensors."""
import ctypes

import pytest
import torch

import fpn_fixture
from gfnet_amd import _lib
from gfnet_amd.model import fpn


def test_abi_declares_the_three_entry_points():
    vp, i, f, d, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_int64
    assert _lib.PROTOTYPES["gfn_conv2d_bn_act_train_ws_bytes"] == (i64, [i] * 9)
    assert _lib.PROTOTYPES["gfn_conv2d_bn_act_train_fwd"] == (i, [vp, i, vp, i] + [vp] * 11 + [i] * 7 + [f, d, d, vp, i64, vp])
    assert _lib.PROTOTYPES["gfn_conv2d_bn_act_train_bwd"] == (i, [vp, vp, i, vp, i] + [vp] * 11 + [i] * 7 + [f, i, vp, i64, vp])
    assert {"gfn_conv2d_bn_act_train_fwd", "gfn_conv2d_bn_act_train_bwd"} <= _lib.STATUS_FUNCS
    assert "gfn_conv2d_bn_act_train_ws_bytes" not in _lib.STATUS_FUNCS  # a size, not a status
    assert (_lib.CBT_NEED_X, _lib.CBT_NEED_W, _lib.CBT_NEED_BN) == (1, 2, 4)
    L = _lib.lib()
    for name in ("gfn_conv2d_bn_act_train_ws_bytes", "gfn_conv2d_bn_act_train_fwd", "gfn_conv2d_bn_act_train_bwd"):
        getattr(L, name)


def test_workspace_sizes():
    L = _lib.lib()
    fwd = int(L.gfn_conv2d_bn_act_train_ws_bytes(8, 0, 2, 40, 56, 8, 5, 1, 0))
    bwd = int(L.gfn_conv2d_bn_act_train_ws_bytes(8, 0, 2, 40, 56, 8, 5, 1, 1))
    assert 0 < fwd < bwd and fwd % 16 == 0 and bwd % 16 == 0
    assert bwd >= 4 * 2 * 8 * 40 * 56  # the gu map
    assert L.gfn_conv2d_bn_act_train_ws_bytes(8, 0, 0, 40, 56, 8, 5, 1, 1) == 0 and L.gfn_conv2d_bn_act_train_ws_bytes(8, 0, 2, 40, 56, 8, 4, 1, 1) == 0
    # the shipped layers at 16 images of 448 x 448: the partial weight gradients stay within 16 MiB, whatever the layer
    for C0, C1, Cout, K, S, H in ((3, 0, 8, 7, 1, 448), (8, 0, 8, 5, 1, 448), (64, 64, 64, 3, 1, 56), (64, 32, 32, 3, 1, 112), (32, 0, 64, 3, 2, 112)):
        Ho = (H + S - 1) // S
        total = int(L.gfn_conv2d_bn_act_train_ws_bytes(C0, C1, 16, H, H, Cout, K, S, 1))
        gu = 4 * 16 * Cout * Ho * Ho
        assert gu < total <= gu + (20 << 20), (C0, C1, Cout, K, S, total - gu)


def test_forward_refuses_bad_arguments_before_any_launch():
    """Argument errors return before any HIP call, so this runs without a GPU; the dummy pointers are never read."""
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p(ctypes.addressof(buf))
    q = ctypes.c_void_p(ctypes.addressof(buf) + 16)
    r = ctypes.c_void_p(ctypes.addressof(buf) + 32)

    def call(x0=p, C0=3, x1=None, C1=0, weight=p, conv_bias=None, bn_w=p, bn_b=p, rm=p, rv=p, residual=None, u=q, mean=p, invstd=p, out=r, B=1,
             H=8, W=8, Cout=8, K=3, stride=1, act=1, momentum=0.1, eps=1e-5, ws=p, ws_bytes=1 << 30):
        return L.gfn_conv2d_bn_act_train_fwd(x0, C0, x1, C1, weight, conv_bias, bn_w, bn_b, rm, rv, residual, u, mean, invstd, out, B, H, W, Cout,
                                             K, stride, act, 0.1, momentum, eps, ws, ws_bytes, None)

    bad = [(dict(x0=None), "null"), (dict(weight=None), "null"), (dict(bn_w=None), "null"), (dict(bn_b=None), "null"), (dict(rm=None), "null"),
           (dict(rv=None), "null"), (dict(u=None), "null"), (dict(mean=None), "null"), (dict(invstd=None), "null"), (dict(out=None), "null"),
           (dict(C1=4), "null"),
           (dict(K=2), "kernel size 2"), (dict(K=9), "kernel size 9"), (dict(stride=3), "stride 3"), (dict(stride=0), "stride 0"),
           (dict(act=3), "act 3"), (dict(act=-1), "act -1"),
           (dict(C0=1, H=32768, W=16384), "2^31"), (dict(C0=1, Cout=256, H=2048, W=1024), "2^31"), (dict(C1=64, x1=p, H=4096, W=2048), "2^31"),
           (dict(Cout=0), "Cout"), (dict(Cout=257), "Cout"), (dict(C0=0), "C0"), (dict(H=0), "H=0"), (dict(C0=65536, H=2, W=2), "65535"),
           (dict(H=1, W=1), "more than one value per channel"), (dict(H=2, W=2, stride=2), "more than one value per channel"),
           (dict(momentum=1.5), "momentum"), (dict(momentum=-0.1), "momentum"), (dict(eps=-1.0), "eps"),
           (dict(u=r), "of their own"), (dict(out=p), "of their own")]
    for kwargs, text in bad:
        assert call(**kwargs) == _lib.ERR_INVALID_ARG == -1, kwargs
        assert text in L.gfn_last_error().decode(), (kwargs, L.gfn_last_error().decode())
    assert call(ws=None) == _lib.ERR_SCRATCH and call(ws_bytes=16) == _lib.ERR_SCRATCH
    assert call(B=0) == _lib.OK == 0
    assert call(B=0, x0=None, out=None, ws=None) == 0  # an empty batch reads nothing
    with pytest.raises(_lib.GfnError, match="gfn_conv2d_bn_act_train_fwd failed"):
        _lib.checked().gfn_conv2d_bn_act_train_fwd(p, 3, None, 0, p, None, p, p, p, p, None, q, p, p, r, 1, 8, 8, 8, 4, 1, 0, 0.1, 0.1, 1e-5, p, 1 << 30,
                                                   None)


def test_backward_refuses_bad_arguments_before_any_launch():
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p(ctypes.addressof(buf))

    def call(gy=p, x0=p, C0=3, x1=None, C1=0, weight=p, bn_w=p, bn_b=p, u=p, mean=p, invstd=p, gx0=p, gx1=None, d_weight=p, d_bn_w=p, d_bn_b=p,
             B=1, H=8, W=8, Cout=8, K=3, stride=1, act=1, need=7, ws=p, ws_bytes=1 << 30):
        return L.gfn_conv2d_bn_act_train_bwd(gy, x0, C0, x1, C1, weight, bn_w, bn_b, u, mean, invstd, gx0, gx1, d_weight, d_bn_w, d_bn_b, B, H, W,
                                             Cout, K, stride, act, 0.1, need, ws, ws_bytes, None)

    bad = [(dict(gy=None), "null"), (dict(x0=None), "null"), (dict(weight=None), "null"), (dict(bn_w=None), "null"), (dict(bn_b=None), "null"),
           (dict(u=None), "null"), (dict(mean=None), "null"), (dict(invstd=None), "null"), (dict(C1=4), "null"),
           (dict(gx0=None), "need mask"), (dict(C1=4, x1=p), "need mask"), (dict(d_weight=None), "need mask"), (dict(d_bn_w=None), "need mask"),
           (dict(d_bn_b=None), "need mask"), (dict(need=8), "unknown need"), (dict(need=-1), "unknown need"),
           (dict(K=2), "kernel size 2"), (dict(stride=3), "stride 3"), (dict(act=3), "act 3"), (dict(Cout=257), "Cout"), (dict(C0=0), "C0"),
           (dict(C0=1, H=32768, W=16384), "2^31"), (dict(H=1, W=1), "more than one value per channel")]
    for kwargs, text in bad:
        assert call(**kwargs) == _lib.ERR_INVALID_ARG == -1, kwargs
        assert text in L.gfn_last_error().decode(), (kwargs, L.gfn_last_error().decode())
    assert call(ws=None) == _lib.ERR_SCRATCH and call(ws_bytes=16) == _lib.ERR_SCRATCH
    assert call(B=0) == 0 and call(need=0) == 0
    assert call(need=0, gy=None, gx0=None, d_weight=None, d_bn_w=None, d_bn_b=None, ws=None) == 0  # nothing asked for, nothing read
    assert call(need=4, gx0=None, d_weight=None, ws=None) == _lib.ERR_SCRATCH  # only the named pointers are needed


def test_switch_defaults_to_torch_and_is_validated():
    chs = fpn_fixture.FEAT_CHS
    for make in (lambda **k: fpn.FPNEncoder(chs, **k), lambda **k: fpn.FPNDecoder_concat(chs, **k), lambda **k: fpn.merge_layer(64, **k),
                 lambda **k: fpn.Conv2d(3, 8, 3, padding=1, **k)):
        m = make()
        assert m.train_conv_impl == "torch" and m.conv_impl == "hip"
        assert make(train_conv_impl="hip").train_conv_impl == "hip"
        with pytest.raises(ValueError, match="train_conv_impl"):
            make(train_conv_impl="miopen")
    enc = fpn.FPNEncoder(chs, train_conv_impl="hip")
    assert all(c.train_conv_impl == "hip" for c in enc.children())
    x = torch.zeros(1, 3, 8, 8)
    # _use_hip is what it was: the new switch does not enter it, and on the CPU neither HIP path is taken
    enc.train(True)
    assert not fpn._use_hip(enc, x) and not fpn._use_train_hip(enc, x)
    enc.train(False)
    assert not fpn._use_hip(enc, x) and not fpn._use_train_hip(enc, x)
    enc.train_conv_impl = "cudnn"
    assert not fpn._use_hip(enc, x)
    with pytest.raises(ValueError, match="train_conv_impl"):
        enc(x)
    enc.train_conv_impl = "hip"
    enc.train(True)
    out = enc(torch.rand(2, 3, 8, 8))  # CPU tensors in train(): the torch path
    assert out[3].requires_grad


def test_fpn_train_impl_of_the_backbone():
    from gfnet_amd.reference_backbone import ReferenceBackbone, reference_backbone
    from test_fpn_gpu import StubVit

    conf = {"dino_cfg": {"d_model": 32,
                         "decoder_cfg": {"num_cross_attn": 2, "init_values": 1.0, "prev_values": 0.5, "nhead": 8, "attention_type": "FLASH2",
                                         "ffn_type": "ffn", "softmax_scale": "entropy_invariance", "train_avg_length": 1024,
                                         "self_cross_types": None, "post_norm": False, "pre_norm_query": True, "no_combine_norm": False}},
            "encoder_cfg": {"feat_chs": [64, 32, 16, 8]}}
    for make in (ReferenceBackbone, reference_backbone):
        with pytest.raises(ValueError, match="fpn_train_impl"):
            make(conf, vit=StubVit(), decoder="hip", fpn="checkout", fpn_train_impl="hip")
        with pytest.raises(ValueError, match="fpn_train_impl"):
            make(conf, vit=StubVit(), decoder="hip", fpn="hip", fpn_train_impl="cudnn")
    bb = ReferenceBackbone(conf, vit=StubVit(), decoder="hip", fpn="hip", fpn_train_impl="hip")
    assert bb.encoder.train_conv_impl == bb.decoder.train_conv_impl == bb.merge_layer.train_conv_impl == "hip"
    bb = ReferenceBackbone(conf, vit=StubVit(), decoder="hip", fpn="hip")
    assert bb.encoder.train_conv_impl == bb.decoder.train_conv_impl == bb.merge_layer.train_conv_impl == "torch"


def test_ops_refuse_cpu_tensors():
    from gfnet_amd import ops

    x, w, s = torch.zeros(1, 3, 8, 8), torch.zeros(8, 3, 3, 3), torch.ones(8)
    with pytest.raises(_lib.GfnError, match="no CPU path"):
        ops.conv2d_bn_act_train(x, w, None, s, s, s.clone(), s.clone(), None, 0.1, 1e-5)
    with pytest.raises(_lib.GfnError, match="no CPU path"):
        ops.conv2d_bn_act_train_fwd(x, w, None, s, s, s.clone(), s.clone(), 0.1, 1e-5)
    with pytest.raises(_lib.GfnError, match="no CPU path"):
        ops.conv2d_bn_act_train_bwd(torch.zeros(1, 8, 8, 8), x, w, s, s, torch.zeros(1, 8, 8, 8), s, s)
    with pytest.raises(ValueError, match="act"):
        ops.conv2d_bn_act_train(x, w, None, s, s, s.clone(), s.clone(), None, 0.1, 1e-5, act="relu")
    with pytest.raises(ValueError, match="momentum"):
        ops.conv2d_bn_act_train(x, w, None, s, s, s.clone(), s.clone(), None, None, 1e-5)


def test_torch_training_path_reproduces_the_reference_modules_step():
    """fp32 on the CPU, where the module takes its torch path whatever the switches say, against the reference's own fp32 step: maps,
    buffers and gradients within 4 x the reference's fp32-vs-float64 difference (checked by the GPU file's comparison)."""
    from conftest import load_golden
    from make_golden_fpn_train import SHAPE, train_step
    from test_fpn_cpu import run_modules
    from test_fpn_train_gpu import build, compare_to_golden

    for impl in ("torch", "hip"):
        mods = build(torch.float32, "cpu", impl)
        images, side = fpn_fixture.inputs(SHAPE)
        compare_to_golden(f"cpu torch path ({impl})", train_step(mods, run_modules, images, side), load_golden("g17_fpn_train"))
