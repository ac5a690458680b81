"""The FPN decoder's 2x upsample inside the training op, as far as it goes without a GPU: the three gfn_conv2d_up_bn_act_train_*
entry points are declared, exported and bound from the header, the backward workspace grows by exactly the gradient of the doubled
map, bad arguments are refused before any launch (odd sizes and stride 2 with up0 among them), the "hip_fused" value of
train_conv_impl / fpn_train_impl is accepted where it belongs and refused where it does not, on the CPU in train() it is the torch
path bit for bit, and the new kernels spill nothing."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

import fpn_fixture
from conftest import ROOT
from gfnet_amd import _lib
from gfnet_amd.model import fpn

NAMES = ("gfn_conv2d_up_bn_act_train_ws_bytes", "gfn_conv2d_up_bn_act_train_fwd", "gfn_conv2d_up_bn_act_train_bwd")


def test_abi_declares_the_three_up_entry_points():
    """The old prototypes with `int up0` after C0."""
    vp, i, f, d, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_int64
    assert _lib.PROTOTYPES[NAMES[0]] == (i64, [i] * 10)
    assert _lib.PROTOTYPES[NAMES[1]] == (i, [vp, i, i, vp, i] + [vp] * 11 + [i] * 7 + [f, d, d, vp, i64, vp])
    assert _lib.PROTOTYPES[NAMES[2]] == (i, [vp, vp, i, i, vp, i] + [vp] * 11 + [i] * 7 + [f, i, vp, i64, vp])
    assert set(NAMES[1:]) <= _lib.STATUS_FUNCS and NAMES[0] not in _lib.STATUS_FUNCS  # a size, not a status
    assert set(NAMES) <= set(_lib.exported_symbols())
    L = _lib.lib()
    for name in NAMES:
        getattr(L, name)


def test_workspace_sizes_with_up0():
    L = _lib.lib()
    up, plain = L.gfn_conv2d_up_bn_act_train_ws_bytes, L.gfn_conv2d_bn_act_train_ws_bytes
    # up0 = 0 is the old entry point
    for backward in (0, 1):
        assert up(16, 0, 8, 2, 40, 56, 8, 3, 1, backward) == plain(16, 8, 2, 40, 56, 8, 3, 1, backward) > 0
        assert up(16, 0, 8, 2, 41, 55, 8, 3, 2, backward) == plain(16, 8, 2, 41, 55, 8, 3, 2, backward) > 0
    # refused sizes: odd H or W, stride 2, and what the old entry point refuses
    assert up(16, 1, 8, 2, 41, 56, 8, 3, 1, 1) == 0 and up(16, 1, 8, 2, 40, 55, 8, 3, 1, 1) == 0 and up(16, 1, 8, 2, 40, 56, 8, 3, 2, 1) == 0
    assert up(16, 1, 8, 0, 40, 56, 8, 3, 1, 1) == 0 and up(16, 1, 8, 2, 40, 56, 8, 4, 1, 1) == 0 and up(0, 1, 8, 2, 40, 56, 8, 3, 1, 1) == 0
    # the forward needs nothing more; the backward exactly the gradient of the doubled x0, (B, C0, H, W) floats rounded up to 4 (the
    # weight gradient's channel groups shrink with up0, the number and size of its partials do not depend on them)
    for C0, C1, B, H, W, Cout, K in ((16, 8, 2, 40, 56, 8, 3), (3, 5, 2, 14, 22, 5, 5), (64, 32, 16, 112, 112, 32, 3), (8, 0, 3, 2, 6, 8, 1)):
        assert up(C0, 1, C1, B, H, W, Cout, K, 1, 0) == plain(C0, C1, B, H, W, Cout, K, 1, 0)
        grown = int(up(C0, 1, C1, B, H, W, Cout, K, 1, 1)) - int(plain(C0, C1, B, H, W, Cout, K, 1, 1))
        assert grown == 4 * ((B * C0 * H * W + 3) // 4 * 4), (C0, C1, grown)
        assert int(up(C0, 1, C1, B, H, W, Cout, K, 1, 1)) % 16 == 0


def dummies():
    buf = ctypes.create_string_buffer(64)
    return buf, [ctypes.c_void_p(ctypes.addressof(buf) + 16 * k) for k in range(3)]


def test_up_forward_refuses_bad_arguments_before_any_launch():
    """Argument errors return before any HIP call, so this runs without a GPU; the dummy pointers are never read."""
    L = _lib.lib()
    buf, (p, q, r) = dummies()

    def call(x0=p, C0=3, up0=1, x1=None, C1=0, weight=p, conv_bias=None, bn_w=p, bn_b=p, rm=p, rv=p, residual=None, u=q, mean=p, invstd=p, out=r,
             B=1, H=8, W=8, Cout=8, K=3, stride=1, act=1, momentum=0.1, eps=1e-5, ws=p, ws_bytes=1 << 30):
        return L.gfn_conv2d_up_bn_act_train_fwd(x0, C0, up0, x1, C1, weight, conv_bias, bn_w, bn_b, rm, rv, residual, u, mean, invstd, out, B, H, W,
                                                Cout, K, stride, act, 0.1, momentum, eps, ws, ws_bytes, None)

    bad = [(dict(H=7), "H and W must be even"), (dict(W=9), "H and W must be even"), (dict(H=1, W=1), "H and W must be even"),
           (dict(stride=2), "up0 needs stride 1"),
           (dict(x0=None), "null"), (dict(weight=None), "null"), (dict(bn_w=None), "null"), (dict(bn_b=None), "null"), (dict(rm=None), "null"),
           (dict(rv=None), "null"), (dict(u=None), "null"), (dict(mean=None), "null"), (dict(invstd=None), "null"), (dict(out=None), "null"),
           (dict(C1=4), "null"),
           (dict(K=2), "kernel size 2"), (dict(stride=3), "stride 3"), (dict(act=3), "act 3"), (dict(Cout=257), "Cout"), (dict(C0=0), "C0"),
           (dict(C0=1, H=32768, W=16384), "2^31"), (dict(momentum=1.5), "momentum"), (dict(u=r), "of their own")]
    for kwargs, text in bad:
        assert call(**kwargs) == _lib.ERR_INVALID_ARG == -1, kwargs
        msg = L.gfn_last_error().decode()
        assert text in msg and "gfn_conv2d_up_bn_act_train_fwd" in msg, (kwargs, msg)
    assert call(ws=None) == _lib.ERR_SCRATCH and call(ws_bytes=16) == _lib.ERR_SCRATCH
    assert call(B=0) == _lib.OK == 0 and call(B=0, x0=None, out=None, ws=None) == 0
    # up0 = 0 is the old entry point: odd sizes and stride 2 are fine there (the workspace check is reached)
    assert call(up0=0, H=7, W=9, ws=None) == _lib.ERR_SCRATCH and call(up0=0, stride=2, ws=None) == _lib.ERR_SCRATCH
    with pytest.raises(_lib.GfnError, match="gfn_conv2d_up_bn_act_train_fwd failed"):
        _lib.checked().gfn_conv2d_up_bn_act_train_fwd(p, 3, 1, None, 0, p, None, p, p, p, p, None, q, p, p, r, 1, 7, 8, 8, 3, 1, 0, 0.1, 0.1, 1e-5, p,
                                                      1 << 30, None)
    del buf


def test_up_backward_refuses_bad_arguments_before_any_launch():
    L = _lib.lib()
    buf, (p, _, _) = dummies()

    def call(gy=p, x0=p, C0=3, up0=1, x1=None, C1=0, weight=p, bn_w=p, bn_b=p, u=p, mean=p, invstd=p, gx0=p, gx1=None, d_weight=p, d_bn_w=p,
             d_bn_b=p, B=1, H=8, W=8, Cout=8, K=3, stride=1, act=1, need=7, ws=p, ws_bytes=1 << 30):
        return L.gfn_conv2d_up_bn_act_train_bwd(gy, x0, C0, up0, x1, C1, weight, bn_w, bn_b, u, mean, invstd, gx0, gx1, d_weight, d_bn_w, d_bn_b, B,
                                                H, W, Cout, K, stride, act, 0.1, need, ws, ws_bytes, None)

    bad = [(dict(H=7), "H and W must be even"), (dict(W=9), "H and W must be even"), (dict(stride=2), "up0 needs stride 1"),
           (dict(gy=None), "null"), (dict(x0=None), "null"), (dict(weight=None), "null"), (dict(bn_w=None), "null"), (dict(bn_b=None), "null"),
           (dict(u=None), "null"), (dict(mean=None), "null"), (dict(invstd=None), "null"), (dict(C1=4), "null"),
           (dict(gx0=None), "need mask"), (dict(C1=4, x1=p), "need mask"), (dict(d_weight=None), "need mask"), (dict(d_bn_w=None), "need mask"),
           (dict(need=8), "unknown need"), (dict(need=-1), "unknown need"),
           (dict(K=2), "kernel size 2"), (dict(stride=3), "stride 3"), (dict(act=3), "act 3"), (dict(Cout=257), "Cout"), (dict(C0=0), "C0")]
    for kwargs, text in bad:
        assert call(**kwargs) == _lib.ERR_INVALID_ARG == -1, kwargs
        msg = L.gfn_last_error().decode()
        assert text in msg and "gfn_conv2d_up_bn_act_train_bwd" in msg, (kwargs, msg)
    assert call(ws=None) == _lib.ERR_SCRATCH and call(ws_bytes=16) == _lib.ERR_SCRATCH
    # a workspace of the up0 = 0 size is too small: the gradient of the doubled map lies behind it
    assert call(ws_bytes=int(L.gfn_conv2d_bn_act_train_ws_bytes(3, 0, 1, 8, 8, 8, 3, 1, 1))) == _lib.ERR_SCRATCH
    assert call(B=0) == 0 and call(need=0) == 0
    assert call(need=0, gy=None, gx0=None, d_weight=None, d_bn_w=None, d_bn_b=None, ws=None) == 0  # nothing asked for, nothing read
    assert call(need=4, gx0=None, d_weight=None, ws=None) == _lib.ERR_SCRATCH  # only the named pointers are needed
    del buf


def test_hip_fused_is_a_training_switch_only():
    chs = fpn_fixture.FEAT_CHS
    assert fpn.TRAIN_CONV_IMPLS == ("hip", "hip_fused", "torch") and fpn.CONV_IMPLS == ("hip", "torch")
    for make in (lambda **k: fpn.FPNEncoder(chs, **k), lambda **k: fpn.FPNDecoder_concat(chs, **k), lambda **k: fpn.merge_layer(64, **k),
                 lambda **k: fpn.Conv2d(3, 8, 3, padding=1, **k)):
        m = make(train_conv_impl="hip_fused")
        assert m.train_conv_impl == "hip_fused" and m.conv_impl == "hip"
        assert make().train_conv_impl == "torch" and make(train_conv_impl="hip").train_conv_impl == "hip"
        with pytest.raises(ValueError, match="^conv_impl"):
            make(conv_impl="hip_fused")
        with pytest.raises(ValueError, match="train_conv_impl"):
            make(train_conv_impl="hip_fuse")
    enc = fpn.FPNEncoder(chs, train_conv_impl="hip_fused")
    assert all(c.train_conv_impl == "hip_fused" for c in enc.children())
    x = torch.zeros(1, 3, 8, 8)
    enc.train(True)
    assert not fpn._use_hip(enc, x) and not fpn._use_train_hip(enc, x)  # CPU tensors: the torch path
    enc.conv_impl = "hip_fused"
    with pytest.raises(ValueError, match="^conv_impl"):
        enc(x)


def test_fpn_train_impl_hip_fused_of_the_backbone():
    from gfnet_amd.reference_backbone import ReferenceBackbone, reference_backbone
    from test_fpn_gpu import StubVit
    from test_fpn_train_gpu import E2E_CONF

    conf = {"dino_cfg": E2E_CONF["dino_cfg"], "encoder_cfg": E2E_CONF["encoder_cfg"]}
    for make in (ReferenceBackbone, reference_backbone):
        with pytest.raises(ValueError, match="fpn_train_impl"):
            make(conf, vit=StubVit(), decoder="hip", fpn="checkout", fpn_train_impl="hip_fused")
    bb = ReferenceBackbone(conf, vit=StubVit(), decoder="hip", fpn="hip", fpn_train_impl="hip_fused")
    assert bb.encoder.train_conv_impl == bb.decoder.train_conv_impl == bb.merge_layer.train_conv_impl == "hip_fused"
    assert all(c.train_conv_impl == "hip_fused" for c in bb.encoder.children())


def test_hip_fused_on_the_cpu_is_the_torch_path_bit_for_bit():
    """train() on CPU tensors: maps, buffers and gradients under "hip_fused" equal those under "torch" exactly."""
    from make_golden_fpn_train import SHAPE, train_step
    from test_fpn_cpu import run_modules
    from test_fpn_train_gpu import build

    images, side = fpn_fixture.inputs(SHAPE)
    want = train_step(build(torch.float32, "cpu", "torch"), run_modules, images, side)
    got = train_step(build(torch.float32, "cpu", "hip_fused"), run_modules, images, side)
    assert set(got) == set(want) and any(k.startswith("grad/") for k in want)
    for k in want:
        assert torch.equal(got[k], want[k]), k


def test_fpn_training_kernels_have_no_spills_and_no_scratch():
    """tools/kernel_regs.py on csrc/fpn_conv_train.o: the transposed upsample and the four up0 instantiations of the weight gradient
    (K = 1, 3, 5, 7) are there, and no kernel of the file spills a vector or scalar register, uses scratch or takes more than 64 KiB
    of static LDS."""
    obj = os.path.join(ROOT, "gfnet_amd", "csrc", "fpn_conv_train.o")
    if not os.path.exists(obj):
        from gfnet_amd import build

        build.build()
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), obj, "ft_"], capture_output=True, text=True,
                         check=True).stdout
    rows = [ln for ln in out.splitlines() if "ft_" in ln]
    assert sum("ft_up2_adjoint_kernel" in ln for ln in rows) == 1, out
    assert sum("ft_wgrad_kernel<true" in ln for ln in rows) == 4 and sum("ft_wgrad_kernel<false, 0>" in ln for ln in rows) == 1, out
    for ln in rows:
        f = ln.split()
        vals = {f[k]: f[k + 1] for k in range(len(f) - 1) if f[k] in ("spill", "sspill", "scratch")}
        assert vals == {"spill": "0", "sspill": "0", "scratch": "0"}, ln
        assert int(f[f.index("lds") + 1]) <= 64 * 1024, ln
