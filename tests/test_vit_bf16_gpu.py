"""The bf16 class of ops.ls_add_layernorm (csrc/layernorm.hip) and of the native DINOv2 ViT (gfnet_amd/model/dinov2.py, impl="hip")
on the GPU, as tests/test_vit_gpu.py tests the fp16 and fp32 classes.

The seam, against float64 of the same bf16-rounded inputs:
  x_out   one bf16 ulp at max|x_out|, 2^(floor(log2 v) - 7) (the fused multiply-add is rounded once; a half-ulp rounding and its tie)
  h       against float64 LayerNorm of x_out AS THE KERNEL STORED IT (the statistics are taken from the rounded stream):
          max(4 * E32, 2^-20 * max|h|) + 2^-8 * max|h|; E32 = F.layer_norm in float32 on the CPU against float64 (4 for the summation
          order), the last term the one final rounding to a format with 8 significand bits.
The model, in bf16 with impl="hip", against the same module in float64: at most 2 x the error of the same module's impl="torch" bf16
run on the same GPU (the project's margin for this comparison in tests/test_vit_gpu.py: the fused seam rounds once where torch rounds
twice, and P is rounded).  The margin is measured against the torch path, never against the code under test.

Measured on an MI355X: MEASURED below, from the figures every test prints before it asserts.
"""
import functools
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from gfnet_amd import ops
from gfnet_amd.model import dinov2

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import vit_fixture  # noqa: E402

pytestmark = pytest.mark.gpu

MEASURED = """
seam in bf16, error / bound, worst case over rows 1, 7, 1025 x C 72, 128, 1024 and the fused and plain modes:
x_out 0.50 (half an ulp, as it must be)   h 0.86 (7x128 plain: err 1.4e-02, bound 1.6e-02)
variance of rows with mean 1e3 (row variance of the stored values 0.54 .. 0.89): 0.52 (err 1.6e-02, bound 3.0e-02)
model (width 128, 2 blocks, 2 heads of 64), error against the float64 module: impl "hip" / impl "torch" in bf16 on the GPU
native  patch tokens 5.0e-02 / 4.6e-02   cls token 2.1e-02 / 2.3e-02   x_prenorm 4.7e-02 / 3.7e-02   (values up to 4.7)
wide    patch tokens 4.7e-02 / 4.8e-02   cls token 2.8e-02 / 3.5e-02   x_prenorm 3.5e-02 / 4.4e-02
tall    patch tokens 4.2e-02 / 4.7e-02   cls token 2.5e-02 / 1.7e-02   x_prenorm 3.8e-02 / 3.8e-02
worst hip / torch ratio 1.49 (tall, cls token) against the margin of 2
"""

DEV = "cuda"
EPS = 1e-6
BF = torch.bfloat16


def _ulp(value):
    return 2.0 ** (math.floor(math.log2(value)) - 7)


def _h_bound(x_stored, w, b):
    """(float64 LayerNorm of the stored stream, bound on h)."""
    h64 = F.layer_norm(x_stored.double(), x_stored.shape[-1:], w.double(), b.double(), EPS)
    e32 = float((F.layer_norm(x_stored.float(), x_stored.shape[-1:], w.float(), b.float(), EPS).double() - h64).abs().max())
    hmax = float(h64.abs().max())
    return h64, max(4 * e32, 2.0 ** -20 * hmax) + 2.0 ** -8 * hmax


@functools.lru_cache(maxsize=None)
def seam_inputs(rows, C):
    g = torch.Generator().manual_seed(rows * 8209 + C * 3 + 2)
    x, y = 2.0 * torch.randn(rows, C, generator=g), torch.randn(rows, C, generator=g)
    gamma, w, b = 0.75 + 0.35 * torch.rand(C, generator=g), 0.6 + 0.8 * torch.rand(C, generator=g), 0.4 * torch.rand(C, generator=g) - 0.2
    return tuple(t.to(BF) for t in (x, y, gamma, w, b))  # rounded to the storage type: what kernel and oracle both read


@pytest.mark.parametrize("C", [72, 128, 1024])
@pytest.mark.parametrize("rows", [1, 7, 1025])
def test_seam_modes_against_float64(rows, C):
    x, y, gamma, w, b = seam_inputs(rows, C)
    xd, yd, gd, wd, bd = (t.to(DEV) for t in (x, y, gamma, w, b))
    xo64 = x.double() + gamma.double() * y.double()
    xb = _ulp(float(xo64.abs().max()))

    def check(tag, xo, h, x_ref, want_h=True):
        if x_ref is not None:
            err = float((xo.double().cpu() - x_ref).abs().max())
            print(f"seam {rows}x{C} bf16 {tag} x_out: err {err:.3e} bound {xb:.3e} ratio {err / xb:.3f}")
            assert xo.dtype == BF and err <= xb, (tag, err, xb)
        if want_h:
            h64, hb = _h_bound(xo.cpu(), w, b)
            err = float((h.double().cpu() - h64).abs().max())
            print(f"seam {rows}x{C} bf16 {tag} h: err {err:.3e} bound {hb:.3e} ratio {err / hb:.3f}")
            assert h.dtype == BF and torch.isfinite(h).all() and err <= hb, (tag, err, hb)

    xo, h = ops.ls_add_layernorm(xd, yd, gd, wd, bd, EPS)  # fused
    assert xo.data_ptr() != xd.data_ptr() and torch.equal(xd.cpu(), x)
    check("fused", xo, h, xo64)
    x2, h2 = ops.ls_add_layernorm(xd, None, None, wd, bd, EPS)  # plain LayerNorm: x comes back as it is
    assert x2.data_ptr() == xd.data_ptr() and torch.equal(xd.cpu(), x)
    check("plain", x2, h2, None)
    xo3, h3 = ops.ls_add_layernorm(xd, yd, gd, None, None, EPS)  # residual only: the same stream bit for bit
    assert h3 is None and torch.equal(xo3, xo)
    xi = xd.clone().view(1, rows, C)  # in place, on a 3-d view
    xo4, h4 = ops.ls_add_layernorm(xi, yd.view(1, rows, C), gd, wd, bd, EPS, inplace=True)
    assert xo4.data_ptr() == xi.data_ptr() and torch.equal(xi.view(rows, C), xo) and torch.equal(h4.view(rows, C), h)


def test_variance_of_a_row_far_from_zero():
    """Rows with mean 1e3 and spread 1, drawn and then rounded to bf16 (the ulp there is 4 below 1024 and 8 above, so a row holds 1000
    and a few of its neighbours 996, 1004, ...; variance below 1): E[x^2] - mean^2 in fp32 loses that variance (1e6 * 2^-24 = 0.06
    against it), the two-pass sum over the stored values does not."""
    g = torch.Generator().manual_seed(11)
    x = (1000.0 + torch.randn(7, 1024, generator=g)).to(BF)
    w, b = (0.6 + 0.8 * torch.rand(1024, generator=g)).to(BF), torch.zeros(1024, dtype=BF)
    var = x.double().var(1, unbiased=False)
    assert float(var.min()) > 0.0, var  # the rounded rows still vary: there is a variance to lose
    _, h = ops.ls_add_layernorm(x.to(DEV), None, None, w.to(DEV), b.to(DEV), EPS)
    h64, hb = _h_bound(x, w, b)
    err = float((h.double().cpu() - h64).abs().max())
    print(f"variance bf16: err {err:.3e} bound {hb:.3e} ratio {err / hb:.3f} (row variance {float(var.min()):.3f} .. {float(var.max()):.3f})")
    assert h.dtype == BF and torch.isfinite(h).all() and err <= hb


def test_seam_still_refuses_mixed_dtypes():
    x = torch.zeros(2, 64, device=DEV, dtype=BF)
    with pytest.raises(TypeError, match="one dtype"):
        ops.ls_add_layernorm(x, None, None, x[0].half(), x[0], EPS)
    with pytest.raises(TypeError, match="one dtype"):
        ops.ls_add_layernorm(x.float(), x, x[0], x[0], x[0], EPS)


# ---- the model ------------------------------------------------------------------------------------------------------------------
def small_vit(impl, device="cpu", dtype=torch.float32):
    m = dinov2.DinoVisionTransformer(impl=impl, **vit_fixture.CONFIG)
    vit_fixture.fill(m)
    return m.train(False).to(device, dtype)


@functools.lru_cache(maxsize=None)
def float64_features(name):
    with torch.no_grad():
        return small_vit("torch", dtype=torch.float64).forward_features(vit_fixture.inputs(name).double())


@pytest.mark.parametrize("name", [s[0] for s in vit_fixture.INPUTS])
def test_native_model_bf16_against_float64(name):
    want = float64_features(name)
    x = vit_fixture.inputs(name).to(DEV, BF)
    hip, tor = small_vit("hip", DEV, BF), small_vit("torch", DEV, BF)
    with torch.no_grad():
        got, ref = hip.forward_features(x), tor.forward_features(x)
    assert set(got) == set(ref) == {"x_norm_clstoken", "x_norm_patchtokens", "x_prenorm", "masks"} and got["masks"] is None
    for o in vit_fixture.OUTPUTS + ("x_prenorm",):
        assert got[o].dtype == BF and got[o].shape == want[o].shape and torch.isfinite(got[o]).all()
        e_hip = float((got[o].double().cpu() - want[o]).abs().max())
        e_tor = float((ref[o].double().cpu() - want[o]).abs().max())
        print(f"vit bf16 {name} {o}: hip err {e_hip:.3e}  torch bf16 err {e_tor:.3e}  margin {2 * e_tor:.3e}  max|v| {float(want[o].abs().max()):.2f}")
        assert e_hip <= 2 * e_tor, (o, e_hip, e_tor)


def test_every_bf16_block_takes_two_seam_launches_and_one_bf16_attention_launch(monkeypatch):
    calls = []
    real_attn, real_seam, real_block = ops.self_attention_bf16, ops.ls_add_layernorm, dinov2.Block.forward_hip

    def attn(qkv, scale):
        assert qkv.dtype == BF
        calls.append("attn")
        return real_attn(qkv, scale)

    def attn_fp16(qkv, scale):
        calls.append("attn_fp16")
        raise AssertionError("the fp16 op was called for a bf16 model")

    def seam(x, y, *a, **k):
        assert x.dtype == BF
        calls.append("plain" if y is None else "seam")
        return real_seam(x, y, *a, **k)

    def block(self, *a, **k):
        calls.append("block")
        return real_block(self, *a, **k)

    monkeypatch.setattr(ops, "self_attention_bf16", attn)
    monkeypatch.setattr(ops, "self_attention", attn_fp16)
    monkeypatch.setattr(ops, "ls_add_layernorm", seam)
    monkeypatch.setattr(dinov2.Block, "forward_hip", block)
    m = small_vit("hip", DEV, BF)
    x = vit_fixture.inputs("wide").to(DEV, BF)
    with torch.no_grad():
        m.forward_features(x)
    depth = vit_fixture.CONFIG["depth"]
    assert calls == ["plain"] + ["block", "attn", "seam", "seam"] * depth, calls  # (block 0's norm1 is the one plain LayerNorm)
    # masks, fp32 and impl="torch" run the torch ops: no launch of either kind
    del calls[:]
    with torch.no_grad():
        m.forward_features(x, masks=torch.zeros(2, 24, dtype=torch.bool, device=DEV))
        small_vit("torch", DEV, BF).forward_features(x)
        m.float().forward_features(x.float())
    assert calls == []


def test_backbone_in_the_bf16_class_runs_the_vit_on_its_own_kernels():
    from gfnet_amd.reference_backbone import ReferenceBackbone

    conf = {"dino_cfg": {"d_model": 128,
                         "decoder_cfg": {"num_cross_attn": 2, "init_values": 1.0, "prev_values": 0.5, "nhead": 8, "attention_type": "FLASH2",
                                         "ffn_type": "ffn", "softmax_scale": "entropy_invariance", "train_avg_length": 1024,
                                         "self_cross_types": None, "post_norm": False, "pre_norm_query": True, "no_combine_norm": False}},
            "encoder_cfg": {"feat_chs": [64, 32, 16, 8]},
            "matcher": {"num_grid": [32, 32, 64, 128, 256], "radius": [7, 6, 4, 2, 0], "displacement_dim": [64, 64, 32, 16, 8],
                        "num_itr": [1, 1, 1, 1, 1]}}
    torch.manual_seed(0)
    vit = small_vit("hip")
    bb = ReferenceBackbone(conf, vit=vit, amp_dtype=BF, decoder="hip", fpn="hip", dino="hip").to(DEV).train(False)
    images = torch.rand(2, 3, 112, 112, device=DEV) * 2 - 1
    seen, seen_fp16 = [], []
    real, real_fp16 = ops.self_attention_bf16, ops.self_attention
    try:
        ops.self_attention_bf16 = lambda qkv, scale: (seen.append((tuple(qkv.shape), qkv.dtype)), real(qkv, scale))[1]
        ops.self_attention = lambda qkv, scale: (seen_fp16.append(tuple(qkv.shape)), real_fp16(qkv, scale))[1]
        with torch.no_grad():
            pa, pb = bb(images)
    finally:
        ops.self_attention_bf16, ops.self_attention = real, real_fp16
    assert all(p.dtype == BF for p in bb.dino[0].parameters())  # the backbone cast the ViT to amp_dtype
    assert seen == [((2, 65, 3, 2, 64), BF)] * vit_fixture.CONFIG["depth"] and seen_fp16 == []  # once per block, on the bf16 kernel
    want = {"16": (1, 64, 8, 8), "8": (1, 64, 14, 14), "4": (1, 32, 28, 28), "2": (1, 16, 56, 56), "1": (1, 8, 112, 112)}  # the fp16 run's
    for p in (pa, pb):
        assert {k: tuple(v.shape) for k, v in p.items()} == want
        assert all(torch.isfinite(v).all() for v in p.values())
