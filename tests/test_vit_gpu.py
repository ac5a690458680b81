"""ops.ls_add_layernorm (csrc/layernorm.hip) and the native DINOv2 ViT (gfnet_amd/model/dinov2.py, impl="hip") on the GPU.

The seam, against float64 of the same rounded inputs:
  x_out   one ulp of the storage type at max|x_out| (the fused multiply-add is rounded once; a half-ulp rounding and its tie)
  h       against float64 LayerNorm of x_out AS THE KERNEL STORED IT (the statistics are taken from the rounded stream):
          fp32 class max(4 * E32, 2^-20 * max|h|), E32 = F.layer_norm in float32 on the CPU against float64 (4 for the summation
          order); fp16 class that plus 2^-11 * max|h|, the one final rounding.
The model, in fp16 with impl="hip", against the same module in float64: at most 2 x the error of the same module's impl="torch"
fp16 run on the GPU (the reference's arithmetic class; 2 because the fused seam rounds once where torch rounds twice, and P is
rounded).

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
seam, error / bound, worst case over rows 1, 7, 1025 x C 72, 128, 1024 and the fused and plain modes:
fp16   x_out 0.50 (half an ulp, as it must be)   h 0.81 (7x1024 plain: err 1.9e-03, bound 2.4e-03)
fp32   x_out 0.50                                h 0.18 (1x72 fused)
variance of rows with mean 1e3: fp16 0.60, fp32 0.11 (err 4.3e-05, bound 3.8e-04)
model (width 128, 2 blocks, 2 heads of 64), error against the float64 module: impl "hip" / impl "torch" in fp16 on the GPU
native  patch tokens 5.9e-03 / 5.2e-03   cls token 3.5e-03 / 3.0e-03   x_prenorm 5.0e-03 / 5.0e-03   (values up to 4.7)
wide    patch tokens 5.0e-03 / 6.3e-03   cls token 2.7e-03 / 3.9e-03   x_prenorm 5.3e-03 / 4.5e-03
tall    patch tokens 5.5e-03 / 5.9e-03   cls token 4.0e-03 / 3.3e-03   x_prenorm 5.4e-03 / 5.4e-03
"""

DEV = "cuda"
EPS = 1e-6


def _ulp(dtype, value):
    return 2.0 ** (math.floor(math.log2(value)) - (10 if dtype == torch.float16 else 23))


def _ln64(x, w, b):
    return F.layer_norm(x.double(), x.shape[-1:], w.double(), b.double(), EPS)


def _h_bound(dtype, x_stored, w, b):
    """(float64 LayerNorm of the stored stream, bound on h)."""
    h64 = _ln64(x_stored, w, b)
    e32 = float((F.layer_norm(x_stored.float(), x_stored.shape[-1:], w.float(), b.float(), EPS).double() - h64).abs().max())
    hmax = float(h64.abs().max())
    return h64, max(4 * e32, 2.0 ** -20 * hmax) + (2.0 ** -11 * hmax if dtype == torch.float16 else 0.0)


@functools.lru_cache(maxsize=None)
def seam_inputs(rows, C, dtype):
    g = torch.Generator().manual_seed(rows * 8209 + C * 3 + (1 if dtype == torch.float16 else 0))
    x, y = 2.0 * torch.randn(rows, C, generator=g), torch.randn(rows, C, generator=g)
    gamma, w, b = 0.75 + 0.35 * torch.rand(C, generator=g), 0.6 + 0.8 * torch.rand(C, generator=g), 0.4 * torch.rand(C, generator=g) - 0.2
    return tuple(t.to(dtype) for t in (x, y, gamma, w, b))  # rounded to the storage type: what kernel and oracle both read


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "fp32"])
@pytest.mark.parametrize("C", [72, 128, 1024])
@pytest.mark.parametrize("rows", [1, 7, 1025])
def test_seam_modes_against_float64(rows, C, dtype):
    x, y, gamma, w, b = seam_inputs(rows, C, dtype)
    xd, yd, gd, wd, bd = (t.to(DEV) for t in (x, y, gamma, w, b))
    xo64 = x.double() + gamma.double() * y.double()
    xb = _ulp(dtype, float(xo64.abs().max()))

    def check(tag, xo, h, x_ref, want_h=True):
        if x_ref is not None:
            err = float((xo.double().cpu() - x_ref).abs().max())
            print(f"seam {rows}x{C} {str(dtype)[6:]} {tag} x_out: err {err:.3e} bound {xb:.3e} ratio {err / xb:.3f}")
            assert xo.dtype == dtype and err <= xb, (tag, err, xb)
        if want_h:
            h64, hb = _h_bound(dtype, xo.cpu(), w, b)
            err = float((h.double().cpu() - h64).abs().max())
            print(f"seam {rows}x{C} {str(dtype)[6:]} {tag} h: err {err:.3e} bound {hb:.3e} ratio {err / hb:.3f}")
            assert h.dtype == dtype and torch.isfinite(h).all() and err <= hb, (tag, err, hb)

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


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "fp32"])
def test_variance_of_a_row_far_from_zero(dtype):
    """Rows with mean 1e3 and spread 1: E[x^2] - mean^2 in fp32 loses the variance (1e6 * 2^-24 = 0.06 against 1 or less), the
    two-pass sum does not."""
    g = torch.Generator().manual_seed(11)
    x = (1000.0 + torch.randn(7, 1024, generator=g)).to(dtype)
    w, b = (0.6 + 0.8 * torch.rand(1024, generator=g)).to(dtype), torch.zeros(1024, dtype=dtype)
    _, h = ops.ls_add_layernorm(x.to(DEV), None, None, w.to(DEV), b.to(DEV), EPS)
    h64, hb = _h_bound(dtype, x, w, b)
    err = float((h.double().cpu() - h64).abs().max())
    print(f"variance {str(dtype)[6:]}: err {err:.3e} bound {hb:.3e} ratio {err / hb:.3f} (row variance {float(x.double().var(1).min()):.3f})")
    assert err <= hb


def test_seam_refuses_what_it_cannot_run():
    from gfnet_amd import _lib

    x = torch.zeros(2, 1020, device=DEV)
    with pytest.raises(_lib.GfnError, match="multiple of 8"):
        ops.ls_add_layernorm(x, None, None, x[0], x[0], EPS)
    x = torch.zeros(2, 64, device=DEV)
    with pytest.raises(TypeError, match="one dtype"):
        ops.ls_add_layernorm(x, None, None, x[0].half(), x[0], EPS)
    with pytest.raises(ValueError, match="nothing to compute"):
        ops.ls_add_layernorm(x, None, None, None, None, EPS)


# ---- the model ------------------------------------------------------------------------------------------------------------------
def small_vit(impl, device="cpu", dtype=torch.float32):
    cfg = {k: v for k, v in vit_fixture.CONFIG.items()}
    m = dinov2.DinoVisionTransformer(impl=impl, **cfg)
    vit_fixture.fill(m)
    return m.train(False).to(device, dtype)


@functools.lru_cache(maxsize=None)
def float64_features(name):
    with torch.no_grad():
        return small_vit("torch", dtype=torch.float64).forward_features(vit_fixture.inputs(name).double())


@pytest.mark.parametrize("name", [s[0] for s in vit_fixture.INPUTS])
def test_native_model_fp16_against_float64(name):
    want = float64_features(name)
    x = vit_fixture.inputs(name).to(DEV, torch.float16)
    hip, tor = small_vit("hip", DEV, torch.float16), small_vit("torch", DEV, torch.float16)
    with torch.no_grad():
        got, ref = hip.forward_features(x), tor.forward_features(x)
    assert set(got) == set(ref) == {"x_norm_clstoken", "x_norm_patchtokens", "x_prenorm", "masks"} and got["masks"] is None
    for o in vit_fixture.OUTPUTS + ("x_prenorm",):
        assert got[o].dtype == torch.float16 and got[o].shape == want[o].shape and torch.isfinite(got[o]).all()
        e_hip = float((got[o].double().cpu() - want[o]).abs().max())
        e_tor = float((ref[o].double().cpu() - want[o]).abs().max())
        print(f"vit {name} {o}: hip err {e_hip:.3e}  torch fp16 err {e_tor:.3e}  margin {2 * e_tor:.3e}  max|v| {float(want[o].abs().max()):.2f}")
        assert e_hip <= 2 * e_tor, (o, e_hip, e_tor)


def test_every_block_takes_two_seam_launches_and_one_attention_launch(monkeypatch):
    calls = []
    real_attn, real_seam, real_block = ops.self_attention, ops.ls_add_layernorm, dinov2.Block.forward_hip

    def attn(qkv, scale):
        calls.append("attn")
        return real_attn(qkv, scale)

    def seam(x, y, *a, **k):
        calls.append("plain" if y is None else "seam")
        return real_seam(x, y, *a, **k)

    def block(self, *a, **k):
        calls.append("block")
        return real_block(self, *a, **k)

    monkeypatch.setattr(ops, "self_attention", attn)
    monkeypatch.setattr(ops, "ls_add_layernorm", seam)
    monkeypatch.setattr(dinov2.Block, "forward_hip", block)
    m = small_vit("hip", DEV, torch.float16)
    x = vit_fixture.inputs("wide").to(DEV, torch.float16)
    with torch.no_grad():
        m.forward_features(x)
    depth = vit_fixture.CONFIG["depth"]
    assert calls == ["plain"] + ["block", "attn", "seam", "seam"] * depth, calls  # (block 0's norm1 is the one plain LayerNorm)
    # masks, fp32 and impl="torch" run the torch ops: no launch of either kind
    del calls[:]
    with torch.no_grad():
        m.forward_features(x, masks=torch.zeros(2, 24, dtype=torch.bool, device=DEV))
        m.float().forward_features(x.float())
        small_vit("torch", DEV, torch.float16).forward_features(x)
    assert calls == []


def test_backbone_with_all_three_native_parts_runs_end_to_end():
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
    bb = ReferenceBackbone(conf, vit=vit, decoder="hip", fpn="hip", dino="hip").to(DEV).train(False)
    images = torch.rand(2, 3, 112, 112, device=DEV) * 2 - 1
    seen = []
    real = ops.self_attention
    try:
        ops.self_attention = lambda qkv, scale: (seen.append(tuple(qkv.shape)), real(qkv, scale))[1]
        with torch.no_grad():
            pa, pb = bb(images)
    finally:
        ops.self_attention = real
    assert seen == [(2, 65, 3, 2, 64)] * vit_fixture.CONFIG["depth"]  # the ViT ran in fp16 on its own kernels
    want = {"16": (1, 64, 8, 8), "8": (1, 64, 14, 14), "4": (1, 32, 28, 28), "2": (1, 16, 56, 56), "1": (1, 8, 112, 112)}
    for p in (pa, pb):
        assert {k: tuple(v.shape) for k, v in p.items()} == want
        assert all(torch.isfinite(v).all() for v in p.values())
