"""The native DINOv2 ViT as far as it goes without a GPU: the module's torch path against the reference's own module
(tests/golden/g16_dinov2.npz, made by tests/golden/make_golden_vit.py), its parameter names, the definition of the attention op, the
opt-in wiring into the reference backbone and the C ABI's refusals."""
import ctypes
import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import vit_fixture
from conftest import ROOT, load_golden
from gfnet_amd import _lib, ops
from gfnet_amd.model import dinov2


def small_vit(impl="hip"):
    m = dinov2.DinoVisionTransformer(impl=impl, **vit_fixture.CONFIG)
    return m, vit_fixture.fill(m)


def test_abi_declares_both_entry_points_and_refuses_bad_arguments_before_any_launch():
    """Argument errors return before any HIP call, so this runs without a GPU; the dummy pointers are never read."""
    vp, i, i64, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    assert _lib.PROTOTYPES["gfn_self_attn_fwd"] == (i, [vp, i, i, i, i, i, f, vp, vp])
    assert _lib.PROTOTYPES["gfn_ls_add_layernorm_fwd"] == (i, [vp, vp, vp, vp, vp, f, i, i64, i, vp, vp, vp])
    assert {"gfn_self_attn_fwd", "gfn_ls_add_layernorm_fwd"} <= _lib.STATUS_FUNCS
    assert {"gfn_self_attn_fwd", "gfn_ls_add_layernorm_fwd"} <= set(_lib.exported_symbols())
    L = _lib.lib()
    assert L.gfn_abi_version() == 1
    buf = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p(ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16)

    def attn(qkv=p, dtype=_lib.GFN_F16, B=1, N=32, H=2, D=64, scale=0.125, out=p):
        return L.gfn_self_attn_fwd(qkv, dtype, B, N, H, D, scale, out, None)

    bad = [(dict(D=8), "head dim 8"), (dict(D=32), "head dim 32"), (dict(D=128), "head dim 128"), (dict(dtype=_lib.GFN_F32), "dtype"),
           (dict(N=0), "N=0"), (dict(H=0), "H=0"), (dict(B=-1), "B=-1"), (dict(qkv=None), "qkv"), (dict(out=None), "out"),
           (dict(scale=float("inf")), "scale"), (dict(scale=float("nan")), "scale"), (dict(B=65536, H=65536), "grid"),
           (dict(qkv=ctypes.c_void_p(p.value + 2)), "aligned")]
    for kwargs, text in bad:
        assert attn(**kwargs) == _lib.ERR_INVALID_ARG == -1, kwargs
        assert text in L.gfn_last_error().decode(), (kwargs, L.gfn_last_error().decode())
    assert attn(B=0) == _lib.OK == 0
    assert attn(B=0, qkv=None, out=None) == 0  # an empty batch reads nothing

    def seam(x=p, y=p, gamma=p, weight=p, bias=p, eps=1e-6, dtype=_lib.GFN_F16, rows=4, C=128, x_out=p, h_out=None):
        # (h_out defaults to NULL here: a good call with h_out would want a second buffer that aliases nothing)
        return L.gfn_ls_add_layernorm_fwd(x, y, gamma, weight, bias, eps, dtype, rows, C, x_out, h_out, None)

    q = ctypes.c_void_p(p.value + 16)
    bad = [(dict(C=1020), "multiple of 8"), (dict(C=8200), "multiple of 8"), (dict(C=16384), "8192"), (dict(C=0), "multiple of 8"),
           (dict(dtype=2), "dtype"), (dict(rows=-1), "rows"), (dict(eps=-1.0), "eps"), (dict(eps=float("nan")), "eps"),
           (dict(x=None), "(x)"), (dict(gamma=None), "(gamma)"), (dict(x_out=None), "(x_out)"),
           (dict(h_out=q, weight=None), "(weight)"), (dict(h_out=q, bias=None), "(bias)"),
           (dict(y=None, h_out=None), "nothing to compute"), (dict(h_out=p), "alias"),
           (dict(x=ctypes.c_void_p(p.value + 2)), "aligned")]
    for kwargs, text in bad:
        assert seam(**kwargs) == _lib.ERR_INVALID_ARG == -1, kwargs
        assert text in L.gfn_last_error().decode(), (kwargs, L.gfn_last_error().decode())
    assert seam(rows=0) == 0 and seam(rows=0, x=None, x_out=None) == 0
    with pytest.raises(_lib.GfnError, match="gfn_self_attn_fwd failed"):
        _lib.checked().gfn_self_attn_fwd(p, _lib.GFN_F16, 1, 32, 2, 8, 0.125, p, None)


def test_ops_refuse_cpu_tensors():
    with pytest.raises(_lib.GfnError, match="no CPU path"):
        ops.self_attention(torch.zeros(1, 4, 3, 1, 64, dtype=torch.float16), 0.125)
    x = torch.zeros(2, 64)
    with pytest.raises(_lib.GfnError, match="no CPU path"):
        ops.ls_add_layernorm(x, x, x[0], x[0], x[0], 1e-6)


def test_reference_self_attention_is_sdpa_on_the_permuted_tensors():
    g = torch.Generator().manual_seed(3)
    qkv = torch.randn(2, 37, 3, 3, 64, generator=g, dtype=torch.float64)
    for scale in (64 ** -0.5, 0.0, 0.7):
        q, k, v = qkv.permute(2, 0, 3, 1, 4).unbind(0)  # attention.py:79-81
        want = F.scaled_dot_product_attention(q, k, v, scale=scale).transpose(1, 2)
        got = ops.reference_self_attention(qkv, scale)
        assert got.shape == (2, 37, 3, 64) and float((got - want).abs().max()) <= 1e-14
    assert ops.reference_self_attention(qkv.float(), 0.125).dtype == torch.float32


@pytest.mark.parametrize("name", [s[0] for s in vit_fixture.INPUTS])
def test_torch_path_reproduces_the_reference_modules_features(name):
    """fp32 on the CPU against the reference's own DinoVisionTransformer, within 4 x that module's fp32-vs-float64 difference."""
    g = load_golden("g16_dinov2")
    m, _ = small_vit()
    m.train(False)
    with torch.no_grad():
        got = m.forward_features(vit_fixture.inputs(name))
    assert set(got) == {"x_norm_clstoken", "x_norm_patchtokens", "x_prenorm", "masks"} and got["masks"] is None
    for o in vit_fixture.OUTPUTS:
        want, e32 = g[f"{name}/{o}"], float(g[f"{name}/{o}/fp32_vs_fp64"])
        assert 1e-7 < e32 < 1e-5, (o, e32)  # a unit of fp32 rounding on these values, not zero and not a blunder
        assert tuple(got[o].shape) == want.shape
        err = float(np.abs(got[o].numpy().astype(np.float64) - want).max())
        print(f"{name}/{o}: max err {err:.3e}, bound {4 * e32:.3e}")
        assert err <= 4 * e32, (name, o, err, 4 * e32)


def test_pos_encoding_early_return_and_cache():
    m, _ = small_vit()
    x = torch.zeros(1, 26, 128)
    assert m.interpolate_pos_encoding(x, 70, 70) is m.pos_embed  # the native square grid
    a = m.interpolate_pos_encoding(torch.zeros(1, 25, 128), 56, 84)
    assert a.shape == (1, 25, 128) and m.interpolate_pos_encoding(torch.zeros(1, 25, 128), 56, 84) is a  # cached per grid
    b = m.interpolate_pos_encoding(torch.zeros(1, 25, 128), 84, 56)
    assert b is not a and not torch.equal(a, b)  # the two orders are two grids
    vit_fixture.fill(m, seed=5)  # new parameters: the cached table is not served again
    c = m.interpolate_pos_encoding(torch.zeros(1, 25, 128), 56, 84)
    assert c is not a and not torch.equal(a, c)


def test_state_dict_keys_are_the_references():
    g = load_golden("g16_dinov2")
    m, keys = small_vit()
    assert keys == [str(k) for k in g["keys"]]
    m2, _ = small_vit()
    state = vit_fixture.state_dict(m2, seed=9)
    res = m2.load_state_dict(state, strict=True)
    assert not res.missing_keys and not res.unexpected_keys and torch.equal(m2.blocks[1].ls2.gamma, state["blocks.1.ls2.gamma"])
    assert not any(p.requires_grad for p in m.parameters())
    with torch.device("meta"):
        large = dinov2.vit_large()
    assert {k: list(v.shape) for k, v in large.state_dict().items()} == json.loads(str(g["large"]))
    assert large.impl == "hip" and large.embed_dim == 16 * dinov2.HIP_HEAD_DIM and len(large.blocks) == 24


def test_unused_settings_raise_at_construction():
    for kwargs, text in ((dict(ffn_layer="swiglu"), "ffn_layer"), (dict(ffn_layer="swiglufused"), "ffn_layer"),
                         (dict(block_chunks=1), "block_chunks"), (dict(drop_path_rate=0.1), "drop_path_rate")):
        with pytest.raises(NotImplementedError, match=text):
            dinov2.DinoVisionTransformer(**{**vit_fixture.CONFIG, **kwargs})
    with pytest.raises(ValueError, match="impl"):
        dinov2.DinoVisionTransformer(impl="xformers", **vit_fixture.CONFIG)


# a stand-in checkout whose model/transformer raises on import: with dino="hip" nothing of it is needed
STANDIN = {"model/__init__.py": "", "model/transformer/__init__.py": "raise ImportError('the stand-in checkout has no DINOv2')\n"}

CHILD = """
import os, sys
import torch
sys.path.insert(0, os.environ["GFNET_TEST_GOLDEN_DIR"])
import vit_fixture
conf = {"dino_cfg": {"d_model": 128,
                     "decoder_cfg": {"num_cross_attn": 2, "init_values": 1.0, "prev_values": 0.5, "nhead": 8, "attention_type": "FLASH2",
                                     "ffn_type": "ffn", "softmax_scale": "entropy_invariance", "train_avg_length": 1024,
                                     "self_cross_types": None, "post_norm": False, "pre_norm_query": True, "no_combine_norm": False}},
        "encoder_cfg": {"feat_chs": [64, 32, 16, 8]},
        "matcher": {"num_grid": [32, 32, 64, 128, 256], "radius": [7, 6, 4, 2, 0], "displacement_dim": [64, 64, 32, 16, 8],
                    "num_itr": [1, 1, 1, 1, 1]}}
import compat
import gfnet_amd.reference_backbone as rb
from gfnet_amd.model import dinov2
# the native builder asks this module for vit_large at call time: a small model in its place keeps the test quick, and its state
# dict stands for the checkpoint (no test reaches the download branch)
asked = []
def tiny_vit_large(**kwargs):
    asked.append(kwargs)
    return dinov2.DinoVisionTransformer(**vit_fixture.CONFIG)
dinov2.vit_large = tiny_vit_large
state = vit_fixture.state_dict(dinov2.DinoVisionTransformer(**vit_fixture.CONFIG))
"""


def _child(code, tmp_path, env=None):
    root = tmp_path / "checkout"
    for rel, text in STANDIN.items():
        f = root / rel
        f.parent.mkdir(parents=True, exist_ok=True)
        f.write_text(text)
    e = dict(os.environ)
    for k in ("GFNET_COMPAT_BACKBONE", "GFNET_COMPAT_DECODER", "GFNET_COMPAT_FPN", "GFNET_COMPAT_DINO", "GFNET_DINOV2_WEIGHTS"):
        e.pop(k, None)
    e["PYTHONPATH"] = os.pathsep.join([os.path.join(ROOT, "compat"), ROOT, str(root)])
    e["GFNET_TEST_GOLDEN_DIR"] = os.path.join(ROOT, "tests", "golden")
    e.update(env or {})
    script = tmp_path / "child.py"
    script.write_text(CHILD + textwrap.dedent(code))
    r = subprocess.run([sys.executable, str(script)], env=e, capture_output=True, text=True, cwd="/", timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip().endswith("ok")


def test_wiring_dino_hip_builds_the_native_vit_without_a_checkouts_transformer(tmp_path):
    _child("""
    bb = compat.reference_backbone(conf, dino_weights=state, decoder="hip", fpn="hip", dino="hip")
    vit = bb.dino[0]
    assert type(vit) is dinov2.DinoVisionTransformer and not vit.training and vit.impl == "hip"
    assert asked == [dict(img_size=518, patch_size=14, init_values=1.0, ffn_layer="mlp", block_chunks=0)]
    assert torch.equal(vit.blocks[1].ls2.gamma, state["blocks.1.ls2.gamma"]) and torch.equal(vit.pos_embed, state["pos_embed"])
    assert not any(k.startswith("dino.") for k in bb.state_dict())  # the ViT stays out of the backbone's state dict
    assert "model.transformer" not in sys.modules and "model.FPN" not in sys.modules and "model.crossview_decoder_light" not in sys.modules
    # the assembled backbone runs end to end on the CPU (torch paths) and hands out the five levels
    bb2 = compat.ReferenceBackbone(conf, dino_weights=state, decoder="hip", fpn="hip", dino="hip", amp=False)
    bb2.dino_decoder.attn_impl = "torch"
    for blk in bb2.dino_decoder.cross_attn_blocks:
        blk.attn.attn_impl = "torch"
    bb2.train(False)
    with torch.no_grad():
        pa, pb = bb2(torch.rand(2, 3, 56, 56))
    assert {k: tuple(v.shape) for k, v in pa.items()} == {"16": (1, 64, 4, 4), "8": (1, 64, 7, 7), "4": (1, 32, 14, 14),
                                                          "2": (1, 16, 28, 28), "1": (1, 8, 56, 56)}
    assert all(torch.isfinite(v).all() for v in list(pa.values()) + list(pb.values()))
    assert "model.transformer" not in sys.modules
    # the default still builds the checkout's ViT through _build_vit
    called = []
    rb._build_vit = lambda w: (called.append(w), vit)[1]
    assert compat.reference_backbone(conf, dino_weights=state, decoder="hip", fpn="hip").dino[0] is vit and called == [state]
    assert compat.ReferenceBackbone(conf, dino_weights=state, decoder="hip", fpn="hip", dino="checkout").dino[0] is vit and len(called) == 2
    for make in (compat.reference_backbone, compat.ReferenceBackbone):
        try:
            make(conf, vit=vit, decoder="hip", fpn="hip", dino="xformers")
        except ValueError as e:
            assert "dino" in str(e)
        else:
            raise AssertionError("unknown dino accepted")
    print("ok")
    """, tmp_path)


def test_default_dino_imports_the_checkouts_transformer(tmp_path):
    _child("""
    try:
        compat.reference_backbone(conf, dino_weights=state, decoder="hip", fpn="hip")
    except ImportError as e:
        assert "stand-in" in str(e)
    else:
        raise AssertionError("the default must still build the checkout's ViT")
    assert asked == []
    print("ok")
    """, tmp_path)


def test_wiring_environment_switch_on_the_reference_constructor_path(tmp_path):
    env = {"GFNET_COMPAT_BACKBONE": "reference", "GFNET_COMPAT_DECODER": "hip", "GFNET_COMPAT_FPN": "hip"}
    _child("""
    rb._load_dino_weights = lambda vit, w: vit  # (the reference's constructor passes no weights: this is where the download would be)
    from model.network import GFNet
    model = GFNet(conf=conf)
    assert type(model.backbone.dino[0]) is dinov2.DinoVisionTransformer and len(asked) == 1
    assert "model.transformer" not in sys.modules and "model.FPN" not in sys.modules
    print("ok")
    """, tmp_path, env={**env, "GFNET_COMPAT_DINO": "hip"})
    # without the switch the same constructor still asks for the checkout's ViT
    _child("""
    called = []
    rb._build_vit = lambda w: (called.append(w), torch.nn.Linear(1, 1))[1]
    from model.network import GFNet
    GFNet(conf=conf)
    assert called == [None] and asked == []
    print("ok")
    """, tmp_path, env=env)
