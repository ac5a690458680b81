"""The cross-view decoder and its attention op, as far as they go without a GPU: the C ABI, the op's refusals, the native module
against the reference's own (tests/golden/g14_crossview_decoder.npz, made by tests/golden/make_golden_decoder.py from the
reference's CrossVITDecoder_noself) and the opt-in wiring into the reference backbone."""
import ctypes
import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

from gfnet_amd import _lib, ops
from gfnet_amd.model.crossview_decoder import CrossViewDecoder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "g14_crossview_decoder.npz")


def load_golden():
    """(conf, state dict fp32, x, y fp32, (out_x, out_y) fp32, (B, H, W), the generator's fp32-vs-float64 difference)."""
    z = np.load(GOLDEN)
    state = {k[len("param/"):]: torch.from_numpy(z[k].astype(np.float32)) for k in z.files if k.startswith("param/")}
    x, y = (torch.from_numpy(z[k].astype(np.float32)) for k in ("x", "y"))
    outs = tuple(torch.from_numpy(z[k]) for k in ("out_x", "out_y"))
    return json.loads(str(z["conf"])), state, x, y, outs, tuple(int(v) for v in z["grid"]), float(z["fp32_vs_fp64"])


def test_abi_declares_both_entry_points_with_the_headers_signatures():
    vp, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert _lib.PROTOTYPES["gfn_cross_attn_fwd"] == (i, [vp, vp, vp, i, i, i, i, i, i, f, vp, vp, vp])
    assert _lib.PROTOTYPES["gfn_cross_attn_bwd"] == (i, [vp, vp, vp, vp, vp, vp, i, i, i, i, i, i, f, vp, vp, vp, vp])
    assert {"gfn_cross_attn_fwd", "gfn_cross_attn_bwd"} <= _lib.STATUS_FUNCS
    L = ctypes.CDLL(_lib.LIB_PATH)  # the symbols are exported (loading the library needs no GPU)
    assert L.gfn_cross_attn_fwd and L.gfn_cross_attn_bwd


def test_head_dim_other_than_8_is_refused_before_anything_is_launched():
    """Argument errors return before any HIP call, so this runs without a GPU: null pointers never get read."""
    L = _lib.lib()
    for D in (4, 16, 64):
        assert L.gfn_cross_attn_fwd(None, None, None, _lib.GFN_F16, 1, 32, 32, 8, D, 1.0, None, None, None) == _lib.ERR_INVALID_ARG
        assert "head dim" in L.gfn_last_error().decode() and str(D) in L.gfn_last_error().decode()
        assert L.gfn_cross_attn_bwd(None, None, None, None, None, None, _lib.GFN_F32, 1, 32, 32, 8, D, 1.0, None, None, None,
                                    None) == _lib.ERR_INVALID_ARG
    assert L.gfn_cross_attn_fwd(None, None, None, 7, 1, 32, 32, 8, 8, 1.0, None, None, None) == _lib.ERR_INVALID_ARG  # dtype
    assert L.gfn_cross_attn_fwd(None, None, None, _lib.GFN_F16, 1, 32, 0, 8, 8, 1.0, None, None, None) == _lib.ERR_INVALID_ARG  # Nk = 0
    assert L.gfn_cross_attn_fwd(None, None, None, _lib.GFN_F16, 1, 32, 32, 8, 8, 1.0, None, None, None) == _lib.ERR_INVALID_ARG  # null


def test_cpu_tensors_raise():
    q = torch.randn(1, 4, 2, 8)
    with pytest.raises(_lib.GfnError, match="no CPU path"):
        ops.cross_attention(q, q, q, 0.5)
    with pytest.raises(_lib.GfnError, match="no CPU path"):
        ops.cross_attention(q.requires_grad_(), q, q, 0.5)


def test_reference_cross_attention_is_the_definition():
    """Against explicit loops in float64, and differentiable in any dtype."""
    g = torch.Generator().manual_seed(3)
    q, k, v = torch.randn(2, 5, 3, 8, generator=g).double(), torch.randn(2, 7, 3, 8, generator=g).double(), torch.randn(2, 7, 3, 8, generator=g).double()
    out = ops.reference_cross_attention(q, k, v, 0.3)
    for b in range(2):
        for h in range(3):
            p = torch.softmax(q[b, :, h] @ k[b, :, h].T * 0.3, dim=-1)
            assert torch.allclose(out[b, :, h], p @ v[b, :, h], rtol=0, atol=1e-14)
    assert ops.reference_cross_attention(q.half().float(), k.float(), v.float(), 0.3).dtype == torch.float32
    assert torch.allclose(ops.reference_cross_attention(q, k, v, 0.0), v.mean(1, keepdim=True).expand_as(q), rtol=0, atol=1e-14)


def test_native_decoder_has_the_goldens_parameters_and_loads_them_strictly():
    conf, state, *_ = load_golden()
    dec = CrossViewDecoder(conf, attn_impl="torch")
    own = dec.state_dict()
    assert set(own) == set(state)
    for k, v in state.items():
        assert tuple(own[k].shape) == tuple(v.shape), k
    res = dec.load_state_dict(state, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    names = {k.split(".", 2)[2] for k in state if k.startswith("cross_attn_blocks.0.")}
    assert names == {"norm1.weight", "norm1.bias", "attn.q_proj.weight", "attn.k_proj.weight", "attn.v_proj.weight", "attn.proj.weight",
                     "attn.proj.bias", "ls1.gamma", "norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight",
                     "mlp.fc2.bias", "ls2.gamma"}


def test_native_decoder_reproduces_the_reference_modules_maps():
    """attn_impl="torch" in fp32 on the CPU against the reference module's fp32 maps.  Bound: 4 x the largest difference between
    the reference module's own fp32 and float64 runs (stored by the generator: 2.6e-6 on maps up to 7.7); the 4 covers the
    attention core's summation order (the generator's flash_attn_func stand-in sums in float64, this one in fp32)."""
    conf, state, x, y, outs, (B, H, W), e32 = load_golden()
    dec = CrossViewDecoder(conf, attn_impl="torch")
    dec.load_state_dict(state, strict=True)
    dec.train(False)
    with torch.no_grad():
        got = dec(x, y, vit_shape=(B, 3, H, W))
    assert 1e-7 < e32 < 1e-4  # a unit of fp32 rounding on these maps, not zero and not a blunder
    for name, a, b in zip("xy", got, outs):
        assert a.shape == b.shape == (B, conf["encoder_cfg"]["feat_chs"][0], H, W)
        err = float((a - b).abs().max())
        print(f"map {name}: max err {err:.3e}, bound {4 * e32:.3e}")
        assert err <= 4 * e32, (name, err, 4 * e32)
    # both directions share one launch: swapping the inputs swaps the outputs
    with torch.no_grad():
        sw = dec(y, x, vit_shape=(B, 3, H, W))
    assert torch.equal(sw[0], got[1]) and torch.equal(sw[1], got[0])


@pytest.mark.parametrize("key,value", [("ffn_type", "glu"), ("post_norm", True), ("pre_norm_query", False), ("attention_type", "Linear"),
                                       ("attn_drop", 0.1)])
def test_unsupported_settings_raise_at_construction_naming_the_key(key, value):
    conf = load_golden()[0]
    conf["dino_cfg"]["decoder_cfg"][key] = value
    with pytest.raises(NotImplementedError, match=key):
        CrossViewDecoder(conf)
    with pytest.raises(ValueError, match="attn_impl"):
        CrossViewDecoder(load_golden()[0], attn_impl="flash")


# a stand-in checkout written here: the two modules the backbone assembly takes from the user's checkout, with its interfaces
STANDIN = {
    "model/__init__.py": "",
    "model/FPN.py": """
import torch
import torch.nn as nn


class Swish(nn.Module):
    def forward(self, x):
        return x * torch.sigmoid(x)


class FPNEncoder(nn.Module):
    def __init__(self, feat_chs):
        super().__init__()
        self.stem = nn.Conv2d(3, feat_chs[0], 1)


class FPNDecoder_concat(nn.Module):
    def __init__(self, feat_chs):
        super().__init__()
        self.head = nn.Conv2d(feat_chs[0], feat_chs[0], 1)
""",
    "model/crossview_decoder_light.py": """
import torch.nn as nn


class CrossVITDecoder_noself(nn.Module):
    def __init__(self, conf, upsample=False):
        super().__init__()
        self.standin = nn.Linear(conf["dino_cfg"]["d_model"], conf["encoder_cfg"]["feat_chs"][0])
""",
}

CHILD = """
import json, os, sys
import numpy as np
import torch
z = np.load(os.environ["GFNET_TEST_GOLDEN"])
conf = json.loads(str(z["conf"]))
conf["matcher"] = {"num_grid": [32, 32, 64, 128, 256], "radius": [7, 6, 4, 2, 0], "displacement_dim": [64, 64, 32, 16, 8],
                   "num_itr": [1, 1, 1, 1, 1]}
golden_keys = {"dino_decoder." + k[len("param/"):] for k in z.files if k.startswith("param/")}
vit = torch.nn.Linear(1, 1)
import compat
from gfnet_amd.model.crossview_decoder import CrossViewDecoder
assert compat.CrossViewDecoder is CrossViewDecoder
"""


def _child(code, tmp_path, env=None, with_decoder_module=True):
    root = tmp_path / "checkout"
    for rel, text in STANDIN.items():
        if rel.endswith("crossview_decoder_light.py") and not with_decoder_module:
            continue
        f = root / rel
        f.parent.mkdir(parents=True, exist_ok=True)
        f.write_text(text)
    e = dict(os.environ)
    for k in ("GFNET_COMPAT_BACKBONE", "GFNET_COMPAT_DECODER"):
        e.pop(k, None)
    e["PYTHONPATH"] = os.pathsep.join([os.path.join(ROOT, "compat"), ROOT, str(root)])
    e["GFNET_TEST_GOLDEN"] = GOLDEN
    e.update(env or {})
    script = tmp_path / "child.py"
    script.write_text(CHILD + textwrap.dedent(code))
    r = subprocess.run([sys.executable, str(script)], env=e, capture_output=True, text=True, cwd="/", timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip().endswith("ok")


def test_wiring_decoder_hip_builds_the_native_decoder_without_the_checkouts(tmp_path):
    _child("""
    assert compat.checkout_available("hip") and not compat.checkout_available()
    bb = compat.reference_backbone(conf, vit=vit, decoder="hip")
    assert type(bb.dino_decoder) is CrossViewDecoder and bb.dino_decoder.attn_impl == "hip"
    assert "model.crossview_decoder_light" not in sys.modules
    assert {k for k in bb.state_dict() if k.startswith("dino_decoder.")} == golden_keys
    state = {"dino_decoder." + k[len("param/"):]: torch.from_numpy(z[k].astype(np.float32)) for k in z.files if k.startswith("param/")}
    res = bb.load_state_dict(state, strict=False)
    assert not res.unexpected_keys and not any(k.startswith("dino_decoder.") for k in res.missing_keys)
    try:
        compat.reference_backbone(conf, vit=vit)  # the default still wants the checkout's decoder module, absent in this checkout
    except ImportError as e:
        assert "crossview_decoder_light" in str(e)
    else:
        raise AssertionError("decoder left out must ask for the checkout's module")
    try:
        compat.reference_backbone(conf, vit=vit, decoder="flash")
    except ValueError as e:
        assert "decoder" in str(e)
    else:
        raise AssertionError("unknown decoder accepted")
    print("ok")
    """, tmp_path, with_decoder_module=False)


def test_wiring_default_keeps_the_checkouts_decoder(tmp_path):
    _child("""
    import model.crossview_decoder_light as cvd
    bb = compat.reference_backbone(conf, vit=vit)
    assert type(bb.dino_decoder) is cvd.CrossVITDecoder_noself
    assert type(compat.reference_backbone(conf, vit=vit, decoder="checkout").dino_decoder) is cvd.CrossVITDecoder_noself
    print("ok")
    """, tmp_path)


@pytest.mark.parametrize("decoder_env", [None, "hip"])
def test_wiring_environment_switch_on_the_reference_constructor_path(tmp_path, decoder_env):
    env = {"GFNET_COMPAT_BACKBONE": "reference"}
    if decoder_env:
        env["GFNET_COMPAT_DECODER"] = decoder_env
    _child("""
    import gfnet_amd.reference_backbone as rb
    import model.crossview_decoder_light as cvd
    rb._build_vit = lambda w: vit
    from model.network import GFNet
    model = GFNet(conf=conf)
    want = CrossViewDecoder if os.environ.get("GFNET_COMPAT_DECODER") == "hip" else cvd.CrossVITDecoder_noself
    assert type(model.backbone.dino_decoder) is want, type(model.backbone.dino_decoder)
    print("ok")
    """, tmp_path, env=env)
