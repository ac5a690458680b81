"""The fused cross-view decoder block (csrc/decoder_block.hip, ops.decoder_qkv / ops.decoder_post, CrossViewDecoder's
block_impl="hip", ReferenceBackbone's decoder="hip_fused") as far as it goes without a GPU: the C ABI and its refusals, which
return before anything is launched, the ops' refusal of CPU tensors, and the module's fallback to the torch blocks."""
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
    vp, i, i64, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    assert _lib.PROTOTYPES["gfn_decoder_qkv_fwd"] == (i, [vp, vp, vp, f, vp, vp, vp, i, i, i, vp, vp, vp, vp])
    assert _lib.PROTOTYPES["gfn_decoder_post_fwd"] == (i, [vp, vp, vp, vp, vp, vp, vp, f, vp, vp, vp, vp, vp, i64, i, i, vp, vp])
    assert {"gfn_decoder_qkv_fwd", "gfn_decoder_post_fwd"} <= _lib.STATUS_FUNCS
    assert {"gfn_decoder_qkv_fwd", "gfn_decoder_post_fwd"} <= set(_lib.exported_symbols())
    L = ctypes.CDLL(_lib.LIB_PATH)  # the symbols are exported (loading the library needs no GPU)
    assert L.gfn_decoder_qkv_fwd and L.gfn_decoder_post_fwd


# a host buffer stands in for every pointer: 16-byte aligned and never read, because every call below returns before a launch
_BUF = ctypes.create_string_buffer(64)
P = ctypes.c_void_p((ctypes.addressof(_BUF) + 15) & ~15)


def qkv(B2=2, N=32, C=64, ptrs=None):
    p = [P] * 9 if ptrs is None else ptrs
    return _lib.lib().gfn_decoder_qkv_fwd(p[0], p[1], p[2], 1e-5, p[3], p[4], p[5], B2, N, C, p[6], p[7], p[8], None)


def post(rows=32, C=64, hidden=256, ptrs=None):
    p = [P] * 13 if ptrs is None else ptrs
    return _lib.lib().gfn_decoder_post_fwd(*p[:7], 1e-5, *p[7:12], rows, C, hidden, p[12], None)


def last_error():
    return _lib.lib().gfn_last_error().decode()


def test_unsupported_sizes_are_refused_before_anything_is_launched():
    """Argument errors return before any HIP call, so this runs without a GPU; each leaves its reason in gfn_last_error()."""
    E = _lib.ERR_INVALID_ARG
    assert qkv(C=32) == E and "C must be 64" in last_error() and "32" in last_error()
    assert post(C=32) == E and "C must be 64" in last_error()
    assert post(hidden=128) == E and "hidden width must be 256" in last_error() and "128" in last_error()
    assert qkv(B2=3) == E and "even" in last_error()
    assert qkv(N=0) == E and "bad size" in last_error()
    assert qkv(B2=-2) == E and post(rows=-1) == E
    assert qkv(B2=2 ** 16, N=2 ** 15) == E and "2^31" in last_error()


def test_null_and_misaligned_pointers_are_refused_naming_the_argument():
    E = _lib.ERR_INVALID_ARG
    names = ["x", "norm_weight", "norm_bias", "wq", "wk", "wv", "q", "k", "v"]
    for i, name in enumerate(names):
        assert qkv(ptrs=[None if j == i else P for j in range(9)]) == E
        assert "null pointer" in last_error() and f"({name})" in last_error()
    names = ["x", "attn", "wproj", "bproj", "gamma1", "norm_weight", "norm_bias", "w1", "b1", "w2", "b2", "gamma2", "x_out"]
    for i, name in enumerate(names):
        assert post(ptrs=[None if j == i else P for j in range(13)]) == E
        assert "null pointer" in last_error() and f"({name})" in last_error()
    off = ctypes.c_void_p(P.value + 4)
    assert qkv(ptrs=[off] + [P] * 8) == E and "16-byte aligned" in last_error()
    assert post(ptrs=[P] * 12 + [off]) == E and "x_out" in last_error()


def test_an_empty_batch_is_ok_without_a_launch():
    """A batch of 0 returns GFN_OK before the pointers are looked at and before any HIP call."""
    assert qkv(B2=0, ptrs=[None] * 9) == _lib.OK
    assert post(rows=0, ptrs=[None] * 13) == _lib.OK


def block_args():
    C, Hd = ops.DECODER_DIM, ops.DECODER_HIDDEN
    z = torch.zeros
    return dict(X=z(2, 5, C), attn=z(2, 5, 8, 8, dtype=torch.float16), wproj=z(C, C), bproj=z(C), gamma1=z(C), norm_weight=z(C), norm_bias=z(C),
                eps=1e-5, w1=z(Hd, C), b1=z(Hd), w2=z(C, Hd), b2=z(C), gamma2=z(C))


def test_cpu_tensors_raise():
    a = block_args()
    with pytest.raises(_lib.GfnError, match="no CPU path"):
        ops.decoder_qkv(a["X"], a["norm_weight"], a["norm_bias"], 1e-5, a["wproj"], a["wproj"], a["wproj"])
    with pytest.raises(_lib.GfnError, match="no CPU path"):
        ops.decoder_post(**a)


def test_block_impl_is_checked_at_construction():
    conf = load_golden()[0]
    with pytest.raises(ValueError, match="block_impl"):
        CrossViewDecoder(conf, block_impl="flash")
    assert CrossViewDecoder(conf).block_impl == "torch"  # the default: every existing construction is what it was
    assert CrossViewDecoder(conf, attn_impl="torch", block_impl="hip").block_impl == "hip"


def test_block_impl_hip_on_the_cpu_is_the_torch_path_and_reproduces_the_reference_modules_maps():
    """Off the GPU block_impl="hip" runs the torch blocks: against the golden maps within the existing CPU bound (4 x the reference
    module's own fp32-vs-float64 difference), and bit for bit what block_impl="torch" gives."""
    conf, state, x, y, outs, (B, H, W), e32 = load_golden()
    maps = {}
    for impl in ("hip", "torch"):
        dec = CrossViewDecoder(conf, attn_impl="torch", block_impl=impl)
        dec.load_state_dict(state, strict=True)
        with torch.no_grad():
            maps[impl] = dec.train(False)(x, y, vit_shape=(B, 3, H, W))
    assert 1e-7 < e32 < 1e-4
    for name, a, t, b in zip("xy", maps["hip"], maps["torch"], outs):
        err = float((a - b).abs().max())
        print(f"map {name}: max err {err:.3e}, bound {4 * e32:.3e}")
        assert err <= 4 * e32, (name, err, 4 * e32)
        assert torch.equal(a, t)


# a stand-in checkout WITHOUT the decoder module: decoder="hip_fused" must not ask for it
STANDIN_FPN = """
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
"""

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
"""


def _child(code, tmp_path, env=None):
    root = tmp_path / "checkout"
    (root / "model").mkdir(parents=True)
    (root / "model" / "__init__.py").write_text("")
    (root / "model" / "FPN.py").write_text(STANDIN_FPN)
    e = dict(os.environ)
    for k in ("GFNET_COMPAT_BACKBONE", "GFNET_COMPAT_DECODER", "GFNET_COMPAT_FPN", "GFNET_COMPAT_DINO"):
        e.pop(k, None)
    e["PYTHONPATH"] = os.pathsep.join([os.path.join(ROOT, "compat"), ROOT, str(root)])
    e["GFNET_TEST_GOLDEN"] = GOLDEN
    e.update(env or {})
    script = tmp_path / "child.py"
    script.write_text(CHILD + textwrap.dedent(code))
    r = subprocess.run([sys.executable, str(script)], env=e, capture_output=True, text=True, cwd="/", timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip().endswith("ok")


def test_wiring_decoder_hip_fused_builds_the_native_decoder_with_fused_blocks_without_the_checkouts(tmp_path):
    _child("""
    assert compat.checkout_available("hip_fused") and not compat.checkout_available()
    bb = compat.reference_backbone(conf, vit=vit, decoder="hip_fused")
    assert type(bb.dino_decoder) is CrossViewDecoder
    assert bb.dino_decoder.block_impl == "hip" and bb.dino_decoder.attn_impl == "hip"
    assert "model.crossview_decoder_light" not in sys.modules
    assert {k for k in bb.state_dict() if k.startswith("dino_decoder.")} == golden_keys
    # "hip" keeps its meaning
    assert compat.reference_backbone(conf, vit=vit, decoder="hip").dino_decoder.block_impl == "torch"
    print("ok")
    """, tmp_path)


def test_wiring_environment_switch_selects_the_fused_blocks(tmp_path):
    _child("""
    import gfnet_amd.reference_backbone as rb
    rb._build_vit = lambda w: vit
    from model.network import GFNet
    model = GFNet(conf=conf)
    assert type(model.backbone.dino_decoder) is CrossViewDecoder and model.backbone.dino_decoder.block_impl == "hip"
    assert "model.crossview_decoder_light" not in sys.modules
    print("ok")
    """, tmp_path, env={"GFNET_COMPAT_BACKBONE": "reference", "GFNET_COMPAT_DECODER": "hip_fused"})
