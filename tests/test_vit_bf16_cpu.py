"""The bf16 class of the native DINOv2 ViT as far as it goes without a GPU: the op's name and its refusals, the header's words, the
C ABI's argument checks with GFN_BF16 (which return before any HIP call), and the CPU model, which stays on the torch path."""
import ctypes
import os
import re

import pytest
import torch

import vit_fixture
from conftest import ROOT
from gfnet_amd import _lib, ops
from gfnet_amd.model import dinov2

BF = torch.bfloat16


def test_self_attention_bf16_exists_and_refuses_cpu_tensors_as_self_attention_does():
    with pytest.raises(_lib.GfnError, match="no CPU path") as fp16:
        ops.self_attention(torch.zeros(1, 4, 3, 1, 64, dtype=torch.float16), 0.125)
    with pytest.raises(_lib.GfnError, match="no CPU path") as bf16:
        ops.self_attention_bf16(torch.zeros(1, 4, 3, 1, 64, dtype=BF), 0.125)
    assert str(bf16.value) == str(fp16.value)
    with pytest.raises(ValueError, match=r"self_attention_bf16: qkv \(B,N,3,H,D\)"):
        ops.self_attention_bf16(torch.zeros(1, 4, 1, 64, dtype=BF), 0.125)


def test_seam_refuses_cpu_bf16_tensors_for_the_device_not_for_the_dtype():
    x = torch.zeros(2, 64, dtype=BF)
    with pytest.raises(_lib.GfnError, match="no CPU path"):
        ops.ls_add_layernorm(x, x, x[0], x[0], x[0], 1e-6)
    assert "bfloat16" in ops.ls_add_layernorm.__doc__ or "bf16" in ops.ls_add_layernorm.__doc__


def _comment_before(header, name):
    """The comment block that precedes the prototype of `name`."""
    at = re.search(r"^int " + name + r"\(", header, re.M).start()
    start = header.rfind("/*", 0, at)
    assert header.find("*/", start) < at
    return header[start:at]


def test_header_names_bf16_at_both_entry_points():
    """gfn_self_attn_fwd takes GFN_BF16; gfn_ls_add_layernorm_fwd keeps refusing it and says where bf16 tensors go."""
    with open(os.path.join(ROOT, "include", "gfnet_hip.h")) as f:
        header = f.read()
    for name in ("gfn_self_attn_fwd", "gfn_ls_add_layernorm_fwd", "gfn_ls_add_layernorm_bf16_fwd"):
        assert "GFN_BF16" in _comment_before(header, name), name
    assert "gfn_ls_add_layernorm_bf16_fwd" in _comment_before(header, "gfn_ls_add_layernorm_fwd")
    assert "N * max|v|" in _comment_before(header, "gfn_self_attn_fwd")  # the documented limit of the bf16 accumulator


def test_abi_takes_bf16_through_the_same_argument_checks():
    """Argument errors return before any HIP call, so this runs without a GPU; the dummy pointers are never read.  Every call here
    is refused or empty: none launches."""
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p(ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16)
    E = _lib.ERR_INVALID_ARG

    def last():
        return L.gfn_last_error().decode()

    assert L.gfn_self_attn_fwd(p, _lib.GFN_BF16, 0, 32, 2, 64, 0.125, p, None) == _lib.OK  # an empty batch: accepted, nothing read
    assert L.gfn_self_attn_fwd(p, _lib.GFN_BF16, 1, 32, 2, 32, 0.125, p, None) == E and "head dim 32" in last()
    assert L.gfn_self_attn_fwd(None, _lib.GFN_BF16, 1, 32, 2, 64, 0.125, p, None) == E and "null pointer (qkv)" in last()
    assert L.gfn_self_attn_fwd(p, _lib.GFN_BF16, 1, 32, 2, 64, float("nan"), p, None) == E and "scale" in last()
    assert L.gfn_self_attn_fwd(p, _lib.GFN_F32, 1, 32, 2, 64, 0.125, p, None) == E and "GFN_F16 or GFN_BF16" in last()
    assert L.gfn_self_attn_fwd(p, 3, 1, 32, 2, 64, 0.125, p, None) == E and "dtype" in last()

    # the seam's bf16 class is an entry point of its own, without a dtype argument, with the fp16 one's checks under its own name
    vp, i, i64, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    assert _lib.PROTOTYPES["gfn_ls_add_layernorm_bf16_fwd"] == (i, [vp, vp, vp, vp, vp, f, i64, i, vp, vp, vp])
    assert "gfn_ls_add_layernorm_bf16_fwd" in _lib.STATUS_FUNCS and "gfn_ls_add_layernorm_bf16_fwd" in _lib.exported_symbols()

    def seam(x=p, rows=4, C=128, **kw):
        a = dict(y=p, gamma=p, weight=p, bias=p, eps=1e-6, x_out=p, h_out=None)
        a.update(kw)
        return L.gfn_ls_add_layernorm_bf16_fwd(x, a["y"], a["gamma"], a["weight"], a["bias"], a["eps"], rows, C, a["x_out"], a["h_out"], None)

    q = ctypes.c_void_p(p.value + 16)
    assert seam(rows=0) == _lib.OK and seam(rows=0, x=None, x_out=None) == _lib.OK
    for kwargs, text in [(dict(C=1020), "multiple of 8"), (dict(C=16384), "8192"), (dict(rows=-1), "rows"), (dict(eps=-1.0), "eps"),
                         (dict(x=None), "(x)"), (dict(gamma=None), "(gamma)"), (dict(h_out=q, weight=None), "(weight)"),
                         (dict(y=None, h_out=None), "nothing to compute"), (dict(h_out=p), "alias"),
                         (dict(x=ctypes.c_void_p(p.value + 2)), "aligned")]:
        assert seam(**kwargs) == E, kwargs
        assert text in last() and "gfn_ls_add_layernorm_bf16_fwd" in last(), (kwargs, last())
    # the entry point with a dtype keeps refusing GFN_BF16, and names this one
    assert L.gfn_ls_add_layernorm_fwd(p, p, p, p, p, 1e-6, _lib.GFN_BF16, 4, 128, p, None, None) == E
    assert "dtype" in last() and "gfn_ls_add_layernorm_bf16_fwd" in last()


def test_cpu_bf16_model_runs_the_torch_path_bit_for_bit(monkeypatch):
    def never(*a, **k):
        raise AssertionError("a HIP op was called for CPU tensors")

    monkeypatch.setattr(ops, "self_attention_bf16", never, raising=True)  # (raising: the name must exist)
    monkeypatch.setattr(ops, "self_attention", never)
    monkeypatch.setattr(ops, "ls_add_layernorm", never)
    models = {}
    for impl in dinov2.IMPLS:
        m = dinov2.DinoVisionTransformer(impl=impl, **vit_fixture.CONFIG)
        vit_fixture.fill(m)
        models[impl] = m.train(False).to(BF)
    x = vit_fixture.inputs("wide").to(BF)
    assert not models["hip"]._use_hip(x, None)
    assert torch.bfloat16 in dinov2.HIP_DTYPES and torch.float16 in dinov2.HIP_DTYPES and torch.float32 not in dinov2.HIP_DTYPES
    with torch.no_grad():
        got, ref = models["hip"].forward_features(x), models["torch"].forward_features(x)
    for o in vit_fixture.OUTPUTS + ("x_prenorm",):
        assert got[o].dtype == BF and torch.isfinite(got[o]).all() and torch.equal(got[o], ref[o]), o
