"""The cross-view decoder's bf16 class (GFN_BF16 in csrc/cross_attn.hip, the gfn_decoder_*_bf16_* entry points of
csrc/decoder_block.hip, ops.cross_attention_bf16, the decoder ops' dtype=torch.bfloat16, CrossViewDecoder under bf16 autocast) as
far as it goes without a GPU: the C ABI and its refusals, which return before anything is launched, the ops' refusal of CPU tensors,
the module's fallback off the GPU, and the calibration helpers tests/test_decoder_bf16_gpu.py takes its units from."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from gfnet_amd import _lib, ops
from gfnet_amd.model.crossview_decoder import CrossViewDecoder
from test_decoder_block_cpu import P, block_args, last_error, load_golden
from test_decoder_train_cpu import BIG_WS, POST_PTRS, QKV_PTRS, ws_bytes
from test_decoder_train_gpu import (C, EPS, POST_NAMES, POST_PARAMS, QKV_NAMES, QKV_PARAMS, definition_post, definition_qkv, leaves,
                                    params)

vp, i32, i64, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
NEW = ("gfn_decoder_qkv_bf16_fwd", "gfn_decoder_post_bf16_fwd", "gfn_decoder_qkv_bf16_bwd", "gfn_decoder_post_bf16_bwd")
FWD_QKV_PTRS = ["x", "norm_weight", "norm_bias", "wq", "wk", "wv", "q", "k", "v"]
FWD_POST_PTRS = ["x", "attn", "wproj", "bproj", "gamma1", "norm_weight", "norm_bias", "w1", "b1", "w2", "b2", "gamma2", "x_out"]


# ---- calibration helpers, shared with the GPU file ---------------------------------------------------------------------------------
def bf(t):
    """Rounded to what bfloat16 holds (to nearest even), in t's dtype."""
    return t.bfloat16().to(t.dtype)


def rbf(t):
    """bf16 rounding in float64 with the identity as its derivative"""
    return t + (t.detach().bfloat16().double() - t.detach())


def autocast_bf16(enabled=True):
    return torch.autocast(device_type="cpu", dtype=torch.bfloat16, enabled=enabled)


def post_grads(X, attn, p, G, dtype):
    """(forward, name -> gradient of sum(definition_post(X, attn, p) * G)), float64 tensors, evaluated in `dtype`: torch.float64, or
    torch.bfloat16 = fp32 tensors under CPU bf16 autocast (attn then as it is stored, bf16)."""
    wide = (lambda t: t.double()) if dtype == torch.float64 else (lambda t: t)
    X, G = wide(X).clone().requires_grad_(), wide(G)
    attn = (attn.double() if dtype == torch.float64 else attn).clone().requires_grad_()
    p = leaves(p, POST_PARAMS, wide)
    with autocast_bf16(dtype == torch.bfloat16):
        out = definition_post(X, attn, p)
        loss = (out * G).sum()
    grads = torch.autograd.grad(loss, [X, attn] + [getattr(p, k) for k in POST_PARAMS])
    return out.detach().double(), {k: g.double() for k, g in zip(POST_NAMES, grads)}


def qkv_grads(X, p, G, dtype):
    """((q, k', v'), name -> gradient of sum(q * Gq) + sum(k' * Gk) + sum(v' * Gv)), k' and v' at the other view's batch entry"""
    wide = (lambda t: t.double()) if dtype == torch.float64 else (lambda t: t)
    X, G = wide(X).clone().requires_grad_(), wide(G)
    p = leaves(p, QKV_PARAMS, wide)
    B = X.shape[0] // 2
    with autocast_bf16(dtype == torch.bfloat16):
        q, k, v = definition_qkv(X, p)
        k, v = k.roll(B, 0), v.roll(B, 0)
        loss = (q * G[1]).sum() + (k * G[2]).sum() + (v * G[3]).sum()
    grads = torch.autograd.grad(loss, [X] + [getattr(p, k) for k in QKV_PARAMS])
    return tuple(t.detach().double() for t in (q, k, v)), {k: g.double() for k, g in zip(QKV_NAMES, grads)}


def test_cpu_bf16_autocast_hands_back_bf16_at_the_projections_and_fp32_at_the_norms():
    """What the units of the GPU file stand on: under torch.autocast("cpu", dtype=torch.bfloat16) a Linear's output is bf16 (so the
    unit holds the roundings of the reference's class) and LayerNorm's is fp32; the helpers return float64 and the rounding helpers
    round to nearest even and keep NaN and inf."""
    p = params()
    X = torch.randn(2, 5, C, generator=torch.Generator().manual_seed(1))
    with autocast_bf16():
        q, k, v = definition_qkv(X, p)
        n = F.layer_norm(X, (C,), p.nw1, p.nb1, EPS)
        out = definition_post(X, torch.zeros(2, 5, 8, 8, dtype=torch.bfloat16), p)
    assert q.dtype == k.dtype == v.dtype == torch.bfloat16 and n.dtype == torch.float32 and out.dtype == torch.float32
    (q64, _, _), grads = qkv_grads(X, p, torch.ones(4, 2, 5, C), torch.bfloat16)
    assert q64.dtype == torch.float64 and torch.equal(q64, q.double()) and all(g.dtype == torch.float64 for g in grads.values())
    t = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 3e38, float("inf"), float("nan")])
    r = bf(t)
    assert r[0] == 1.0 and r[1] == 1.0 + 2.0 ** -6 and r[2] == bf(torch.tensor(3e38)) and torch.isinf(r[3]) and torch.isnan(r[4])  # ties to even
    assert torch.isfinite(r[2])  # 3e38 is far outside fp16 and inside bf16
    x = torch.tensor([1.0 + 2.0 ** -8], dtype=torch.float64, requires_grad=True)
    y = rbf(3 * x)
    assert float(y.detach()) == float(torch.tensor(3 * (1.0 + 2.0 ** -8)).bfloat16()) and float(torch.autograd.grad(y, x)[0]) == 3.0


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_abi_declares_the_four_entry_points_with_their_siblings_signatures():
    for kind in ("qkv", "post"):
        for d in ("fwd", "bwd"):
            assert _lib.PROTOTYPES[f"gfn_decoder_{kind}_bf16_{d}"] == _lib.PROTOTYPES[f"gfn_decoder_{kind}_{d}"]
    assert _lib.PROTOTYPES["gfn_decoder_qkv_bf16_fwd"] == (i32, [vp, vp, vp, f32, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp])
    assert _lib.PROTOTYPES["gfn_decoder_post_bf16_bwd"] == (i32, [vp] * 7 + [f32] + [vp] * 6 + [i64, i32, i32] + [vp] * 12 + [vp, i64, vp])
    assert set(NEW) <= _lib.STATUS_FUNCS and set(NEW) <= set(_lib.exported_symbols())
    L = ctypes.CDLL(_lib.LIB_PATH)  # the symbols are exported (loading the library needs no GPU)
    assert all(getattr(L, n) for n in NEW)
    assert _lib.GFN_BF16 == 2 and _lib.lib().gfn_abi_version() == 1


def qkv_fwd(B2=2, N=32, C=64, ptrs=None):
    p = [P] * 9 if ptrs is None else ptrs
    return _lib.lib().gfn_decoder_qkv_bf16_fwd(p[0], p[1], p[2], 1e-5, p[3], p[4], p[5], B2, N, C, p[6], p[7], p[8], None)


def post_fwd(rows=32, C=64, hidden=256, ptrs=None):
    p = [P] * 13 if ptrs is None else ptrs
    return _lib.lib().gfn_decoder_post_bf16_fwd(*p[:7], 1e-5, *p[7:12], rows, C, hidden, p[12], None)


def qkv_bwd(B2=2, N=32, C=64, ptrs=None, ws=BIG_WS):
    p = [P] * 16 if ptrs is None else ptrs
    return _lib.lib().gfn_decoder_qkv_bf16_bwd(p[0], p[1], p[2], 1e-5, *p[3:9], B2, N, C, *p[9:15], p[15], ws, None)


def post_bwd(rows=32, C=64, hidden=256, ptrs=None, ws=BIG_WS):
    p = [P] * 26 if ptrs is None else ptrs
    return _lib.lib().gfn_decoder_post_bf16_bwd(*p[:7], 1e-5, *p[7:13], rows, C, hidden, *p[13:25], p[25], ws, None)


CALLS = ((qkv_fwd, FWD_QKV_PTRS, "gfn_decoder_qkv_bf16_fwd"), (post_fwd, FWD_POST_PTRS, "gfn_decoder_post_bf16_fwd"),
         (qkv_bwd, QKV_PTRS, "gfn_decoder_qkv_bf16_bwd"), (post_bwd, POST_PTRS, "gfn_decoder_post_bf16_bwd"))


def test_unsupported_sizes_are_refused_before_anything_is_launched_under_the_bf16_names():
    E = _lib.ERR_INVALID_ARG
    for call, _, name in CALLS:
        assert call(C=32) == E and "C must be 64" in last_error() and "32" in last_error() and name in last_error()
    for call in (post_fwd, post_bwd):
        assert call(hidden=128) == E and "hidden width must be 256" in last_error() and "128" in last_error()
        assert call(rows=-1) == E
    for call in (qkv_fwd, qkv_bwd):
        assert call(B2=3) == E and "even" in last_error()
        assert call(N=0) == E and "bad size" in last_error()
        assert call(B2=-2) == E
        assert call(B2=2 ** 16, N=2 ** 15) == E and "2^31" in last_error()


def test_null_and_misaligned_pointers_are_refused_naming_the_argument():
    E = _lib.ERR_INVALID_ARG
    off = ctypes.c_void_p(P.value + 4)
    for call, names, _ in CALLS:
        for i, name in enumerate(names):
            assert call(ptrs=[None if j == i else P for j in range(len(names))]) == E
            assert "null pointer" in last_error() and f"({name})" in last_error()
            assert call(ptrs=[off if j == i else P for j in range(len(names))]) == E
            assert "16-byte aligned" in last_error() and name in last_error()


def test_a_short_workspace_is_refused_and_one_size_serves_both_classes():
    E = _lib.ERR_INVALID_ARG
    for call, rows in ((lambda **k: qkv_bwd(B2=2, N=1024, **k), 2048), (lambda **k: post_bwd(rows=2048, **k), 2048)):
        assert call(ws=ws_bytes(rows) - 1) == E and "ws_bytes" in last_error() and "too small" in last_error()
        assert str(ws_bytes(rows)) in last_error()
        assert call(ws=0) == E


def test_an_empty_problem_is_ok_without_a_launch():
    assert qkv_fwd(B2=0, ptrs=[None] * 9) == _lib.OK and post_fwd(rows=0, ptrs=[None] * 13) == _lib.OK
    assert qkv_bwd(B2=0, ptrs=[None] * 16, ws=0) == _lib.OK and post_bwd(rows=0, ptrs=[None] * 26, ws=0) == _lib.OK


def test_cross_attn_takes_the_bf16_code_and_still_refuses_other_head_dims_and_codes():
    L = _lib.lib()
    E = _lib.ERR_INVALID_ARG
    assert L.gfn_cross_attn_fwd(None, None, None, _lib.GFN_BF16, 1, 32, 32, 8, 16, 1.0, None, None, None) == E
    assert "head dim" in last_error() and "16" in last_error() and "dtype" not in last_error()
    assert L.gfn_cross_attn_bwd(None, None, None, None, None, None, _lib.GFN_BF16, 1, 32, 32, 8, 16, 1.0, None, None, None, None) == E
    assert "head dim" in last_error()
    # D = 8 with the bf16 code gets past the dtype check: what is refused next is the null pointer
    assert L.gfn_cross_attn_fwd(None, None, None, _lib.GFN_BF16, 1, 32, 32, 8, 8, 1.0, None, None, None) == E and "null pointer" in last_error()
    assert L.gfn_cross_attn_bwd(None, None, None, None, None, None, _lib.GFN_BF16, 1, 32, 32, 8, 8, 1.0, None, None, None, None) == E
    assert "null pointer" in last_error()
    assert L.gfn_cross_attn_fwd(None, None, None, _lib.GFN_BF16, 0, 32, 32, 8, 8, 1.0, None, None, None) == _lib.OK  # empty
    for code in (3, 7, -1):
        assert L.gfn_cross_attn_fwd(None, None, None, code, 1, 32, 32, 8, 8, 1.0, None, None, None) == E and "dtype" in last_error()


# ---- the ops -----------------------------------------------------------------------------------------------------------------------
def test_the_new_ops_refuse_cpu_tensors():
    q = torch.randn(1, 4, 2, 8).bfloat16()
    with pytest.raises(_lib.GfnError, match="no CPU path"):
        ops.cross_attention_bf16(q, q, q, 0.5)
    with pytest.raises(_lib.GfnError, match="no CPU path"):
        ops.cross_attention_bf16(q.clone().requires_grad_(), q, q, 0.5)
    with pytest.raises(_lib.GfnError, match="no CPU path"):
        ops.cross_attention_bf16_fwd(q, q, q, 0.5)
    with pytest.raises(_lib.GfnError, match="no CPU path"):
        ops.cross_attention_bf16_bwd(q, q, q, q, torch.zeros(1, 2, 4), q, 0.5)
    a = block_args()
    a["attn"] = a["attn"].bfloat16()
    g = torch.zeros(2, 5, 8, 8, dtype=torch.bfloat16)
    qkv = (a["X"], a["norm_weight"], a["norm_bias"], 1e-5, a["wproj"], a["wproj"], a["wproj"])
    for call in (lambda: ops.decoder_qkv(*qkv, dtype=torch.bfloat16), lambda: ops.decoder_post(**a, dtype=torch.bfloat16),
                 lambda: ops.decoder_qkv_bwd(*qkv, g, g, g, dtype=torch.bfloat16),
                 lambda: ops.decoder_post_bwd(**a, gX_out=torch.zeros_like(a["X"]), dtype=torch.bfloat16),
                 lambda: ops.decoder_qkv_train(*qkv, dtype=torch.bfloat16), lambda: ops.decoder_post_train(**a, dtype=torch.bfloat16)):
        with pytest.raises(_lib.GfnError, match="no CPU path"):
            call()


def test_a_dtype_that_is_no_class_is_a_type_error():
    a = block_args()
    qkv = (a["X"], a["norm_weight"], a["norm_bias"], 1e-5, a["wproj"], a["wproj"], a["wproj"])
    for call in (lambda: ops.decoder_qkv(*qkv, dtype=torch.float32), lambda: ops.decoder_post(**a, dtype=torch.float64),
                 lambda: ops.decoder_qkv_train(*qkv, dtype=torch.float32), lambda: ops.decoder_post_train(**a, dtype=torch.int16)):
        with pytest.raises(TypeError, match="float16 or torch.bfloat16"):
            call()


# ---- the module --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("amp", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_on_the_cpu_under_autocast_the_module_falls_back_the_same_way_in_both_classes(amp):
    """CPU tensors under CPU autocast: neither kernel class is taken, whatever the switches say; with the torch attention the fused
    switches give the torch blocks' maps bit for bit, and with attn_impl="hip" the attention op refuses the CPU tensors under its own
    name (not with a dtype error)."""
    conf, state, x, y, _, (B, H, W), _ = load_golden()
    shape = (B, 3, H, W)
    maps = {}
    for impl in ("hip", "torch"):
        dec = CrossViewDecoder(conf, attn_impl="torch", block_impl=impl, train_block_impl=impl)
        dec.load_state_dict(state, strict=True)
        dec.train(False)
        with torch.no_grad(), torch.autocast(device_type="cpu", dtype=amp):
            assert not dec._fused(x, y) and not dec._train_fused(x, y)
            maps[impl] = dec(x, y, vit_shape=shape)
    for a, b in zip(maps["hip"], maps["torch"]):
        assert a.dtype == torch.float32 and torch.isfinite(a).all() and torch.equal(a, b)
    dec = CrossViewDecoder(conf, attn_impl="hip", block_impl="hip", train_block_impl="hip")
    dec.load_state_dict(state, strict=True)
    for mode in (False, True):
        dec.train(mode)
        with torch.autocast(device_type="cpu", dtype=amp):
            assert not dec._fused(x, y) and not dec._train_fused(x, y)
            with pytest.raises(_lib.GfnError, match="no CPU path"):
                dec(x, y, vit_shape=shape)
