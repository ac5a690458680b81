"""Thin Python bindings of the C-ABI entry points (include/gfnet_hip.h) on torch device tensors.

Each function cites the reference code it stands in for (paths relative to KN-Zhang/GFNet).
torch supplies device memory and the current HIP stream; every result comes from csrc/*.hip.
There is no CPU implementation here: CPU tensors raise.
"""
import collections
import functools
import math

import numpy as np
import torch

from . import _lib
from ._lib import c_vp, f32c, featc, ptr, require_gpu, stream_ptr

_L = _lib.checked  # every status-returning entry point raises GfnError by itself, under its own name


# bench.py sets this to a dict {name: [(start_event, end_event), ...]} to time individual launches
# with HIP events on the launch stream; None (the default) costs nothing.
kernel_events = None
# bench.py / tools set this to a dict to collect, per local-correlation call (name -> [(tiles left to the second launch,
# cells redone per tap, tiles staged in halves), ...]), the counters the kernels leave in the scratch header; costs a device sync per call.
kernel_counters = None
# the kernels read fp16 feature maps directly (BASELINE config 5): no widened copy is made
NATIVE_FP16 = True
# Large windows (r >= 5 on 64-channel maps) multiply on the matrix core with split-bf16 operands by default: every product is exact to
# 2^-17 relative, so a correlation value is within 2^-17 * sum_c |f0_c * f1_c| / sqrt(C) of the fp32 result (a few 1e-6 on unit-scale
# features, but proportional to the operands' magnitude, not to the result's: strongly cancelling sums lose relative accuracy).
# True keeps every radius on the fp32 FMA kernels (C-ABI variant 4), bit-identical to the round-1 kernel.
LOCAL_CORR_FP32 = False
# refiner_input writes the tile plan of the local correlation that follows it from extra workgroups of its own launch.  bench.py
# switches this off for a few untimed steps so that the plan becomes the correlation call's own first launch and lands inside its
# event bracket (`roofline.frac_incl_plan`).
FUSE_PLAN = True


def _timed(name, launch):
    if kernel_events is None or name not in kernel_events:
        return launch()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = launch()
    e1.record()
    kernel_events[name].append((e0, e1))
    return r


def corr_softargmax(feat0, feat1, symmetric=False):
    """pos_embed(corr_volume(feat0, feat1)) without writing the volume (model/network.py:251-252, 415-440).
    feat0 (B,C,H0,W0), feat1 (B,C,H1,W1) -> flow (B,2,H0,W0).  symmetric=True: the result has 2B
    directions, (feat0 vs feat1) then (feat1 vs feat0) -- the reference's concatenated batch
    (network.py:213-222) without copying the features.  With grad mode on and a map that requires grad, the flow is
    differentiable (gfn_corr_softargmax_bwd); every other call is the plain launch."""
    if torch.is_grad_enabled() and (feat0.requires_grad or feat1.requires_grad):
        return _CorrSoftargmaxFn.apply(feat0, feat1, symmetric)
    return _corr_softargmax(feat0, feat1, symmetric)[0]


def _corr_softargmax(feat0, feat1, symmetric):
    """The forward launch; returns (flow, f0, f1, dtype code) with the maps as the kernel read them."""
    dev = require_gpu(feat0, feat1)
    (f0, dt0), (f1, dt1) = featc(feat0), featc(feat1)
    if dt0 != dt1:
        f0, f1, dt0 = f32c(f0), f32c(f1), _lib.GFN_F32
    B, C, H0, W0 = f0.shape
    B1, C1, H1, W1 = f1.shape
    if B1 != B or C1 != C:
        raise ValueError("feat0/feat1 batch or channel mismatch")
    nb = 2 * B if symmetric else B
    flow = torch.empty((nb, 2, H0, W0), device=dev, dtype=torch.float32)
    # workspace of the split-bf16 path (64-channel maps): the caller owns every buffer (include/gfnet_hip.h); a fresh tensor per call
    # (the caching allocator hands the same block back; not the per-stream scratch, whose header the local correlation keeps zeroed)
    nws = int(_L().gfn_corr_softargmax_ws_bytes(nb, C, H1, W1))
    ws = torch.empty(nws, device=dev, dtype=torch.uint8) if nws > 0 else None
    _L().gfn_corr_softargmax_fwd_ws(ptr(f0), ptr(f1), dt0, ptr(flow), nb, C, H0, W0, H1, W1, 1 if symmetric else 0,
                                    ptr(ws), nws, stream_ptr(dev))
    return flow, f0, f1, dt0


def corr_softargmax_bwd(f0, f1, flow, grad_flow, symmetric=False, need_f0=True, need_f1=True):
    """Gradients of corr_softargmax's flow with respect to f0 and f1 (fp32, None where not asked for) given grad_flow = dL/dflow:
    the backward of the reference's pos_embed(corr_volume(f0, f1)) (model/network.py:415-440) without the volume or its gradient
    (csrc/corr_softargmax_bwd.hip).  f0 / f1 as the forward read them (fp32 or fp16, same dtype), flow its output."""
    dev = require_gpu(f0, f1, flow, grad_flow)
    (a, dt0), (b, dt1) = featc(f0), featc(f1)
    if dt0 != dt1:
        a, b, dt0 = f32c(a), f32c(b), _lib.GFN_F32
    B, C, H0, W0 = a.shape
    _, _, H1, W1 = b.shape
    nb = 2 * B if symmetric else B
    fl, g = f32c(flow), f32c(grad_flow)
    if tuple(fl.shape) != (nb, 2, H0, W0) or tuple(g.shape) != (nb, 2, H0, W0):
        raise ValueError("corr_softargmax_bwd: flow / grad_flow must be (B,2,H0,W0) of the forward")
    g0 = torch.empty(a.shape, device=dev, dtype=torch.float32) if need_f0 else None
    g1 = torch.empty(b.shape, device=dev, dtype=torch.float32) if need_f1 else None
    nws = int(_L().gfn_corr_softargmax_bwd_ws_bytes(nb, C, H0, W0, H1, W1))
    ws = torch.empty(nws, device=dev, dtype=torch.uint8) if nws > 0 else None
    _L().gfn_corr_softargmax_bwd(ptr(a), ptr(b), dt0, ptr(fl), ptr(g), ptr(g0), ptr(g1), nb, C, H0, W0, H1, W1,
                                 1 if symmetric else 0, ptr(ws), nws, stream_ptr(dev))
    return g0, g1


class _CorrSoftargmaxFn(torch.autograd.Function):
    """corr_softargmax with a backward: the same launch forward (same bits), gfn_corr_softargmax_bwd backward."""

    @staticmethod
    def forward(ctx, feat0, feat1, symmetric):
        flow, f0, f1, _ = _corr_softargmax(feat0, feat1, symmetric)
        ctx.save_for_backward(f0, f1, flow)
        ctx.symmetric = symmetric
        ctx.dtypes = (feat0.dtype, feat1.dtype)
        return flow

    @staticmethod
    def backward(ctx, grad_flow):
        f0, f1, flow = ctx.saved_tensors
        n0, n1 = ctx.needs_input_grad[:2]
        g0, g1 = corr_softargmax_bwd(f0, f1, flow, grad_flow, ctx.symmetric, need_f0=n0, need_f1=n1)
        return (g0.to(ctx.dtypes[0]) if g0 is not None else None, g1.to(ctx.dtypes[1]) if g1 is not None else None, None)


def reference_cross_attention(q, k, v, scale):
    """The definition cross_attention computes, in plain torch on any device and in any floating dtype (float64 included), for
    tests and for the decoder's attn_impl="torch": q (B,Nq,H,D), k, v (B,Nk,H,D) -> out (B,Nq,H,D) with, per batch and head,
    out = softmax_j(scale * q . k_j) v_j.  Differentiable through torch autograd.

    This restates the published definition of flash-attn's flash_attn_func(q, k, v, dropout_p=0, softmax_scale=scale, causal=False),
    which the reference calls at model/transformer/layers/attention.py:252; it is NOT pinned against flash_attn itself, which is
    absent here, as cv2 and kornia are for the stages that restate them."""
    s = torch.einsum("bihd,bjhd->bhij", q, k) * scale
    return torch.einsum("bhij,bjhd->bihd", torch.softmax(s, dim=-1), v)


_F16_F32 = (torch.float16, torch.float32)
_BF16 = (torch.bfloat16,)
_DTYPE_CODES = {torch.float16: _lib.GFN_F16, torch.bfloat16: _lib.GFN_BF16, torch.float32: _lib.GFN_F32}


def _attn_args(what, names, allowed, *tensors):
    """The tensors as the attention kernels read them (contiguous, 16-byte aligned, one dtype out of `allowed`) and the dtype code."""
    dev = require_gpu(*tensors)
    dtypes = sorted({str(t.dtype) for t in tensors})
    if len(dtypes) != 1 or tensors[0].dtype not in allowed:
        want = " or ".join(str(d).replace("torch.", "") for d in allowed)
        if len(tensors) == 1:
            raise TypeError(f"{what}: {names} must be {want}, got {dtypes[0]}")
        raise TypeError(f"{what}: {names} must share one dtype, {want}, got {dtypes}")
    out = []
    for t in tensors:
        t = t.contiguous()
        out.append(t.clone() if t.data_ptr() % 16 else t)
    return dev, out, _DTYPE_CODES[tensors[0].dtype]


def cross_attention_fwd(q, k, v, scale, allowed=_F16_F32):
    """The forward launch (gfn_cross_attn_fwd): returns (out, lse, q, k, v) with q, k, v as the kernel read them; lse (B,H,Nq) fp32.
    `allowed`: the dtypes this name takes (cross_attention_bf16_fwd is this function with bfloat16 alone)."""
    if q.dim() != 4 or k.dim() != 4 or k.shape != v.shape or q.shape[0] != k.shape[0] or q.shape[2:] != k.shape[2:]:
        raise ValueError(f"cross_attention: q (B,Nq,H,D) and k, v (B,Nk,H,D) expected, got {tuple(q.shape)}, {tuple(k.shape)}, {tuple(v.shape)}")
    dev, (q, k, v), dt = _attn_args("cross_attention", "q, k and v", allowed, q, k, v)
    B, Nq, H, D = q.shape
    Nk = k.shape[1]
    out = torch.empty_like(q)
    lse = torch.empty((B, H, Nq), device=dev, dtype=torch.float32)
    _timed("cross_attn_fwd", lambda: _L().gfn_cross_attn_fwd(ptr(q), ptr(k), ptr(v), dt, B, Nq, Nk, H, D, float(scale), ptr(out), ptr(lse),
                                                             stream_ptr(dev)))
    return out, lse, q, k, v


def cross_attention_bwd(q, k, v, out, lse, dout, scale, allowed=_F16_F32):
    """(dq, dk, dv) of cross_attention given dout = dL/dout and the forward's out and lse (gfn_cross_attn_bwd): no atomics, so two
    calls give the same bits; in fp16 the results are rounded once and overflow to inf.  `allowed` as in cross_attention_fwd."""
    dev, (q, k, v, out, dout), dt = _attn_args("cross_attention_bwd", "q, k and v", allowed, q, k, v, out, dout)
    B, Nq, H, D = q.shape
    Nk = k.shape[1]
    if dout.shape != q.shape or out.shape != q.shape or tuple(lse.shape) != (B, H, Nq):
        raise ValueError("cross_attention_bwd: out and dout must have q's shape and lse must be (B,H,Nq) of the forward")
    lse = f32c(lse)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    _timed("cross_attn_bwd", lambda: _L().gfn_cross_attn_bwd(ptr(q), ptr(k), ptr(v), ptr(out), ptr(lse), ptr(dout), dt, B, Nq, Nk, H, D,
                                                             float(scale), ptr(dq), ptr(dk), ptr(dv), stream_ptr(dev)))
    return dq, dk, dv


class _CrossAttentionFn(torch.autograd.Function):
    """cross_attention with a backward; saves q, k, v, out and lse, never the Nq x Nk matrix."""

    @staticmethod
    def forward(ctx, q, k, v, scale, allowed=_F16_F32):
        out, lse, q, k, v = cross_attention_fwd(q, k, v, scale, allowed)
        ctx.save_for_backward(q, k, v, out, lse)
        ctx.scale, ctx.allowed = scale, allowed
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, out, lse = ctx.saved_tensors
        dq, dk, dv = cross_attention_bwd(q, k, v, out, lse, dout.to(q.dtype), ctx.scale, ctx.allowed)
        return dq, dk, dv, None, None


def cross_attention(q, k, v, scale, _allowed=_F16_F32):
    """The attention core of the reference's CrossFlashAttention2 (model/transformer/layers/attention.py:252, flash_attn_func with
    dropout 0 and causal=False) at head dim 8: q (B,Nq,H,8), k, v (B,Nk,H,8), fp16 or fp32 -> out of q's shape and dtype =
    softmax(scale * q k^T) v per batch and head.  Differentiable (gfn_cross_attn_bwd).  CPU tensors raise: reference_cross_attention
    is the definition for every device, this is the product path.  bf16 tensors are refused here and taken by cross_attention_bf16."""
    if torch.is_grad_enabled() and (q.requires_grad or k.requires_grad or v.requires_grad):
        return _CrossAttentionFn.apply(q, k, v, float(scale), _allowed)
    return cross_attention_fwd(q, k, v, scale, _allowed)[0]


def cross_attention_bf16(q, k, v, scale):
    """cross_attention for the bf16 autocast class: q (B,Nq,H,8), k, v (B,Nk,H,8) bfloat16 -> out bfloat16, the same kernels on
    v_mfma_f32_32x32x8_bf16 (gfn_cross_attn_fwd / _bwd with GFN_BF16).  Softmax, lse, P and dS are fp32 as in the fp16 class; results
    are rounded to bf16 to nearest even once, and with fp32's exponent range nothing overflows or is clamped.  Differentiable; any
    other dtype raises TypeError."""
    return cross_attention(q, k, v, scale, _BF16)


def cross_attention_bf16_fwd(q, k, v, scale):
    """cross_attention_fwd for bfloat16 q, k, v: (out, lse, q, k, v)."""
    return cross_attention_fwd(q, k, v, scale, _BF16)


def cross_attention_bf16_bwd(q, k, v, out, lse, dout, scale):
    """cross_attention_bwd for bfloat16 tensors: (dq, dk, dv) in bfloat16, rounded once."""
    return cross_attention_bwd(q, k, v, out, lse, dout, scale, _BF16)


def reference_self_attention(qkv, scale):
    """The definition self_attention computes, in plain torch on any device and in any floating dtype (float64 included), for tests:
    qkv (B,N,3,H,D), the packed projection -> out (B,N,H,D) with, per batch and head, out_i = sum_j softmax_j(scale * q_i . k_j) v_j
    for q = qkv[:, :, 0], k = qkv[:, :, 1], v = qkv[:, :, 2].  It is what the reference's Attention.forward computes with
    F.scaled_dot_product_attention on the permuted tensors (model/transformer/layers/attention.py:79-97)."""
    q, k, v = qkv.unbind(2)
    return reference_cross_attention(q, k, v, scale)


def _self_attention(what, allowed, qkv, scale):
    """The one body of self_attention and self_attention_bf16 (gfn_self_attn_fwd): `allowed` is the dtype the name `what` takes."""
    if qkv.dim() != 5 or qkv.shape[2] != 3:
        raise ValueError(f"{what}: qkv (B,N,3,H,D) expected, got {tuple(qkv.shape)}")
    dev, (qkv,), dt = _attn_args(what, "qkv", allowed, qkv)
    B, N, _, H, D = qkv.shape
    out = torch.empty((B, N, H, D), device=dev, dtype=qkv.dtype)
    _timed("self_attn_fwd", lambda: _L().gfn_self_attn_fwd(ptr(qkv), dt, B, N, H, D, float(scale), ptr(out), stream_ptr(dev)))
    return out


def self_attention(qkv, scale):
    """The attention core of the reference's ViT (model/transformer/layers/attention.py:96, F.scaled_dot_product_attention) at head
    dim 64 on the packed projection: qkv (B,N,3,H,64) fp16, as `self.qkv(x).reshape(B, N, 3, H, C // H)` gives it -> out
    (B,N,H,64) fp16 = softmax(scale * q k^T) v per batch and head, so `out.reshape(B, N, C)` feeds proj (gfn_self_attn_fwd: one
    launch, nothing N x N written).  Forward only, no autograd.  CPU tensors raise: reference_self_attention is the definition for
    every device, this is the product path.  bf16 tensors are refused here and taken by self_attention_bf16."""
    return _self_attention("self_attention", (torch.float16,), qkv, scale)


def self_attention_bf16(qkv, scale):
    """self_attention for the bf16 autocast class: qkv (B,N,3,H,64) bfloat16 -> out (B,N,H,64) bfloat16, the same kernel on
    v_mfma_f32_32x32x16_bf16 (gfn_self_attn_fwd with GFN_BF16).  Scores, maximum, exp2 and the row sum are fp32 as in the fp16 class;
    P and the results are rounded to bf16 to nearest even once each.  With fp32's exponent range nothing overflows on the way out and
    nothing is clamped; results are finite where N * max|v| is below fp32's largest value.  Any other dtype raises TypeError; CPU
    tensors raise."""
    return _self_attention("self_attention_bf16", _BF16, qkv, scale)


def ls_add_layernorm(x, y, gamma, weight, bias, eps, inplace=False):
    """The seam of a ViT block in one launch (gfn_ls_add_layernorm_fwd, for bfloat16 gfn_ls_add_layernorm_bf16_fwd; reference model/transformer/layers/block.py:83-106):

        x_out = x + gamma * y          h = LayerNorm(x_out) * weight + bias over the last dim, from x_out as stored

    x, y (..., C) of one shape, gamma, weight, bias (C), all fp16, all bf16 or all fp32, C a multiple of 8 up to 8192.  y None: the plain
    LayerNorm of x (gamma is not read).  weight None: only the residual update (bias and eps are not read).  inplace=True writes
    x_out into x (which must then be contiguous).  Returns (x_out, h): x itself where y is None, h None where weight is None.
    Contiguous CUDA tensors, the current stream, no autograd."""
    tensors = {"x": x, "y": y, "gamma": gamma if y is not None else None, "weight": weight, "bias": bias if weight is not None else None}
    dev = require_gpu(*tensors.values())
    if x.dtype not in _DTYPE_CODES or any(t is not None and t.dtype != x.dtype for t in tensors.values()):
        raise TypeError("ls_add_layernorm: every tensor must share one dtype, float16, bfloat16 or float32, got "
                        f"{ {n: str(t.dtype) for n, t in tensors.items() if t is not None} }")
    if y is None and weight is None:
        raise ValueError("ls_add_layernorm: nothing to compute (y and weight are both None)")
    C = x.shape[-1]
    if y is not None and (y.shape != x.shape or gamma is None or tuple(gamma.shape) != (C,)):
        raise ValueError(f"ls_add_layernorm: y must have x's shape {tuple(x.shape)} and gamma must be ({C},)")
    if weight is not None and (bias is None or tuple(weight.shape) != (C,) or tuple(bias.shape) != (C,)):
        raise ValueError(f"ls_add_layernorm: weight and bias must be ({C},)")
    if inplace and y is not None and not x.is_contiguous():
        raise ValueError("ls_add_layernorm: inplace=True needs a contiguous x")
    x, y, gamma, weight, bias = (None if t is None else t.detach().contiguous() for t in (x, y, tensors["gamma"], weight, tensors["bias"]))
    x_out = None if y is None else (x if inplace else torch.empty_like(x))
    h = None if weight is None else torch.empty_like(x)
    rows = x.numel() // C if C else 0
    head = (ptr(x), ptr(y), ptr(gamma), ptr(weight), ptr(bias), float(eps))
    tail = (rows, C, ptr(x_out), ptr(h), stream_ptr(dev))
    if x.dtype == torch.bfloat16:  # the bf16 class is an entry point of its own, named for it
        _timed("ls_add_layernorm", lambda: _L().gfn_ls_add_layernorm_bf16_fwd(*head, *tail))
    else:
        _timed("ls_add_layernorm", lambda: _L().gfn_ls_add_layernorm_fwd(*head, _DTYPE_CODES[x.dtype], *tail))
    return (x if y is None else x_out), h


DECODER_DIM, DECODER_HIDDEN = 64, 256  # the width and hidden width decoder_qkv and decoder_post are built for (8 heads of 8)


def _decoder_args(what, tensors, shapes, forward_only=True):
    """The named tensors as the decoder-block kernels read them: CUDA, contiguous, the dtype and shape listed in `shapes`
    (name -> (dtype, shape)), 16-byte aligned (a misaligned parameter view is copied); no autograd.  forward_only=False (the
    backward ops, which are what autograd calls) leaves out the refusal of tensors that require grad."""
    dev = require_gpu(*tensors.values())
    out = {}
    for name, t in tensors.items():
        dtype, shape = shapes[name]
        if t.dtype != dtype:
            raise TypeError(f"{what}: {name} must be {str(dtype).replace('torch.', '')}, got {str(t.dtype).replace('torch.', '')}")
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{what}: {name} must be {tuple(shape)}, got {tuple(t.shape)}")
        if not t.is_contiguous():
            raise ValueError(f"{what}: {name} must be contiguous")
        if forward_only and torch.is_grad_enabled() and t.requires_grad:
            raise RuntimeError(f"{what}: {name} requires grad, and this op is forward only (inference; call it under torch.no_grad())")
        t = t.detach()
        out[name] = t.clone() if t.data_ptr() % 16 else t
    return dev, out


_DECODER_CLASSES = {torch.float16: "", torch.bfloat16: "_bf16"}  # the element of a decoder-block class -> its entry points' infix


def _decoder_entry(what, stem, direction, dtype):
    """gfn_decoder_<stem>[_bf16]_<direction> of the class whose 16-bit tensors are `dtype`; any other dtype is a TypeError."""
    if dtype not in _DECODER_CLASSES:
        raise TypeError(f"{what}: dtype must be torch.float16 or torch.bfloat16 (the two classes the blocks are built in), got {dtype}")
    return getattr(_L(), f"gfn_decoder_{stem}{_DECODER_CLASSES[dtype]}_{direction}")


def decoder_qkv(X, norm_weight, norm_bias, eps, wq, wk, wv, dtype=torch.float16):
    """What a cross-view decoder block does before its attention, in one launch (gfn_decoder_qkv_fwd; reference
    model/transformer/layers/block.py:327 and attention.py:236-238) in the fp16 autocast class:

        q = wq . fp16(LayerNorm(X))        k = wk . fp16(X)        v = wv . fp16(X)        each rounded to fp16 once

    X (2B, N, 64) fp32, the residual stream cat(x, y) of both views; norm_weight, norm_bias (64) and wq, wk, wv (64, 64) fp32 as the
    module stores them.  Returns q, k, v (2B, N, 8, 8) fp16 for ops.cross_attention, with k and v of batch entry b written at
    (b + B) mod 2B: every view's queries meet the OTHER view's keys, without the concatenated copy.  Contiguous CUDA tensors, the
    current stream, forward only: raises if grad mode is on and an input requires grad.

    dtype=torch.bfloat16 is the bf16 autocast class (gfn_decoder_qkv_bf16_fwd): read bf16 for fp16 above; q, k, v are bfloat16, for
    ops.cross_attention_bf16."""
    what, C = "decoder_qkv", DECODER_DIM
    entry = _decoder_entry(what, "qkv", "fwd", dtype)
    if X.dim() != 3 or X.shape[0] % 2 or X.shape[1] < 1:
        raise ValueError(f"{what}: X must be (2B, N, {C}) with an even batch and N >= 1, got {tuple(X.shape)}")
    f32 = torch.float32
    dev, t = _decoder_args(what, {"X": X, "norm_weight": norm_weight, "norm_bias": norm_bias, "wq": wq, "wk": wk, "wv": wv},
                           {"X": (f32, (X.shape[0], X.shape[1], C)), "norm_weight": (f32, (C,)), "norm_bias": (f32, (C,)),
                            "wq": (f32, (C, C)), "wk": (f32, (C, C)), "wv": (f32, (C, C))})
    B2, N = X.shape[:2]
    q, k, v = (torch.empty((B2, N, 8, C // 8), device=dev, dtype=dtype) for _ in range(3))
    _timed("decoder_qkv", lambda: entry(ptr(t["X"]), ptr(t["norm_weight"]), ptr(t["norm_bias"]), float(eps), ptr(t["wq"]), ptr(t["wk"]),
                                        ptr(t["wv"]), B2, N, C, ptr(q), ptr(k), ptr(v), stream_ptr(dev)))
    return q, k, v


def decoder_post(X, attn, wproj, bproj, gamma1, norm_weight, norm_bias, eps, w1, b1, w2, b2, gamma2, inplace=False, dtype=torch.float16):
    """What a cross-view decoder block does after its attention, in one launch (gfn_decoder_post_fwd; reference
    model/transformer/layers/attention.py:255, block.py:327-328, mlp.py, layer_scale.py) in the fp16 autocast class:

        x1    = X  + gamma1 * (wproj . attn + bproj)
        X_out = x1 + gamma2 * (w2 . fp16(GELU(w1 . fp16(LayerNorm(x1)) + b1)) + b2)          GELU in its exact erf form

    X (..., 64) fp32, attn of as many rows of 64 in fp16 (ops.cross_attention's (2B, N, 8, 8) output as it is); wproj (64, 64),
    w1 (256, 64), w2 (64, 256), bproj, gamma1, norm_weight, norm_bias, b2, gamma2 (64) and b1 (256) fp32 as the module stores them.
    Returns X_out, fp32 of X's shape; inplace=True writes it over X.  Contiguous CUDA tensors, the current stream, forward only:
    raises if grad mode is on and an input requires grad.

    dtype=torch.bfloat16 is the bf16 autocast class (gfn_decoder_post_bf16_fwd): read bf16 for fp16 above; attn must be bfloat16."""
    what, C, Hd = "decoder_post", DECODER_DIM, DECODER_HIDDEN
    entry = _decoder_entry(what, "post", "fwd", dtype)
    if X.dim() < 1 or X.shape[-1] != C:
        raise ValueError(f"{what}: X must be (..., {C}), got {tuple(X.shape)}")
    if attn.numel() != X.numel():
        raise ValueError(f"{what}: attn must hold X's {X.numel() // C} rows of {C}, got {tuple(attn.shape)}")
    f32 = torch.float32
    vec = (f32, (C,))
    dev, t = _decoder_args(what, {"X": X, "attn": attn, "wproj": wproj, "bproj": bproj, "gamma1": gamma1, "norm_weight": norm_weight,
                                  "norm_bias": norm_bias, "w1": w1, "b1": b1, "w2": w2, "b2": b2, "gamma2": gamma2},
                           {"X": (f32, X.shape), "attn": (dtype, attn.shape), "wproj": (f32, (C, C)), "bproj": vec, "gamma1": vec,
                            "norm_weight": vec, "norm_bias": vec, "w1": (f32, (Hd, C)), "b1": (f32, (Hd,)), "w2": (f32, (C, Hd)), "b2": vec,
                            "gamma2": vec})
    out = t["X"] if inplace else torch.empty_like(t["X"])
    _timed("decoder_post", lambda: entry(
        ptr(t["X"]), ptr(t["attn"]), ptr(t["wproj"]), ptr(t["bproj"]), ptr(t["gamma1"]), ptr(t["norm_weight"]), ptr(t["norm_bias"]), float(eps),
        ptr(t["w1"]), ptr(t["b1"]), ptr(t["w2"]), ptr(t["b2"]), ptr(t["gamma2"]), X.numel() // C, C, Hd, ptr(out), stream_ptr(dev)))
    if inplace and out.data_ptr() != X.data_ptr():  # (a misaligned X was copied for the kernel)
        X.copy_(out)
    return X if inplace else out


def _decoder_bwd_ws(dev, rows):
    nws = int(_L().gfn_decoder_bwd_ws_bytes(rows))
    return torch.empty(max(nws, 16), device=dev, dtype=torch.uint8), nws


def decoder_qkv_bwd(X, norm_weight, norm_bias, eps, wq, wk, wv, gq, gk, gv, dtype=torch.float16):
    """The backward of decoder_qkv (gfn_decoder_qkv_bwd), differentiating the forward as the kernel computes it with every fp16
    rounding taken as the identity: X and the parameters as decoder_qkv took them, gq, gk, gv (2B, N, 8, 8) fp16 as
    cross_attention_bwd returns them (gk and gv of a row are read where its k and v were written, at the other view's batch entry).
    Returns (gX, g_wq, g_wk, g_wv, g_norm_weight, g_norm_bias), all fp32.  No atomics: two calls give the same bits.
    dtype=torch.bfloat16: the bf16 class (gfn_decoder_qkv_bf16_bwd), gq, gk, gv bfloat16."""
    what, C = "decoder_qkv_bwd", DECODER_DIM
    entry = _decoder_entry(what, "qkv", "bwd", dtype)
    if X.dim() != 3 or X.shape[0] % 2 or X.shape[1] < 1:
        raise ValueError(f"{what}: X must be (2B, N, {C}) with an even batch and N >= 1, got {tuple(X.shape)}")
    f32, B2, N = torch.float32, X.shape[0], X.shape[1]
    grad = (dtype, (B2, N, 8, C // 8))
    dev, t = _decoder_args(what, {"X": X, "norm_weight": norm_weight, "norm_bias": norm_bias, "wq": wq, "wk": wk, "wv": wv, "gq": gq, "gk": gk,
                                  "gv": gv},
                           {"X": (f32, (B2, N, C)), "norm_weight": (f32, (C,)), "norm_bias": (f32, (C,)), "wq": (f32, (C, C)),
                            "wk": (f32, (C, C)), "wv": (f32, (C, C)), "gq": grad, "gk": grad, "gv": grad}, forward_only=False)
    gX = torch.empty((B2, N, C), device=dev, dtype=f32)
    g_wq, g_wk, g_wv = (torch.empty((C, C), device=dev, dtype=f32) for _ in range(3))
    g_nw, g_nb = (torch.empty((C,), device=dev, dtype=f32) for _ in range(2))
    ws, nws = _decoder_bwd_ws(dev, B2 * N)
    _timed("decoder_qkv_bwd", lambda: entry(
        ptr(t["X"]), ptr(t["norm_weight"]), ptr(t["norm_bias"]), float(eps), ptr(t["wq"]), ptr(t["wk"]), ptr(t["wv"]), ptr(t["gq"]), ptr(t["gk"]),
        ptr(t["gv"]), B2, N, C, ptr(gX), ptr(g_wq), ptr(g_wk), ptr(g_wv), ptr(g_nw), ptr(g_nb), ptr(ws), nws, stream_ptr(dev)))
    return gX, g_wq, g_wk, g_wv, g_nw, g_nb


def decoder_post_bwd(X, attn, wproj, bproj, gamma1, norm_weight, norm_bias, eps, w1, b1, w2, b2, gamma2, gX_out, dtype=torch.float16):
    """The backward of decoder_post (gfn_decoder_post_bwd): X, attn and the parameters as decoder_post took them (x1, norm2, fc1 and
    the GELU are recomputed from them, nothing of the forward is saved), gX_out fp32 of X's shape.  Returns (gX, g_attn, g_wproj,
    g_bproj, g_gamma1, g_norm_weight, g_norm_bias, g_w1, g_b1, g_w2, g_b2, g_gamma2): gX fp32 of X's shape, g_attn fp16 of attn's
    shape (rounded once, overflow to inf: the dout of cross_attention_bwd), the rest fp32 of the parameters' shapes.  No atomics:
    two calls give the same bits.  dtype=torch.bfloat16: the bf16 class (gfn_decoder_post_bf16_bwd), attn and g_attn bfloat16."""
    what, C, Hd = "decoder_post_bwd", DECODER_DIM, DECODER_HIDDEN
    entry = _decoder_entry(what, "post", "bwd", dtype)
    if X.dim() < 1 or X.shape[-1] != C:
        raise ValueError(f"{what}: X must be (..., {C}), got {tuple(X.shape)}")
    if attn.numel() != X.numel():
        raise ValueError(f"{what}: attn must hold X's {X.numel() // C} rows of {C}, got {tuple(attn.shape)}")
    f32 = torch.float32
    vec = (f32, (C,))
    dev, t = _decoder_args(what, {"X": X, "attn": attn, "wproj": wproj, "bproj": bproj, "gamma1": gamma1, "norm_weight": norm_weight,
                                  "norm_bias": norm_bias, "w1": w1, "b1": b1, "w2": w2, "b2": b2, "gamma2": gamma2, "gX_out": gX_out},
                           {"X": (f32, X.shape), "attn": (dtype, attn.shape), "wproj": (f32, (C, C)), "bproj": vec, "gamma1": vec,
                            "norm_weight": vec, "norm_bias": vec, "w1": (f32, (Hd, C)), "b1": (f32, (Hd,)), "w2": (f32, (C, Hd)), "b2": vec,
                            "gamma2": vec, "gX_out": (f32, X.shape)}, forward_only=False)
    rows = X.numel() // C
    gX, g_attn = torch.empty_like(t["X"]), torch.empty_like(t["attn"])
    names = ("wproj", "bproj", "gamma1", "norm_weight", "norm_bias", "w1", "b1", "w2", "b2", "gamma2")
    grads = [torch.empty_like(t[n]) for n in names]
    ws, nws = _decoder_bwd_ws(dev, rows)
    _timed("decoder_post_bwd", lambda: entry(
        ptr(t["X"]), ptr(t["attn"]), ptr(t["wproj"]), ptr(t["bproj"]), ptr(t["gamma1"]), ptr(t["norm_weight"]), ptr(t["norm_bias"]), float(eps),
        ptr(t["w1"]), ptr(t["b1"]), ptr(t["w2"]), ptr(t["b2"]), ptr(t["gamma2"]), ptr(t["gX_out"]), rows, C, Hd, ptr(gX), ptr(g_attn),
        *(ptr(g) for g in grads), ptr(ws), nws, stream_ptr(dev)))
    return (gX, g_attn, *grads)


class _DecoderQkvFn(torch.autograd.Function):
    """decoder_qkv with a backward: the same launch forward (same bits), decoder_qkv_bwd backward; saves its inputs only."""

    @staticmethod
    def forward(ctx, X, norm_weight, norm_bias, eps, wq, wk, wv, dtype=torch.float16):
        ctx.save_for_backward(X, norm_weight, norm_bias, wq, wk, wv)
        ctx.eps, ctx.dtype = eps, dtype
        return decoder_qkv(X, norm_weight, norm_bias, eps, wq, wk, wv, dtype=dtype)  # (grad mode is off in here)

    @staticmethod
    def backward(ctx, gq, gk, gv):
        X, norm_weight, norm_bias, wq, wk, wv = ctx.saved_tensors
        gq, gk, gv = (g.to(ctx.dtype).contiguous() for g in (gq, gk, gv))
        gX, g_wq, g_wk, g_wv, g_nw, g_nb = decoder_qkv_bwd(X, norm_weight, norm_bias, ctx.eps, wq, wk, wv, gq, gk, gv, dtype=ctx.dtype)
        return gX, g_nw, g_nb, None, g_wq, g_wk, g_wv, None


class _DecoderPostFn(torch.autograd.Function):
    """decoder_post (not in place) with a backward: saves X, attn and the parameters; everything between them is recomputed."""

    @staticmethod
    def forward(ctx, X, attn, wproj, bproj, gamma1, norm_weight, norm_bias, eps, w1, b1, w2, b2, gamma2, dtype=torch.float16):
        ctx.save_for_backward(X, attn, wproj, bproj, gamma1, norm_weight, norm_bias, w1, b1, w2, b2, gamma2)
        ctx.eps, ctx.dtype = eps, dtype
        return decoder_post(X, attn, wproj, bproj, gamma1, norm_weight, norm_bias, eps, w1, b1, w2, b2, gamma2, inplace=False, dtype=dtype)

    @staticmethod
    def backward(ctx, gX_out):
        X, attn, wproj, bproj, gamma1, norm_weight, norm_bias, w1, b1, w2, b2, gamma2 = ctx.saved_tensors
        g = decoder_post_bwd(X, attn, wproj, bproj, gamma1, norm_weight, norm_bias, ctx.eps, w1, b1, w2, b2, gamma2,
                             gX_out.to(torch.float32).contiguous(), dtype=ctx.dtype)
        return (*g[:7], None, *g[7:], None)


def decoder_qkv_train(X, norm_weight, norm_bias, eps, wq, wk, wv, dtype=torch.float16):
    """decoder_qkv, differentiable with respect to X and the five parameters (gfn_decoder_qkv_bwd): the training forward is the
    same launch, in the reference's fp16 autocast class (model/network.py:171), or with dtype=torch.bfloat16 in its bf16 one.
    Saves its inputs, nothing else."""
    _decoder_entry("decoder_qkv_train", "qkv", "fwd", dtype)
    return _DecoderQkvFn.apply(X, norm_weight, norm_bias, float(eps), wq, wk, wv, dtype)


def decoder_post_train(X, attn, wproj, bproj, gamma1, norm_weight, norm_bias, eps, w1, b1, w2, b2, gamma2, dtype=torch.float16):
    """decoder_post(..., inplace=False), differentiable with respect to X, attn and the ten parameters (gfn_decoder_post_bwd).
    Saves its inputs, nothing else: x1, norm2, the 256-wide fc1 and GELU outputs are recomputed in the backward.
    dtype=torch.bfloat16: the bf16 class, attn and its gradient bfloat16."""
    _decoder_entry("decoder_post_train", "post", "fwd", dtype)
    return _DecoderPostFn.apply(X, attn, wproj, bproj, gamma1, norm_weight, norm_bias, float(eps), w1, b1, w2, b2, gamma2, dtype)


CONV_ACTS = {None: 0, "none": 0, "leaky_relu": 1, "swish": 2}


def conv2d_bn_act(x0, weight, scale, shift, x1=None, up0=False, residual=None, stride=1, act=None, slope=0.1):
    """One FPN layer in inference as one launch (gfn_conv2d_bn_act_fwd; reference model/FPN.py:95-128 and :43-66):

        out = act(conv(cat(x0', x1), weight) * scale[c] + shift[c]) + residual        zero padding K // 2

    x0 (B, C0, H, W), or with up0 (B, C0, H/2, W/2) read through F.interpolate(scale_factor=2, mode="bilinear",
    align_corners=False) without writing the doubled map; x1 (B, C1, H, W) or None; weight (Cout, C0 + C1, K, K), K in 1, 3, 5, 7;
    scale, shift (Cout): BatchNorm and the conv bias folded; residual of the output's shape or None (it may be x0 or x1); stride 1
    or 2; act None, "leaky_relu" (with slope) or "swish".  Contiguous fp32 CUDA tensors, the current stream, no autograd."""
    if act not in CONV_ACTS:
        raise ValueError(f"conv2d_bn_act: act must be one of {list(CONV_ACTS)}, got {act!r}")
    tensors = {"x0": x0, "weight": weight, "scale": scale, "shift": shift, "x1": x1, "residual": residual}
    dev = require_gpu(*tensors.values())
    for name, t in tensors.items():
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise TypeError(f"conv2d_bn_act: {name} must be a contiguous float32 tensor, got {t.dtype}, contiguous={t.is_contiguous()}")
    if x0.dim() != 4 or weight.dim() != 4 or weight.shape[2] != weight.shape[3]:
        raise ValueError(f"conv2d_bn_act: x0 (B,C0,H,W) and weight (Cout,Cin,K,K) expected, got {tuple(x0.shape)}, {tuple(weight.shape)}")
    B, C0 = x0.shape[:2]
    H, W = (2 * x0.shape[2], 2 * x0.shape[3]) if up0 else x0.shape[2:]
    C1 = 0 if x1 is None else x1.shape[1]
    Cout, Cin, K, _ = weight.shape
    if x1 is not None and (x1.dim() != 4 or x1.shape[0] != B or tuple(x1.shape[2:]) != (H, W)):
        raise ValueError(f"conv2d_bn_act: x1 must be ({B}, C1, {H}, {W}), got {tuple(x1.shape)}")
    if Cin != C0 + C1 or tuple(scale.shape) != (Cout,) or tuple(shift.shape) != (Cout,):
        raise ValueError(f"conv2d_bn_act: weight takes {Cin} channels but the inputs have {C0} + {C1}; scale and shift must be ({Cout},), "
                         f"got {tuple(scale.shape)}, {tuple(shift.shape)}")
    if stride not in (1, 2):
        raise ValueError(f"conv2d_bn_act: stride must be 1 or 2, got {stride!r}")
    out = torch.empty((B, Cout, (H + stride - 1) // stride, (W + stride - 1) // stride), device=dev, dtype=torch.float32)
    if residual is not None and residual.shape != out.shape:
        raise ValueError(f"conv2d_bn_act: residual must have the output's shape {tuple(out.shape)}, got {tuple(residual.shape)}")
    _timed("conv2d_bn_act", lambda: _L().gfn_conv2d_bn_act_fwd(ptr(x0), C0, int(bool(up0)), ptr(x1), C1, ptr(weight), ptr(scale), ptr(shift),
                                                               ptr(residual), ptr(out), B, H, W, Cout, K, stride, CONV_ACTS[act],
                                                               float(slope), stream_ptr(dev)))
    return out


def conv2d_pack_half(weight):
    """The (Cout, Cin, K, K) weight rounded once to fp16 and packed for gfn_conv2d_bn_act_half_fwd (include/gfnet_hip.h):

        packed[co, cg, u, c] = weight[co, 8 cg + c, u // K, u % K]        (CoutP, ceil(Cin / 8), UP, 8), fp16

    with UP = K K rounded up to a multiple of 4 and CoutP = Cout rounded up to a multiple of 16 below 32 output channels, of 32 from
    there; zero past Cin, K K and Cout.  A few torch ops on the weight's device; nothing is cached."""
    if weight.dim() != 4 or weight.shape[2] != weight.shape[3]:
        raise ValueError(f"conv2d_pack_half: weight (Cout,Cin,K,K) expected, got {tuple(weight.shape)}")
    Cout, Cin, K, _ = weight.shape
    CG, UP, n = -(-Cin // 8), -(-K * K // 4) * 4, 16 if Cout < 32 else 32
    w = weight.detach().to(torch.float16).reshape(Cout, Cin, K * K)
    w = torch.nn.functional.pad(w, (0, UP - K * K, 0, CG * 8 - Cin, 0, -(-Cout // n) * n - Cout))
    return w.reshape(-1, CG, 8, UP).permute(0, 1, 3, 2).contiguous()


def conv2d_bn_act_half(x0, weight, scale, shift, x1=None, up0=False, residual=None, stride=1, act=None, slope=0.1):
    """conv2d_bn_act in the fp16 class (gfn_conv2d_bn_act_half_fwd, csrc/fpn_conv_half.hip): the same layer, the same arguments, with
    x0, x1 and residual contiguous fp16 CUDA tensors and an fp16 result; scale and shift stay fp32.  weight is the layer's own
    (Cout, Cin, K, K) weight, fp32 or fp16: it is rounded to fp16 and packed here at every call (conv2d_pack_half).  Cout must be a
    multiple of 8.  fp16 x fp16 products summed in fp32 on the matrix core, the epilogue in fp32, one rounding at the store, overflow
    to inf; with up0 the interpolated operand is rounded to fp16 once.  No autograd."""
    if act not in CONV_ACTS:
        raise ValueError(f"conv2d_bn_act_half: act must be one of {list(CONV_ACTS)}, got {act!r}")
    tensors = {"x0": x0, "weight": weight, "scale": scale, "shift": shift, "x1": x1, "residual": residual}
    dev = require_gpu(*tensors.values())
    for name, t in tensors.items():
        want = (torch.float32,) if name in ("scale", "shift") else (torch.float16, torch.float32) if name == "weight" else (torch.float16,)
        if t is not None and (t.dtype not in want or not t.is_contiguous()):
            raise TypeError(f"conv2d_bn_act_half: {name} must be a contiguous {' or '.join(str(d)[6:] for d in want)} tensor, got "
                            f"{t.dtype}, contiguous={t.is_contiguous()}")
    if x0.dim() != 4 or weight.dim() != 4 or weight.shape[2] != weight.shape[3]:
        raise ValueError(f"conv2d_bn_act_half: x0 (B,C0,H,W) and weight (Cout,Cin,K,K) expected, got {tuple(x0.shape)}, {tuple(weight.shape)}")
    B, C0 = x0.shape[:2]
    H, W = (2 * x0.shape[2], 2 * x0.shape[3]) if up0 else x0.shape[2:]
    C1 = 0 if x1 is None else x1.shape[1]
    Cout, Cin, K, _ = weight.shape
    if x1 is not None and (x1.dim() != 4 or x1.shape[0] != B or tuple(x1.shape[2:]) != (H, W)):
        raise ValueError(f"conv2d_bn_act_half: x1 must be ({B}, C1, {H}, {W}), got {tuple(x1.shape)}")
    if Cin != C0 + C1 or tuple(scale.shape) != (Cout,) or tuple(shift.shape) != (Cout,):
        raise ValueError(f"conv2d_bn_act_half: weight takes {Cin} channels but the inputs have {C0} + {C1}; scale and shift must be "
                         f"({Cout},), got {tuple(scale.shape)}, {tuple(shift.shape)}")
    if stride not in (1, 2):
        raise ValueError(f"conv2d_bn_act_half: stride must be 1 or 2, got {stride!r}")
    out = torch.empty((B, Cout, (H + stride - 1) // stride, (W + stride - 1) // stride), device=dev, dtype=torch.float16)
    if residual is not None and residual.shape != out.shape:
        raise ValueError(f"conv2d_bn_act_half: residual must have the output's shape {tuple(out.shape)}, got {tuple(residual.shape)}")
    packed = conv2d_pack_half(weight)
    _timed("conv2d_bn_act_half", lambda: _L().gfn_conv2d_bn_act_half_fwd(ptr(x0), C0, int(bool(up0)), ptr(x1), C1, ptr(packed), ptr(scale),
                                                                         ptr(shift), ptr(residual), ptr(out), B, H, W, Cout, K, stride,
                                                                         CONV_ACTS[act], float(slope), stream_ptr(dev)))
    return out


def conv2d_bn_act_tf32(x0, weight, scale, shift, x1=None, up0=False, residual=None, stride=1, act=None, slope=0.1):
    """conv2d_bn_act in the reference's TF32 class (gfn_conv2d_bn_act_tf32_fwd, csrc/fpn_conv_tf32.hip; the class is stated in
    include/gfnet_hip.h): the same layer, the same arguments and checks, contiguous fp32 CUDA tensors in and an fp32 result.  The
    operands of every product are split into two bf16 halves (16 significant bits against TF32's 11) and multiplied on the matrix
    core, the sums and the epilogue are fp32.  weight is the layer's own fp32 (Cout, Cin, K, K) weight: it is split and packed on the
    device inside the call.  Cout must be a multiple of 8.  No autograd."""
    if act not in CONV_ACTS:
        raise ValueError(f"conv2d_bn_act_tf32: act must be one of {list(CONV_ACTS)}, got {act!r}")
    tensors = {"x0": x0, "weight": weight, "scale": scale, "shift": shift, "x1": x1, "residual": residual}
    dev = require_gpu(*tensors.values())
    for name, t in tensors.items():
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise TypeError(f"conv2d_bn_act_tf32: {name} must be a contiguous float32 tensor, got {t.dtype}, contiguous={t.is_contiguous()}")
    if x0.dim() != 4 or weight.dim() != 4 or weight.shape[2] != weight.shape[3]:
        raise ValueError(f"conv2d_bn_act_tf32: x0 (B,C0,H,W) and weight (Cout,Cin,K,K) expected, got {tuple(x0.shape)}, {tuple(weight.shape)}")
    B, C0 = x0.shape[:2]
    H, W = (2 * x0.shape[2], 2 * x0.shape[3]) if up0 else x0.shape[2:]
    C1 = 0 if x1 is None else x1.shape[1]
    Cout, Cin, K, _ = weight.shape
    if x1 is not None and (x1.dim() != 4 or x1.shape[0] != B or tuple(x1.shape[2:]) != (H, W)):
        raise ValueError(f"conv2d_bn_act_tf32: x1 must be ({B}, C1, {H}, {W}), got {tuple(x1.shape)}")
    if Cin != C0 + C1 or tuple(scale.shape) != (Cout,) or tuple(shift.shape) != (Cout,):
        raise ValueError(f"conv2d_bn_act_tf32: weight takes {Cin} channels but the inputs have {C0} + {C1}; scale and shift must be "
                         f"({Cout},), got {tuple(scale.shape)}, {tuple(shift.shape)}")
    if stride not in (1, 2):
        raise ValueError(f"conv2d_bn_act_tf32: stride must be 1 or 2, got {stride!r}")
    out = torch.empty((B, Cout, (H + stride - 1) // stride, (W + stride - 1) // stride), device=dev, dtype=torch.float32)
    if residual is not None and residual.shape != out.shape:
        raise ValueError(f"conv2d_bn_act_tf32: residual must have the output's shape {tuple(out.shape)}, got {tuple(residual.shape)}")
    nws = int(_L().gfn_conv2d_bn_act_tf32_ws_bytes(C0, C1, Cout, K))
    ws = torch.empty(max(nws, 16), device=dev, dtype=torch.uint8)
    _timed("conv2d_bn_act_tf32", lambda: _L().gfn_conv2d_bn_act_tf32_fwd(ptr(x0), C0, int(bool(up0)), ptr(x1), C1, ptr(weight), ptr(scale),
                                                                         ptr(shift), ptr(residual), ptr(out), B, H, W, Cout, K, stride,
                                                                         CONV_ACTS[act], float(slope), ptr(ws), nws, stream_ptr(dev)))
    return out


CONV_TRAIN_PRECISIONS = ("fp32", "tf32")  # "tf32": the split-bf16 class of include/gfnet_hip.h on the matrix core, fp32 maps


def _check_train_precision(what, precision):
    if precision not in CONV_TRAIN_PRECISIONS:
        raise ValueError(f"{what}: precision must be one of {CONV_TRAIN_PRECISIONS}, got {precision!r}")


def _conv2d_train_entries(direction, up0, C0, precision):
    """(ws_bytes, entry, the arguments that stand for C0) of a training direction in a precision class."""
    L = _L()
    if precision == "tf32":  # one set of entries, up0 always among the arguments
        return L.gfn_conv2d_bn_act_train_tf32_ws_bytes, getattr(L, f"gfn_conv2d_bn_act_train_tf32_{direction}"), (C0, int(bool(up0)))
    # the entry points with the upsample inside only when asked: every other call keeps its launches
    if up0:
        return L.gfn_conv2d_up_bn_act_train_ws_bytes, getattr(L, f"gfn_conv2d_up_bn_act_train_{direction}"), (C0, 1)
    return L.gfn_conv2d_bn_act_train_ws_bytes, getattr(L, f"gfn_conv2d_bn_act_train_{direction}"), (C0,)


def _conv2d_train_args(what, x0, x1, weight, residual, vectors, stride, act, up0=False):
    """The refusals of conv2d_bn_act, for the training entry points; vectors: name -> (Cout,) tensor or None.  Returns
    (dev, B, C0, C1, H, W, Cout, K, Ho, Wo); with up0 x0 is the coarse map and H, W are twice its height and width."""
    if act not in CONV_ACTS:
        raise ValueError(f"{what}: act must be one of {list(CONV_ACTS)}, got {act!r}")
    tensors = {"x0": x0, "weight": weight, "x1": x1, "residual": residual, **vectors}
    dev = require_gpu(*tensors.values())
    for name, t in tensors.items():
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise TypeError(f"{what}: {name} must be a contiguous float32 tensor, got {t.dtype}, contiguous={t.is_contiguous()}")
    if x0.dim() != 4 or weight.dim() != 4 or weight.shape[2] != weight.shape[3]:
        raise ValueError(f"{what}: x0 (B,C0,H,W) and weight (Cout,Cin,K,K) expected, got {tuple(x0.shape)}, {tuple(weight.shape)}")
    B, C0 = x0.shape[:2]
    H, W = (2 * x0.shape[2], 2 * x0.shape[3]) if up0 else x0.shape[2:]
    C1 = 0 if x1 is None else x1.shape[1]
    Cout, Cin, K, _ = weight.shape
    if x1 is not None and (x1.dim() != 4 or x1.shape[0] != B or tuple(x1.shape[2:]) != (H, W)):
        raise ValueError(f"{what}: x1 must be ({B}, C1, {H}, {W}), got {tuple(x1.shape)}")
    if Cin != C0 + C1:
        raise ValueError(f"{what}: weight takes {Cin} channels but the inputs have {C0} + {C1}")
    if up0 and stride != 1:
        raise ValueError(f"{what}: up0 needs stride 1, got {stride!r}")
    for name, t in vectors.items():
        if t is not None and tuple(t.shape) != (Cout,):
            raise ValueError(f"{what}: {name} must be ({Cout},), got {tuple(t.shape)}")
    if stride not in (1, 2):
        raise ValueError(f"{what}: stride must be 1 or 2, got {stride!r}")
    Ho, Wo = (H + stride - 1) // stride, (W + stride - 1) // stride
    if residual is not None and tuple(residual.shape) != (B, Cout, Ho, Wo):
        raise ValueError(f"{what}: residual must have the output's shape {(B, Cout, Ho, Wo)}, got {tuple(residual.shape)}")
    return dev, B, C0, C1, H, W, Cout, K, Ho, Wo


def conv2d_bn_act_train_fwd(x0, weight, conv_bias, bn_weight, bn_bias, running_mean, running_var, momentum, eps, x1=None, residual=None,
                            stride=1, act=None, slope=0.1, up0=False, precision="fp32"):
    """The forward launches of conv2d_bn_act_train (gfn_conv2d_bn_act_train_fwd; with up0 gfn_conv2d_up_bn_act_train_fwd, x0 the
    coarse map; with precision="tf32" gfn_conv2d_bn_act_train_tf32_fwd): returns (out, u, mean, invstd) -- u the raw convolution
    output without the conv bias -- and updates running_mean / running_var in place.  Contiguous float32 CUDA tensors."""
    what = "conv2d_bn_act_train"
    _check_train_precision(what, precision)
    if bn_weight is None or bn_bias is None or running_mean is None or running_var is None:
        raise ValueError(f"{what}: BatchNorm's weight, bias and running statistics are needed (affine, track_running_stats)")
    dev, B, C0, C1, H, W, Cout, K, Ho, Wo = _conv2d_train_args(
        what, x0, x1, weight, residual, {"conv_bias": conv_bias, "bn_weight": bn_weight, "bn_bias": bn_bias, "running_mean": running_mean,
                                         "running_var": running_var}, stride, act, up0)
    out, u = (torch.empty((B, Cout, Ho, Wo), device=dev, dtype=torch.float32) for _ in range(2))
    mean, invstd = torch.empty(Cout, device=dev, dtype=torch.float32), torch.empty(Cout, device=dev, dtype=torch.float32)
    size, entry, c0 = _conv2d_train_entries("fwd", up0, C0, precision)
    nws = int(size(*c0, C1, B, H, W, Cout, K, stride, 0))
    ws = torch.empty(max(nws, 16), device=dev, dtype=torch.uint8)
    _timed("conv2d_bn_act_train_fwd", lambda: entry(
        ptr(x0), *c0, ptr(x1), C1, ptr(weight), ptr(conv_bias), ptr(bn_weight), ptr(bn_bias), ptr(running_mean), ptr(running_var), ptr(residual),
        ptr(u), ptr(mean), ptr(invstd), ptr(out), B, H, W, Cout, K, stride, CONV_ACTS[act], float(slope), float(momentum), float(eps), ptr(ws),
        nws, stream_ptr(dev)))
    return out, u, mean, invstd


def conv2d_bn_act_train_bwd(gy, x0, weight, bn_weight, bn_bias, u, mean, invstd, x1=None, stride=1, act=None, slope=0.1,
                            need=(True, True, True), buffers=None, up0=False, precision="fp32"):
    """Gradients of conv2d_bn_act_train's out given gy = dL/dout and what the forward saved (gfn_conv2d_bn_act_train_bwd; with up0
    gfn_conv2d_up_bn_act_train_bwd, x0 the coarse map and gx0 of its shape; with precision="tf32"
    gfn_conv2d_bn_act_train_tf32_bwd, the stride-1 input gradient on the matrix core): returns (gx0, gx1, d_weight, d_bn_weight, d_bn_bias),
    None where `need` = (inputs, weight, BatchNorm) says so or x1 is None.  buffers: a
    dict under those five names of tensors to write into instead of fresh ones; one that `need` does not ask for is handed to the
    library all the same and comes back untouched.  Every result is reproducible bit for bit."""
    what = "conv2d_bn_act_train_bwd"
    _check_train_precision(what, precision)
    dev, B, C0, C1, H, W, Cout, K, Ho, Wo = _conv2d_train_args(
        what, x0, x1, weight, None, {"bn_weight": bn_weight, "bn_bias": bn_bias, "mean": mean, "invstd": invstd}, stride, act, up0)
    for name, t in (("gy", gy), ("u", u)):
        if t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != (B, Cout, Ho, Wo):
            raise ValueError(f"{what}: {name} must be a contiguous float32 {(B, Cout, Ho, Wo)}, got {t.dtype} {tuple(t.shape)}")
    require_gpu(gy, u)
    n_x, n_w, n_bn = (bool(n) for n in need)
    mask = (_lib.CBT_NEED_X if n_x else 0) | (_lib.CBT_NEED_W if n_w else 0) | (_lib.CBT_NEED_BN if n_bn else 0)
    buffers = dict(buffers or {})
    shapes = {"gx0": (n_x, tuple(x0.shape)), "gx1": (n_x and C1 > 0, (B, C1, H, W)), "d_weight": (n_w, tuple(weight.shape)),
              "d_bn_weight": (n_bn, (Cout,)), "d_bn_bias": (n_bn, (Cout,))}
    for name, (wanted, shape) in shapes.items():
        t = buffers.get(name)
        if t is None:
            buffers[name] = torch.empty(shape, device=dev, dtype=torch.float32) if wanted else None
        elif t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != shape or not t.is_cuda:
            raise ValueError(f"{what}: buffer {name} must be a contiguous float32 CUDA tensor of shape {shape}")
    if mask:
        size, entry, c0 = _conv2d_train_entries("bwd", up0, C0, precision)
        nws = int(size(*c0, C1, B, H, W, Cout, K, stride, 1))
        ws = torch.empty(max(nws, 16), device=dev, dtype=torch.uint8)
        _timed("conv2d_bn_act_train_bwd", lambda: entry(
            ptr(gy), ptr(x0), *c0, ptr(x1), C1, ptr(weight), ptr(bn_weight), ptr(bn_bias), ptr(u), ptr(mean), ptr(invstd), ptr(buffers["gx0"]),
            ptr(buffers["gx1"]), ptr(buffers["d_weight"]), ptr(buffers["d_bn_weight"]), ptr(buffers["d_bn_bias"]), B, H, W, Cout, K, stride,
            CONV_ACTS[act], float(slope), mask, ptr(ws), nws, stream_ptr(dev)))
    return tuple(buffers[name] if wanted else None for name, (wanted, _) in shapes.items())


class _Conv2dBnActTrainFn(torch.autograd.Function):
    """One FPN layer in training mode: saves x0, x1, u, mean, invstd and the parameters -- not the normalised map, the activation's
    mask or sigmoid, or the concatenation, which the backward recomputes from u or never needs.  With up0 the saved x0 is the coarse
    map and so is the gx0 that comes back: the doubled map exists in neither direction."""

    @staticmethod
    def forward(ctx, x0, x1, weight, conv_bias, bn_weight, bn_bias, residual, running_mean, running_var, momentum, eps, stride, act, slope,
                up0, precision):
        out, u, mean, invstd = conv2d_bn_act_train_fwd(x0, weight, conv_bias, bn_weight, bn_bias, running_mean, running_var, momentum, eps,
                                                       x1=x1, residual=residual, stride=stride, act=act, slope=slope, up0=up0,
                                                       precision=precision)
        if any(ctx.needs_input_grad):
            ctx.save_for_backward(x0, x1, weight, bn_weight, bn_bias, u, mean, invstd)
            ctx.meta = (stride, act, slope, None if conv_bias is None else conv_bias.shape, up0, precision)
        return out

    @staticmethod
    def backward(ctx, gy):
        x0, x1, weight, bn_weight, bn_bias, u, mean, invstd = ctx.saved_tensors
        stride, act, slope, bias_shape, up0, precision = ctx.meta
        n = ctx.needs_input_grad
        gy = gy.contiguous()
        gx0, gx1, d_w, d_g, d_b = conv2d_bn_act_train_bwd(gy, x0, weight, bn_weight, bn_bias, u, mean, invstd, x1=x1, stride=stride, act=act,
                                                          slope=slope, need=(n[0] or n[1], n[2], n[4] or n[5]), up0=up0,
                                                          precision=precision)
        # the conv bias cancels in u - mean: its gradient is exactly zero
        d_cb = torch.zeros(bias_shape, device=gy.device, dtype=torch.float32) if n[3] and bias_shape is not None else None
        return (gx0 if n[0] else None, gx1 if n[1] else None, d_w, d_cb, d_g if n[4] else None, d_b if n[5] else None,
                gy if n[6] else None) + (None,) * 9


def conv2d_bn_act_train(x0, weight, conv_bias, bn_weight, bn_bias, running_mean, running_var, num_batches_tracked, momentum, eps, x1=None,
                        residual=None, stride=1, act=None, slope=0.1, up0=False, precision="fp32"):
    """One FPN layer under model.train() with a backward, all in csrc/fpn_conv_train.hip (reference model/FPN.py:95-128, :43-66,
    model/network.py:66, 182, which torch autograd differentiates there):

        u = conv(cat(x0', x1), weight)       out = act(batch_norm(u + conv_bias; the batch's own statistics)) + residual

    x0 (B, C0, H, W), or with up0 (B, C0, H/2, W/2) read in both directions through F.interpolate(scale_factor=2, mode="bilinear",
    align_corners=False) without writing the doubled map (stride 1 only; x1 and residual at (H, W), the gradient of x0 at its own
    coarse shape); x1 (B, C1, H, W) or None; weight (Cout, C0 + C1, K, K), K in 1, 3, 5, 7, zero padding K // 2, stride 1 or 2;
    conv_bias (Cout) or None; bn_weight, bn_bias, running_mean, running_var (Cout); residual of the output's shape or None (it may be x0
    or x1); act None, "leaky_relu" (with slope) or "swish".  Contiguous float32 CUDA tensors, the current stream.  The concatenation is not
    written in either direction.
    running_mean / running_var are updated in place with `momentum` (a float) as torch does (unbiased variance, the conv bias in the
    mean), their version counters are bumped and num_batches_tracked, when given, is incremented -- also without grad mode (train()
    under no_grad: forward and buffers only, nothing saved).  Gradients flow to x0, x1, residual (gy itself), weight, bn_weight and
    bn_bias; the conv bias's gradient is returned as EXACT zeros: in front of batch statistics it cancels in u - mean, so the true
    gradient is zero (torch's autograd returns rounding noise around 1e-7 there).  Only u is kept between the directions; identical
    calls give identical bits.
    precision "fp32" (the default) or "tf32": the reference's TF32 class as include/gfnet_hip.h states it -- the forward convolution
    the stride-1 input gradient and the stride-1 weight gradient (without up0) with split-bf16 operands on the matrix core
    (csrc/fpn_conv_tf32.hip), every map still fp32; the stride-2 input gradient, the stride-2 and up0 weight gradients and a
    convolution whose output channels are no multiple of 8 stay on the fp32 kernels.  Any other value raises ValueError."""
    _check_train_precision("conv2d_bn_act_train", precision)
    if momentum is None:
        raise ValueError("conv2d_bn_act_train: momentum must be a float (cumulative averaging, momentum=None, is not supported)")
    out = _Conv2dBnActTrainFn.apply(x0, x1, weight, conv_bias, bn_weight, bn_bias, residual, running_mean, running_var, float(momentum),
                                    float(eps), stride, act, float(slope), bool(up0), precision)
    # the kernels wrote the buffers through raw pointers: tell autograd's version counters
    torch.autograd.graph.increment_version(running_mean)
    torch.autograd.graph.increment_version(running_var)
    if num_batches_tracked is not None:
        num_batches_tracked.add_(1)
    return out


def corr_volume(feat0, feat1, with_flow=False):
    """GFNet.corr_volume (model/network.py:415-428): (B,H1,W1,H0,W0) = f0^T f1 / sqrt(C)."""
    dev = require_gpu(feat0, feat1)
    f0, f1 = f32c(feat0), f32c(feat1)
    B, C, H0, W0 = f0.shape
    _, _, H1, W1 = f1.shape
    vol = torch.empty((B, H1, W1, H0, W0), device=dev, dtype=torch.float32)
    flow = torch.empty((B, 2, H0, W0), device=dev, dtype=torch.float32) if with_flow else None
    _L().gfn_corr_volume_fwd(ptr(f0), ptr(f1), ptr(vol), ptr(flow), B, C, H0, W0, H1, W1, stream_ptr(dev))
    return (vol, flow) if with_flow else vol


def pos_embed(corr_vol):
    """GFNet.pos_embed (model/network.py:430-440) on an explicit volume (B,H1,W1,H0,W0) -> (B,2,H0,W0)."""
    dev = require_gpu(corr_vol)
    v = f32c(corr_vol)
    B, H1, W1, H0, W0 = v.shape
    flow = torch.empty((B, 2, H0, W0), device=dev, dtype=torch.float32)
    _L().gfn_pos_embed_fwd(ptr(v), ptr(flow), B, H0, W0, H1, W1, stream_ptr(dev))
    return flow


def refiner_input(num_grid, x, y, flow, disp_w, disp_b, local_radius, scale_factor=1.0, corr_in_other=True, reuse=None,
                  sample_mode="bilinear", deterministic=None):
    """The concat tensor `d` of ConvRefiner.forward (model/network.py:533-558):
    cat(grid_sample(x, cell centres), grid_sample(y, flow), disp_emb(40/32*scale_factor*(flow-centres)),
    local_correlation(...)) -- every slice written in place by the HIP kernels, no torch.cat.
    If flow has twice the batch of x/y the call is symmetric: directions (x vs y) then (y vs x).
    reuse: the `d` an earlier call returned for the SAME x and num_grid (the previous refiner iteration at this scale): it is
    overwritten in place except for its grid_feature planes, which depend on x and the grid only.
    sample_mode: ConvRefiner(sample_mode=...) (network.py:464, 537, 547, 553-554), "bilinear", "nearest" or "bicubic"; padding is
    zeros as in the reference.  Other than bilinear, all three gathers take the general per-tap kernels (csrc/grid_modes.hip,
    csrc/local_corr_modes.hip), never the tiled correlation or its plan.
    With grad mode on and any of x, y, flow, disp_w, disp_b requiring grad, a bilinear call on a plain batch is differentiable
    (_RefinerInputFn: the same launches forward, gfn_refiner_input_bwd backward; `reuse` is not taken, an autograd graph keeps d);
    a symmetric batch that needs gradients raises NotImplementedError, as training does.  Every other call is the plain launch.
    deterministic: which backward the differentiable call gets (refiner_input_bwd's keyword): None (default) is
    torch.are_deterministic_algorithms_enabled() at the time of this forward, so torch.use_deterministic_algorithms(True) makes
    y's gradient bit-reproducible; the forward's bits do not depend on it."""
    if sample_mode == "bilinear" and torch.is_grad_enabled() and any(t.requires_grad for t in (x, y, flow, disp_w, disp_b)):
        if flow.shape[0] != x.shape[0]:
            raise NotImplementedError("training-mode refiner input needs a plain batch (flow and features of equal batch size)")
        return _RefinerInputFn.apply(x, y, flow, disp_w, disp_b, int(num_grid), int(local_radius), float(scale_factor), bool(corr_in_other),
                                     resolve_deterministic(deterministic))
    return _refiner_input(num_grid, x, y, flow, disp_w, disp_b, local_radius, scale_factor, corr_in_other, reuse, sample_mode)[0]


def resolve_deterministic(deterministic):
    """A `deterministic` keyword as a bool: None follows torch.are_deterministic_algorithms_enabled() now."""
    return torch.are_deterministic_algorithms_enabled() if deterministic is None else bool(deterministic)


def _refiner_input(num_grid, x, y, flow, disp_w, disp_b, local_radius, scale_factor, corr_in_other, reuse, sample_mode):
    """The forward launches; returns (d, y, flow, disp_w) with the inputs as the kernels read them."""
    general = sample_mode != "bilinear"
    if general:
        sm, _ = _lib.mode_codes(sample_mode, "zeros", "refiner_input")
    dev = require_gpu(x, y, flow, disp_w, disp_b)
    (x, dtx), (y, dty), fl = featc(x), featc(y), f32c(flow)
    if dtx != dty:
        x, y, dtx = f32c(x), f32c(y), _lib.GFN_F32
    Bi, C, Hs, Ws = x.shape
    G = int(num_grid)
    B = fl.shape[0]
    symmetric = B == 2 * Bi
    if tuple(y.shape) != (Bi, C, Hs, Ws) or tuple(fl.shape[1:]) != (2, G, G) or B not in (Bi, 2 * Bi):
        raise ValueError(f"refiner_input: y must be {(Bi, C, Hs, Ws)} and flow (B or 2B,2,{G},{G}), got {tuple(y.shape)}, {tuple(fl.shape)}")
    w = f32c(disp_w).reshape(-1, 2)
    bvec = f32c(disp_b).reshape(-1)
    Dd = w.shape[0]
    r = int(local_radius)
    K = (2 * r + 1) ** 2 if corr_in_other else 0
    CH = 2 * C + Dd + K
    keep = reuse is not None
    if keep:
        if tuple(reuse.shape) != (B, CH, G, G) or reuse.dtype != torch.float32 or not reuse.is_contiguous() or reuse.device != dev:
            raise ValueError("refiner_input: `reuse` must be the tensor an earlier call with the same shapes returned")
        d = reuse
    else:
        d = torch.empty((B, CH, G, G), device=dev, dtype=torch.float32)
    st = stream_ptr(dev)
    mode = (1 if symmetric else 0) | (_lib.RI_KEEP_GRID_FEATURE if keep else 0)
    disp_scale = float(40 / 32 * scale_factor)
    ri_args = (ptr(x), ptr(y), dtx, ptr(fl), ptr(w), ptr(bvec), ptr(d), CH * G * G, B, C, Hs, Ws, G, Dd, disp_scale, mode)
    if general:  # the per-tap kernels of every mode: no tile plan, no scratch
        _L().gfn_refiner_input_mode_fwd_dt(*ri_args, sm, st)
        if corr_in_other:
            out = d[:, 2 * C + Dd:]
            _L().gfn_local_corr_mode_fwd(ptr(d), CH * G * G, ptr(y), ptr(x) if symmetric else None, dtx, ptr(fl), c_vp(out.data_ptr()),
                                         CH * G * G, B, C, G, Hs, Ws, r, 0, Hs, Ws, sm, _lib.PADDING_MODES["zeros"], st)
        return d, y, fl, w
    # shapes the lean local-correlation path takes are planned inside the refiner-input launch (both only read the flow)
    plans = FUSE_PLAN and corr_in_other and bool(_L().gfn_local_corr_plans(C, Hs, Ws, G, r, dtx))
    if corr_in_other:
        nscr = int(_L().gfn_local_corr_scratch_bytes(B, G))
        scr = _lib.scratch(dev, nscr)
    if plans:
        _L().gfn_refiner_input_plan_fwd_dt(*ri_args, r, ptr(scr), nscr, st)
    else:
        _L().gfn_refiner_input_fwd_dt(*ri_args, st)
    if corr_in_other:
        out = d[:, 2 * C + Dd:]
        name = f"local_corr_c{C}_h{Hs}_g{G}_r{r}"
        _timed(name, lambda: _L().gfn_local_corr_fwd_dt(ptr(d), CH * G * G, ptr(y), ptr(x) if symmetric else None, dtx, ptr(fl),
                                                        c_vp(out.data_ptr()), CH * G * G, B, C, G, Hs, Ws, r, 0, Hs, Ws,
                                                        (8 if plans else 0) | (4 if LOCAL_CORR_FP32 and r >= 5 else 0),
                                                        ptr(scr), nscr, st))
        if kernel_counters is not None:
            hdr = scr[:8].cpu()  # synchronises; header layout: csrc/local_corr.hip kTodoHdr
            kernel_counters.setdefault(name, []).append((int(hdr[3]), int(hdr[5]), int(hdr[7])))
    return d, y, fl, w


def refiner_input_bwd(grad_d, y, flow, disp_w, local_radius, scale_factor=1.0, corr_in_other=True, need=(True,) * 5, deterministic=False):
    """Gradients of refiner_input's d (bilinear, plain batch) with respect to (x, y, flow, disp_w, disp_b) given grad_d = dL/dd:
    fp32 tensors, None where `need` says so (csrc/refiner_input_bwd.hip).  y (B,C,Hs,Ws) fp32 or fp16, flow (B,2,G,G) and disp_w
    (Dd,2) as the forward read them.  The local correlation passes its feature0 gradient on to x (gfn_local_corr_mode_bwd_f0 on
    grad_d's last planes); its feature1 and coordinates are detached, as in the reference (utils/local_correlation.py:54-60).
    deterministic=False: dy is accumulated with fp32 atomics and its last bits can differ between runs; every other result is
    reproducible.  deterministic=True (gfn_refiner_input_bwd_det): dy is the same sum in 64-bit fixed point, scaled per sample by
    the largest finite |grad| of its x_hat planes -- the same bits on every run, whatever order the cells are visited in, NaN where
    a non-finite gradient lands; the other four results are the plain call's bits.  It takes a workspace of 8 bytes and a bit per
    element of dy."""
    dev = require_gpu(grad_d, y, flow, disp_w)
    (y, dt), fl, g = featc(y), f32c(flow), f32c(grad_d)
    w = f32c(disp_w).reshape(-1, 2)
    B, C, Hs, Ws = y.shape
    G, Dd, r = fl.shape[-1], w.shape[0], int(local_radius)
    K = (2 * r + 1) ** 2 if corr_in_other else 0
    CH = 2 * C + Dd + K
    if tuple(fl.shape) != (B, 2, G, G) or tuple(g.shape) != (B, CH, G, G):
        raise ValueError(f"refiner_input_bwd: flow must be (B,2,G,G) and grad_d {(B, CH, G, G)}, got {tuple(fl.shape)}, {tuple(g.shape)}")
    st = stream_ptr(dev)
    n_x, n_y, n_f, n_w, n_b = need
    gf0 = None
    if n_x and corr_in_other:
        gk = g[:, 2 * C + Dd:]
        gf0 = torch.empty((B, C, G, G), device=dev, dtype=torch.float32)
        _L().gfn_local_corr_mode_bwd_f0(c_vp(gk.data_ptr()), CH * G * G, ptr(f32c(y)), None, ptr(fl), ptr(gf0), C * G * G, B, C, G,
                                        Hs, Ws, r, 0, Hs, Ws, _lib.SAMPLE_MODES["bilinear"], _lib.PADDING_MODES["zeros"], st)

    def out(wanted, *shape):
        return torch.empty(shape, device=dev, dtype=torch.float32) if wanted else None

    dx, dy, dfl = out(n_x, B, C, Hs, Ws), out(n_y, B, C, Hs, Ws), out(n_f, B, 2, G, G)
    dw, db = out(n_w, Dd, 2), out(n_b, Dd)
    nscr = int(_L().gfn_refiner_input_bwd_scratch_bytes(B, G, Dd)) if (n_w or n_b) else 0
    scr = torch.empty(nscr, device=dev, dtype=torch.uint8) if nscr > 0 else None  # (not the per-stream scratch: its header stays zeroed)
    args = (ptr(g), CH * G * G, ptr(y), dt, ptr(fl), ptr(w), ptr(gf0), ptr(dx), ptr(dy), ptr(dfl), ptr(dw), ptr(db), B, C, Hs, Ws, G, Dd, K,
            float(40 / 32 * scale_factor), ptr(scr), nscr)
    if deterministic:
        nws = int(_L().gfn_refiner_input_bwd_det_ws_bytes(B, C, Hs, Ws)) if n_y else 0
        ws = torch.empty(nws // 8, device=dev, dtype=torch.int64) if nws > 0 else None  # (8-byte aligned; the call clears it)
        _L().gfn_refiner_input_bwd_det(*args, ptr(ws), nws, st)
    else:
        _L().gfn_refiner_input_bwd(*args, st)
    return dx, dy, dfl, dw, db


class _RefinerInputFn(torch.autograd.Function):
    """refiner_input with a backward: the same launches forward (same bits, the planned lean route included), saving only y, flow
    and disp_w; refiner_input_bwd backward."""

    @staticmethod
    def forward(ctx, x, y, flow, disp_w, disp_b, num_grid, local_radius, scale_factor, corr_in_other, deterministic=False):
        d, yk, fl, w = _refiner_input(num_grid, x, y, flow, disp_w, disp_b, local_radius, scale_factor, corr_in_other, None, "bilinear")
        ctx.save_for_backward(yk, fl, w)
        ctx.meta = (local_radius, scale_factor, corr_in_other, tuple(t.dtype for t in (x, y, flow, disp_w, disp_b)), disp_w.shape, disp_b.shape)
        ctx.deterministic = deterministic  # resolved when the forward ran
        return d

    @staticmethod
    def backward(ctx, grad_d):
        yk, fl, w = ctx.saved_tensors
        r, scale_factor, corr_in_other, dtypes, w_shape, b_shape = ctx.meta
        grads = list(refiner_input_bwd(grad_d, yk, fl, w, r, scale_factor, corr_in_other, need=ctx.needs_input_grad[:5],
                                       deterministic=ctx.deterministic))
        if grads[3] is not None:
            grads[3] = grads[3].reshape(w_shape)
        if grads[4] is not None:
            grads[4] = grads[4].reshape(b_shape)
        return tuple(None if t is None else t.to(dt) for t, dt in zip(grads, dtypes)) + (None,) * 5


def grid_sample(x, grid, mode="bilinear", padding_mode="zeros"):
    """F.grid_sample(x, grid, mode, padding_mode, align_corners=False); mode "bilinear" / "nearest" / "bicubic", padding_mode
    "zeros" / "border" / "reflection".  Returns fp32; fp16 input is read as stored (the widening is exact)."""
    sm, pm = _lib.mode_codes(mode, padding_mode, "grid_sample")
    dev = require_gpu(x, grid)
    (x, dtx), g = featc(x), f32c(grid)
    B, C, H, W = x.shape
    _, Ho, Wo, _ = g.shape
    if tuple(g.shape) != (B, Ho, Wo, 2):
        raise ValueError(f"grid_sample: grid must be (B,Ho,Wo,2) with B={B}, got {tuple(g.shape)}")
    out = torch.empty((B, C, Ho, Wo), device=dev, dtype=torch.float32)
    _L().gfn_grid_sample_mode_fwd(ptr(x), dtx, ptr(g), ptr(out), C * Ho * Wo, B, C, H, W, Ho, Wo, sm, pm, stream_ptr(dev))
    return out


def interpolate_bilinear(x, size):
    """F.interpolate(x, size=size, mode='bilinear', align_corners=False) (model/network.py:238-249,271-281)."""
    dev = require_gpu(x)
    x = f32c(x)
    B, C, H, W = x.shape
    Ho, Wo = (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))
    out = torch.empty((B, C, Ho, Wo), device=dev, dtype=torch.float32)
    _L().gfn_interp_bilinear_fwd(ptr(x), ptr(out), B * C, H, W, Ho, Wo, stream_ptr(dev))
    return out


class _ResizeBilinearFn(torch.autograd.Function):
    """interpolate_bilinear with a backward: the same launch forward, gfn_interp_bilinear_bwd (a gather, no atomics) backward."""

    @staticmethod
    def forward(ctx, x, size):
        ctx.meta = (x.shape, x.dtype)
        return interpolate_bilinear(x, size)

    @staticmethod
    def backward(ctx, grad_out):
        (B, C, H, W), dtype = ctx.meta
        dev = require_gpu(grad_out)
        g = f32c(grad_out)
        Ho, Wo = g.shape[2:]
        grad_in = torch.empty((B, C, H, W), device=dev, dtype=torch.float32)
        _L().gfn_interp_bilinear_bwd(ptr(g), ptr(grad_in), B * C, H, W, Ho, Wo, stream_ptr(dev))
        return grad_in.to(dtype), None


def resize_bilinear(x, size):
    """A differentiable F.interpolate(x, size=size, mode='bilinear', align_corners=False): interpolate_bilinear's launch and bits
    forward (fp32 out), and a backward that gathers instead of scattering with atomics as torch's does on the GPU -- the same bits on
    every run, and no refusal under torch.use_deterministic_algorithms(True).  interpolate_bilinear itself stays graph-free."""
    require_gpu(x)
    if torch.is_grad_enabled() and x.requires_grad:
        return _ResizeBilinearFn.apply(x, size)
    return interpolate_bilinear(x, size)


def interpolate_bilinear_pair(a, b, size):
    """interpolate_bilinear of two tensors with the same batch and spatial size in one launch (flow + certainty,
    model/network.py:238-249,271-281)."""
    dev = require_gpu(a, b)
    a, b = f32c(a), f32c(b)
    B, Ca, H, W = a.shape
    if b.shape[0] != B or tuple(b.shape[2:]) != (H, W):
        raise ValueError(f"interpolate_bilinear_pair: {tuple(a.shape)} vs {tuple(b.shape)}")
    Cb = b.shape[1]
    Ho, Wo = (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))
    oa = torch.empty((B, Ca, Ho, Wo), device=dev, dtype=torch.float32)
    ob = torch.empty((B, Cb, Ho, Wo), device=dev, dtype=torch.float32)
    _L().gfn_interp_bilinear_pair_fwd(ptr(a), ptr(oa), B * Ca, ptr(b), ptr(ob), B * Cb, H, W, Ho, Wo, stream_ptr(dev))
    return oa, ob


def flow_update_(flow, certainty, delta, disp_prev, scale, W0, H0, zero_small=True, first_iteration=True):
    """In place: model/network.py:262-268.  delta is the refiner output (B,3,G,G) (channels 0,1 =
    displacement, 2 = certainty increment); disp_prev (B,2,G,G) carries the previous displacement."""
    dev = require_gpu(flow, certainty, delta, disp_prev)
    B, _, G, _ = flow.shape
    if tuple(certainty.shape) != (B, 1, G, G) or tuple(disp_prev.shape) != (B, 2, G, G) or \
            tuple(delta.shape[:1] + delta.shape[2:]) != (B, G, G) or delta.shape[1] < 3:
        raise ValueError("flow_update_: inconsistent shapes")
    for t in (flow, certainty, disp_prev):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError("flow_update_: flow/certainty/disp_prev must be contiguous fp32 (updated in place)")
    dl = f32c(delta)
    _L().gfn_flow_update_fwd(ptr(flow), ptr(certainty), ptr(dl), dl.shape[1] * G * G, ptr(disp_prev), B, G, int(scale),
                             int(W0), int(H0), 1 if zero_small else 0, 1 if first_iteration else 0, stream_ptr(dev))
    return flow, certainty


def _plane_view(t, planes, G):
    """(tensor, batch stride) of a (B, >=planes, G, G) fp32 tensor whose planes are contiguous (a channel slice is fine)."""
    if t.dtype == torch.float32 and t.stride(3) == 1 and t.stride(2) == G and t.stride(1) == G * G:
        return t, (t.stride(0) if t.shape[0] > 1 else t.shape[1] * G * G)
    t = f32c(t)
    return t, t.shape[1] * G * G


def flow_update(flow, certainty, d_flow, d_cert, disp_prev, scale, W0, H0, zero_small=True, first_iteration=True):
    """model/network.py:262-268 out of place: returns (flow + displacement(d_flow), certainty + d_cert) as new tensors (the
    reference keeps every iteration's result); d_flow (B,2,G,G) / d_cert (B,1,G,G) may be channel slices of one tensor.
    disp_prev=None (first iteration of a scale that has only one): the displacement is not stored.  With grad mode on and an
    input that requires grad, both results are differentiable (_FlowUpdateFn); every other call is the plain launch."""
    if torch.is_grad_enabled() and (flow.requires_grad or certainty.requires_grad or d_flow.requires_grad or d_cert.requires_grad):
        return _FlowUpdateFn.apply(flow, certainty, d_flow, d_cert, disp_prev, scale, W0, H0, zero_small, first_iteration)
    return _flow_update(flow, certainty, d_flow, d_cert, disp_prev, scale, W0, H0, zero_small, first_iteration)


def _flow_update(flow, certainty, d_flow, d_cert, disp_prev, scale, W0, H0, zero_small, first_iteration, size_next=None):
    dev = require_gpu(flow, certainty, d_flow, d_cert, *(() if disp_prev is None else (disp_prev,)))
    B, _, G, _ = flow.shape
    if tuple(certainty.shape) != (B, 1, G, G) or tuple(d_flow.shape) != (B, 2, G, G) or tuple(d_cert.shape) != (B, 1, G, G) or \
            (disp_prev is not None and tuple(disp_prev.shape) != (B, 2, G, G)):
        raise ValueError("flow_update: inconsistent shapes")
    if disp_prev is None:
        if not first_iteration:
            raise ValueError("flow_update: disp_prev=None is only valid for the first (and only) iteration of a scale")
    elif disp_prev.dtype != torch.float32 or not disp_prev.is_contiguous():
        raise ValueError("flow_update: disp_prev must be contiguous fp32 (updated in place)")
    fi, ci = f32c(flow), f32c(certainty)
    df, df_bs = _plane_view(d_flow, 2, G)
    dc, dc_bs = _plane_view(d_cert, 1, G)
    fo, co = torch.empty_like(fi), torch.empty_like(ci)
    if size_next is not None:  # flow_update_resize
        Gn = int(size_next)
        fn = torch.empty((B, 2, Gn, Gn), device=dev, dtype=torch.float32)
        cn = torch.empty((B, 1, Gn, Gn), device=dev, dtype=torch.float32)
        _L().gfn_flow_update_resize_fwd(ptr(fi), ptr(ci), ptr(fo), ptr(co), c_vp(df.data_ptr()), df_bs, c_vp(dc.data_ptr()), dc_bs,
                                        ptr(disp_prev), B, G, int(scale), int(W0), int(H0), 1 if zero_small else 0,
                                        1 if first_iteration else 0, ptr(fn), ptr(cn), Gn, stream_ptr(dev))
        return fo, co, fn, cn
    _L().gfn_flow_update_out_fwd(ptr(fi), ptr(ci), ptr(fo), ptr(co), c_vp(df.data_ptr()), df_bs, c_vp(dc.data_ptr()), dc_bs,
                                 ptr(disp_prev), B, G, int(scale), int(W0), int(H0), 1 if zero_small else 0,
                                 1 if first_iteration else 0, stream_ptr(dev))
    return fo, co


# forward_pyramids ends a scale with flow_update_resize where it can; False keeps the two launches (the comparison the tests make)
FUSE_UPDATE_RESIZE = True


def flow_update_resize(flow, certainty, d_flow, d_cert, disp_prev, scale, W0, H0, size_next, zero_small=True, first_iteration=True):
    """flow_update followed by interpolate_bilinear_pair of its results to the (size_next, size_next) grid in one launch
    (model/network.py:262-268 + 271-281): returns (flow, certainty, flow_next, cert_next), bit for bit what the two calls
    return, and leaves disp_prev as flow_update does.  size_next must be the grid size or twice it (anything else is an error:
    make the two calls).  Inference only: no backward."""
    return _flow_update(flow, certainty, d_flow, d_cert, disp_prev, scale, W0, H0, zero_small, first_iteration, size_next=size_next)


class _FlowUpdateFn(torch.autograd.Function):
    """flow_update with a backward.  displacement = scale * (d_flow / (4 W0, 4 H0)) (network.py:262-263), so d flow_out / d d_flow
    = scale / (4 W0) and scale / (4 H0); flow and both certainty terms pass their gradient through.  With zero_small (eval with
    grad: network.py:264-265, `displacement[mask] = 0`) the cells the kernel zeroed get no gradient: the kernel stores the
    displacement it applied in disp_prev (a scratch plane when the caller has none), and a zeroed cell is a stored 0 from a
    d_flow that is not 0."""

    @staticmethod
    def forward(ctx, flow, certainty, d_flow, d_cert, disp_prev, scale, W0, H0, zero_small, first_iteration):
        dp = disp_prev
        if zero_small and dp is None:
            dp = torch.empty(flow.shape, device=flow.device, dtype=torch.float32)
        fo, co = _flow_update(flow, certainty, d_flow, d_cert, dp, scale, W0, H0, zero_small, first_iteration)
        mask = ((dp == 0) & (d_flow != 0)) if zero_small else None
        ctx.save_for_backward(mask)
        ctx.factors = (float(scale) / (4 * W0), float(scale) / (4 * H0))
        ctx.dtypes = (flow.dtype, certainty.dtype, d_flow.dtype, d_cert.dtype)
        return fo, co

    @staticmethod
    def backward(ctx, g_flow, g_cert):
        (mask,) = ctx.saved_tensors
        fx, fy = ctx.factors
        g_d = torch.stack((g_flow[:, 0] * fx, g_flow[:, 1] * fy), dim=1)
        if mask is not None:
            g_d = g_d.masked_fill(mask, 0.0)
        n = ctx.needs_input_grad
        dt = ctx.dtypes
        return (g_flow.to(dt[0]) if n[0] else None, g_cert.to(dt[1]) if n[1] else None, g_d.to(dt[2]) if n[2] else None,
                g_cert.to(dt[3]) if n[3] else None, None, None, None, None, None, None)


def match_post(flow, certainty, cert16=None, symmetric=True):
    """model/network.py:332-338 + 358-384: returns warp (B,G,2G,4)/(B,G,G,4) and certainty (B,G,2G)/(B,G,G)."""
    dev = require_gpu(flow, certainty, cert16)
    fl, ce = f32c(flow), f32c(certainty)
    nb, _, G, _ = fl.shape
    if tuple(ce.shape) != (nb, 1, G, G) or (cert16 is not None and cert16.shape[0] != nb) or (symmetric and nb % 2):
        raise ValueError("match_post: inconsistent shapes")
    B = nb // 2 if symmetric else nb
    Gw = 2 * G if symmetric else G
    c16 = f32c(cert16) if cert16 is not None else None
    Gc = c16.shape[-1] if c16 is not None else 0
    warp = torch.empty((B, G, Gw, 4), device=dev, dtype=torch.float32)
    cout = torch.empty((B, G, Gw), device=dev, dtype=torch.float32)
    _L().gfn_match_post_fwd(ptr(fl), ptr(ce), ptr(c16), ptr(warp), ptr(cout), B, G, Gc, 1 if symmetric else 0,
                            stream_ptr(dev))
    return warp, cout


KDE_CULL_MIN_STD = _lib.KDE_SORTED_MIN_STD


def kde_density(x, y=None, std=0.1, y_row_stride=None, cull=None, round_fp16=False):
    """sum_m exp(-|x_n - y_m|^2/(2 std^2)); x (N,D) or (Bt,N,D); y defaults to x.  fp32.
    round_fp16: coordinates rounded to fp16 first (what GFNet.sample hands to kde(); sums stay fp32).
    cull (default: automatic for 4-D points, N >= 4096): sort the points along a Morton curve of the
    A-image coordinates and skip blocks of reference points beyond 6.7 std (terms < 2^-32).
    The culled routes form the exponent on the matrix core as |x|^2 + |y|^2 - 2 x.y; they hold the 1e-4 parity for
    |coordinate| <= 16 std (include/gfnet_hip.h).  For image coordinates in [-1, 1] that is std >= KDE_CULL_MIN_STD: below it
    the automatic rule takes the dense difference-form kernels (exact at any std and extent) and cull=True is refused.  The
    extent of the points is not checked: points far outside the image at a small std belong on cull=False."""
    dev = require_gpu(x, y)
    xs = f32c(x)
    squeeze = xs.dim() == 2
    if squeeze:
        xs = xs[None]
    Bt, N, D = xs.shape
    if y is None:
        ys, M, rs, bs = xs, N, D, N * D
    else:
        ys = f32c(y)
        if ys.dim() == 2:
            ys = ys[None]
        M, rs, bs = ys.shape[1], D, ys.shape[1] * D
    if y_row_stride is not None:  # strided view of ys (x[::down]) without a copy
        rs = int(y_row_stride)
        M = (ys.shape[1] * D + rs - 1) // rs
    if cull is None:
        cull = D == 4 and N >= 4096 and M >= 4096 and KDE_CULL_MIN_STD <= std <= 0.2
    elif cull and D == 4 and not std >= KDE_CULL_MIN_STD:
        raise ValueError(f"kde_density: cull=True needs std >= {KDE_CULL_MIN_STD} (got {std}): the matrix-core exponent loses the "
                         "1e-4 parity below it; use cull=False")
    if cull and D == 4:
        if y_row_stride is not None:
            ys = ys[:, ::rs // D].contiguous()
        same = y is None and y_row_stride is None
        out = _kde_culled(xs, xs if same else ys, std, same, dev, round_fp16)
        return out[0] if squeeze else out
    if round_fp16:  # only the culled path rounds on the device
        same_t = ys is xs
        xs = xs.half().float()
        ys = xs if same_t else ys.half().float()
    out = torch.empty((Bt, N), device=dev, dtype=torch.float32)
    nscr = int(_L().gfn_kde_scratch_floats(Bt, N, M, D))
    scratch = torch.empty((max(nscr, 4),), device=dev, dtype=torch.float32)
    _L().gfn_kde_density(ptr(xs), ptr(ys), ptr(out), Bt, N, M, D, rs, bs, float(std), ptr(scratch), nscr,
                         stream_ptr(dev))
    return out[0] if squeeze else out


def _morton_sorted(pts, dev, long_perm=True):
    """(sorted points, permutation): rows stably ordered by the Morton key of their A-image position (one HIP launch:
    in-LDS two-pass radix sort per row, the same permutation as torch.sort(keys, stable=True))."""
    Bt, N, _ = pts.shape
    pts = f32c(pts)
    out = torch.empty_like(pts)
    perm = torch.empty((Bt, N), device=dev, dtype=torch.int32)
    tmp = torch.empty((Bt, N), device=dev, dtype=torch.int32)
    _L().gfn_kde_morton_sort(ptr(pts), ptr(out), ptr(perm), ptr(tmp), Bt, N, stream_ptr(dev))
    return out, (perm.long() if long_perm else perm)


def _kde_culled(xs, ys, std, same, dev, round_fp16=False):
    Bt, N, _ = xs.shape
    M = ys.shape[1]
    xsort, perm = _morton_sorted(xs, dev, long_perm=False)
    ysort = xsort if same else _morton_sorted(ys, dev, long_perm=False)[0]
    out = torch.empty((Bt, N), device=dev, dtype=torch.float32)
    nscr = int(_L().gfn_kde_sorted_scratch_floats(Bt, N, M))
    scratch = torch.empty((nscr,), device=dev, dtype=torch.float32)
    # perm: the densities are written straight back in the caller's order
    _L().gfn_kde_density_sorted(ptr(xsort), ptr(ysort), ptr(out), ptr(perm), Bt, N, M, float(std), 1 if round_fp16 else 0, ptr(scratch), nscr,
                                stream_ptr(dev))
    return out


def threshold_certainty(certainty, thresh):
    """certainty[certainty > thresh] = 1 on a copy (model/network.py:391-393)."""
    dev = require_gpu(certainty)
    c = f32c(certainty)
    out = torch.empty_like(c)
    _L().gfn_threshold_certainty(ptr(c), ptr(out), c.numel(), float(thresh), stream_ptr(dev))
    return out


def balance_weights(density, min_density=10.0, floor_p=1e-7, round_fp16=False):
    """p = 1/(density+1); p[density < 10] = 1e-7 (model/network.py:409-410).  round_fp16: the density is rounded to fp16
    first, as kde(half=True) returns it."""
    dev = require_gpu(density)
    d = f32c(density)
    p = torch.empty_like(d)
    _L().gfn_balance_weights(ptr(d), ptr(p), d.numel(), float(min_density), float(floor_p), 1 if round_fp16 else 0, stream_ptr(dev))
    return p


def gather_matches(matches, certainty, idx, one_above=None):
    """(matches[b, idx[b]], certainty[b, idx[b]]) for a batch (model/network.py:403-404, 414) in one launch; one_above:
    certainties above it come back as 1 (the threshold of network.py:391-393 applied on the fly)."""
    dev = require_gpu(matches, certainty, idx)
    m, c = f32c(matches), f32c(certainty)
    Bt, N, four = m.shape
    K = idx.shape[1]
    if four != 4 or tuple(c.shape) != (Bt, N) or idx.shape[0] != Bt or idx.dtype != torch.int64:
        raise ValueError("gather_matches: matches (Bt,N,4), certainty (Bt,N), idx (Bt,K) int64")
    idx = idx.contiguous()
    om = torch.empty((Bt, K, 4), device=dev, dtype=torch.float32)
    oc = torch.empty((Bt, K), device=dev, dtype=torch.float32)
    _L().gfn_gather_matches(ptr(m), ptr(c), ptr(idx), ptr(om), ptr(oc), Bt, N, K,
                            float("inf") if one_above is None else float(one_above), stream_ptr(dev))
    return om, oc


def sample_without_replacement(weights, num_samples, seed=None, one_above=None):
    """torch.multinomial(weights, num_samples, replacement=False) for a (Bt,N) batch (model/network.py:400-402, 411-413):
    exponential race, one HIP launch pair; indices come back in increasing order.  seed=None draws one from torch's
    default CPU generator, so torch.manual_seed() makes runs repeatable.  one_above: weights above it count as 1."""
    dev = require_gpu(weights)
    w = f32c(weights)
    if w.dim() != 2:
        raise ValueError("sample_without_replacement: weights must be (Bt, N)")
    Bt, N = w.shape
    K = int(num_samples)
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    out = torch.empty((Bt, K), device=dev, dtype=torch.int64)
    scratch = torch.empty((Bt * (N + 2048),), device=dev, dtype=torch.int32)
    _L().gfn_sample_without_replacement(ptr(w), N, ptr(out), ptr(scratch), Bt, N, K, int(seed) & (2 ** 64 - 1),
                                        float("inf") if one_above is None else float(one_above), stream_ptr(dev))
    return out


def convert_matches(matches, wA, hA, wB, hB):
    """estimation.py:26-45 on the device: (...,4) normalised warp rows -> pixel (x,y,u,v), float32."""
    dev = require_gpu(matches)
    m = f32c(matches)
    out = torch.empty_like(m)
    n = m.numel() // 4
    _L().gfn_convert_matches(ptr(m), ptr(out), n, float(wA), float(hA), float(wB), float(hB), stream_ptr(dev))
    return out


def find_homography(pts, thresh=3.0, iters=2000, seed=0, lm_iters=10, stage=0, return_mask=False, confidence=0.99999,
                    return_iters=False):
    """Batched stand-in for cv2.findHomography(pos_a, pos_b, cv2.RANSAC, confidence=0.99999, ransacReprojThreshold=thresh)
    (estimation.py:66-72), on the device.  pts (Bt,N,4) or (N,4) pixel (x,y,u,v).  confidence: OpenCV's termination rule
    (the iteration bound follows the best inlier ratio; `iters` = maxIters); 0 scores all `iters` hypotheses.
    Returns H (Bt,3,3) float64, inlier counts (Bt,), chosen hypothesis index (Bt,) [, mask (Bt,N) uint8] [, iteration bound at
    exit (Bt,)]."""
    dev = require_gpu(pts)
    p = f32c(pts)
    if p.dim() == 2:
        p = p[None]
    Bt, N, _ = p.shape
    H = torch.empty((Bt, 3, 3), device=dev, dtype=torch.float64)
    ninl = torch.empty((Bt,), device=dev, dtype=torch.int32)
    best = torch.empty((Bt,), device=dev, dtype=torch.int32)
    used = torch.empty((Bt,), device=dev, dtype=torch.int32) if return_iters else None
    mask = torch.empty((Bt, N), device=dev, dtype=torch.uint8) if return_mask else None
    nb = int(_L().gfn_homography_scratch_bytes(Bt, int(iters)))
    scratch = torch.empty((nb // 8 + 1,), device=dev, dtype=torch.float64)
    _L().gfn_homography_ransac_ex(ptr(p), Bt, N, float(thresh), int(iters), float(confidence or 0.0), int(seed), int(lm_iters),
                                  int(stage), ptr(H), ptr(ninl), ptr(best), ptr(mask), ptr(used), ptr(scratch), nb, stream_ptr(dev))
    out = (H, ninl, best)
    if return_mask:
        out = out + (mask,)
    return out + (used,) if return_iters else out


def homography_dlt(pts, weight=None):
    """One-shot weighted normalised DLT over all correspondences ("grid-DLT").  pts (Bt,N,4) pixels,
    weight (Bt,N) or None -> H (Bt,3,3) float64, ok (Bt,) int32."""
    dev = require_gpu(pts, weight)
    p = f32c(pts)
    if p.dim() == 2:
        p = p[None]
    Bt, N, _ = p.shape
    w = f32c(weight).reshape(Bt, N) if weight is not None else None
    H = torch.empty((Bt, 3, 3), device=dev, dtype=torch.float64)
    ok = torch.empty((Bt,), device=dev, dtype=torch.int32)
    _L().gfn_homography_dlt(ptr(p), ptr(w), Bt, N, ptr(H), ptr(ok), stream_ptr(dev))
    return H, ok


IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


def resize_normalise(im, size, mode="bicubic", mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """get_tuple_transform_ops(resize=size, mode, normalize=True) of the reference (utils/utils.py:18-27) on a
    (B,>=3,H,W) float image batch in [0,1]: F.interpolate(mode, align_corners=False, antialias=False) + (x-mean)/std on
    the first three channels, one HIP kernel.  mode: 'bicubic' or 'bilinear' (the reference's mode=2)."""
    import ctypes

    dev = require_gpu(im)
    if im.dim() != 4 or im.shape[1] < 3:
        raise ValueError("resize_normalise: expected (B, >=3, H, W)")
    if mode not in ("bilinear", "bicubic"):
        raise ValueError("resize_normalise: mode must be 'bilinear' or 'bicubic'")
    x = f32c(im)
    B, C, H, W = x.shape
    Ho, Wo = (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))
    out = torch.empty((B, 3, Ho, Wo), device=dev, dtype=torch.float32)
    m3, s3 = (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std)
    _L().gfn_resize_normalize_fwd(ptr(x), C * H * W, ptr(out), B, H, W, Ho, Wo, 1 if mode == "bicubic" else 0, m3, s3,
                                  stream_ptr(dev))
    return out


def conv_block_pack(dw_w, dw_b, bn_alpha, bn_beta, pw_w, pw_b):
    """Pack one ConvRefiner block (model/network.py:471-487) for conv_block: dw_w (C,25) or (C,1,5,5),
    dw_b (C) or None, eval-mode BatchNorm as y = x*alpha + beta, pw_w (M,C[,1,1]), pw_b (M)."""
    return _conv_block_pack("gfn_conv_block_pack", dw_w, dw_b, bn_alpha, bn_beta, pw_w, pw_b)


def conv_block_pack_bf16(dw_w, dw_b, bn_alpha, bn_beta, pw_w, pw_b):
    """conv_block_pack for conv_block_bf16: the same arguments, layout and size, with the two 16-bit sections (the 1x1 weights and the
    banded depthwise taps) rounded to bf16 instead of fp16.  A block packed here goes to conv_block_bf16 and nowhere else."""
    return _conv_block_pack("gfn_conv_block_pack_bf16", dw_w, dw_b, bn_alpha, bn_beta, pw_w, pw_b)


def _conv_block_pack(entry, dw_w, dw_b, bn_alpha, bn_beta, pw_w, pw_b):
    dev = require_gpu(dw_w, pw_w)
    C, M = dw_w.shape[0], pw_w.shape[0]
    dw_w, pw_w = f32c(dw_w.reshape(C, 25)), f32c(pw_w.reshape(M, C))
    al, be, pb = f32c(bn_alpha), f32c(bn_beta), f32c(pw_b)
    db = f32c(dw_b) if dw_b is not None else None
    packed = torch.empty(int(_L().gfn_conv_block_packed_floats(C, M)), device=dev, dtype=torch.float32)
    getattr(_L(), entry)(ptr(dw_w), ptr(db) if db is not None else None, ptr(al), ptr(be), ptr(pw_w), ptr(pb), ptr(packed),
                         C, M, stream_ptr(dev))
    return packed


def conv_block(x, packed, M, out=None, variant=0, t_scratch=None):
    """Conv2d(C,C,5,pad 2,groups=C) -> BatchNorm2d(eval) -> ReLU -> Conv2d(C,M,1) in one kernel
    (model/network.py:471-487).  variant bit 0: the two-pass form (bit-identical to the fused one);
    bit 1: 1x1 conv with fp16 operands (W and the ReLU output rounded to fp16, fp32 accumulation) --
    the reference's autocast numerics class (amp=True refiners) -- instead of fp32 throughout."""
    dev = require_gpu(x, packed)
    x = f32c(x)
    B, C, G, G2 = x.shape
    if G != G2:
        raise ValueError("conv_block: square grids only")
    if packed.numel() != int(_L().gfn_conv_block_packed_floats(C, M)):
        raise ValueError("conv_block: packed parameters do not match (C=%d, M=%d)" % (C, M))
    if out is None:
        out = torch.empty((B, M, G, G), device=dev, dtype=torch.float32)
    if ((variant & 1) or G % 4) and t_scratch is None:
        t_scratch = torch.empty_like(x)
    _timed("conv_block_c%d_g%d" % (C, G), lambda: _L().gfn_conv_block_fwd(
        ptr(x), ptr(packed), ptr(out), ptr(t_scratch) if t_scratch is not None else None, B, C, M, G, int(variant),
        stream_ptr(dev)))
    return out


def conv_block_half(x, packed, C, M, out=None, out_half=True):
    """conv_block on fp16 maps (the reference's amp=True class, model/network.py:560-562): x is (B,C,G,G) float32 or a
    half map (B,ceil(C/2),G,G,2) float16 (channel pairs side by side); returns a half map (B,ceil(M/2),G,G,2), or (B,M,G,G)
    float32 with out_half=False.  The autocast class: depthwise 5x5 and 1x1 operands fp16 (the input halo, the folded taps, the
    ReLU output and the 1x1 weights are rounded), every accumulation, BatchNorm and ReLU fp32 (include/gfnet_hip.h)."""
    return _conv_block_16(_MAP_HALF, x, packed, C, M, out, out_half)


def conv_block_bf16(x, packed, C, M, out=None, out_bf16=True):
    """conv_block on bf16 maps -- the refiners under torch.autocast(dtype=torch.bfloat16) (model/network.py:560-562 with
    amp_dtype=torch.bfloat16), the class a bf16-trained model is evaluated in: x is (B,C,G,G) float32 or a bf16 map
    (B,ceil(C/2),G,G,2) bfloat16 (the half map's layout); packed comes from conv_block_pack_bf16; returns a bf16 map
    (B,ceil(M/2),G,G,2), or (B,M,G,G) float32 with out_bf16=False.  conv_block_half's kernel on the bf16 matrix instructions: the input
    halo, the folded taps, the ReLU output and the 1x1 weights are rounded to bf16, every accumulation, BatchNorm and ReLU fp32;
    nothing that is finite in fp32 overflows (include/gfnet_hip.h)."""
    return _conv_block_16(_MAP_BF16, x, packed, C, M, out, out_bf16)


# What differs between conv_block_half and conv_block_bf16: name, entry point, torch dtype and GFN_* constant of a 16-bit map
_MAP_HALF = ("conv_block_half", "gfn_conv_block_half_fwd", torch.float16, _lib.GFN_F16, "half")
_MAP_BF16 = ("conv_block_bf16", "gfn_conv_block_bf16_fwd", torch.bfloat16, _lib.GFN_BF16, "bf16")


def _conv_block_16(cls, x, packed, C, M, out, out_16):
    name, entry, dt16, gfn16, word = cls
    dev = require_gpu(x, packed)
    x_16 = x.dtype == dt16
    if x_16:
        if x.dim() != 5 or x.shape[1] != (C + 1) // 2 or x.shape[4] != 2 or not x.is_contiguous():
            raise ValueError("%s: a %s map is a contiguous (B, ceil(C/2), G, G, 2) %s tensor" % (name, word, str(dt16)[6:]))
    else:
        if x.dim() == 5 and x.dtype in (torch.float16, torch.bfloat16):
            raise ValueError("%s: x is a %s map; this entry takes float32 (B, C, G, G) or a %s map" % (name, str(x.dtype)[6:], word))
        x = f32c(x)
        if x.dim() != 4 or x.shape[1] != C:
            raise ValueError("%s: x must be (B, C, G, G)" % name)
    B, G, G2 = x.shape[0], x.shape[2], x.shape[3]
    if G != G2:
        raise ValueError("%s: square grids only" % name)
    if packed.numel() != int(_L().gfn_conv_block_packed_floats(C, M)):
        raise ValueError("%s: packed parameters do not match (C=%d, M=%d)" % (name, C, M))
    shape = (B, (M + 1) // 2, G, G, 2) if out_16 else (B, M, G, G)
    dt = dt16 if out_16 else torch.float32
    if out is None or tuple(out.shape) != shape or out.dtype != dt:
        out = torch.empty(shape, device=dev, dtype=dt)
    _timed("%s_c%d_g%d" % (name, C, G), lambda: getattr(_L(), entry)(
        ptr(x), gfn16 if x_16 else _lib.GFN_F32, ptr(packed), ptr(out), gfn16 if out_16 else _lib.GFN_F32, B, C, M, G, stream_ptr(dev)))
    return out


def half_map_to_float(h, C):
    """(B, ceil(C/2), G, G, 2) float16 half map -> (B, C, G, G) float32 (tests, debugging)."""
    B, NP, G, G2, _ = h.shape
    return h.permute(0, 1, 4, 2, 3).reshape(B, 2 * NP, G, G2)[:, :C].float()


def bf16_map_to_float(h, C):
    """(B, ceil(C/2), G, G, 2) bfloat16 map -> (B, C, G, G) float32 (tests, debugging)."""
    return half_map_to_float(h, C)


CONV_ROUTE_FIELDS = ("fused", "TW", "MT", "NS", "NB", "KW", "F16", "HIN", "HOUT", "MM", "ngrp", "nwork", "tpb", "VEC", "nblk", "mt",
                     "tiles_x", "tiles_y")


def conv_block_route(B, C, M, G, variant=None, x_half=None, out_half=None, x_bf16=None, out_bf16=None):
    """The launch decision of conv_block (give `variant`), conv_block_half (give `x_half` and `out_half`) or conv_block_bf16 (give
    `x_bf16` and `out_bf16`) for a shape, as a dict over CONV_ROUTE_FIELDS (F16, HIN, HOUT: 16-bit operands and maps of the entry's class): gfn_conv_block_route (include/gfnet_hip.h), the struct the launchers switch on.  Answered on the host,
    no GPU needed.  None where the entry point would refuse the shape."""
    import ctypes

    route = (ctypes.c_int * _lib.CBR_FIELDS)()
    if variant is not None:
        n = _L().gfn_conv_block_route(_lib.CBR_ENTRY_FWD, int(variant), 0, B, C, M, G, route, _lib.CBR_FIELDS)
    elif x_bf16 is not None or out_bf16 is not None:
        if x_half is not None or out_half is not None:
            raise ValueError("conv_block_route: x_half / out_half and x_bf16 / out_bf16 name two different entry points")
        n = _L().gfn_conv_block_route(_lib.CBR_ENTRY_BF16, _lib.GFN_BF16 if x_bf16 else _lib.GFN_F32,
                                      _lib.GFN_BF16 if out_bf16 else _lib.GFN_F32, B, C, M, G, route, _lib.CBR_FIELDS)
    else:
        n = _L().gfn_conv_block_route(_lib.CBR_ENTRY_HALF, _lib.GFN_F16 if x_half else _lib.GFN_F32,
                                      _lib.GFN_F16 if out_half else _lib.GFN_F32, B, C, M, G, route, _lib.CBR_FIELDS)
    if n != _lib.CBR_FIELDS:
        return None
    return {f: int(route[_lib.CBR_GEMM_MT if f == "mt" else getattr(_lib, "CBR_" + f.upper())]) for f in CONV_ROUTE_FIELDS}


def pointwise_conv(t, w, bias, out=None):
    """Conv2d(K, M, 1)(t) for a few output channels: out_conv (model/network.py:505,563).  w (M,K)."""
    dev = require_gpu(t, w)
    t, w, bias = f32c(t), f32c(w), f32c(bias)
    B, K, G, G2 = t.shape
    M = bias.shape[0]
    if out is None:
        out = torch.empty((B, M, G, G2), device=dev, dtype=torch.float32)
    _timed("pw_m%d_k%d_g%d" % (M, K, G), lambda: _L().gfn_pointwise_conv_fwd(
        ptr(w), ptr(bias), ptr(t), ptr(out), B, M, K, G * G2, stream_ptr(dev)))
    return out


# The three classes of the training conv block: what differs between conv_block_train (fp32 maps, csrc/conv_stack_train.hip),
# conv_block_train_amp (fp16 maps, csrc/conv_stack_train_half.hip) and conv_block_train_bf16 (bf16 maps,
# csrc/conv_stack_train_bf16.hip).  label: in messages and _timed names; ws_bytes / fwd / bwd: the entry points; map_dtype: u, y, gy;
# x_dtype: x may also have map_dtype and the entry points are told its dtype
_TrainClass = collections.namedtuple("_TrainClass", "label ws_bytes fwd bwd map_dtype x_dtype")
_FP32 = _TrainClass("conv_block_train", "gfn_conv_block_train_ws_bytes", "gfn_conv_block_train_fwd", "gfn_conv_block_train_bwd",
                    torch.float32, False)
_AMP = _TrainClass("conv_block_train_amp", "gfn_conv_block_train_half_ws_bytes", "gfn_conv_block_train_half_fwd",
                   "gfn_conv_block_train_half_bwd", torch.float16, True)
_BF16 = _TrainClass("conv_block_train_bf16", "gfn_conv_block_train_bf16_ws_bytes", "gfn_conv_block_train_bf16_fwd",
                    "gfn_conv_block_train_bf16_bwd", torch.bfloat16, True)
_MAP_DTYPE_ARG = {torch.float32: _lib.GFN_F32, torch.float16: _lib.GFN_F16, torch.bfloat16: _lib.GFN_BF16}


def _conv_block_train_args(cls, x, dw_w, dw_b, bn_weight, bn_bias, running_mean, running_var, pw_w, pw_b):
    """Shape and dtype checks of a training conv block of class cls; returns (B, C, M, G)."""
    what, amp = cls.label, cls.x_dtype
    if x.dim() != 4 or x.shape[2] != x.shape[3]:
        raise ValueError(f"{what}: x must be (B,C,G,G) on a square grid, got {tuple(x.shape)}")
    B, C, G, _ = x.shape
    M = pw_w.shape[0]
    params = {"dw_w": (dw_w, C * 25), "bn_weight": (bn_weight, C), "bn_bias": (bn_bias, C), "running_mean": (running_mean, C),
              "running_var": (running_var, C), "pw_w": (pw_w, M * C), "pw_b": (pw_b, M)}
    if dw_b is not None:
        params["dw_b"] = (dw_b, C)
    for name, (t, n) in params.items():
        if t is None:
            raise ValueError(f"{what}: {name} is missing")
        if t.dtype != torch.float32:
            raise ValueError(f"{what}: {name} must be float32 ({'parameters stay fp32 in the autocast class' if amp else 'the fp32 training class'}), "
                             f"got {t.dtype}")
        if t.numel() != n:
            raise ValueError(f"{what}: {name} has {t.numel()} elements, C={C} and M={M} need {n}")
    if x.dtype != torch.float32 and not (amp and x.dtype == cls.map_dtype):
        also = f" (a first block) or {str(cls.map_dtype).replace('torch.', '')}" if amp else ""
        raise ValueError(f"{what}: x must be float32{also}, got {x.dtype}")
    if B * G * G < 2:
        raise ValueError(f"{what}: batch statistics need more than one value per channel")
    return B, C, M, G


def _x_dtype_arg(cls, x):
    """The x_dtype argument of cls's entry points, where they take one."""
    return (_MAP_DTYPE_ARG[x.dtype],) if cls.x_dtype else ()


def _conv_block_train_fwd(cls, x, dw_w, dw_b, bn_weight, bn_bias, running_mean, running_var, momentum, eps, pw_w, pw_b):
    dev = require_gpu(x, dw_w, pw_w, running_mean, running_var)
    B, C, M, G = _conv_block_train_args(cls, x, dw_w, dw_b, bn_weight, bn_bias, running_mean, running_var, pw_w, pw_b)
    if not (running_mean.is_contiguous() and running_var.is_contiguous()):
        raise ValueError(f"{cls.label}: the running statistics are updated in place and must be contiguous")
    x, dw_w, pw_w = x.contiguous(), dw_w.contiguous(), pw_w.contiguous()
    u = torch.empty((B, C, G, G), device=dev, dtype=cls.map_dtype)
    y = torch.empty((B, M, G, G), device=dev, dtype=cls.map_dtype)
    mean, invstd = torch.empty(C, device=dev, dtype=torch.float32), torch.empty(C, device=dev, dtype=torch.float32)
    nws = int(getattr(_L(), cls.ws_bytes)(B, C, M, G, 0))
    ws = torch.empty(max(nws, 16), device=dev, dtype=torch.uint8)
    _timed("%s_fwd_c%d_g%d" % (cls.label, C, G), lambda: getattr(_L(), cls.fwd)(
        ptr(x), *_x_dtype_arg(cls, x), ptr(dw_w), ptr(dw_b.contiguous()) if dw_b is not None else None, ptr(bn_weight.contiguous()),
        ptr(bn_bias.contiguous()), ptr(running_mean), ptr(running_var), ptr(pw_w), ptr(pw_b.contiguous()), ptr(u), ptr(mean), ptr(invstd),
        ptr(y), B, C, M, G, float(momentum), float(eps), ptr(ws), nws, stream_ptr(dev)))
    return y, u, mean, invstd


def _conv_block_train_bwd(cls, gy, x, u, mean, invstd, dw_w, bn_weight, bn_bias, pw_w, need, has_dw_bias):
    dev = require_gpu(gy, x, u)
    gy = gy.to(cls.map_dtype).contiguous()
    B, C, G, _ = x.shape
    M = pw_w.shape[0]
    if tuple(gy.shape) != (B, M, G, G):
        raise ValueError(f"{cls.label}_bwd: grad_y must be {(B, M, G, G)}, got {tuple(gy.shape)}")
    if cls.x_dtype and (u.dtype != cls.map_dtype or x.dtype not in (torch.float32, cls.map_dtype) or tuple(u.shape) != (B, C, G, G)
                        or not u.is_contiguous() or not x.is_contiguous()):
        raise ValueError(f"{cls.label}_bwd: x and u are the contiguous maps of the forward, u {str(cls.map_dtype).replace('torch.', '')}")
    n_x, n_dww, n_dwb, n_g, n_b, n_pww, n_pwb = need
    n_dwb = n_dwb and has_dw_bias
    mask = (_lib.CBT_NEED_X if n_x else 0) | (_lib.CBT_NEED_DW if (n_dww or n_dwb) else 0) | \
        (_lib.CBT_NEED_BN if (n_g or n_b) else 0) | (_lib.CBT_NEED_PW if (n_pww or n_pwb) else 0)

    def out(bit, *shape, dtype=torch.float32):
        return torch.empty(shape, device=dev, dtype=dtype) if mask & bit else None

    gx = out(_lib.CBT_NEED_X, B, C, G, G, dtype=x.dtype if cls.x_dtype else torch.float32)
    d_dww, d_dwb = out(_lib.CBT_NEED_DW, C, 25), (out(_lib.CBT_NEED_DW, C) if has_dw_bias else None)
    d_g, d_b = out(_lib.CBT_NEED_BN, C), out(_lib.CBT_NEED_BN, C)
    d_pww, d_pwb = out(_lib.CBT_NEED_PW, M, C), out(_lib.CBT_NEED_PW, M)
    if mask:
        nws = int(getattr(_L(), cls.ws_bytes)(B, C, M, G, 1))
        ws = torch.empty(max(nws, 16), device=dev, dtype=torch.uint8)
        _timed("%s_bwd_c%d_g%d" % (cls.label, C, G), lambda: getattr(_L(), cls.bwd)(
            ptr(gy), ptr(x), *_x_dtype_arg(cls, x), ptr(u), ptr(mean), ptr(invstd), ptr(dw_w), ptr(bn_weight), ptr(bn_bias), ptr(pw_w), ptr(gx),
            ptr(d_dww), ptr(d_dwb), ptr(d_g), ptr(d_b), ptr(d_pww), ptr(d_pwb), B, C, M, G, mask, ptr(ws), nws, stream_ptr(dev)))
    grads = (gx, d_dww, d_dwb, d_g, d_b, d_pww, d_pwb)
    return tuple(g if want else None for g, want in zip(grads, (n_x, n_dww, n_dwb, n_g, n_b, n_pww, n_pwb)))


class _ConvBlockTrainFn(torch.autograd.Function):
    """A training conv block of class cls (the last argument): saves x in its own dtype, u, mean, invstd and the fp32 parameters the
    backward reads -- not t = relu(bn(u)), which both directions recompute from u."""

    @staticmethod
    def forward(ctx, x, dw_w, dw_b, bn_weight, bn_bias, pw_w, pw_b, running_mean, running_var, momentum, eps, cls):
        C, M = x.shape[1], pw_w.shape[0]
        xk, dww, pww = x.contiguous(), dw_w.reshape(C, 25).contiguous(), pw_w.reshape(M, C).contiguous()
        bnw, bnb = bn_weight.contiguous(), bn_bias.contiguous()
        y, u, mean, invstd = _conv_block_train_fwd(cls, xk, dww, dw_b, bnw, bnb, running_mean, running_var, momentum, eps, pww, pw_b)
        ctx.save_for_backward(xk, u, mean, invstd, dww, bnw, bnb, pww)
        ctx.meta = (cls, dw_w.shape, pw_w.shape, dw_b is not None)
        return y

    @staticmethod
    def backward(ctx, gy):
        xk, u, mean, invstd, dww, bnw, bnb, pww = ctx.saved_tensors
        cls, dw_shape, pw_shape, has_bias = ctx.meta
        g = list(_conv_block_train_bwd(cls, gy, xk, u, mean, invstd, dww, bnw, bnb, pww, ctx.needs_input_grad[:7], has_bias))
        if g[1] is not None:
            g[1] = g[1].reshape(dw_shape)
        if g[5] is not None:
            g[5] = g[5].reshape(pw_shape)
        return tuple(g) + (None,) * 5


def _conv_block_train(cls, x, dw_w, dw_b, bn_weight, bn_bias, running_mean, running_var, num_batches_tracked, momentum, eps, pw_w, pw_b):
    if momentum is None:
        raise ValueError(f"{cls.label}: momentum must be a float (cumulative averaging, momentum=None, is not supported)")
    require_gpu(x, dw_w, pw_w, running_mean, running_var)
    _conv_block_train_args(cls, x, dw_w, dw_b, bn_weight, bn_bias, running_mean, running_var, pw_w, pw_b)
    y = _ConvBlockTrainFn.apply(x, dw_w, dw_b, bn_weight, bn_bias, pw_w, pw_b, running_mean, running_var, float(momentum), float(eps), cls)
    # the kernels wrote the buffers through raw pointers: tell autograd's version counters
    torch.autograd.graph.increment_version(running_mean)
    torch.autograd.graph.increment_version(running_var)
    if num_batches_tracked is not None:
        num_batches_tracked.add_(1)
    return y


def conv_block_train_fwd(x, dw_w, dw_b, bn_weight, bn_bias, running_mean, running_var, momentum, eps, pw_w, pw_b):
    """The forward launches of conv_block_train: returns (y, u, mean, invstd) and updates running_mean / running_var in place
    (csrc/conv_stack_train.hip).  Tensors as the kernels read them: contiguous float32."""
    return _conv_block_train_fwd(_FP32, x, dw_w, dw_b, bn_weight, bn_bias, running_mean, running_var, momentum, eps, pw_w, pw_b)


def conv_block_train_bwd(gy, x, u, mean, invstd, dw_w, bn_weight, bn_bias, pw_w, need=(True,) * 7, has_dw_bias=True):
    """Gradients of conv_block_train's y with respect to (x, dw_w, dw_b, bn_weight, bn_bias, pw_w, pw_b) given gy = dL/dy and what
    the forward saved; None where `need` says so.  Weight and bias of one layer come from the same launches (the C ABI's need
    mask has one bit per pair); every result is reproducible bit for bit."""
    return _conv_block_train_bwd(_FP32, gy, x, u, mean, invstd, dw_w, bn_weight, bn_bias, pw_w, need, has_dw_bias)


def conv_block_train(x, dw_w, dw_b, bn_weight, bn_bias, running_mean, running_var, num_batches_tracked, momentum, eps, pw_w, pw_b):
    """Conv2d(C,C,5,pad 2,groups=C[,bias]) -> BatchNorm2d in training mode -> ReLU -> Conv2d(C,M,1) with a backward, all in
    csrc/conv_stack_train.hip: one block of ConvRefiner under model.train() (model/network.py:471-487, 560-563), the fp32 class.
    x (B,C,G,G); dw_w (C,1,5,5) or (C,25); dw_b (C) or None (use_bias_block_1=False); bn_weight, bn_bias (C); pw_w (M,C[,1,1]);
    pw_b (M); everything float32.  The batch's statistics normalise; running_mean / running_var (C) are updated in place with
    `momentum` (a float) as torch does (unbiased variance) and num_batches_tracked, when given, is incremented -- also without grad
    mode (train() under no_grad).  The buffers' version counters are bumped, so whatever caches on them (ConvRefiner.folded_stack)
    sees the change.  Gradients flow to x and the seven parameters; identical calls give identical bits."""
    return _conv_block_train(_FP32, x, dw_w, dw_b, bn_weight, bn_bias, running_mean, running_var, num_batches_tracked, momentum, eps, pw_w,
                             pw_b)


def conv_block_train_amp_fwd(x, dw_w, dw_b, bn_weight, bn_bias, running_mean, running_var, momentum, eps, pw_w, pw_b):
    """The forward launches of conv_block_train_amp: returns (y, u, mean, invstd) -- y (B,M,G,G) and u (B,C,G,G) float16, mean and
    invstd float32 -- and updates running_mean / running_var in place (csrc/conv_stack_train_half.hip).  x contiguous float32 or
    float16, parameters contiguous float32."""
    return _conv_block_train_fwd(_AMP, x, dw_w, dw_b, bn_weight, bn_bias, running_mean, running_var, momentum, eps, pw_w, pw_b)


def conv_block_train_amp_bwd(gy, x, u, mean, invstd, dw_w, bn_weight, bn_bias, pw_w, need=(True,) * 7, has_dw_bias=True):
    """Gradients of conv_block_train_amp's y with respect to (x, dw_w, dw_b, bn_weight, bn_bias, pw_w, pw_b) given gy = dL/dy (rounded
    to float16 if it is not) and what the forward saved; None where `need` says so.  gx has x's dtype -- float32, unrounded, for a
    first block -- and the parameter gradients are float32; every result is reproducible bit for bit."""
    return _conv_block_train_bwd(_AMP, gy, x, u, mean, invstd, dw_w, bn_weight, bn_bias, pw_w, need, has_dw_bias)


def conv_block_train_amp(x, dw_w, dw_b, bn_weight, bn_bias, running_mean, running_var, num_batches_tracked, momentum, eps, pw_w, pw_b):
    """conv_block_train in the class the reference trains its refiners in -- fp16 autocast around block1 + hidden_blocks
    (model/network.py:90-152, 560-562; trainer/train.py:29-43) -- on csrc/conv_stack_train_half.hip.  x (B,C,G,G) float32 (a stack's
    first block: rounded to fp16 on load) or float16 (the previous block's y); returns y (B,M,G,G) float16.  Parameters and their
    gradients are float32 (autocast would round the gradients to fp16; this class does not); the gradient of x has x's dtype.  Maps
    in HBM (u, y, the backward's intermediate and gx) are fp16, every sum fp32, the three 1x1 products fp16 operands on the matrix
    core with fp32 accumulators; rounding overflows to inf, so a GradScaler (ops.FusedAdamWStep) sees a loss scale that is too large.
    Running buffers, num_batches_tracked, momentum and eps as conv_block_train; identical calls give identical bits."""
    return _conv_block_train(_AMP, x, dw_w, dw_b, bn_weight, bn_bias, running_mean, running_var, num_batches_tracked, momentum, eps, pw_w,
                             pw_b)


def conv_block_train_bf16_fwd(x, dw_w, dw_b, bn_weight, bn_bias, running_mean, running_var, momentum, eps, pw_w, pw_b):
    """The forward launches of conv_block_train_bf16: returns (y, u, mean, invstd) -- y (B,M,G,G) and u (B,C,G,G) bfloat16, mean and
    invstd float32 -- and updates running_mean / running_var in place (csrc/conv_stack_train_bf16.hip).  x contiguous float32 or
    bfloat16, parameters contiguous float32."""
    return _conv_block_train_fwd(_BF16, x, dw_w, dw_b, bn_weight, bn_bias, running_mean, running_var, momentum, eps, pw_w, pw_b)


def conv_block_train_bf16_bwd(gy, x, u, mean, invstd, dw_w, bn_weight, bn_bias, pw_w, need=(True,) * 7, has_dw_bias=True):
    """Gradients of conv_block_train_bf16's y with respect to (x, dw_w, dw_b, bn_weight, bn_bias, pw_w, pw_b) given gy = dL/dy (rounded
    to bfloat16 if it is not) and what the forward saved; None where `need` says so.  gx has x's dtype -- float32, unrounded, for a
    first block -- and the parameter gradients are float32; every result is reproducible bit for bit."""
    return _conv_block_train_bwd(_BF16, gy, x, u, mean, invstd, dw_w, bn_weight, bn_bias, pw_w, need, has_dw_bias)


def conv_block_train_bf16(x, dw_w, dw_b, bn_weight, bn_bias, running_mean, running_var, num_batches_tracked, momentum, eps, pw_w, pw_b):
    """conv_block_train in the bf16 autocast class -- what torch.autocast(dtype=torch.bfloat16) around block1 + hidden_blocks
    (model/network.py:560-562) of a refiner built with amp_dtype=torch.bfloat16 runs -- on csrc/conv_stack_train_bf16.hip.  x (B,C,G,G)
    float32 (a stack's first block: rounded to bf16 on load) or bfloat16 (the previous block's y); float16 raises ValueError; returns
    y (B,M,G,G) bfloat16.  Parameters and their gradients are float32 (autocast would round the gradients to bf16; this class does
    not); the gradient of x has x's dtype.  Maps in HBM (u, y, the backward's intermediate and gx) are bf16, every sum fp32, the three
    1x1 products bf16 operands on the matrix core with fp32 accumulators; rounding is to nearest even without a clamp.  bf16 has
    fp32's exponent range, so the step needs no loss scale: a gradient scaled by a power of two is the unscaled one times that power,
    bit for bit.  Running buffers, num_batches_tracked, momentum and eps as conv_block_train; identical calls give identical bits."""
    return _conv_block_train(_BF16, x, dw_w, dw_b, bn_weight, bn_bias, running_mean, running_var, num_batches_tracked, momentum, eps, pw_w,
                             pw_b)


# ---- the training loss (losses/robust_loss.py) -------------------------------------------------------------------------------------
def _ptr_array(tensors):
    """A host array of RL_MAX_ITR device pointers (NULL where `tensors` has None or ends)."""
    arr = (c_vp * _lib.RL_MAX_ITR)()
    for k, t in enumerate(tensors):
        arr[k] = t.data_ptr() if t is not None else None
    return arr


def _robust_loss_scale_args(what, flows, certs, H, prev_epe, im_A_coords):
    """Shape and dtype checks of one scale; returns (B, h, w, ph, pw).  Tensors as the kernels read them: contiguous float32."""
    n = len(flows)
    if not 1 <= n <= _lib.RL_MAX_ITR or len(certs) != n:
        raise ValueError(f"{what}: a scale has 1..{_lib.RL_MAX_ITR} iterations, each with a flow and a certainty; got {n} flows, {len(certs)} certainties")
    if flows[0].dim() != 4 or flows[0].shape[1] != 2:
        raise ValueError(f"{what}: a flow must be (B,2,h,w), got {tuple(flows[0].shape)}")
    B, _, h, w = flows[0].shape
    maps = [("flow", f, (B, 2, h, w)) for f in flows] + [("certainty", c, (B, 1, h, w)) for c in certs] + [("H", H, (B, 3, 3))]
    if prev_epe is not None:
        if prev_epe.dim() != 3 or prev_epe.shape[0] != B:
            raise ValueError(f"{what}: prev_epe must be (B,ph,pw) with B = {B}, got {tuple(prev_epe.shape)}")
        maps.append(("prev_epe", prev_epe, tuple(prev_epe.shape)))
    if im_A_coords is not None:
        maps.append(("im_A_coords", im_A_coords, (B, 2, h, w)))
    for name, t, shape in maps:
        if tuple(t.shape) != shape:
            raise ValueError(f"{what}: {name} must be {shape}, got {tuple(t.shape)} (flows and certainties of one scale share a grid)")
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError(f"{what}: {name} must be contiguous float32, got {t.dtype}")
    ph, pw = (prev_epe.shape[1], prev_epe.shape[2]) if prev_epe is not None else (0, 0)
    return B, h, w, ph, pw


def robust_loss_scale_fwd(flows, certs, H, ext_a, ext_b, a, cs, ce_weight, iteration_base, pck_thresh, prev_epe=None, prev_thresh=0.0,
                          im_A_coords=None, want_epe=False, stats=None):
    """One scale of RobustLosses (losses/robust_loss.py:65-90 and the body of :97-127) in csrc/robust_loss.hip: flows / certs are
    the scale's iterations in order, (B,2,h,w) and (B,1,h,w); H (B,3,3) is H_s2t; ext_a / ext_b are im_A.shape[2] - 1 and
    im_B.shape[2] - 1.  Returns (stats, epe_last): stats the _lib.RL_STATS floats of include/gfnet_hip.h (loss, ce, reg, count,
    pck_05, ...), written into `stats` when given; epe_last (B,h,w) when want_epe, else None."""
    dev = require_gpu(*flows, *certs, H, prev_epe, im_A_coords, stats)
    B, h, w, ph, pw = _robust_loss_scale_args("robust_loss_scale_fwd", flows, certs, H, prev_epe, im_A_coords)
    if stats is None:
        stats = torch.empty(_lib.RL_STATS, device=dev, dtype=torch.float32)
    epe = torch.empty((B, h, w), device=dev, dtype=torch.float32) if want_epe else None
    nws = int(_L().gfn_robust_loss_ws_bytes(B, h, w, len(flows)))
    ws = _lib.scratch(dev, nws, pool="robust_loss")  # (not the local correlation's: its counters must stay zero)
    _timed("robust_loss_fwd_%dx%d" % (h, w), lambda: _L().gfn_robust_loss_fwd(
        _ptr_array(flows), _ptr_array(certs), len(flows), ptr(H), ptr(im_A_coords), ptr(prev_epe), ph, pw, float(prev_thresh), ptr(epe),
        ptr(stats), B, h, w, float(ext_a), float(ext_b), float(a), float(cs), float(ce_weight), float(iteration_base), float(pck_thresh),
        ptr(ws), nws, stream_ptr(dev)))
    return stats, epe


def robust_loss_scale_bwd(grad_out, stats, flows, certs, H, ext_a, ext_b, a, cs, ce_weight, iteration_base, prev_epe=None,
                          prev_thresh=0.0, im_A_coords=None, need_flow=None, need_cert=None):
    """Gradients of robust_loss_scale_fwd's loss with respect to the flows and certainties, times grad_out (a 0-dim float32 DEVICE
    tensor: no host round trip); `stats` as the forward left it.  need_flow / need_cert: one bool per iteration (default: all).
    Returns (g_flows, g_certs), lists with None where not asked for.  One launch; none when nothing is asked for."""
    n = len(flows)
    need_flow = [True] * n if need_flow is None else list(need_flow)
    need_cert = [True] * n if need_cert is None else list(need_cert)
    dev = require_gpu(grad_out, stats, *flows, *certs, H, prev_epe, im_A_coords)
    B, h, w, ph, pw = _robust_loss_scale_args("robust_loss_scale_bwd", flows, certs, H, prev_epe, im_A_coords)
    if grad_out.numel() != 1 or grad_out.dtype != torch.float32:
        raise ValueError(f"robust_loss_scale_bwd: grad_out must be one float32 value, got {tuple(grad_out.shape)} {grad_out.dtype}")
    g_flows = [torch.empty_like(f) if nf else None for f, nf in zip(flows, need_flow)]
    g_certs = [torch.empty_like(c) if nc else None for c, nc in zip(certs, need_cert)]
    mask = sum(1 << k for k in range(n) if need_flow[k]) | sum(1 << (_lib.RL_MAX_ITR + k) for k in range(n) if need_cert[k])
    if mask:
        _timed("robust_loss_bwd_%dx%d" % (h, w), lambda: _L().gfn_robust_loss_bwd(
            _ptr_array(flows), _ptr_array(certs), n, ptr(H), ptr(im_A_coords), ptr(prev_epe), ph, pw, float(prev_thresh), ptr(stats),
            ptr(grad_out), _ptr_array(g_flows), _ptr_array(g_certs), mask, B, h, w, float(ext_a), float(ext_b), float(a), float(cs),
            float(ce_weight), float(iteration_base), stream_ptr(dev)))
    return g_flows, g_certs


def gt_warp_homography(H, h, w, ext_a, ext_b, im_A_coords=None, normalized=True, return_x1_n=False):
    """get_gt_warp_homography (losses/robust_loss.py:9-42) for an h x w grid: H (B,3,3) -> (x2_n or x2 (B,h,w,2), prob (B,h,w),
    x1_n (B,h,w,2) or None).  ext_a / ext_b: im_A.shape[2] - 1 and im_B.shape[2] - 1."""
    dev = require_gpu(H, im_A_coords)
    if H.dim() != 3 or tuple(H.shape[1:]) != (3, 3):
        raise ValueError(f"gt_warp_homography: H must be (B,3,3), got {tuple(H.shape)}")
    B = H.shape[0]
    H = f32c(H)
    if im_A_coords is not None:
        if tuple(im_A_coords.shape) != (B, 2, h, w):
            raise ValueError(f"gt_warp_homography: im_A_coords must be {(B, 2, h, w)}, got {tuple(im_A_coords.shape)}")
        im_A_coords = f32c(im_A_coords)
    out = torch.empty((B, h, w, 2), device=dev, dtype=torch.float32)
    prob = torch.empty((B, h, w), device=dev, dtype=torch.float32)
    x1n = torch.empty((B, h, w, 2), device=dev, dtype=torch.float32) if return_x1_n else None
    _L().gfn_gt_warp_homography_fwd(ptr(H), ptr(im_A_coords), ptr(out), ptr(prob), ptr(x1n), B, h, w, float(ext_a), float(ext_b),
                                    1 if normalized else 0, stream_ptr(dev))
    return out, prob, x1n


class _RobustLossFn(torch.autograd.Function):
    """The whole loss: forward runs the scales in order (each hands its last end-point error to the next), backward issues one launch
    per scale.  `scales` is a tuple of per-scale dicts (n, a, cs, pck, narrowed, prev_thresh), `common` = (ext_a, ext_b, ce_weight,
    iteration_base); `maps` the flat list per scale of its flows, then its certainties.  Saved: the maps, H, each scale's prev_epe,
    the statistics."""

    @staticmethod
    def forward(ctx, scales, common, H, stats, *maps):
        ext_a, ext_b, ce_weight, iteration_base = common
        maps = [m.detach() for m in maps]
        prev, prevs, at = None, [], 0
        for i, sc in enumerate(scales):
            n = sc["n"]
            flows, certs = maps[at:at + n], maps[at + n:at + 2 * n]
            at += 2 * n
            pe = prev if sc["narrowed"] else None
            prevs.append(pe)
            want = i + 1 < len(scales) and scales[i + 1]["narrowed"]
            _, prev = robust_loss_scale_fwd(flows, certs, H, ext_a, ext_b, sc["a"], sc["cs"], ce_weight, iteration_base, sc["pck"], prev_epe=pe,
                                            prev_thresh=sc["prev_thresh"], want_epe=want, stats=stats[i])
        ctx.save_for_backward(H, stats, *maps)
        ctx.prevs, ctx.scales, ctx.common = prevs, scales, common
        return stats[:, _lib.RL_STAT_LOSS].sum()

    @staticmethod
    def backward(ctx, grad_out):
        H, stats, *maps = ctx.saved_tensors
        ext_a, ext_b, ce_weight, iteration_base = ctx.common
        grad_out = f32c(grad_out)
        need = ctx.needs_input_grad[4:]
        grads, at = [], 0
        for i, sc in enumerate(ctx.scales):
            n = sc["n"]
            gf, gc = robust_loss_scale_bwd(grad_out, stats[i], maps[at:at + n], maps[at + n:at + 2 * n], H, ext_a, ext_b, sc["a"], sc["cs"],
                                           ce_weight, iteration_base, prev_epe=ctx.prevs[i], prev_thresh=sc["prev_thresh"],
                                           need_flow=need[at:at + n], need_cert=need[at + n:at + 2 * n])
            grads += gf + gc
            at += 2 * n
        return (None, None, None, None) + tuple(grads)


def robust_loss(scales, H, ext_a, ext_b, ce_weight, iteration_base, maps):
    """The sum over `scales` of ce_weight * ce_s + reg_s (losses/robust_loss.py:92-128), differentiable in every flow and certainty.
    scales: per scale a dict with n (iterations), a (alpha), cs (c * scale), pck (the pck_05 threshold), narrowed (multiply the mask
    by the previous scale's end-point error below prev_thresh) and prev_thresh; maps: per scale its n flows (B,2,h,w), then its n
    certainties (B,1,h,w).  Returns (loss, stats): a 0-dim tensor and the (len(scales), RL_STATS) statistics, one row per scale
    (ce, reg, count, pck_05 ...: include/gfnet_hip.h).  No host synchronisation; valid under stream capture."""
    dev = require_gpu(H, *maps)
    if sum(2 * sc["n"] for sc in scales) != len(maps):
        raise ValueError("robust_loss: every scale needs n flows followed by n certainties")
    if scales and scales[0]["narrowed"]:
        raise ValueError("robust_loss: the first scale cannot be narrowed, no previous end-point error exists")
    if not scales:
        raise ValueError("robust_loss: no scales")
    stats = torch.empty((len(scales), _lib.RL_STATS), device=dev, dtype=torch.float32)
    maps = [f32c(m) for m in maps]
    loss = _RobustLossFn.apply(tuple(scales), (float(ext_a), float(ext_b), float(ce_weight), float(iteration_base)), f32c(H).detach(), stats,
                               *maps)
    return loss, stats


# ---- training pairs (datasets/generate_random_H_large_size.py, csrc/pair_synth.hip) ---------------------------------------------------
def get_perspective_transform(src, dst, return_ok=False):
    """kornia's get_perspective_transform (generate_random_H_large_size.py:30, 71) for n four-point problems, solved in double on the
    device: src, dst (n,4,2) or (4,2) -> H (n,3,3) float64 with H[2,2] = 1 and dst ~ H src.  return_ok: also the (n,) int32 flags,
    0 where the source points are degenerate (H is then the identity)."""
    dev = require_gpu(src, dst)
    s, d = f32c(src).reshape(-1, 4, 2), f32c(dst).reshape(-1, 4, 2)
    if s.shape != d.shape:
        raise ValueError(f"get_perspective_transform: src {tuple(src.shape)} and dst {tuple(dst.shape)} differ")
    n = s.shape[0]
    H = torch.empty((n, 3, 3), device=dev, dtype=torch.float64)
    ok = torch.empty((n,), device=dev, dtype=torch.int32)
    _L().gfn_perspective_from_points(ptr(s), ptr(d), ptr(H), ptr(ok), n, stream_ptr(dev))
    return (H, ok) if return_ok else H


def _source_table(imgs, what):
    """The per-sample source records of gfn_warp_perspective_fwd for a (B,C,H,W) tensor or a list of (C,H,W) tensors: returns
    (device pointer array, device (B,3) int32 rows (H, W, channel stride), the tensors the pointers name, C).  A sample is read in
    place when its rows are dense (stride W) -- any batch and channel stride, so views of larger buffers are not copied."""
    samples = list(imgs.unbind(0)) if isinstance(imgs, torch.Tensor) and imgs.dim() == 4 else list(imgs)
    if not samples:
        raise ValueError(f"{what}: no images")
    dev = require_gpu(*samples)
    C, keep, rows = samples[0].shape[0], [], []
    for t in samples:
        if t.dim() != 3 or t.shape[0] != C or t.shape[1] < 1 or t.shape[2] < 1:
            raise ValueError(f"{what}: every image must be (C,H,W) with C = {C}, got {tuple(t.shape)}")
        if t.dtype != torch.float32:
            t = t.float()
        _, h, w = t.shape
        if t.stride(2) != 1 or (h > 1 and t.stride(1) != w) or (C > 1 and t.stride(0) < h * w):
            t = t.contiguous()
        if h * w >= 2 ** 31:
            raise ValueError(f"{what}: an image of {h} x {w} pixels is too large (pixel offsets are 32-bit)")
        keep.append(t)
        rows.append((h, w, t.stride(0) if C > 1 else h * w))
    B = len(keep)
    host = torch.empty(B + (3 * B + 1) // 2, dtype=torch.int64)  # B pointers, then the (B,3) int32 records: one upload
    host[:B] = torch.tensor([t.data_ptr() for t in keep], dtype=torch.int64)
    host[B:].view(torch.int32)[:3 * B] = torch.tensor(rows, dtype=torch.int32).reshape(-1)
    table = host.to(dev)
    return table[:B], table[B:].view(torch.int32), keep, C


_norm_constants = {}


def _mean_std(dev, mean, std, C):
    """(mean, std) of a Normalize as device tensors of C floats, uploaded once per (device, values)"""
    if (mean is None) != (std is None):
        raise ValueError("warp_perspective: mean and std go together")
    if mean is None:
        return None, None
    key = (dev.type, dev.index, tuple(float(v) for v in mean), tuple(float(v) for v in std))
    if len(key[2]) != C or len(key[3]) != C:
        raise ValueError(f"warp_perspective: mean and std need {C} values each")
    if key not in _norm_constants:
        _norm_constants[key] = (torch.tensor(key[2], dtype=torch.float32, device=dev), torch.tensor(key[3], dtype=torch.float32, device=dev))
    return _norm_constants[key]


def _warp(imgs, M, invert, dsize, mean=None, std=None, what="warp_perspective"):
    """gfn_warp_perspective_fwd: output pixel -> source pixel through M (B,3,3) float64 on the device (inverted there first when
    `invert`); imgs as _source_table takes them.  Returns (B,C,Ho,Wo) float32."""
    planes, dims, keep, C = _source_table(imgs, what)
    dev, B = planes.device, planes.shape[0]
    if M.shape != (B, 3, 3) or M.dtype != torch.float64 or M.device != dev or not M.is_contiguous():
        raise ValueError(f"{what}: M must be a contiguous ({B},3,3) float64 tensor on {dev}, got {tuple(M.shape)} {M.dtype} on {M.device}")
    Ho, Wo = int(dsize[0]), int(dsize[1])
    m, s = _mean_std(dev, mean, std, C)
    out = torch.empty((B, C, Ho, Wo), device=dev, dtype=torch.float32)
    _timed("warp_perspective", lambda: _L().gfn_warp_perspective_fwd(ptr(planes), ptr(dims), ptr(M), int(bool(invert)), ptr(out), C * Ho * Wo,
                                                                     B, C, Ho, Wo, ptr(m), ptr(s), stream_ptr(dev)))
    del keep  # (alive until after the launch; the allocator's reuse is ordered on this stream)
    return out


def warp_perspective(img, H, dsize, mean=None, std=None):
    """kornia's warp_perspective(img, H, dsize, mode="bilinear", padding_mode="zeros", align_corners=True)
    (generate_random_H_large_size.py:33, 83): H (B,3,3) maps source pixels to destination pixels and is inverted on the device in
    double; pixel coordinates are evaluated in double, the blend is fp32.  img: (B,C,H,W) or a list of (C,H,W) tensors, which may
    differ in size; dsize = (height, width).  mean / std (C values each): (v - mean[c]) / std[c] fused into the launch."""
    require_gpu(H)
    return _warp(img, H.to(torch.float64).reshape(-1, 3, 3).contiguous(), True, dsize, mean, std)


def random_h_params(draws, crop_size, deform_area, final_size):
    """gfn_random_h_params: draws (B,18) int32 on the device -> dict of H_s2t (B,3,3) float32, H_s2t64, M_A, M_B (B,3,3) float64 and
    ok (B,) int32; M_A and M_B are views of one (2B,3,3) tensor "M"."""
    dev = require_gpu(draws)
    if draws.dim() != 2 or draws.shape[1] != 18 or draws.dtype != torch.int32:
        raise ValueError(f"random_h_params: draws must be (B,18) int32, got {tuple(draws.shape)} {draws.dtype}")
    d = draws.contiguous()
    B = d.shape[0]
    centre = int(crop_size) - 2 * (int(deform_area) // 2)
    H32 = torch.empty((B, 3, 3), device=dev, dtype=torch.float32)
    H64 = torch.empty((B, 3, 3), device=dev, dtype=torch.float64)
    M = torch.empty((2 * B, 3, 3), device=dev, dtype=torch.float64)
    ok = torch.empty((B,), device=dev, dtype=torch.int32)
    _L().gfn_random_h_params(ptr(d), B, int(crop_size), int(deform_area), centre, centre, int(final_size[0]), int(final_size[1]), ptr(H32),
                             ptr(H64), ptr(M[:B]), ptr(M[B:]), ptr(ok), stream_ptr(dev))
    return {"H_s2t": H32, "H_s2t64": H64, "M": M, "M_A": M[:B], "M_B": M[B:], "ok": ok}


def random_h_batch(imgs_a, imgs_b, draws, crop_size, input_size, deformation_ratio, bi, normalize=True, return_warped=False):
    """randomH (generate_random_H_large_size.py:38-85) for a batch, after its pre-resize: imgs_a / imgs_b are B pairs of equally sized
    (3,h,w) device images in [0,1] with h, w > crop_size (lists, or (B,3,h,w) tensors), draws the (B,18) int32 rows of
    datasets.draw_random_h, input_size the final (h, w).  One parameter launch, then ONE warp launch for all 2B images: crop, warp and
    centre crop are a single projective map per image (M_A, M_B), read straight from the sources.  Where the centre crop already has
    input_size the ImageNet Normalize (normalize=True) is fused into that launch; otherwise the warp writes un-normalised centre
    crops and resize_normalise (bicubic) makes the final images, H_s2t carrying the rescale of :77-79.
    Returns a dict: im_A (the imgs_a image under H_1t), im_B (imgs_b under H_2t; the plain centre crop when not bi), both
    (B,3,h,w) float32; H_s2t (B,3,3) float32, im_A pixels -> im_B pixels; H_s2t64, M_A, M_B (float64), ok (B,) int32; and with
    return_warped, warped_img1: the un-normalised im_A warped by H_s2t (:83; two or three more launches)."""
    a = list(imgs_a.unbind(0)) if isinstance(imgs_a, torch.Tensor) else list(imgs_a)
    b = list(imgs_b.unbind(0)) if isinstance(imgs_b, torch.Tensor) else list(imgs_b)
    if len(a) != len(b) or not a:
        raise ValueError(f"random_h_batch: {len(a)} and {len(b)} images")
    B = len(a)
    for x, y in zip(a, b):
        if x.shape != y.shape or x.dim() != 3 or x.shape[0] != 3:
            raise ValueError(f"random_h_batch: a pair must be two (3,h,w) images of one size, got {tuple(x.shape)} and {tuple(y.shape)}")
        if x.shape[1] <= crop_size or x.shape[2] <= crop_size:
            raise ValueError(f"random_h_batch: a {x.shape[1]} x {x.shape[2]} image does not hold a {crop_size} crop (pre-resize it, :45-48)")
    dev = require_gpu(*a, *b)
    crop_size = int(crop_size)
    deform_area = int(crop_size * deformation_ratio)  # :57
    d2 = deform_area // 2
    centre = crop_size - 2 * d2
    out_h, out_w = int(input_size[0]), int(input_size[1])
    draws = torch.as_tensor(draws).to(torch.int32).reshape(B, 18).clone()
    if not bi:  # :27-28 -- image 2's source points are the target points: H_2t is the identity
        draws[:, 10:18] = torch.tensor([d2, d2, crop_size - d2 - 1, d2, crop_size - d2 - 1, crop_size - d2 - 1, d2, crop_size - d2 - 1],
                                       dtype=torch.int32, device=draws.device)
    prm = random_h_params(draws.to(dev), crop_size, deform_area, (out_h, out_w))
    fused = (centre, centre) == (out_h, out_w)
    mean, std = (IMAGENET_MEAN, IMAGENET_STD) if normalize else ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    norm_in_warp = fused and normalize
    both = _warp(a + b, prm["M"], False, (centre, centre), mean if norm_in_warp else None, std if norm_in_warp else None, "random_h_batch")
    final = both if fused else resize_normalise(both, (out_h, out_w), "bicubic", mean, std)
    out = {"im_A": final[:B], "im_B": final[B:], "H_s2t": prm["H_s2t"], "H_s2t64": prm["H_s2t64"], "M_A": prm["M_A"], "M_B": prm["M_B"],
           "ok": prm["ok"]}
    if return_warped:
        if not fused:
            raw_a = resize_normalise(both[:B], (out_h, out_w), "bicubic", (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
        else:
            raw_a = _warp(a, prm["M_A"].contiguous(), False, (centre, centre), what="random_h_batch") if norm_in_warp else both[:B]
        out["warped_img1"] = _warp(raw_a, prm["H_s2t64"], True, (out_h, out_w), what="random_h_batch")
    return out


# ---- photometric augmentation (train.py:74-79, :88-93 initial_transforms; csrc/photometric.hip) -------------------------------------------
PHOTO_OPS = ("brightness", "contrast", "saturation", "hue")  # GFN_PHOTO_* in this order: ColorJitter's fn_idx


def resize_output_size(h, w, size):
    """(h', w') of torchvision's Resize(size) with an int: the short side becomes `size`, the long side int(size * long / short);
    unchanged when the short side already equals `size`."""
    short, long = (w, h) if w <= h else (h, w)
    if short == size:
        return h, w
    new_long = int(size * long / short)
    return (new_long, size) if w <= h else (size, new_long)


@functools.lru_cache(maxsize=256)
def resize_axis_table(n_in, n_out):
    """One axis of Image.resize(BILINEAR) as gfn_photo_resize_u8 reads it: (int32 array of n_out (min, count) pairs, then n_out rows of
    `taps` weights; taps).  Resample.c's precompute_coeffs and normalize_coeffs_8bpc, in double, in its order of operations."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 1.0 * fs
    taps = int(math.ceil(support)) * 2 + 1
    centre = (np.arange(n_out) + 0.5) * scale
    ss = 1.0 / fs
    lo = np.maximum((centre - support + 0.5).astype(np.int64), 0)
    count = np.minimum((centre + support + 0.5).astype(np.int64), n_in) - lo
    k = np.arange(taps)
    x = np.abs(((k[None, :] + lo[:, None]) - centre[:, None] + 0.5) * ss)
    w = np.where((x < 1.0) & (k[None, :] < count[:, None]), 1.0 - x, 0.0)
    total = np.zeros(n_out)
    for j in range(taps):  # summed in tap order, as the C loop does
        total = total + w[:, j]
    w = np.where(total[:, None] != 0.0, w / np.where(total == 0.0, 1.0, total)[:, None], w)
    fixed = (0.5 + w * (1 << 22)).astype(np.int64)
    table = np.concatenate([np.stack([lo, count], 1).reshape(-1), fixed.reshape(-1)]).astype(np.int32)
    table.setflags(write=False)
    return table, taps


def box_blur_radius(radius):
    """The fractional box radius of ImageFilter.GaussianBlur(radius)'s three box passes (BoxBlur.c _gaussian_blur_radius), with its
    float variables and double intermediates."""
    f32 = np.float32
    sigma2 = f32(f32(radius) * f32(radius) / f32(3))
    L = f32(math.sqrt(12.0 * float(sigma2) + 1.0))
    l = f32(math.floor((float(L) - 1.0) / 2.0))
    a = f32(f32(f32(2) * l + f32(1)) * f32(f32(l * f32(l + f32(1))) - f32(f32(3) * sigma2)))
    a = f32(a / f32(f32(6) * f32(sigma2 - f32(f32(l + f32(1)) * f32(l + f32(1))))))
    return float(f32(l + a))


def _photo_records(params, n):
    """The (n, GFN_PHOTO_REC) int32 records of gfn_photo_jitter_blur from n dicts with the keys of datasets.draw_photometric."""
    if len(params) != n:
        raise ValueError(f"photo_augment: {len(params)} parameter records for {n} images")
    rec = np.zeros((n, _lib.PHOTO_REC), dtype=np.int32)
    flt = rec.view(np.float32)
    for i, p in enumerate(params):
        order = [int(v) for v in p.get("order", (0, 1, 2, 3))]
        if sorted(order) != [0, 1, 2, 3]:
            raise ValueError(f"photo_augment: order must be a permutation of 0..3, got {order}")
        rec[i, :4] = order
        mask = 0
        for k, name in enumerate(PHOTO_OPS[:3]):
            v = p.get(name)
            if v is not None:
                if not v >= 0.0:
                    raise ValueError(f"photo_augment: {name} factor {v} is negative")
                flt[i, 4 + k] = v
                mask |= 1 << k
        if p.get("hue") is not None:
            if not -0.5 <= p["hue"] <= 0.5:
                raise ValueError(f"photo_augment: hue factor {p['hue']} is not in [-0.5, 0.5]")
            rec[i, 7] = int(p["hue"] * 255) & 255
            mask |= 1 << _lib.PHOTO_HUE
        rec[i, 8] = 1 if p.get("grayscale") else 0
        if p.get("blur_radius"):
            R = box_blur_radius(p["blur_radius"])
            if not 0.0 <= R < 2.0:
                raise ValueError(f"photo_augment: blur radius {p['blur_radius']} gives a box radius of {R}; the kernel's halo holds < 2")
            flt[i, 9] = R
        rec[i, 10] = mask
    return rec


def _photo_images(images, what):
    samples = list(images.unbind(0)) if isinstance(images, torch.Tensor) and images.dim() == 4 else list(images)
    dev = require_gpu(*samples)
    keep = []
    for t in samples:
        if t.dim() != 3 or t.shape[2] != 3 or t.dtype != torch.uint8 or t.shape[0] < 1 or t.shape[1] < 1:
            raise ValueError(f"{what}: every image must be (h,w,3) uint8, got {tuple(t.shape)} {t.dtype}")
        h, w, _ = t.shape
        if h > 32768 or w > 32768:
            raise ValueError(f"{what}: an image of {h} x {w} pixels is too large (32768 per side)")
        if t.stride(2) != 1 or t.stride(1) != 3 or (h > 1 and t.stride(0) < 3 * w) or t.stride(0) >= 2 ** 31:
            t = t.contiguous()
        keep.append(t)
    return keep, dev


def _photo_run(images, size, params, out, what):
    """Resize (size not None) and / or augment (params not None) a batch: ONE upload of every table, then at most three launches
    (resize, stats when some image has contrast on, jitter + blur), whatever the number of images; no host synchronisation."""
    if out not in ("float", "uint8"):
        raise ValueError(f"{what}: out must be 'float' or 'uint8', got {out!r}")
    keep, dev = _photo_images(images, what)
    n = len(keep)
    if n == 0:
        return []
    if n > 65535:
        raise ValueError(f"{what}: {n} images in one batch (at most 65535)")
    mid_hw = [resize_output_size(t.shape[0], t.shape[1], int(size)) if size is not None else (t.shape[0], t.shape[1]) for t in keep]
    resized = [i for i, t in enumerate(keep) if mid_hw[i] != (t.shape[0], t.shape[1])]
    mid = list(keep)
    if resized:
        buf = torch.empty(sum(3 * mid_hw[i][0] * mid_hw[i][1] for i in resized), device=dev, dtype=torch.uint8)
        off = 0
        for i in resized:
            h, w = mid_hw[i]
            mid[i] = buf[off:off + 3 * h * w].view(h, w, 3)
            off += 3 * h * w
    res = mid
    if not resized and params is None:
        return res  # nothing to resize: no table, no launch
    if params is not None:
        rec = _photo_records(params, n)
        per = 3 if out == "uint8" else 12  # bytes per pixel: float planes start on 4-byte boundaries
        buf = torch.empty(sum(per * h * w for h, w in mid_hw), device=dev, dtype=torch.uint8)
        res, off = [], 0
        for h, w in mid_hw:
            piece = buf[off:off + per * h * w]
            res.append(piece.view(h, w, 3) if out == "uint8" else piece.view(torch.float32).view(3, h, w))
            off += per * h * w
    # the tables, in one host array: n source, n intermediate and n output pointers and n zeroed sums (int64), then (int32) the
    # source and intermediate (H, W, row stride) rows, the resize records, the chain records and the coefficient tables
    RZ, PR = _lib.PHOTO_RESIZE_REC, _lib.PHOTO_REC
    coef, coef_at, rz = [], {}, np.zeros((n, RZ), dtype=np.int32)
    for i in resized:
        (h, w, _), (ho, wo) = keep[i].shape, mid_hw[i]
        at = []
        for key in ((w, wo), (h, ho)):
            if key not in coef_at:
                table, taps = resize_axis_table(*key)
                coef_at[key] = (sum(len(c) for c in coef), taps)
                coef.append(table)
            at.extend(coef_at[key])
        rz[i] = (ho, wo, *at)

    def dims(ts):  # (H, W, row stride in bytes): a view that was not resized keeps its own stride as the intermediate image too
        return np.array([(t.shape[0], t.shape[1], t.stride(0) if t.shape[0] > 1 else 3 * t.shape[1]) for t in ts], dtype=np.int32).reshape(-1)

    ints = [dims(keep), dims(mid), rz.reshape(-1),
            rec.reshape(-1) if params is not None else np.zeros(n * PR, dtype=np.int32)] + coef
    n_int = sum(len(a) for a in ints)
    host = np.zeros(4 * n + (n_int + 1) // 2, dtype=np.int64)
    host[:n] = [t.data_ptr() for t in keep]
    host[n:2 * n] = [t.data_ptr() for t in mid]
    host[2 * n:3 * n] = [t.data_ptr() for t in res]
    host[4 * n:].view(np.int32)[:n_int] = np.concatenate(ints)
    table = torch.from_numpy(host).to(dev)
    tab32 = table[4 * n:].view(torch.int32)
    src_dims, mid_dims, recs, prm, coefs = tab32[:3 * n], tab32[3 * n:6 * n], tab32[6 * n:6 * n + RZ * n], \
        tab32[(6 + RZ) * n:(6 + RZ + PR) * n], tab32[(6 + RZ + PR) * n:]
    stream = stream_ptr(dev)
    if resized:
        _timed("photo_resize", lambda: _L().gfn_photo_resize_u8(ptr(table[:n]), ptr(src_dims), ptr(table[n:2 * n]), ptr(recs), ptr(coefs), n,
                                                                 max(mid_hw[i][0] for i in resized), max(mid_hw[i][1] for i in resized), stream))
    if params is not None:
        sums = table[3 * n:4 * n]
        contrast = [mid_hw[i] for i in range(n) if (rec[i, 10] >> _lib.PHOTO_CONTRAST) & 1]
        if contrast:
            _timed("photo_stats", lambda: _L().gfn_photo_stats(ptr(table[n:2 * n]), ptr(mid_dims), ptr(prm), ptr(sums), n,
                                                               max(h for h, _ in contrast), max(w for _, w in contrast), stream))
        _timed("photo_jitter_blur", lambda: _L().gfn_photo_jitter_blur(ptr(table[n:2 * n]), ptr(mid_dims), ptr(prm), ptr(sums), ptr(table[2 * n:3 * n]),
                                                                       int(out == "uint8"), n, max(h for h, _ in mid_hw),
                                                                       max(w for _, w in mid_hw), stream))
    del keep, mid  # (alive until after the launches; the allocator's reuse is ordered on this stream)
    return res


def photo_resize(images, size):
    """torchvision's Resize(size) on PIL images (train.py:75), i.e. Pillow's Image.resize(BILINEAR), for a batch: images is a list of
    (h,w,3) uint8 device tensors of any sizes, or one (N,h,w,3) tensor.  Returns a list of (h',w',3) uint8 tensors, bit for bit
    Pillow's; an image whose short side already is `size` comes back as it is.  One upload and one launch."""
    return _photo_run(images, int(size), None, "uint8", "photo_resize")


def photo_augment(images, params, out="float", resize=None):
    """ColorJitter, RandomGrayscale, RandomGaussianBlur and ToTensor (train.py:76-78, :89-92) with Pillow's arithmetic for a batch of
    (h,w,3) uint8 device images (a list, or one (N,h,w,3) tensor).  params: one dict per image as datasets.draw_photometric makes
    them -- "order" (a permutation of 0..3 = brightness, contrast, saturation, hue), "brightness" / "contrast" / "saturation" / "hue"
    (a factor, or None = off), "grayscale" (bool), "blur_radius" (GaussianBlur's radius, or None).  out="float": a list of (3,h,w)
    float32 tensors = u8 / 255 (ToTensor); "uint8": (h,w,3) uint8.  resize: first Resize(resize), in the same upload.  One upload
    and at most two launches (three with resize), whatever the number of images."""
    return _photo_run(images, resize, list(params), out, "photo_augment")
