"""The cross-view decoder's bf16 class on the GPU: ops.cross_attention_bf16 (GFN_BF16 in csrc/cross_attn.hip), the decoder block ops
with dtype=torch.bfloat16 (the gfn_decoder_*_bf16_* entry points of csrc/decoder_block.hip), CrossViewDecoder under bf16 autocast
and ReferenceBackbone(amp_dtype=torch.bfloat16).  Inputs, definitions, parameter sets and cases are those of test_cross_attn_gpu.py,
test_decoder_block_gpu.py and test_decoder_train_gpu.py, with what those round to fp16 rounded to bf16 instead.

Attention.  Oracle: ops.reference_cross_attention and its autograd in float64 on the CPU, on the bf16-representable values the
kernel receives.  Bounds: the fp16 class's with bf16's half-ulp 2^-8 in place of 2^-11:
  forward   2^-8 * max|out| + the fp32 bound (the one final rounding; P is not rounded)        lse   the fp32 bound
  backward  4 * E_bf16 + 2^-8 * max|grad|; E_bf16 = the float64 error of `emulate_bf16_class`, test_cross_attn_gpu.py's
            emulate_fp16_class restated with .bfloat16() roundings: a CPU emulation written here, never the kernel.

Blocks and module.  Oracle: float64 autograd through definition_qkv / definition_post (the module: attn_impl="torch" in float64).
Unit: e_bf16 = the error of the same expression from torch on the CPU under torch.autocast("cpu", dtype=torch.bfloat16) against
that float64 result, per case and per tensor, never fixed.  Bound: 4 * e_bf16, the project's bound for an autocast class.  A unit of
zero is treated as in test_decoder_train_gpu.py: only where the oracle is exactly zero too (the constant family's wproj and gamma1
gradients), and there the kernels owe exact zeros.

Every comparison prints err, unit or bound, and their ratio before it asserts.  MEASURED below holds the worst ratios.
"""
import functools
import math

import pytest
import synth
import torch

import test_cross_attn_gpu as att
import test_decoder_block_gpu as blk
import test_decoder_train_gpu as trn
from gfnet_amd import ops
from test_decoder_bf16_cpu import autocast_bf16, bf, post_grads, qkv_grads

pytestmark = pytest.mark.gpu

# worst err / bound per tensor on an MI355X (filled in from the figures the tests print)
MEASURED = """
attention    out 0.42 (1x32x32x1 normal: err 1.9e-03, bound 4.6e-03)   lse 0.20 (1x1600x1600x8)   dq 0.25   dk 0.25   dv 0.20
             range case (dv up to 7.5e4, past fp16): all finite, dq 0.25, dk 0.25, dv 0.18 (err 1.9e+02 against a bound of 1.0e+03)
post         X_out 0.21 ((2, 37) large)   gX 0.27   g_attn 0.30 ((2, 1) mean50)   wproj 0.24   bproj 0.22   gamma1 0.22   norm2 weight 0.28
             norm2 bias 0.27   w1 0.33 ((2, 1) mean50: err 3.3e-02 against e_bf16 2.5e-02)   b1 0.22   w2 0.24   b2 0.00   gamma2 0.23
qkv          q, k, v 0.25 (the error equals the unit: both are one bf16 rounding of the result)   gX 0.23   wq 0.18   wk 0.20   wv 0.18
             norm1 weight 0.25   norm1 bias 0.25
module       torch blocks around the bf16 attention: maps 0.24 / 0.26.  block_impl="hip": maps 0.17 / 0.21.  train_block_impl="hip":
             maps 0.17 / 0.21, input gradients 0.18 / 0.30, parameter gradients 0.42 at worst (cross_attn_blocks.0.norm1.bias: err
             9.9e-02 against e_bf16 5.9e-02)
"""

DEV = "cuda"
BF16 = torch.bfloat16
EPS, C = trn.EPS, trn.C
HALF_ULP = 2.0 ** -8


# ---- attention ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def attn_inputs(shape, family):
    """test_cross_attn_gpu.inputs with q, k, v and dout rounded on to bf16-representable values (the scale stays the family's)."""
    q, k, v, dout, scale = att.inputs(shape, family)
    return bf(q), bf(k), bf(v), bf(dout), scale


def emulate_bf16_class(q, k, v, dout, scale):
    """The kernel's bf16 numeric class on the CPU: bf16 values in, every product and sum fp32, delta = sum_j P dP / sum_j P, P and dS
    kept fp32, results rounded to bf16.  (dq, dk, dv) as float64."""
    s = torch.einsum("bihd,bjhd->bhij", q, k) * scale
    p = torch.softmax(s, dim=-1)
    dp = torch.einsum("bihd,bjhd->bhij", dout, v)
    delta = (p * dp).sum(-1, keepdim=True) / p.sum(-1, keepdim=True)
    ds = p * (dp - delta)
    dq = torch.einsum("bhij,bjhd->bihd", ds, k) * scale
    dk = torch.einsum("bhij,bihd->bjhd", ds, q) * scale
    dv = torch.einsum("bhij,bihd->bjhd", p, dout)
    return tuple(t.bfloat16().double() for t in (dq, dk, dv))


def attn_bounds(q, k, v, dout, scale):
    """(float64 results, per-tensor bounds of the bf16 class) for out, lse, dq, dk, dv."""
    o64 = att.reference(q, k, v, dout, scale, torch.float64)
    o32 = att.reference(q.clone(), k.clone(), v.clone(), dout, scale, torch.float32)  # (it marks fp32 inputs as leaves in place)
    b32 = [max(4 * float((a - b).abs().max()), 2.0 ** -20 * float(o.abs().max())) for a, b, o in zip(o32, o64, o64)]
    ebf = [float((a - b).abs().max()) for a, b in zip(emulate_bf16_class(q, k, v, dout, scale), o64[2:])]
    bounds = [HALF_ULP * float(o64[0].abs().max()) + b32[0], b32[1]] + [4 * e + HALF_ULP * float(o.abs().max()) for e, o in zip(ebf, o64[2:])]
    return o64, bounds


@functools.lru_cache(maxsize=None)
def attn_oracle(shape, family):
    return attn_bounds(*attn_inputs(shape, family))


def run_attention(shape, family, dout_scale=1.0):
    """(out, lse, dq, dk, dv) of ops.cross_attention_bf16 and its backward on the GPU, as float64 CPU tensors."""
    q, k, v, dout, scale = attn_inputs(shape, family)
    q, k, v = (t.to(DEV, BF16).requires_grad_() for t in (q, k, v))
    out, lse, *_ = ops.cross_attention_bf16_fwd(q.detach(), k.detach(), v.detach(), scale)
    got = ops.cross_attention_bf16(q, k, v, scale)
    assert torch.equal(got, out)  # the autograd path is the same launch
    grads = torch.autograd.grad(got, (q, k, v), (dout * dout_scale).to(DEV, BF16))
    assert got.dtype == BF16 and all(g.dtype == BF16 for g in grads) and lse.dtype == torch.float32
    return tuple(t.detach().double().cpu() for t in (out, lse) + tuple(grads))


def check_attention(shape, family):
    o64, bounds = attn_oracle(shape, family)
    got = run_attention(shape, family)
    rows = []
    for name, a, b, bound in zip(att.NAMES, got, o64, bounds):
        assert a.shape == b.shape, name
        assert torch.isfinite(a).all(), f"{name}: non-finite values"
        err = float((a - b).abs().max())
        print(f"attention bf16 {shape} {family} {name}: err {err:.3e} bound {bound:.3e} ratio {err / bound if bound else 0.0:.3f}")
        rows.append((name, err, bound))
    for name, err, bound in rows:
        assert err <= bound, (shape, family, name, err, bound)
    return got, bounds


@pytest.mark.parametrize("family", att.FAMILIES)
@pytest.mark.parametrize("shape", att.SMALL, ids=lambda s: "x".join(map(str, s)))
def test_attention_small_shapes_against_float64(shape, family):
    got, bounds = check_attention(shape, family)
    q, k, v, dout, scale = attn_inputs(shape, family)
    B, Nq, Nk, H = shape
    if family == "dominant":  # out is the dominating key's v, to the forward bound
        assert float((got[0] - v[:, torch.arange(Nq) % Nk].double()).abs().max()) <= bounds[0]
    if family == "scale0":  # out is the mean of v, lse = log Nk, and nothing flows to q and k
        assert float((got[0] - v.double().mean(1, keepdim=True)).abs().max()) <= bounds[0]
        assert float((got[1] - math.log(Nk)).abs().max()) <= bounds[1]
        assert not got[2].any() and not got[3].any()
    if family in ("max_last", "max_first"):  # the family is still what it says after the rounding to bf16
        s = torch.einsum("bihd,bjhd->bhij", q.double(), k.double())
        assert (s.argmax(-1) == (Nk - 1 if family == "max_last" else 0)).all()
    if Nk == 1:
        assert float((got[0] - v.double().expand(B, Nq, H, 8)).abs().max()) <= bounds[0]


def test_attention_the_560_pass_shape_against_float64():
    check_attention(att.BIG, "normal")


@pytest.mark.parametrize("shape", [att.SMALL[1], att.BIG], ids=lambda s: "x".join(map(str, s)))
def test_attention_forward_and_backward_are_deterministic(shape):
    a, b = run_attention(shape, "normal"), run_attention(shape, "normal")
    for name, x, y in zip(att.NAMES, a, b):
        assert torch.equal(x, y), name


def test_attention_has_fp32s_range_where_fp16_overflows():
    """The fp16 overflow case's input (dout / 16 scaled by 65536 on 1x129x33x8 max_first, where dv leaves fp16's range): every entry
    is finite and within the bf16 bound of the scaled problem.  No inf, no clamp."""
    shape, family, k_scale = att.SMALL[2], "max_first", 65536.0 / 16
    q, k, v, dout, scale = attn_inputs(shape, family)
    assert torch.equal(bf(dout * k_scale), dout * k_scale)  # (a power of two: the scaled dout is what the kernel receives)
    o64, bounds = attn_bounds(q, k, v, dout * k_scale, scale)
    assert float(o64[4].abs().max()) > 65504  # the case does leave fp16's range
    got = run_attention(shape, family, dout_scale=k_scale)
    for name, a, b, bound in list(zip(att.NAMES, got, o64, bounds))[2:]:
        err = float((a - b).abs().max())
        print(f"attention bf16 range {name}: max|ref| {float(b.abs().max()):.3e} err {err:.3e} bound {bound:.3e} ratio {err / bound:.3f}")
        assert torch.isfinite(a).all() and err <= bound, (name, err, bound)


def test_attention_names_keep_their_dtypes_apart():
    q = torch.zeros(1, 32, 4, 8, device=DEV)
    with pytest.raises(TypeError, match="bfloat16"):
        ops.cross_attention_bf16(q.half(), q.half(), q.half(), 1.0)
    with pytest.raises(TypeError, match="bfloat16"):
        ops.cross_attention_bf16(q, q, q, 1.0)
    with pytest.raises(TypeError, match="float16 or float32"):
        ops.cross_attention(q.bfloat16(), q.bfloat16(), q.bfloat16(), 1.0)


# ---- blocks ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def block_rows(shape, family):
    """test_decoder_train_gpu.rows with attn and the gradients of q, k, v rounded to bf16 (what the bf16 attention hands the blocks)."""
    X, attn, G = trn.rows(shape, family)
    G = G.clone()
    G[1:] = bf(G[1:])
    return X, attn.float().bfloat16(), G


@functools.lru_cache(maxsize=None)
def block_references(shape, family, which):
    """name -> (float64 result, e_bf16) for the forward outputs ("out"; "q", "k", "v" where the kernel writes them) and every gradient;
    computed once per case and shared."""
    X, attn, G = block_rows(shape, family)
    p = trn.block_params(family)
    if which == "post":
        (w_out, want), (e_out, emu) = (post_grads(X, attn, p, G[0], dt) for dt in (torch.float64, BF16))
        want, emu = {**want, "out": w_out}, {**emu, "out": e_out}
    else:
        (w_out, want), (e_out, emu) = (qkv_grads(X, p, G, dt) for dt in (torch.float64, BF16))
        want, emu = {**want, **dict(zip("qkv", w_out))}, {**emu, **dict(zip("qkv", e_out))}
    return {k: (want[k], float((emu[k] - want[k]).abs().max())) for k in want}


def compare(what, got, ref):
    want, unit = ref
    got = got.double().cpu().reshape(want.shape)
    err = float((got - want).abs().max())
    print(f"{what}: err {err:.3e}  e_bf16 {unit:.3e}  err / (4 e_bf16) {err / (4 * unit) if unit else float('inf'):.3f}"
          f"  max|ref| {float(want.abs().max()):.3e}")
    if not want.any() and unit == 0:
        # the constant family's attention rows and bproj are zero: the gradients of wproj and gamma1 are sums of exact zeros in float64
        # and under autocast alike, there is no unit to scale a bound with, and the kernels owe exact zeros
        assert what.endswith(("constant wproj", "constant g1")) and not got.any(), what
        return
    assert unit > 0, what
    assert torch.isfinite(got).all() and err <= 4 * unit, (what, err, 4 * unit)


def run_post(X, attn, p, **kw):
    return ops.decoder_post(X, attn, p.wproj, p.bproj, p.g1, p.nw2, p.nb2, EPS, p.w1, p.b1, p.w2, p.b2, p.g2, dtype=BF16, **kw)


def run_post_bwd(X, attn, p, G):
    return ops.decoder_post_bwd(X, attn, p.wproj, p.bproj, p.g1, p.nw2, p.nb2, EPS, p.w1, p.b1, p.w2, p.b2, p.g2, G, dtype=BF16)


def run_qkv(X, p):
    return ops.decoder_qkv(X, p.nw1, p.nb1, EPS, p.wq, p.wk, p.wv, dtype=BF16)


def run_qkv_bwd(X, p, G):
    gq, gk, gv = (g.bfloat16().reshape(X.shape[0], X.shape[1], 8, 8) for g in G[1:])
    return ops.decoder_qkv_bwd(X, p.nw1, p.nb1, EPS, p.wq, p.wk, p.wv, gq, gk, gv, dtype=BF16)


@pytest.mark.parametrize("shape,family", trn.CASES, ids=trn.IDS)
def test_post_forward_and_backward_against_float64_autograd(shape, family):
    X, attn, G = block_rows(shape, family)
    ref = block_references(shape, family, "post")
    p = trn.gpu(trn.block_params(family))
    with torch.no_grad():
        out = run_post(X.to(DEV), attn.to(DEV), p)
    got = run_post_bwd(X.to(DEV), attn.to(DEV), p, G[0].to(DEV))
    assert out.dtype == torch.float32 and out.shape == X.shape
    assert got[0].dtype == torch.float32 and got[1].dtype == BF16 and got[1].shape == attn.shape
    compare(f"decoder_post bf16 {shape} {family} out", out, ref["out"])
    for name, t in zip(trn.POST_NAMES, got):
        compare(f"decoder_post_bwd bf16 {shape} {family} {name}", t, ref[name])


@pytest.mark.parametrize("shape,family", trn.CASES, ids=trn.IDS)
def test_qkv_forward_and_backward_against_float64_autograd(shape, family):
    X, _, G = block_rows(shape, family)
    ref = block_references(shape, family, "qkv")
    p = trn.gpu(trn.block_params(family))
    with torch.no_grad():
        qkv = run_qkv(X.to(DEV), p)
    got = run_qkv_bwd(X.to(DEV), p, G.to(DEV))
    for name, t in zip("qkv", qkv):
        assert t.dtype == BF16 and t.shape == (shape[0], shape[1], 8, 8)
        compare(f"decoder_qkv bf16 {shape} {family} {name}", t, ref[name])
    for name, t in zip(trn.QKV_NAMES, got):
        assert t.dtype == torch.float32
        compare(f"decoder_qkv_bwd bf16 {shape} {family} {name}", t, ref[name])


def test_two_calls_give_the_same_bits_and_a_tokens_result_does_not_depend_on_its_tile():
    """67,584 rows: every output of two identical calls, forward and backward, is bit-identical, and with the tokens of both views
    permuted the same way the row-wise results (X_out, q, gX, g_attn, the qkv backward's gX) are the permuted results bit for bit."""
    X, attn, G = (t.to(DEV) for t in block_rows(trn.BIG, "normal"))
    p = trn.gpu(trn.params())
    perm = torch.randperm(trn.BIG[1], generator=torch.Generator().manual_seed(5)).to(DEV)
    with torch.no_grad():
        fwd, fwd2 = (run_post(X, attn, p),) + run_qkv(X, p), (run_post(X, attn, p),) + run_qkv(X, p)
        Xp, attnp, Gp = X[:, perm].contiguous(), attn[:, perm].contiguous(), G[:, :, perm].contiguous()
        fwdp = (run_post(Xp, attnp, p),) + run_qkv(Xp, p)
    post, post2 = run_post_bwd(X, attn, p, G[0]), run_post_bwd(X, attn, p, G[0])
    qkv, qkv2 = run_qkv_bwd(X, p, G), run_qkv_bwd(X, p, G)
    for a, b in zip(fwd + post + qkv, fwd2 + post2 + qkv2):
        assert torch.equal(a, b)
    postp, qkvp = run_post_bwd(Xp, attnp, p, Gp[0]), run_qkv_bwd(Xp, p, Gp)
    for view in (0, 1):
        for i in range(4):  # X_out, q, and k, v (which sit at the other view's entry in both calls alike)
            assert torch.equal(fwdp[i][view], fwd[i][view][perm]), i
        assert torch.equal(postp[0][view], post[0][view][perm]) and torch.equal(postp[1][view], post[1][view][perm])
        assert torch.equal(qkvp[0][view], qkv[0][view][perm])


def test_a_class_takes_its_own_element_only():
    """dtype=torch.bfloat16 with fp16 tensors raises TypeError, and the default class with bf16 tensors does too."""
    X, attn, G = (t.to(DEV) for t in block_rows((2, 37), "normal"))
    p = trn.gpu(trn.params())
    g16 = [g.half().reshape(2, 37, 8, 8) for g in G[1:]]
    with torch.no_grad():
        with pytest.raises(TypeError, match="attn must be bfloat16, got float16"):
            run_post(X, attn.half(), p)
        with pytest.raises(TypeError, match="attn must be bfloat16, got float16"):
            run_post_bwd(X, attn.half(), p, G[0])
        with pytest.raises(TypeError, match="gq must be bfloat16, got float16"):
            ops.decoder_qkv_bwd(X, p.nw1, p.nb1, EPS, p.wq, p.wk, p.wv, *g16, dtype=BF16)
        with pytest.raises(TypeError, match="attn must be float16, got bfloat16"):
            blk.run_post(X, attn, p)
        with pytest.raises(TypeError, match="attn must be float16, got bfloat16"):
            trn.run_post_bwd(X, attn, p, G[0])
        with pytest.raises(TypeError, match="gq must be float16, got bfloat16"):
            ops.decoder_qkv_bwd(X, p.nw1, p.nb1, EPS, p.wq, p.wk, p.wv, *(g.bfloat16() for g in g16))
        with pytest.raises(TypeError, match="attn must be bfloat16, got float32"):
            run_post(X, attn.float(), p)
        with pytest.raises(TypeError, match="X must be float32"):
            run_qkv(X.bfloat16(), p)


def test_autograd_through_the_three_bf16_ops_is_the_explicit_chain_bit_for_bit():
    X, _, G = (t.to(DEV) for t in block_rows((2, 37), "normal"))
    p = trn.gpu(trn.params())
    scale = 0.3
    lp = trn.cast(p, lambda t: t.clone().requires_grad_())
    Xl = X.clone().requires_grad_()
    q, k, v = ops.decoder_qkv_train(Xl, lp.nw1, lp.nb1, EPS, lp.wq, lp.wk, lp.wv, dtype=BF16)
    assert q.dtype == BF16
    out = ops.decoder_post_train(Xl, ops.cross_attention_bf16(q, k, v, scale), lp.wproj, lp.bproj, lp.g1, lp.nw2, lp.nb2, EPS, lp.w1, lp.b1,
                                 lp.w2, lp.b2, lp.g2, dtype=BF16)
    (out * G[0]).sum().backward()
    with torch.no_grad():
        q0, k0, v0 = run_qkv(X, p)
        a, lse, *_ = ops.cross_attention_bf16_fwd(q0, k0, v0, scale)
        assert torch.equal(out, run_post(X, a, p))
        post = run_post_bwd(X, a, p, G[0])
        dq, dk, dv = ops.cross_attention_bf16_bwd(q0, k0, v0, a, lse, post[1], scale)
        qkv = ops.decoder_qkv_bwd(X, p.nw1, p.nb1, EPS, p.wq, p.wk, p.wv, dq, dk, dv, dtype=BF16)
    assert torch.equal(Xl.grad, post[0] + qkv[0])
    for name, g in list(zip(trn.POST_PARAMS, post[2:])) + list(zip(trn.QKV_PARAMS, qkv[1:])):
        assert torch.equal(getattr(lp, name).grad, g), name


# ---- the module --------------------------------------------------------------------------------------------------------------------
def module_check(what, a, e, b):
    unit, err = float((e.double() - b).abs().max()), float((a.double().cpu() - b).abs().max())
    print(f"bf16 decoder {what}: err {err:.3e}  e_bf16 {unit:.3e}  err / (4 e_bf16) {err / (4 * unit) if unit else float('inf'):.3f}"
          f"  max|ref| {float(b.abs().max()):.3e}")
    assert unit > 0 and a.shape == b.shape and torch.isfinite(a).all() and err <= 4 * unit, (what, err, 4 * unit)


@functools.lru_cache(maxsize=None)
def eval_references():
    """(float64 maps, maps of the torch module on the CPU under bf16 autocast) on the g14 golden, eval()."""
    _, _, x, y, (B, H, W) = blk.load_golden()
    with torch.no_grad():
        want = blk.decoder("torch", "torch", dtype=torch.float64)(x.double(), y.double(), vit_shape=(B, 3, H, W))
        with autocast_bf16():
            emu = blk.decoder("torch", "torch")(x, y, vit_shape=(B, 3, H, W))
    return want, emu


def test_module_with_the_hip_attention_and_torch_blocks_runs_under_bf16_autocast():
    """attn_impl="hip", the default blocks: q, k, v come out of the projections in bf16 and the module takes ops.cross_attention_bf16
    (before the bf16 class this call raised TypeError)."""
    _, _, x, y, (B, H, W) = blk.load_golden()
    want, emu = eval_references()
    dec = blk.decoder("hip", "torch", DEV)
    with torch.no_grad(), torch.autocast(device_type="cuda", dtype=BF16):
        assert not dec._fused(x.to(DEV), y.to(DEV))
        got = dec(x.to(DEV), y.to(DEV), vit_shape=(B, 3, H, W))
    for name, a, e, b in zip("xy", got, emu, want):
        module_check(f"torch blocks, map {name}", a, e, b)


def test_module_with_fused_blocks_under_bf16_autocast():
    """block_impl="hip" on the g14 golden under CUDA bf16 autocast against the float64 module within 4 e_bf16 per map; swapping the
    views swaps the maps bit for bit."""
    _, _, x, y, (B, H, W) = blk.load_golden()
    shape = (B, 3, H, W)
    want, emu = eval_references()
    dec = blk.decoder("hip", "hip", DEV)
    with torch.no_grad(), torch.autocast(device_type="cuda", dtype=BF16):
        assert dec._fused(x.to(DEV), y.to(DEV))
        got = dec(x.to(DEV), y.to(DEV), vit_shape=shape)
        swapped = dec(y.to(DEV), x.to(DEV), vit_shape=shape)
    for name, a, e, b in zip("xy", got, emu, want):
        assert a.dtype == torch.float32
        module_check(f"fused blocks, map {name}", a, e, b)
    assert torch.equal(swapped[0], got[1]) and torch.equal(swapped[1], got[0])


def test_a_fused_bf16_forward_of_four_blocks_is_three_launches_per_block():
    conf, _, x, y, (B, H, W) = blk.load_golden()
    conf["dino_cfg"]["decoder_cfg"]["num_cross_attn"] = 4
    torch.manual_seed(7)
    dec = blk.CrossViewDecoder(conf, attn_impl="hip", block_impl="hip").train(False).to(DEV)
    names = ("decoder_qkv", "cross_attn_fwd", "decoder_post")
    ops.kernel_events = {n: [] for n in names}
    try:
        with torch.no_grad(), torch.autocast(device_type="cuda", dtype=BF16):
            dec(x.to(DEV), y.to(DEV), vit_shape=(B, 3, H, W))
        torch.cuda.synchronize()
        counts = {n: len(v) for n, v in ops.kernel_events.items()}
    finally:
        ops.kernel_events = None
    blocks = conf["dino_cfg"]["decoder_cfg"]["num_cross_attn"]
    assert blocks == 4 and counts == {n: blocks for n in names}, counts


def module_grads(dec, x, y, Gx, Gy, shape, autocast=None):
    """test_decoder_train_gpu.module_grads under bf16 autocast"""
    x, y = x.clone().requires_grad_(), y.clone().requires_grad_()
    dec.zero_grad()
    with torch.autocast(device_type=autocast or "cpu", dtype=BF16, enabled=autocast is not None):
        mx, my = dec(x, y, vit_shape=shape)
    ((mx * Gx).sum() + (my * Gy).sum()).backward()
    return (mx.detach(), my.detach()), (x.grad, y.grad), {k: p.grad.clone() for k, p in dec.named_parameters()}


def test_module_trains_its_blocks_in_hip_under_bf16_autocast():
    """train_block_impl="hip" on the g14 golden in train() under CUDA bf16 autocast: maps, both input gradients and every parameter
    gradient (proj.weight included) against the float64 module within 4 e_bf16 per tensor."""
    _, _, x, y, (B, H, W) = trn.load_golden()
    shape = (B, 3, H, W)
    Gx, Gy = (torch.from_numpy(synth.lattice_normalish((B, 64, H, W), s)) for s in (41, 42))
    want = module_grads(trn.decoder("torch", dtype=torch.float64), x.double(), y.double(), Gx.double(), Gy.double(), shape)
    emu = module_grads(trn.decoder("torch"), x, y, Gx, Gy, shape, autocast="cpu")
    dec = trn.decoder("hip", DEV, train_block_impl="hip")
    xd, yd, Gxd, Gyd = (t.to(DEV) for t in (x, y, Gx, Gy))
    with torch.autocast(device_type="cuda", dtype=BF16):
        assert dec._train_fused(xd, yd) and not dec._fused(xd, yd)
    got = module_grads(dec, xd, yd, Gxd, Gyd, shape, autocast="cuda")
    for i, name in enumerate("xy"):
        module_check(f"trained in hip, map {name}", got[0][i], emu[0][i], want[0][i])
        module_check(f"trained in hip, gradient of {name}", got[1][i], emu[1][i], want[1][i])
    assert set(got[2]) == set(want[2]) and "proj.weight" in got[2]
    for k in want[2]:
        module_check(f"trained in hip, {k}", got[2][k], emu[2][k], want[2][k])


def test_backbone_with_amp_dtype_bf16_reaches_the_bf16_class_in_both_modes(monkeypatch):
    """ReferenceBackbone(amp_dtype=torch.bfloat16, decoder="hip_fused", decoder_train_impl="hip") with the stub ViT of the backbone tests:
    finite pyramids of the right shapes in eval() and in train(), through the bf16 entry points (the dtype the ops are called with)."""
    import fpn_fixture
    from gfnet_amd.reference_backbone import ReferenceBackbone
    from test_fpn_gpu import StubVit
    from test_fpn_train_gpu import E2E_CONF

    seen = {"decoder_qkv": [], "decoder_post": [], "decoder_qkv_train": [], "decoder_post_train": [], "cross_attention_bf16": []}

    def wrap(name, fn):
        def recorded(*a, **k):
            seen[name].append(k.get("dtype"))
            return fn(*a, **k)
        return recorded

    for name in seen:
        monkeypatch.setattr(ops, name, wrap(name, getattr(ops, name)))
    torch.manual_seed(0)
    # (the native FPN in both modes: nothing here goes through the library convolutions and their first-use cost but the stub itself)
    bb = ReferenceBackbone(E2E_CONF, amp_dtype=BF16, vit=StubVit(), decoder="hip_fused", fpn="hip", fpn_train_impl="hip",
                           decoder_train_impl="hip").cuda()
    fpn_fixture.fill({"encoder": bb.encoder, "decoder": bb.decoder, "merge_layer": bb.merge_layer})
    images = torch.from_numpy(synth.lattice_uniform((2, 3, 448, 448), 77)).cuda()
    blocks = E2E_CONF["dino_cfg"]["decoder_cfg"]["num_cross_attn"]
    shapes = {"16": (1, 64, 32, 32), "8": (1, 64, 56, 56), "4": (1, 32, 112, 112), "2": (1, 16, 224, 224), "1": (1, 8, 448, 448)}

    def check(pyramids):
        for pyr in pyramids:
            assert {k: tuple(v.shape) for k, v in pyr.items()} == shapes
            assert all(v.dtype == torch.float32 and bool(torch.isfinite(v).all()) for v in pyr.values())

    bb.train(False)
    with torch.no_grad():
        check(bb(images))
    assert seen["decoder_qkv"] == [BF16] * blocks and seen["decoder_post"] == [BF16] * blocks and len(seen["cross_attention_bf16"]) == blocks
    assert not seen["decoder_qkv_train"]
    bb.train()
    pyramids = bb(images)
    check(pyramids)
    assert seen["decoder_qkv_train"] == [BF16] * blocks and seen["decoder_post_train"] == [BF16] * blocks
    assert len(seen["cross_attention_bf16"]) == 2 * blocks
    sum(pyr["16"].square().mean() for pyr in pyramids).backward()  # the decoder's own maps: the gradient goes through its blocks alone
    for k, p in bb.dino_decoder.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0.0, k
