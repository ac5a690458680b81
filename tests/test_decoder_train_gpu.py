"""Training the cross-view decoder's blocks in HIP on the GPU: ops.decoder_qkv_bwd and ops.decoder_post_bwd
(csrc/decoder_block.hip), the differentiable ops.decoder_qkv_train / ops.decoder_post_train, CrossViewDecoder's
train_block_impl="hip" and ReferenceBackbone's decoder_train_impl="hip".

Oracle: torch autograd through the definition in float64 on the CPU (`definition_qkv` / `definition_post`, restated from
tests/test_decoder_block_gpu.py), with a fixed lattice-normal upstream gradient of order 1.

Unit: e16 = the error of the SAME expression's gradients from torch on the CPU under torch.autocast("cpu", dtype=torch.float16)
against that float64 result, per case and per tensor, never fixed.  Bound: 4 * e16, the project's bound for this class.  Every
comparison asserts e16 > 0 and a finite result, and prints the error against a float64 emulation of the kernels' own class (the
forward's fp16 roundings with the identity as their derivative, g_attn rounded once).

Measured on an MI355X, worst err / (4 e16) per tensor over all cases.  Post backward: gX 0.25, g_attn 0.30, wproj 0.21, bproj 0.16,
gamma1 0.27, norm2 weight 0.35 ((2, 37) large: 7.7e-03 against e16 5.5e-03), norm2 bias 0.29, w1 0.27, b1 0.20, w2 0.21, b2 0.00,
gamma2 0.30.  Qkv backward: gX 0.17, wq 0.20, wk 0.18, wv 0.16, norm1 weight 0.43 ((2, 1) mean50: 2.8e-03 against e16 1.6e-03), norm1
bias 0.22.  The module on the g14 golden: maps 0.16 / 0.18, input gradients 0.21 / 0.23, parameter gradients 0.25 at worst
(cross_attn_blocks.0.attn.k_proj.weight), proj.weight 0.22.  Against their own class: at most 7.6e-04 of a tensor's largest magnitude.
"""
import functools
import json
import os
import types

import numpy as np
import pytest
import synth
import torch
import torch.nn.functional as F

from gfnet_amd import ops
from gfnet_amd.model.crossview_decoder import CrossViewDecoder

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "g14_crossview_decoder.npz")
DEV = "cuda"
C, HID, EPS = 64, 256, 1e-5

# (2B, N): two rows, one lane pair; a tail tile; several tiles and batch entries; 67,584 rows = 2112 tiles, more than the persistent
# grids hold (256 workgroups of 4 waves), so a wave loops and every workgroup contributes a partial
SMALL = [(2, 1), (2, 37)]
FAMILIES = ("normal", "mean50", "constant", "large")
BIG = (2, 33792)
CASES = [(s, f) for s in SMALL for f in FAMILIES] + [((4, 1024), "normal"), (BIG, "normal")]
IDS = [f"{s[0]}x{s[1]}-{f}" for s, f in CASES]
POST_PARAMS = ("wproj", "bproj", "g1", "nw2", "nb2", "w1", "b1", "w2", "b2", "g2")  # decoder_post_bwd's order
POST_NAMES = ("gX", "g_attn") + POST_PARAMS
QKV_PARAMS = ("wq", "wk", "wv", "nw1", "nb1")  # decoder_qkv_bwd's order
QKV_NAMES = ("gX",) + QKV_PARAMS


@functools.lru_cache(maxsize=None)
def params():
    """One block's parameters, fp32 on the CPU, as tests/test_decoder_block_gpu.py draws them (gammas in [0.5, 1.5])."""
    def n(shape, seed, scale=1.0):
        return torch.from_numpy(np.float32(scale / 1.15) * synth.lattice_normalish(shape, seed))

    def u(shape, seed):
        return torch.from_numpy(synth.lattice_uniform(shape, seed))

    return types.SimpleNamespace(
        nw1=1 + 0.25 * u((C,), 11), nb1=0.25 * u((C,), 12), wq=n((C, C), 13, 0.87 / 8), wk=n((C, C), 14, 0.87 / 8), wv=n((C, C), 15, 0.87 / 8),
        wproj=n((C, C), 16, 0.87 / 8), bproj=0.25 * u((C,), 17), g1=1 + 0.5 * u((C,), 18), nw2=1 + 0.25 * u((C,), 19), nb2=0.25 * u((C,), 20),
        w1=n((HID, C), 21, 0.87 / 8), b1=0.25 * u((HID,), 22), w2=n((C, HID), 23, 0.87 / 16), b2=0.25 * u((C,), 24), g2=1 + 0.5 * u((C,), 25))


def cast(p, fn):
    return types.SimpleNamespace(**{k: fn(v) for k, v in vars(p).items()})


def with_(p, **kw):
    return types.SimpleNamespace(**{**vars(p), **kw})


def gpu(p):
    return cast(p, lambda t: t.to(DEV))


@functools.lru_cache(maxsize=None)
def rows(shape, family):
    """(X fp32 (2B, N, 64), attn fp16 (2B, N, 8, 8), upstream gradients fp32 (4, 2B, N, 64): of X_out, q, k, v) on the CPU; the input
    families of tests/test_decoder_block_gpu.py.  The gradients of q, k and v are fp16 values, as cross_attention_bwd writes them."""
    B2, N = shape
    seed = (B2 * 4099 + N) * 7 + FAMILIES.index(family)
    X = torch.from_numpy(synth.lattice_normalish((B2, N, C), seed))
    attn = torch.from_numpy(synth.lattice_normalish((B2, N, 8, 8), seed + 500)).half()
    G = torch.from_numpy(synth.lattice_normalish((4, B2, N, C), seed + 900))
    G[1:] = G[1:].half().float()
    if family == "mean50":
        X = 50 + 1e-2 * X
    elif family == "constant":
        X = (4 * X[..., :1]).expand(B2, N, C).contiguous()
        attn = torch.zeros_like(attn)
    elif family == "large":
        X = 1e3 * X
    return X, attn, G


def block_params(family):
    return with_(params(), bproj=torch.zeros(C)) if family == "constant" else params()


def definition_qkv(X, p):
    """block.py:327's norm1 and attention.py:236-238 in X's dtype; k and v NOT yet moved to the other view's batch entry."""
    return F.linear(F.layer_norm(X, (C,), p.nw1, p.nb1, EPS), p.wq), F.linear(X, p.wk), F.linear(X, p.wv)


def definition_post(X, attn, p):
    """attention.py:255 and the rest of block.py:327-328 (layer_scale.py, mlp.py) in X's dtype."""
    x1 = X + p.g1 * F.linear(attn.reshape(X.shape), p.wproj, p.bproj)
    return x1 + p.g2 * F.linear(F.gelu(F.linear(F.layer_norm(x1, (C,), p.nw2, p.nb2, EPS), p.w1, p.b1)), p.w2, p.b2)


def r16(t):
    """fp16 rounding in float64 with the identity as its derivative"""
    return t + (t.detach().half().double() - t.detach())


def class_qkv(X, p):
    n = F.layer_norm(X, (C,), p.nw1, p.nb1, EPS)
    return tuple(F.linear(r16(a), r16(w)) for a, w in ((n, p.wq), (X, p.wk), (X, p.wv)))


def class_post(X, attn, p):
    x1 = X + p.g1 * F.linear(attn.reshape(X.shape), r16(p.wproj), p.bproj)
    h = r16(F.layer_norm(x1, (C,), p.nw2, p.nb2, EPS))
    return x1 + p.g2 * F.linear(r16(F.gelu(F.linear(h, r16(p.w1), p.b1))), r16(p.w2), p.b2)


def leaves(p, names, fn):
    return with_(p, **{k: fn(getattr(p, k)).clone().requires_grad_() for k in names})


def post_grads(X, attn, p, G, fn, dtype):
    """name -> gradient of sum(fn(X, attn, p) * G), float64 tensors, evaluated in `dtype` (torch.float16: fp32 under CPU autocast)"""
    wide = (lambda t: t.double()) if dtype == torch.float64 else (lambda t: t)
    X, G = wide(X).clone().requires_grad_(), wide(G)
    attn = (attn.double() if dtype == torch.float64 else attn).clone().requires_grad_()
    p = leaves(p, POST_PARAMS, wide)
    with torch.autocast(device_type="cpu", dtype=torch.float16, enabled=dtype == torch.float16):
        loss = (fn(X, attn, p) * G).sum()
    grads = torch.autograd.grad(loss, [X, attn] + [getattr(p, k) for k in POST_PARAMS])
    return {k: g.double() for k, g in zip(POST_NAMES, grads)}


def qkv_grads(X, p, G, fn, dtype):
    """name -> gradient of sum(q * Gq) + sum(k' * Gk) + sum(v' * Gv), k' and v' at the other view's batch entry"""
    wide = (lambda t: t.double()) if dtype == torch.float64 else (lambda t: t)
    X, G = wide(X).clone().requires_grad_(), wide(G)
    p = leaves(p, QKV_PARAMS, wide)
    B = X.shape[0] // 2
    with torch.autocast(device_type="cpu", dtype=torch.float16, enabled=dtype == torch.float16):
        q, k, v = fn(X, p)
        loss = (q * G[1]).sum() + (k.roll(B, 0) * G[2]).sum() + (v.roll(B, 0) * G[3]).sum()
    grads = torch.autograd.grad(loss, [X] + [getattr(p, k) for k in QKV_PARAMS])
    return {k: g.double() for k, g in zip(QKV_NAMES, grads)}


@functools.lru_cache(maxsize=None)
def references(shape, family, which):
    """name -> (float64 gradient, e16, float64 gradient in the kernels' own class); computed once per case and shared"""
    X, attn, G = rows(shape, family)
    p = block_params(family)
    if which == "post":
        want, emu, cls = (post_grads(X, attn, p, G[0], fn, dt) for fn, dt in ((definition_post, torch.float64), (definition_post, torch.float16),
                                                                             (class_post, torch.float64)))
        cls["g_attn"] = cls["g_attn"].half().double()
    else:
        want, emu, cls = (qkv_grads(X, p, G, fn, dt) for fn, dt in ((definition_qkv, torch.float64), (definition_qkv, torch.float16),
                                                                    (class_qkv, torch.float64)))
    return {k: (want[k], float((emu[k] - want[k]).abs().max()), cls[k]) for k in want}


def run_post_bwd(X, attn, p, G):
    return ops.decoder_post_bwd(X, attn, p.wproj, p.bproj, p.g1, p.nw2, p.nb2, EPS, p.w1, p.b1, p.w2, p.b2, p.g2, G)


def run_qkv_bwd(X, p, G):
    gq, gk, gv = (g.half().reshape(X.shape[0], X.shape[1], 8, 8) for g in G[1:])
    return ops.decoder_qkv_bwd(X, p.nw1, p.nb1, EPS, p.wq, p.wk, p.wv, gq, gk, gv)


def compare(what, got, ref):
    want, e16, cls = ref
    got = got.double().cpu().reshape(want.shape)
    err, ecls = float((got - want).abs().max()), float((got - cls).abs().max())
    print(f"{what}: err {err:.3e}  e16 {e16:.3e}  err / (4 e16) {err / (4 * e16) if e16 else float('inf'):.3f}  against its own class {ecls:.3e}"
          f"  max|ref| {float(want.abs().max()):.3e}")
    if not want.any() and e16 == 0:
        # the constant family's attention rows and bproj are zero, so the gradients of wproj and gamma1 are sums of exact zeros in
        # float64 and under autocast alike: there is no unit to scale a bound with, and the kernels owe exact zeros
        assert what.endswith(("constant wproj", "constant g1")) and not got.any(), what
        return
    assert e16 > 0, what
    assert torch.isfinite(got).all() and err <= 4 * e16, (what, err, 4 * e16)


@pytest.mark.parametrize("shape,family", CASES, ids=IDS)
def test_post_bwd_against_float64_autograd(shape, family):
    X, attn, G = rows(shape, family)
    ref = references(shape, family, "post")
    got = run_post_bwd(X.to(DEV), attn.to(DEV), gpu(block_params(family)), G[0].to(DEV))
    assert got[0].dtype == torch.float32 and got[1].dtype == torch.float16 and got[1].shape == attn.shape
    for name, t in zip(POST_NAMES, got):
        compare(f"decoder_post_bwd {shape} {family} {name}", t, ref[name])


@pytest.mark.parametrize("shape,family", CASES, ids=IDS)
def test_qkv_bwd_against_float64_autograd(shape, family):
    X, _, G = rows(shape, family)
    ref = references(shape, family, "qkv")
    got = run_qkv_bwd(X.to(DEV), gpu(block_params(family)), G.to(DEV))
    for name, t in zip(QKV_NAMES, got):
        assert t.dtype == torch.float32
        compare(f"decoder_qkv_bwd {shape} {family} {name}", t, ref[name])


def small_ints(shape, seed, lo, hi):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def test_qkv_bwd_gk_and_gv_reach_the_other_views_rows_exactly_on_small_integers():
    """gq = 0 and small-integer gk, gv, wk, wv, X: gX[b] = gk[(b + B) mod 2B] wk + gv[(b + B) mod 2B] wv and the two weight gradients
    (sums of at most 222 * 16 per element) are exact in every format on the way, so they are compared bit for bit: the mirror of
    test_qkv_k_and_v_are_exact_on_small_integers_and_land_on_the_other_view."""
    B2, N = 6, 37
    X = small_ints((B2, N, C), 1, -4, 4)
    p = with_(params(), wk=small_ints((C, C), 2, -2, 2), wv=small_ints((C, C), 3, -2, 2))
    G = torch.stack((torch.zeros(B2, N, C), torch.zeros(B2, N, C), small_ints((B2, N, C), 4, -4, 4), small_ints((B2, N, C), 5, -4, 4)))
    got = run_qkv_bwd(X.to(DEV), gpu(p), G.to(DEV))
    gk, gv = G[2].roll(-B2 // 2, 0), G[3].roll(-B2 // 2, 0)  # the gradients back at the batch entry whose row produced k and v
    want = gk @ p.wk + gv @ p.wv
    assert float(want.abs().max()) > 50
    for b in range(B2):
        assert torch.equal(got[0][b].cpu(), G[2][(b + B2 // 2) % B2] @ p.wk + G[3][(b + B2 // 2) % B2] @ p.wv), b
    assert torch.equal(got[0].cpu(), want)
    assert torch.equal(got[2].cpu(), gk.reshape(-1, C).T @ X.reshape(-1, C)) and torch.equal(got[3].cpu(), gv.reshape(-1, C).T @ X.reshape(-1, C))
    assert not got[1].any() and not got[4].any() and not got[5].any()  # nothing came through q


def test_post_bwd_with_the_mlp_scaled_to_zero_is_the_proj_branch_exactly():
    """gamma2 = 0: nothing comes back through the MLP, so gX equals gX_out bit for bit, and with small-integer g, gamma1, wproj and
    attn the proj branch is exact: g_attn = fp16((gamma1 g) wproj), g_wproj = gamma1_c sum g_c a_h, g_bproj = gamma1_c sum g_c."""
    shape = (6, 37, C)
    X, a, g = small_ints(shape, 4, -8, 8), small_ints(shape, 5, -3, 3).half(), small_ints(shape, 9, -4, 4)
    p = with_(params(), wproj=small_ints((C, C), 6, -2, 2), bproj=small_ints((C,), 7, -5, 5), g1=small_ints((C,), 8, 1, 3), g2=torch.zeros(C))
    got = dict(zip(POST_NAMES, (t.cpu() for t in run_post_bwd(X.to(DEV), a.to(DEV).reshape(6, 37, 8, 8), gpu(p), g.to(DEV)))))
    assert torch.equal(got["gX"], g)
    want = (g * p.g1) @ p.wproj
    assert 50 < float(want.abs().max()) < 2048 and torch.equal(got["g_attn"].reshape(shape), want.half())
    g2d, a2d = g.reshape(-1, C), a.float().reshape(-1, C)
    assert torch.equal(got["wproj"], p.g1[:, None] * (g2d.T @ a2d)) and torch.equal(got["bproj"], p.g1 * g2d.sum(0))
    for k in ("w1", "b1", "w2", "b2", "nw2", "nb2"):
        assert not got[k].any(), k


def test_two_calls_give_the_same_bits_and_a_rows_gradient_does_not_depend_on_its_position():
    """67,584 rows: every output of two identical calls is bit-identical, and with the tokens of both views permuted the same way gX and
    g_attn (and the qkv backward's gX) are the permuted results bit for bit."""
    X, attn, G = (t.to(DEV) for t in rows(BIG, "normal"))
    p = gpu(params())
    perm = torch.randperm(BIG[1], generator=torch.Generator().manual_seed(5)).to(DEV)
    post, post2 = run_post_bwd(X, attn, p, G[0]), run_post_bwd(X, attn, p, G[0])
    qkv, qkv2 = run_qkv_bwd(X, p, G), run_qkv_bwd(X, p, G)
    for a, b in zip(post + qkv, post2 + qkv2):
        assert torch.equal(a, b)
    postp = run_post_bwd(X[:, perm].contiguous(), attn[:, perm].contiguous(), p, G[0][:, perm].contiguous())
    qkvp = run_qkv_bwd(X[:, perm].contiguous(), p, G[:, :, perm].contiguous())
    for view in (0, 1):
        assert torch.equal(postp[0][view], post[0][view][perm]) and torch.equal(postp[1][view], post[1][view][perm])
        assert torch.equal(qkvp[0][view], qkv[0][view][perm])


def test_a_non_finite_row_of_the_upstream_gradient_stays_in_its_row():
    """A row of inf and a row of nan in gX_out: gX and g_attn are non-finite in those rows and bit-identical to a clean call in every
    other; the parameter gradients are non-finite.  The same for a row of gq in the qkv backward."""
    shape = (6, 100)
    X, attn, G = (t.to(DEV) for t in rows(shape, "normal"))
    p = gpu(params())
    bad = [(1, 17), (4, 99)]
    Gb = G.clone()
    Gb[0][bad[0]], Gb[0][bad[1]] = float("inf"), float("nan")
    Gb[1][bad[0]], Gb[1][bad[1]] = float("nan"), float("inf")
    mask = torch.ones(shape, dtype=torch.bool)
    for b, n in bad:
        mask[b, n] = False
    clean, dirty = run_post_bwd(X, attn, p, G[0]), run_post_bwd(X, attn, p, Gb[0])
    qclean, qdirty = run_qkv_bwd(X, p, G), run_qkv_bwd(X, p, Gb)
    for name, c, d in (("gX", clean[0], dirty[0]), ("g_attn", clean[1], dirty[1]), ("qkv gX", qclean[0], qdirty[0])):
        c, d = c.cpu().reshape(*shape, C), d.cpu().reshape(*shape, C)
        assert torch.isfinite(c).all(), name
        assert torch.equal(c[mask], d[mask]), name
        assert not torch.isfinite(d[~mask]).any(), name
    for name, c, d in zip(POST_PARAMS, clean[2:], dirty[2:]):
        assert torch.isfinite(c).all() and not torch.isfinite(d).all(), name
    assert not torch.isfinite(qdirty[1]).all() and torch.equal(qdirty[2], qclean[2]) and torch.equal(qdirty[3], qclean[3])


def test_autograd_through_the_three_ops_is_the_explicit_chain_bit_for_bit():
    X, _, G = (t.to(DEV) for t in rows((2, 37), "normal"))
    p = gpu(params())
    scale = 0.3
    lp = cast(p, lambda t: t.clone().requires_grad_())
    Xl = X.clone().requires_grad_()
    q, k, v = ops.decoder_qkv_train(Xl, lp.nw1, lp.nb1, EPS, lp.wq, lp.wk, lp.wv)
    out = ops.decoder_post_train(Xl, ops.cross_attention(q, k, v, scale), lp.wproj, lp.bproj, lp.g1, lp.nw2, lp.nb2, EPS, lp.w1, lp.b1, lp.w2,
                                 lp.b2, lp.g2)
    (out * G[0]).sum().backward()
    with torch.no_grad():
        q0, k0, v0 = ops.decoder_qkv(X, p.nw1, p.nb1, EPS, p.wq, p.wk, p.wv)
        a, lse, *_ = ops.cross_attention_fwd(q0, k0, v0, scale)
        assert torch.equal(out, ops.decoder_post(X, a, p.wproj, p.bproj, p.g1, p.nw2, p.nb2, EPS, p.w1, p.b1, p.w2, p.b2, p.g2))
        post = run_post_bwd(X, a, p, G[0])
        dq, dk, dv = ops.cross_attention_bwd(q0, k0, v0, a, lse, post[1], scale)
        qkv = ops.decoder_qkv_bwd(X, p.nw1, p.nb1, EPS, p.wq, p.wk, p.wv, dq, dk, dv)
    assert torch.equal(Xl.grad, post[0] + qkv[0])
    for name, g in list(zip(POST_PARAMS, post[2:])) + list(zip(QKV_PARAMS, qkv[1:])):
        assert torch.equal(getattr(lp, name).grad, g), name


def test_an_overflowing_upstream_gradient_gives_inf_in_g_attn():
    """GradScaler's case: an upstream gradient of order 1 scaled by 65536 whose g_attn = wproj^T (gamma1 g1) leaves fp16's range.
    gamma1 = 1/4 keeps the operand gamma1 g1 inside it (|G| <= 3.4 here) and gamma2 = 2^-10 the MLP branch, so the overflow happens
    where g_attn is rounded, with wproj 16 times its usual size: the result holds inf and no nan, and gX, which is fp32, is finite.
    The parameter gradients, whose operand fp16(g1) overflows, show it too (what a found-inf check sees)."""
    X, attn, G = (t.to(DEV) for t in rows((2, 37), "normal"))
    assert float(G[0].abs().max()) * 65536 / 4 < 65504
    p = with_(params(), g1=torch.full((C,), 0.25), g2=torch.full((C,), 2.0 ** -10), wproj=16 * params().wproj)
    got = run_post_bwd(X, attn, gpu(p), 65536 * G[0])
    assert torch.isinf(got[1]).any() and not torch.isnan(got[1]).any() and torch.isfinite(got[0]).all()
    assert not torch.isfinite(got[2]).all()


# ---- the module ----------------------------------------------------------------------------------------------------------------
def load_golden():
    z = np.load(GOLDEN)
    state = {k[len("param/"):]: torch.from_numpy(z[k].astype(np.float32)) for k in z.files if k.startswith("param/")}
    x, y = (torch.from_numpy(z[k].astype(np.float32)) for k in ("x", "y"))
    return json.loads(str(z["conf"])), state, x, y, tuple(int(v) for v in z["grid"])


def decoder(attn_impl, device="cpu", dtype=torch.float32, **kw):
    conf, state, *_ = load_golden()
    dec = CrossViewDecoder(conf, attn_impl=attn_impl, **kw)
    dec.load_state_dict(state, strict=True)
    return dec.train().to(device, dtype)


def module_grads(dec, x, y, Gx, Gy, shape, autocast=None):
    """(maps, input gradients, name -> parameter gradient) of sum(map_x * Gx) + sum(map_y * Gy) with the module in train()"""
    x, y = x.clone().requires_grad_(), y.clone().requires_grad_()
    dec.zero_grad()
    with torch.autocast(device_type=autocast or "cpu", dtype=torch.float16, enabled=autocast is not None):
        mx, my = dec(x, y, vit_shape=shape)
    ((mx * Gx).sum() + (my * Gy).sum()).backward()
    return (mx.detach(), my.detach()), (x.grad, y.grad), {k: p.grad.clone() for k, p in dec.named_parameters()}


def test_module_trains_its_blocks_in_hip_under_fp16_autocast():
    """train_block_impl="hip" on the g14 golden in train() under CUDA fp16 autocast: every parameter gradient (proj.weight included) and
    both input gradients against the float64 module within 4 e16 per tensor, the maps within the forward's bound; swapping the views
    swaps the input gradients bit for bit."""
    _, _, x, y, (B, H, W) = load_golden()
    shape = (B, 3, H, W)
    Gx, Gy = (torch.from_numpy(synth.lattice_normalish((B, 64, H, W), s)) for s in (41, 42))
    want = module_grads(decoder("torch", dtype=torch.float64), x.double(), y.double(), Gx.double(), Gy.double(), shape)
    emu = module_grads(decoder("torch"), x, y, Gx, Gy, shape, autocast="cpu")
    dec = decoder("hip", DEV, train_block_impl="hip")
    xd, yd, Gxd, Gyd = (t.to(DEV) for t in (x, y, Gx, Gy))
    with torch.autocast(device_type="cuda", dtype=torch.float16):
        assert dec._train_fused(xd, yd) and not dec._fused(xd, yd)
    got = module_grads(dec, xd, yd, Gxd, Gyd, shape, autocast="cuda")
    swapped = module_grads(dec, yd, xd, Gyd, Gxd, shape, autocast="cuda")

    def check(what, a, e, b):
        e16, err = float((e.double() - b).abs().max()), float((a.double().cpu() - b).abs().max())
        print(f"hip-trained decoder {what}: err {err:.3e}  e16 {e16:.3e}  err / (4 e16) {err / (4 * e16) if e16 else float('inf'):.3f}"
              f"  max|ref| {float(b.abs().max()):.3e}")
        assert e16 > 0 and a.shape == b.shape and torch.isfinite(a).all() and err <= 4 * e16, (what, err, 4 * e16)

    for i, name in enumerate("xy"):
        check(f"map {name}", got[0][i], emu[0][i], want[0][i])
        check(f"gradient of {name}", got[1][i], emu[1][i], want[1][i])
    assert set(got[2]) == set(want[2]) and "proj.weight" in got[2]
    for k in want[2]:
        check(k, got[2][k], emu[2][k], want[2][k])
    assert torch.equal(swapped[1][0], got[1][1]) and torch.equal(swapped[1][1], got[1][0])
    assert torch.equal(swapped[0][0], got[0][1]) and torch.equal(swapped[0][1], got[0][0])


COUNTED = ("decoder_qkv", "cross_attention_fwd", "decoder_post", "decoder_post_bwd", "cross_attention_bwd", "decoder_qkv_bwd")


def counting(monkeypatch):
    counts = dict.fromkeys(COUNTED, 0)

    def wrap(name, fn):
        def counted(*a, **k):
            counts[name] += 1
            return fn(*a, **k)
        return counted

    for name in COUNTED:
        monkeypatch.setattr(ops, name, wrap(name, getattr(ops, name)))
    return counts


def test_the_training_path_is_six_launch_groups_per_block_and_only_when_asked(monkeypatch):
    conf, _, x, y, (B, H, W) = load_golden()
    blocks = conf["dino_cfg"]["decoder_cfg"]["num_cross_attn"]
    counts = counting(monkeypatch)
    G = torch.ones((B, 64, H, W), device=DEV)
    module_grads(decoder("hip", DEV, train_block_impl="hip"), x.to(DEV), y.to(DEV), G, G, (B, 3, H, W), autocast="cuda")
    assert blocks >= 1 and counts == dict.fromkeys(COUNTED, blocks), counts
    module_grads(decoder("hip", DEV), x.to(DEV), y.to(DEV), G, G, (B, 3, H, W), autocast="cuda")  # the default: torch blocks
    want = dict.fromkeys(COUNTED, blocks)
    want["cross_attention_fwd"] = want["cross_attention_bwd"] = 2 * blocks  # (the attention core is HIP on both paths)
    assert counts == want, counts
    dec = decoder("hip", DEV, train_block_impl="hip").train(False)  # eval(): not the training path
    with torch.no_grad(), torch.autocast(device_type="cuda", dtype=torch.float16):
        dec(x.to(DEV), y.to(DEV), vit_shape=(B, 3, H, W))
    assert counts["decoder_qkv"] == blocks and counts["decoder_post_bwd"] == blocks


def test_module_without_layerscale_trains_with_a_gamma_of_one():
    """init_values None: the path passes a constant gamma of 1 and no gamma gradient exists; the other gradients against the float64
    module as above."""
    conf, _, x, y, (B, H, W) = load_golden()
    conf["dino_cfg"]["decoder_cfg"]["init_values"] = None
    shape = (B, 3, H, W)
    torch.manual_seed(3)
    dec = CrossViewDecoder(conf, attn_impl="hip", train_block_impl="hip").train()
    ref = CrossViewDecoder(conf, attn_impl="torch").train()
    ref.load_state_dict(dec.state_dict())
    assert not any("gamma" in k for k in dec.state_dict())
    Gx, Gy = (torch.from_numpy(synth.lattice_normalish((B, 64, H, W), s)) for s in (41, 42))
    emu = module_grads(ref, x, y, Gx, Gy, shape, autocast="cpu")
    want = module_grads(ref.double(), x.double(), y.double(), Gx.double(), Gy.double(), shape)
    got = module_grads(dec.to(DEV), x.to(DEV), y.to(DEV), Gx.to(DEV), Gy.to(DEV), shape, autocast="cuda")
    for k in want[2]:
        e16, err = float((emu[2][k].double() - want[2][k]).abs().max()), float((got[2][k].double().cpu() - want[2][k]).abs().max())
        print(f"without LayerScale {k}: err {err:.3e}  e16 {e16:.3e}  err / (4 e16) {err / (4 * e16) if e16 else float('inf'):.3f}")
        assert e16 > 0 and torch.isfinite(got[2][k]).all() and err <= 4 * e16, (k, err, 4 * e16)


def test_an_overflow_reaches_the_found_inf_of_the_fused_step():
    """The loss scaled by 65536 on upstream gradients of order 1: the decoder's gradients hold inf, FusedAdamWStep finds it, skips the
    step (no parameter moves) and halves the scale."""
    from gfnet_amd.trainer import FusedAdamWStep

    _, _, x, y, (B, H, W) = load_golden()
    dec = decoder("hip", DEV, train_block_impl="hip")
    before = {k: p.detach().clone() for k, p in dec.named_parameters()}
    stepper = FusedAdamWStep(list(dec.parameters()), lr=1e-3, init_scale=65536.0, zero_grads=False)
    Gx, Gy = (torch.from_numpy(synth.lattice_normalish((B, 64, H, W), s)).to(DEV) for s in (41, 42))
    with torch.autocast(device_type="cuda", dtype=torch.float16):
        mx, my = dec(x.to(DEV), y.to(DEV), vit_shape=(B, 3, H, W))
    stepper.scale_loss((mx * Gx).sum() + (my * Gy).sum()).backward()
    assert any(not torch.isfinite(p.grad).all() for p in dec.cross_attn_blocks.parameters())
    stepper.step()
    assert float(stepper.last_stats["found_inf"]) != 0.0 and float(stepper._scale) == 32768.0
    for k, p in dec.named_parameters():
        assert torch.equal(p.detach(), before[k]), k


# ---- one training step of a whole model ------------------------------------------------------------------------------------------
def one_training_step(impl, counts):
    """tests/test_fpn_train_gpu.py's one_training_step -- its conf, StubVit and 448 x 448 images -- with decoder="hip_fused" and
    decoder_train_impl=impl: the loss, after checking every dino_decoder parameter's gradient and the path taken."""
    import fpn_fixture
    from gfnet_amd.model.network import GFNet
    from gfnet_amd.reference_backbone import ReferenceBackbone
    from gfnet_amd.trainer import FusedAdamWStep, train_step as trainer_step
    from test_fpn_gpu import StubVit
    from test_fpn_train_gpu import E2E_CONF

    images = torch.from_numpy(synth.lattice_uniform((4, 3, 448, 448), 78)).cuda()
    batch = {"im_A": images[:2], "im_B": images[2:]}

    def objective(out, _):
        loss = torch.zeros((), device="cuda")
        for scale in out.values():
            for d in scale.values():
                loss = loss + d["flow"].float().square().mean() + d["certainty"].float().square().mean()
        return loss

    flags = (torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark)
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    start = dict(counts)
    try:
        torch.manual_seed(0)
        bb = ReferenceBackbone(E2E_CONF, vit=StubVit(), decoder="hip_fused", fpn="hip", decoder_train_impl=impl).cuda()
        fpn_fixture.fill({"encoder": bb.encoder, "decoder": bb.decoder, "merge_layer": bb.merge_layer})
        model = GFNet(E2E_CONF, backbone=bb).cuda()
        model.train()
        stepper = FusedAdamWStep([p for p in model.parameters() if p.requires_grad], lr=1e-4, init_scale=1.0, zero_grads=False)
        res = trainer_step(batch, model, objective, stepper)
    finally:
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = flags
    for k, p in bb.dino_decoder.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0.0, (impl, k)
    blocks = E2E_CONF["dino_cfg"]["decoder_cfg"]["num_cross_attn"]
    ran = {k: counts[k] - start[k] for k in ("decoder_qkv", "decoder_post", "decoder_post_bwd", "decoder_qkv_bwd")}
    assert ran == dict.fromkeys(ran, blocks if impl == "hip" else 0), (impl, ran)
    return float(res["train_loss"])


def test_one_training_step_end_to_end(monkeypatch):
    """One trainer.train_step of a whole model with the decoder's blocks trained in HIP: every dino_decoder parameter gets a finite
    gradient that is not all zero, the loss is finite and the HIP blocks ran.  The loss is printed next to the torch blocks' and
    their difference is not bounded: tests/test_fpn_train_gpu.py documents that the randomly initialised matcher amplifies
    rounding-level differences of its input about a thousandfold, and this path differs from torch's at fp16 rounding level by design
    (the Linear outputs stay fp32 where autocast rounds them).  Measured: 0.67613322 (hip) against 0.67588842 (torch).

    Two whole-model steps at 448 x 448 are what this test is about.  In the order the suite runs it is the first test to train a
    whole model, so it also pays the libraries' first-use cost (21 s here, against about a second for the same two steps in
    tests/test_fpn_train_gpu.py, which runs after it)."""
    counts = counting(monkeypatch)
    hip, ref = one_training_step("hip", counts), one_training_step("torch", counts)
    print(f"one training step: loss {hip:.9e} (decoder_train_impl hip) vs {ref:.9e} (torch)")
    assert np.isfinite(hip) and np.isfinite(ref)
