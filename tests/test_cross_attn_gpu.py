"""ops.cross_attention (csrc/cross_attn.hip) and the native cross-view decoder on the GPU.

Oracle: ops.reference_cross_attention and its autograd in float64 on the CPU, on the values the kernel receives (fp16-rounded for
the fp16 class).  Bounds, per tensor (out, lse, dq, dk, dv):

  fp32 class   max(4 * E32, 2^-20 * max|oracle|); E32 = the same reference run in float32 on the CPU against float64, so it is the
               reference's own arithmetic class and never the kernel; 4 for tile-wise summation order and the hardware exp2; the
               floor is 16 fp32 roundings.
  fp16 forward 2^-11 * max|out| (the one final rounding; P is NOT rounded before P V, so no 2^-11 * max|v| term) + the fp32 bound;
               lse is fp32 in both classes and takes the fp32 bound.
  fp16 backward 4 * E16 + 2^-11 * max|grad|; E16 = the error against float64 of a CPU emulation of the kernel's numeric class
               written here (fp16 inputs, fp32 products and sums, delta = sum_j P dP / sum_j P as the kernel forms it, P and dS NOT
               rounded because the kernel does not round them, results rounded to fp16).

Measured on an MI355X: MEASURED below, from the figures every test prints before it asserts.
"""
import functools
import json
import os

import numpy as np
import pytest
import torch

from gfnet_amd import _lib, ops
from gfnet_amd.model.crossview_decoder import CrossViewDecoder

pytestmark = pytest.mark.gpu

# error / bound, worst case over the small shapes and families and the 1600 x 1600 shape, per tensor (MI355X, ROCm 7.0, torch 2.10):
MEASURED = """
fp32 class   out 0.36 (1x129x33x8 normal)   lse 0.17 (1x1600x1600x8)   dq 0.45 (2x40x77x3 normal)   dk 0.48 (1x1600x1600x8)
             dv 0.77 (2x30x30x8 spread60: err 6.2e-06, bound 8.0e-06)
fp16 class   out 0.66 (2x30x30x8 normal: err 4.8e-04, bound 7.3e-04)   lse 0.18   dq 0.25   dk 0.25   dv 0.19
             backward at 1x1600x1600x8: dq 2.3e-04 / 1.2e-03, dk 2.4e-04 / 1.4e-03, dv 2.1e-04 / 1.2e-03 (E16 = 2.2e-04 .. 2.7e-04)
overflow     dout x 65536 / 16 on 1x129x33x8 max_first: 4 entries of dv past fp16, all inf of the right sign; finite entries
             err 15.8 against a bound of 95.4 (values up to 6e4), dq and dk 3e-03 / 3e-04 against 32
decoder      fp32 maps: err 1.9e-06 / 2.4e-06, bound 1.05e-05.  fp16 autocast maps: err 3.2e-03 / 3.6e-03 on maps up to 7.7; the
             same module on the CPU under fp16 autocast: 2.9e-03 / 3.2e-03, so bounds 1.17e-02 / 1.27e-02.
             gradients of the fp32 module: worst err / bound 0.45 (cross_attn_blocks.1.ls1.gamma)
delta        fp32, 2x30x30x8 max_first (one row with 1 - 1.4e-8 of its weight on a key of norm 30): dq 1.3e-08 / 5.1e-08, dk
             1.4e-09 / 5.8e-09.  With delta = sum_d dout * out from the saved out this case was at 5.6e-06 and 5.9e-07, 110 x its
             bound: the reason the kernel forms sum_j P dP / sum_j P instead
"""

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "g14_crossview_decoder.npz")
DEV = "cuda"

# (B, Nq, Nk, H) at D = 8: one exact tile; tails on both axes with an odd head count; one query and one key past a boundary;
# smaller than a tile (the golden's grid); one key (out = v); keys over two staged chunks, the second with two tiles of which the last
# holds one key (lane half 1 meets nothing there) and queries one tile plus one row; and the 560 pass: 50 key tiles of rescaling
SMALL = [(1, 32, 32, 1), (2, 40, 77, 3), (1, 129, 33, 8), (2, 30, 30, 8), (1, 5, 1, 2), (1, 33, 161, 2)]
BIG = (1, 1600, 1600, 8)
FAMILIES = ("normal", "spread60", "max_last", "max_first", "dominant", "scale0")
NAMES = ("out", "lse", "dq", "dk", "dv")


def _h(t):
    """Rounded to what float16 holds, as float32: inputs both classes can take unchanged."""
    return t.half().float()


@functools.lru_cache(maxsize=None)
def inputs(shape, family):
    """(q, k, v, dout, scale) as fp32 CPU tensors of fp16-representable values."""
    B, Nq, Nk, H = shape
    g = torch.Generator().manual_seed(((B * 131 + Nq) * 131 + Nk) * 131 + H * 7 + FAMILIES.index(family))
    q, k, v = (torch.randn(B, n, H, 8, generator=g) for n in (Nq, Nk, Nk))
    dout = torch.randn(B, Nq, H, 8, generator=g)
    scale = 8 ** -0.5
    if family == "spread60":  # scaled scores spread over +-60
        q, k = _h(q), _h(k)
        scale = 60.0 / float(torch.einsum("bihd,bjhd->bhij", q, k).abs().max())
    elif family in ("max_last", "max_first"):  # every row's maximum in one key, the last or the first
        j = Nk - 1 if family == "max_last" else 0
        q[..., 0] = q[..., 0].abs() + 1.0
        k[..., 0] = -k[..., 0].abs()
        k[:, j] = 0.0
        k[:, j, :, 0] = 30.0
        scale = 1.0
    elif family == "dominant":  # key i % Nk dominates query i by a score gap >= 40: out must be that key's v
        signs = torch.tensor([[1.0 if (j >> d) & 1 else -1.0 for d in range(8)] for j in range(256)])
        kj = signs[torch.arange(Nk) % 256]
        k = (5.0 * kj).view(1, Nk, 1, 8).expand(B, Nk, H, 8).clone()
        q = (4.0 * kj[torch.arange(Nq) % Nk]).view(1, Nq, 1, 8).expand(B, Nq, H, 8).clone()
        scale = 1.0
    elif family == "scale0":
        scale = 0.0
    return _h(q), _h(k), _h(v), _h(dout), scale


def reference(q, k, v, dout, scale, dtype):
    """(out, lse, dq, dk, dv) of the definition and its autograd in `dtype` on the CPU, returned as float64."""
    q, k, v = (t.to(dtype).requires_grad_() for t in (q, k, v))
    out = ops.reference_cross_attention(q, k, v, scale)
    lse = torch.logsumexp(torch.einsum("bihd,bjhd->bhij", q, k) * scale, dim=-1)
    grads = torch.autograd.grad(out, (q, k, v), dout.to(dtype))
    return tuple(t.detach().double() for t in (out, lse) + grads)


def emulate_fp16_class(q, k, v, dout, scale):
    """The kernel's fp16 numeric class on the CPU: fp16 values in, every product and sum fp32, delta = sum_j P dP / sum_j P (the
    saved out is not read by the backward), P and dS kept fp32 (the kernel never rounds them), results rounded to fp16.
    (dq, dk, dv) as float64."""
    s = torch.einsum("bihd,bjhd->bhij", q, k) * scale
    p = torch.softmax(s, dim=-1)
    dp = torch.einsum("bihd,bjhd->bhij", dout, v)
    delta = (p * dp).sum(-1, keepdim=True) / p.sum(-1, keepdim=True)
    ds = p * (dp - delta)
    dq = torch.einsum("bhij,bjhd->bihd", ds, k) * scale
    dk = torch.einsum("bhij,bihd->bjhd", ds, q) * scale
    dv = torch.einsum("bhij,bihd->bjhd", p, dout)
    return tuple(t.half().double() for t in (dq, dk, dv))


@functools.lru_cache(maxsize=None)
def oracle(shape, family):
    """The float64 results, and per tensor the fp32 bound and the fp16 bound (module docstring).  Computed once per case."""
    q, k, v, dout, scale = inputs(shape, family)
    o64 = reference(q, k, v, dout, scale, torch.float64)
    o32 = reference(q, k, v, dout, scale, torch.float32)
    e32 = [float((a - b).abs().max()) for a, b in zip(o32, o64)]
    b32 = [max(4 * e, 2.0 ** -20 * float(o.abs().max())) for e, o in zip(e32, o64)]
    e16 = [float((a - b).abs().max()) for a, b in zip(emulate_fp16_class(q, k, v, dout, scale), o64[2:])]
    b16 = [2.0 ** -11 * float(o64[0].abs().max()) + b32[0], b32[1]] + [4 * e + 2.0 ** -11 * float(o.abs().max()) for e, o in zip(e16, o64[2:])]
    return o64, b32, b16


def run_kernel(shape, family, dtype, dout_scale=1.0):
    """(out, lse, dq, dk, dv) of ops.cross_attention and its backward on the GPU, as float64 CPU tensors."""
    q, k, v, dout, scale = inputs(shape, family)
    q, k, v = (t.to(DEV, dtype).requires_grad_() for t in (q, k, v))
    out, lse, *_ = ops.cross_attention_fwd(q.detach(), k.detach(), v.detach(), scale)
    got = ops.cross_attention(q, k, v, scale)
    assert torch.equal(got, out)  # the autograd path is the same launch
    grads = torch.autograd.grad(got, (q, k, v), (dout * dout_scale).to(DEV, dtype))
    assert got.dtype == dtype and all(g.dtype == dtype for g in grads) and lse.dtype == torch.float32
    return tuple(t.detach().double().cpu() for t in (out, lse) + tuple(grads))


def check(shape, family, dtype):
    o64, b32, b16 = oracle(shape, family)
    got = run_kernel(shape, family, dtype)
    bounds = b32 if dtype == torch.float32 else b16
    worst = []
    for name, a, b, bound in zip(NAMES, got, o64, bounds):
        assert a.shape == b.shape, name
        assert torch.isfinite(a).all(), f"{name}: non-finite values"
        err = float((a - b).abs().max())
        print(f"{shape} {family} {str(dtype)[6:]} {name}: err {err:.3e} bound {bound:.3e} ratio {err / bound if bound else 0.0:.3f}")
        worst.append((name, err, bound))
    for name, err, bound in worst:
        assert err <= bound, (shape, family, dtype, name, err, bound)
    return got, o64, bounds


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("shape", SMALL, ids=lambda s: "x".join(map(str, s)))
def test_small_shapes_against_float64(shape, family, dtype):
    got, o64, bounds = check(shape, family, dtype)
    q, k, v, dout, scale = inputs(shape, family)
    B, Nq, Nk, H = shape
    if family == "dominant":  # out is the dominating key's v, to the forward bound
        want = v[:, torch.arange(Nq) % Nk].double()
        assert float((got[0] - want).abs().max()) <= bounds[0]
    if family == "scale0":  # out is the mean of v, lse = log Nk, and nothing flows to q and k
        assert float((got[0] - v.double().mean(1, keepdim=True)).abs().max()) <= bounds[0]
        assert float((got[1] - np.log(Nk)).abs().max()) <= bounds[1]
        assert not got[2].any() and not got[3].any()
    if family in ("max_last", "max_first"):  # the family is what it says: every row's maximum is that key
        s = torch.einsum("bihd,bjhd->bhij", q.double(), k.double())
        assert (s.argmax(-1) == (Nk - 1 if family == "max_last" else 0)).all()
    if Nk == 1:
        assert float((got[0] - v.double().expand(B, Nq, H, 8)).abs().max()) <= bounds[0]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
def test_the_560_pass_shape_against_float64(dtype):
    check(BIG, "normal", dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("shape", [SMALL[1], BIG], ids=lambda s: "x".join(map(str, s)))
def test_forward_and_backward_are_deterministic(shape, dtype):
    a, b = run_kernel(shape, "normal", dtype), run_kernel(shape, "normal", dtype)
    for name, x, y in zip(NAMES, a, b):
        assert torch.equal(x, y), name


def test_fp16_overflow_is_inf_and_the_rest_stays_in_bound():
    """dout (a unit-scale one divided by 16, so that it stays inside fp16 itself) scaled by 65536: a gradient past fp16's range
    comes out as inf of the right sign (never clamped to 65504, never NaN) and every other entry stays within the fp16 bound of the
    scaled problem.  With every query on key 0, dv of that key sums 129 rows of dout and overflows in some heads."""
    shape, family, k_scale = SMALL[2], "max_first", 65536.0 / 16
    q, k, v, dout, scale = inputs(shape, family)
    o64 = reference(q, k, v, dout * k_scale, scale, torch.float64)[2:]
    emu = emulate_fp16_class(q, k, v, dout * k_scale, scale)
    assert torch.isfinite(_h(dout * k_scale)).all()  # the scaled dout itself is within fp16
    got = run_kernel(shape, family, torch.float16, dout_scale=k_scale)[2:]
    seen_inf = 0
    for name, a, b, e in zip(NAMES[2:], got, o64, emu):
        assert not torch.isnan(a).any(), name
        fin = torch.isfinite(e) & (b.abs() < 60000)
        bound = 4 * float((e - b)[fin].abs().max()) + 2.0 ** -11 * 65504
        must_inf, must_fin = b.abs() > 65520 + bound, b.abs() < 65520 - bound
        assert torch.isinf(a[must_inf]).all() and (torch.sign(a[must_inf]) == torch.sign(b[must_inf])).all(), name
        assert torch.isfinite(a[must_fin]).all(), name
        err = float((a - b)[must_fin].abs().max())
        print(f"overflow {name}: {int(must_inf.sum())} entries past fp16, finite err {err:.3e} bound {bound:.3e}")
        assert err <= bound, (name, err, bound)
        seen_inf += int(must_inf.sum())
    assert seen_inf > 0  # the case does overflow


def test_head_dim_other_than_8_raises():
    q = torch.zeros(1, 32, 4, 16, device=DEV)
    with pytest.raises(_lib.GfnError, match="head dim 16"):
        ops.cross_attention(q, q, q, 1.0)
    with pytest.raises(TypeError, match="float16 or float32"):
        ops.cross_attention(q[..., :8].contiguous().bfloat16(), q[..., :8].contiguous().bfloat16(), q[..., :8].contiguous().bfloat16(), 1.0)


# ---- the decoder module -------------------------------------------------------------------------------------------------------
def load_golden():
    z = np.load(GOLDEN)
    state = {k[len("param/"):]: torch.from_numpy(z[k].astype(np.float32)) for k in z.files if k.startswith("param/")}
    x, y = (torch.from_numpy(z[k].astype(np.float32)) for k in ("x", "y"))
    outs = tuple(torch.from_numpy(z[k]) for k in ("out_x", "out_y"))
    return json.loads(str(z["conf"])), state, x, y, outs, tuple(int(v) for v in z["grid"]), float(z["fp32_vs_fp64"])


def decoder(attn_impl, device="cpu", dtype=torch.float32):
    conf, state, *_ = load_golden()
    dec = CrossViewDecoder(conf, attn_impl=attn_impl)
    dec.load_state_dict(state, strict=True)
    return dec.train(False).to(device, dtype)


def test_decoder_fp32_reproduces_the_reference_modules_maps():
    """attn_impl="hip" in fp32 against the golden maps of the reference's own module, with the CPU test's bound: 4 x the reference
    module's fp32-vs-float64 difference."""
    _, _, x, y, outs, (B, H, W), e32 = load_golden()
    with torch.no_grad():
        got = decoder("hip", DEV)(x.to(DEV), y.to(DEV), vit_shape=(B, 3, H, W))
    for name, a, b in zip("xy", got, outs):
        err = float((a.cpu() - b).abs().max())
        print(f"decoder fp32 map {name}: err {err:.3e} bound {4 * e32:.3e}")
        assert err <= 4 * e32, (name, err)


def test_decoder_under_fp16_autocast():
    """Under fp16 autocast on the GPU against the same module in float64 with attn_impl="torch".  Bound, measured here and not
    derived: 4 x the error of the same module on the CPU under fp16 autocast with attn_impl="torch" against float64 (the 4 for the
    kernel's and the GEMM library's summation order)."""
    _, _, x, y, _, (B, H, W), _ = load_golden()
    shape = (B, 3, H, W)
    with torch.no_grad():
        want = decoder("torch", dtype=torch.float64)(x.double(), y.double(), vit_shape=shape)
        with torch.autocast(device_type="cpu", dtype=torch.float16):
            emu = decoder("torch")(x, y, vit_shape=shape)
        with torch.autocast(device_type="cuda", dtype=torch.float16):
            got = decoder("hip", DEV)(x.to(DEV), y.to(DEV), vit_shape=shape)
    for name, a, e, b in zip("xy", got, emu, want):
        e16 = float((e.double() - b).abs().max())
        err = float((a.double().cpu() - b).abs().max())
        print(f"decoder autocast map {name}: err {err:.3e} cpu-autocast error {e16:.3e} bound {4 * e16:.3e} max|map| {float(b.abs().max()):.2f}")
        assert torch.isfinite(a).all() and err <= 4 * e16, (name, err, 4 * e16)


def test_decoder_gradients_through_the_whole_fp32_module():
    """A scalar loss through the fp32 decoder on the GPU (attention forward and backward in HIP): gradients of every parameter and
    of both token inputs against the float64 CPU module, bound max(4 * E32, 2^-20 * max|oracle|) per tensor with E32 from the fp32
    CPU module (attn_impl="torch")."""
    _, _, x, y, _, (B, H, W), _ = load_golden()
    g = torch.Generator().manual_seed(5)
    wx, wy = torch.randn(B, 64, H, W, generator=g), torch.randn(B, 64, H, W, generator=g)

    def grads(dec, device, dtype):
        xs, ys = (t.to(device, dtype).requires_grad_() for t in (x, y))
        a, b = dec(xs, ys, vit_shape=(B, 3, H, W))
        loss = (a * wx.to(device, dtype)).sum() + (b * wy.to(device, dtype)).sum()
        names = ["x", "y"] + [n for n, _ in dec.named_parameters()]
        gs = torch.autograd.grad(loss, [xs, ys] + list(dec.parameters()))
        return {n: t.detach().double().cpu() for n, t in zip(names, gs)}

    want = grads(decoder("torch", dtype=torch.float64), "cpu", torch.float64)
    cpu32 = grads(decoder("torch"), "cpu", torch.float32)
    got = grads(decoder("hip", DEV), DEV, torch.float32)
    rows = []
    for n, w in want.items():
        bound = max(4 * float((cpu32[n] - w).abs().max()), 2.0 ** -20 * float(w.abs().max()))
        rows.append((float((got[n] - w).abs().max()) / bound, n))
    print(f"decoder gradients: worst err / bound {max(rows)[0]:.3f} at {max(rows)[1]}")
    assert len(rows) == 33 and max(rows)[0] <= 1.0, sorted(rows)[-3:]
