"""ops.self_attention (csrc/self_attn.hip) on the GPU: head dim 64, fp16, forward only, on the packed projection (B, N, 3, H, 64).

Oracle: ops.reference_self_attention in float64 on the CPU, on the fp16 values the kernel receives.  Bound on out, derived and not
tuned (every term is a property of the arithmetic class the header states, none is read off the kernel's results):

    2^-11 * max|out|          the one final rounding to fp16
  + 2^-11 * max|v|            each weight is rounded to fp16 once before P V on the matrix core: a relative 2^-11 per weight, and the
                              weights of a row sum to at most the row sum they are divided by
  + N * 2^-24 * max|v|        a weight below fp16's range (under 2^-24 of its tile's running maximum) is lost or moved by at most
                              2^-25; N of them, against a row sum of at least 1
  + max(4 * E32, 2^-20 * max|oracle|)     the fp32 class exactly as tests/test_cross_attn_gpu.py forms it: E32 = the definition run in
                              float32 on the CPU against float64, 4 for tile-wise summation order and the hardware exp2

Measured on an MI355X: MEASURED below, from the figures every test prints before it asserts.
"""
import functools

import pytest
import torch

from gfnet_amd import _lib, ops

pytestmark = pytest.mark.gpu

# error / bound on an MI355X (ROCm 7.0, torch 2.10), from the printed figures:
MEASURED = """
error / bound, worst case per family over the six shapes:
normal    0.21 (1x32x1: err 4.6e-04, bound 2.2e-03); at 1x1025x2 0.04
spread60  0.45 (2x95x2: err 1.9e-03, bound 4.3e-03); at 1x1025x2 0.23
scale0    0.05 (2x33x3); dominant_first / dominant_last 0.00 (err <= 3.5e-18: the key's v row to the last bit of the oracle)
layout    0 of 12160 values differ in either batch
overflow  |v| = 65504 and 65024: no result inf, none NaN, err 5e-11 (every result is the column's value itself)
"""

DEV = "cuda"
D = 64
# (B, N, H): one exact tile; one row past a tile on both axes with an odd head count; one token; a tail inside the second chunk's
# second tile; 16 heads over 2.5 chunks; the workload's own 1025 = 8 query blocks + 1 row, 16 key chunks + 1 row
SHAPES = [(1, 32, 1), (2, 33, 3), (1, 1, 2), (2, 95, 2), (1, 160, 16), (1, 1025, 2)]
FAMILIES = ("normal", "dominant_first", "dominant_last", "scale0", "spread60")
ids = lambda s: "x".join(map(str, s))  # noqa: E731


@functools.lru_cache(maxsize=None)
def inputs(shape, family):
    """(qkv (B, N, 3, H, 64) as an fp16 CPU tensor, scale, the dominant key or None)."""
    B, N, H = shape
    g = torch.Generator().manual_seed((B * 131 + N) * 131 + H * 7 + FAMILIES.index(family))
    q, k, v = (torch.randn(B, N, H, D, generator=g) for _ in range(3))
    scale, j = D ** -0.5, None
    if family == "spread60":  # scaled scores spread over +-60
        q, k = q.half().float(), k.half().float()
        scale = 60.0 / float(torch.einsum("bihd,bjhd->bhij", q, k).abs().max())
    elif family in ("dominant_first", "dominant_last"):
        # key j (in the first tile: every later tile must leave the maximum alone; in the last: every row rescales there) beats every
        # other key of every query by a score gap of at least 30: q . k_j >= 48, q . k_other <= 0 + noise of deviation 2
        j = min(3, N - 1) if family == "dominant_first" else N - 1
        q[..., 0] = q[..., 0].abs() + 4.0
        k[..., 0] = -k[..., 0].abs()
        k[..., 1:] *= 0.25
        k[:, j] = 0.0
        k[:, j, :, 0] = 12.0
        scale = 1.0
    elif family == "scale0":
        scale = 0.0
    return torch.stack((q, k, v), dim=2).half(), scale, j


@functools.lru_cache(maxsize=None)
def oracle(shape, family):
    """(out in float64, bound): computed once per case."""
    qkv, scale, _ = inputs(shape, family)
    o64 = ops.reference_self_attention(qkv.double(), scale)
    e32 = float((ops.reference_self_attention(qkv.float(), scale).double() - o64).abs().max())
    vmax, omax, N = float(qkv[:, :, 2].abs().max()), float(o64.abs().max()), shape[1]
    bound = 2.0 ** -11 * omax + 2.0 ** -11 * vmax + N * 2.0 ** -24 * vmax + max(4 * e32, 2.0 ** -20 * omax)
    return o64, bound


def run_kernel(qkv, scale):
    out = ops.self_attention(qkv.to(DEV), scale)
    assert out.dtype == torch.float16 and tuple(out.shape) == (qkv.shape[0], qkv.shape[1], qkv.shape[3], D) and out.is_contiguous()
    return out.cpu()


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_shapes_and_families_against_float64(shape, family):
    qkv, scale, j = inputs(shape, family)
    o64, bound = oracle(shape, family)
    got = run_kernel(qkv, scale).double()
    assert torch.isfinite(got).all()
    err = float((got - o64).abs().max())
    print(f"{ids(shape)} {family}: err {err:.3e} bound {bound:.3e} ratio {err / bound:.3f}")
    assert err <= bound, (shape, family, err, bound)
    v = qkv[:, :, 2].double()
    if j is not None:  # out is the dominant key's v row, and the family is what it says
        s = torch.einsum("bihd,bjhd->bhij", qkv[:, :, 0].double(), qkv[:, :, 1].double())
        top2 = s.topk(min(2, shape[1]), dim=-1).values
        assert (s.argmax(-1) == j).all() and (shape[1] == 1 or float((top2[..., 0] - top2[..., 1]).min()) >= 30.0)
        assert float((got - v[:, j:j + 1]).abs().max()) <= bound
    if family == "scale0":  # out is the mean of v
        assert float((got - v.mean(1, keepdim=True)).abs().max()) <= bound


# ---- layout: exact data ---------------------------------------------------------------------------------------------------------
BIT_DIMS = (3, 10, 17, 24, 31, 38, 45, 52)  # where the 8 sign bits of a key's code sit: in all four k-steps of the score product


def _codes(idx):
    c = torch.zeros(len(idx), D)
    for b, d in enumerate(BIT_DIMS):
        c[:, d] = ((idx >> b) & 1).float() * 2 - 1
    return c


def test_layout_exact():
    """Small-integer q and k: query i scores 160 on key pi(i) and at most 120 on any other (codes of +-1 over 8 dims, times 4 and
    5), so after the softmax pi(i) has weight exactly 1 in fp16 and every other key exactly 0.  v holds integers fp16 has exactly and
    that name their own place: head 0 has v[j, d] = 64 (j % 32) + d (the key's place in its tile and the value's place in the row),
    head 1 v[j, d] = 64 (j // 32) + d (the tile).  out must EQUAL v[pi(i)]: a P V product that pairs its two operands in different k
    orders, a swapped row and column, a wrong tile or a wrong d all give other integers."""
    B, N, H = 2, 95, 2
    i = torch.arange(N)
    pis = [(i * 37 + 11) % N, (i * 11 + 5) % N]
    assert all(sorted(p.tolist()) == list(range(N)) and (p != i).any() for p in pis)
    qkv = torch.zeros(B, N, 3, H, D)
    dd = torch.arange(D).float()
    for b, pi in enumerate(pis):
        qkv[b, :, 0] = 4.0 * _codes(pi).unsqueeze(1)
        qkv[b, :, 1] = 5.0 * _codes(i).unsqueeze(1)
        qkv[b, :, 2, 0] = 64.0 * (i % 32).float().unsqueeze(1) + dd
        qkv[b, :, 2, 1] = 64.0 * (i // 32).float().unsqueeze(1) + dd
    assert torch.equal(qkv.half().float(), qkv)  # every value is exact in fp16
    s = torch.einsum("bihd,bjhd->bhij", qkv[:, :, 0], qkv[:, :, 1])
    for b, pi in enumerate(pis):
        assert (s[b].argmax(-1) == pi).all() and float(s[b].max()) == 160.0
        top2 = s[b].topk(2, dim=-1).values
        assert float((top2[..., 0] - top2[..., 1]).min()) >= 40.0
    got = run_kernel(qkv.half(), 1.0).float()
    for b, pi in enumerate(pis):
        want = qkv[b, pi, 2]
        wrong = int((got[b] != want).sum())
        print(f"layout batch {b}: {wrong} of {want.numel()} values differ")
        assert torch.equal(got[b], want), (b, wrong)


def test_identical_calls_give_identical_bits():
    for shape in (SHAPES[3], SHAPES[5]):
        qkv, scale, _ = inputs(shape, "normal")
        assert torch.equal(run_kernel(qkv, scale), run_kernel(qkv, scale))


def test_overflow_is_inf_of_the_right_sign_never_nan_never_clamped():
    """out is a convex combination of v, so in exact arithmetic it cannot leave fp16's range where v is inside it: what CAN push a
    result past 65504 is the rounding margin of the bound above (weights rounded up by 2^-11 against an unrounded row sum).  With v
    = +-65504 per column the exact out is +-65504: every result must be that value or inf of the same sign, never NaN and never a
    clamped neighbour of the wrong side; with v = +-65024 (65504 less 15 of its ulps of 32, more than the bound) every result is
    finite and in bound."""
    shape = (2, 95, 2)
    qkv, scale, _ = inputs(shape, "normal")
    sign = torch.where(torch.arange(D) % 3 == 0, -1.0, 1.0)
    for mag, may_overflow in ((65504.0, True), (65024.0, False)):
        x = qkv.clone()
        x[:, :, 2] = (mag * sign).half()
        o64 = ops.reference_self_attention(x.double(), scale)
        got = run_kernel(x, scale).double()
        bound = 2 * 2.0 ** -11 * mag + shape[1] * 2.0 ** -24 * mag + 2.0 ** -20 * mag
        assert not torch.isnan(got).any()
        inf = torch.isinf(got)
        assert (torch.sign(got) == torch.sign(o64)).all()
        err = float((got - o64)[~inf].abs().max())
        print(f"overflow |v| = {mag}: {int(inf.sum())} of {got.numel()} results inf, finite err {err:.3e} bound {bound:.3e}")
        assert err <= bound
        assert may_overflow or not inf.any()


def test_unsupported_arguments_raise():
    with pytest.raises(_lib.GfnError, match="head dim 32"):
        ops.self_attention(torch.zeros(1, 32, 3, 2, 32, device=DEV, dtype=torch.float16), 1.0)
    with pytest.raises(TypeError, match="float16"):
        ops.self_attention(torch.zeros(1, 32, 3, 2, 64, device=DEV), 1.0)
    with pytest.raises(ValueError, match=r"\(B,N,3,H,D\)"):
        ops.self_attention(torch.zeros(1, 32, 2, 64, device=DEV, dtype=torch.float16), 1.0)
    with pytest.raises(_lib.GfnError, match="scale must be finite"):
        ops.self_attention(torch.zeros(1, 32, 3, 2, 64, device=DEV, dtype=torch.float16), float("inf"))
