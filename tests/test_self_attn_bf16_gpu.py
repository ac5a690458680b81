"""ops.self_attention_bf16 (csrc/self_attn.hip, the __bf16 instantiation) on the GPU: head dim 64, forward only, on the packed
projection (B, N, 3, H, 64) in bfloat16.  The shapes and families are those of tests/test_self_attn_gpu.py.

Oracle: ops.reference_self_attention in float64 on the CPU, on the bf16 values the kernel receives.  Bound on out, derived as that
file derives its own and not tuned (every term is a property of the arithmetic class the header states):

    2^-9 * max|out|           the one final rounding to bf16, a format with 8 significand bits
  + 2^-9 * max|v|             each weight is rounded to bf16 once before P V on the matrix core: a relative 2^-9 per weight, and the
                              weights of a row sum to at most the row sum they are divided by
  + max(4 * E32, 2^-20 * max|oracle|)     the fp32 term as that file forms it: E32 = the definition run in float32 on the CPU
                              against float64, 4 for tile-wise summation order and the hardware exp2

There is no N * 2^-24 term: bf16 has fp32's exponent range, so no weight that fp32 holds is lost to the operand's format.

Measured on an MI355X: MEASURED below, from the figures every test prints before it asserts.
"""
import functools

import pytest
import torch

from gfnet_amd import _lib, ops

pytestmark = pytest.mark.gpu

# error / bound on an MI355X, from the printed figures:
MEASURED = """
error / bound, worst case per family over the six shapes:
normal    0.49 (1x32x1: err 4.4e-03, bound 8.9e-03); at 1x1025x2 0.10
spread60  0.87 (2x95x2: err 1.5e-02, bound 1.7e-02); at 1x1025x2 0.71.  A float64 emulation of the class on the CPU (P and out rounded
          to bf16, everything else exact) has 0.87 as its own worst ratio over the same cases: the class's error, not the kernel's
scale0    0.19 (2x33x3); dominant_first / dominant_last 0.00 (err <= 6.9e-18: the key's v row to the last bit of the oracle)
layout    0 of 12160 values differ in either batch
range     |v| = 2^100: err 9.9e+14, bound 5.0e+27; |v| = 2^-100: err 6.1e-46, bound 3.1e-33; all finite, all signs right
"""

DEV = "cuda"
D = 64
BF = torch.bfloat16
# (B, N, H): one exact tile; one row past a tile on both axes with an odd head count; one token; a tail inside the second chunk's
# second tile; 16 heads over 2.5 chunks; the workload's own 1025 = 8 query blocks + 1 row, 16 key chunks + 1 row
SHAPES = [(1, 32, 1), (2, 33, 3), (1, 1, 2), (2, 95, 2), (1, 160, 16), (1, 1025, 2)]
FAMILIES = ("normal", "dominant_first", "dominant_last", "scale0", "spread60")
ids = lambda s: "x".join(map(str, s))  # noqa: E731


@functools.lru_cache(maxsize=None)
def inputs(shape, family):
    """(qkv (B, N, 3, H, 64) as a bf16 CPU tensor, scale, the dominant key or None)."""
    B, N, H = shape
    g = torch.Generator().manual_seed((B * 131 + N) * 131 + H * 7 + FAMILIES.index(family))
    q, k, v = (torch.randn(B, N, H, D, generator=g) for _ in range(3))
    scale, j = D ** -0.5, None
    if family == "spread60":  # scaled scores spread over +-60
        q, k = q.to(BF).float(), k.to(BF).float()
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
    return torch.stack((q, k, v), dim=2).to(BF), scale, j


def bound_for(qkv, scale, o64):
    e32 = float((ops.reference_self_attention(qkv.float(), scale).double() - o64).abs().max())
    vmax, omax = float(qkv[:, :, 2].double().abs().max()), float(o64.abs().max())
    return 2.0 ** -9 * omax + 2.0 ** -9 * vmax + max(4 * e32, 2.0 ** -20 * omax)


@functools.lru_cache(maxsize=None)
def oracle(shape, family):
    """(out in float64, bound): computed once per case."""
    qkv, scale, _ = inputs(shape, family)
    o64 = ops.reference_self_attention(qkv.double(), scale)
    return o64, bound_for(qkv, scale, o64)


def run_kernel(qkv, scale):
    out = ops.self_attention_bf16(qkv.to(DEV), scale)
    assert out.dtype == BF and tuple(out.shape) == (qkv.shape[0], qkv.shape[1], qkv.shape[3], D) and out.is_contiguous()
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
    5).  With scale = 4 the scaled gap is at least 128; past about 104 the fp32 exponential is exactly zero, so pi(i) has weight
    exactly 1 and every other key exactly 0 (at the fp16 test's gap of 40 a weight of 4e-18 survives in bf16 and leaks into rows whose
    v is 0).  v holds integers of at most 255, which bf16 has exactly, and that name their own place: head 0 has v[j, d] = (j % 32) +
    32 (d % 8) (the key's place in its tile, and d modulo 8), head 1 v[j, d] = (j // 32) + 4 d (the tile, and d).  out must EQUAL
    v[pi(i)]: a P V product that pairs its two operands in different k orders, a swapped row and column, a wrong tile or a wrong d all
    give other integers."""
    B, N, H = 2, 95, 2
    i = torch.arange(N)
    pis = [(i * 37 + 11) % N, (i * 11 + 5) % N]
    assert all(sorted(p.tolist()) == list(range(N)) and (p != i).any() for p in pis)
    qkv = torch.zeros(B, N, 3, H, D)
    dd = torch.arange(D)
    for b, pi in enumerate(pis):
        qkv[b, :, 0] = 4.0 * _codes(pi).unsqueeze(1)
        qkv[b, :, 1] = 5.0 * _codes(i).unsqueeze(1)
        qkv[b, :, 2, 0] = (i % 32).float().unsqueeze(1) + 32.0 * (dd % 8).float()
        qkv[b, :, 2, 1] = (i // 32).float().unsqueeze(1) + 4.0 * dd.float()
    assert float(qkv[:, :, 2].max()) <= 255.0
    assert torch.equal(qkv.to(BF).float(), qkv)  # every value is exact in bf16
    scale = 4.0
    s = scale * torch.einsum("bihd,bjhd->bhij", qkv[:, :, 0].double(), qkv[:, :, 1].double())
    for b, pi in enumerate(pis):
        assert (s[b].argmax(-1) == pi).all() and float(s[b].max()) == 640.0
        top2 = s[b].topk(2, dim=-1).values
        assert float((top2[..., 0] - top2[..., 1]).min()) >= 128.0
    got = run_kernel(qkv.to(BF), scale).float()
    for b, pi in enumerate(pis):
        want = qkv[b, pi, 2]
        wrong = int((got[b] != want).sum())
        print(f"layout batch {b}: {wrong} of {want.numel()} values differ")
        assert torch.equal(got[b], want), (b, wrong)


def test_identical_calls_give_identical_bits():
    for shape in (SHAPES[3], SHAPES[5]):
        qkv, scale, _ = inputs(shape, "normal")
        assert torch.equal(run_kernel(qkv, scale), run_kernel(qkv, scale))


def test_range_far_outside_fp16_is_finite_signed_and_in_bound():
    """bf16 has fp32's exponent range: v = +-2^100 per column (far past fp16's 65504, and 95 * 2^100 far inside fp32's range, the
    limit the header documents) and then +-2^-100 (far below fp16's least subnormal) come back finite, with the right sign and inside
    the bound above, which scales with max|v|.  A kernel that passed through fp16 anywhere gives inf or 0."""
    shape = (2, 95, 2)
    qkv, scale, _ = inputs(shape, "normal")
    sign = torch.where(torch.arange(D) % 3 == 0, -1.0, 1.0)
    for mag in (2.0 ** 100, 2.0 ** -100):
        x = qkv.clone()
        x[:, :, 2] = (mag * sign).to(BF)
        assert torch.equal(x[:, :, 2].double().abs(), torch.full(x[:, :, 2].shape, mag, dtype=torch.float64))
        o64 = ops.reference_self_attention(x.double(), scale)
        bound = bound_for(x, scale, o64)
        got = run_kernel(x, scale).double()
        assert torch.isfinite(got).all() and not torch.isnan(got).any()
        err = float((got - o64).abs().max())
        print(f"range |v| = {mag:.3e}: err {err:.3e} bound {bound:.3e} ratio {err / bound:.3f}")
        assert err <= bound, (mag, err, bound)
        assert (torch.sign(got) == torch.sign(o64)).all() and (got != 0).all()


def test_unsupported_arguments_raise():
    for dtype in (torch.float16, torch.float32):
        with pytest.raises(TypeError, match="bfloat16"):
            ops.self_attention_bf16(torch.zeros(1, 32, 3, 2, 64, device=DEV, dtype=dtype), 1.0)
    with pytest.raises(TypeError, match="float16"):  # the fp16 name keeps refusing everything but float16, bf16 included
        ops.self_attention(torch.zeros(1, 32, 3, 2, 64, device=DEV, dtype=BF), 1.0)
    with pytest.raises(_lib.GfnError, match="head dim 32"):
        ops.self_attention_bf16(torch.zeros(1, 32, 3, 2, 32, device=DEV, dtype=BF), 1.0)
    with pytest.raises(ValueError, match=r"\(B,N,3,H,D\)"):
        ops.self_attention_bf16(torch.zeros(1, 32, 2, 64, device=DEV, dtype=BF), 1.0)
    with pytest.raises(_lib.GfnError, match="scale must be finite"):
        ops.self_attention_bf16(torch.zeros(1, 32, 3, 2, 64, device=DEV, dtype=BF), float("inf"))
