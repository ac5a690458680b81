"""GPU: the inference conv block (csrc/conv_stack.hip, csrc/conv_stack_half.hip, csrc/conv_block_fused.h) on every kernel route
against float64 of its definition: relu((dw5x5(x) + conv bias) * alpha + beta) through a 1x1 conv.

The case table is generated from the route query (gfn_conv_block_route, the struct the launchers switch on): one case per
reachable instantiation (CASES), the edges by name (EDGES), two items per workgroup (TPB_CASES).  tests/test_conv_block_routes_cpu.py
holds the shared inputs, references and bounds, and checks -- without a GPU -- that the tables reach exactly the reachable set and
that every precondition below holds in float64.

Exact data (test_exact_*): small integers all the way, so that every class -- fp32, fp16 1x1 operands, fp16 maps, fused or
two-pass -- has to return the float64 result itself (torch.equal).  A dropped tap, a lost K tile, a stale halo, a wrong slab or a
bias of the wrong item parity has no tolerance to hide in.

Float inputs (test_float_families_against_float64): each class against float64 on exactly the operands it rounds, with a bound per
output element that is derived, not tuned:
  fp32 class           max(4 * E32, 2^-20 * max|ref|), E32 = the definition in float32 on the CPU against float64
  fp16 1x1 operands    sum_k |W16[m,k]| * (2^-11 * |t64[k,n]| + 4 * E_t) + max(4 * E_pw, 2^-20 * max|ref|): the ReLU output is rounded
                       to fp16 once (2^-11 relative) on top of the fp32 depthwise's own error (E_t = float32 on the CPU against
                       float64), and the 1x1 sum runs in fp32 (E_pw likewise, on the rounded operands)
  half-map output      + 2^-11 * |ref[m,n]| for the one final rounding
Families: normal; neg_alpha (every other channel with a negative BatchNorm weight); dead (>= 90 % of the ReLU outputs 0); cancel
(channel pairs cancel in the 1x1 sum: max|ref| < 0.05 * max sum|W||t|); large (ReLU outputs up to 4e3, inside the fp16 range);
border (x of O(100) in the two outermost rings of the map, O(0.01) inside: what a stale halo would show).
"""
import functools

import pytest
import torch

from gfnet_amd import ops
from test_conv_block_routes_cpu import (CLASSES, FAMILIES, exact_inputs, exact_reference, float_inputs, float_preconditions, half_out,
                                        route, route_key, to_half_map)

pytestmark = pytest.mark.gpu

# error / bound on an MI355X, worst element of the worst route per class and family, from the figures every test prints:
MEASURED = """
class     normal  neg_alpha  dead  cancel  large  border      (worst route of the class)
f32        0.29     0.22     0.26   0.28    0.24   0.29
f32_2p     0.18     0.18     0.25   0.36    0.19   0.15
op16       0.97     0.97     0.95   0.94    0.96   0.97       worst: 1x5x61x164 neg_alpha, err 2.016e-03, bound 2.068e-03
op16_2p    0.67     0.71     0.86   0.70    0.63   0.66
map_fh     0.96     0.93     0.92   0.80    0.91   0.90
map_hh     0.94     0.97     0.95   0.92    0.94   0.88
map_hf     0.84     0.78     0.86   0.79    0.82   0.80
The fp16 classes sit close under 1 on the narrow blocks by construction: with C = 3 or 5 the bound is a handful of half-ulp
roundings of the ReLU output, and among 10^4 .. 10^6 outputs one has all of them near the half ulp and of one sign.
exact     0 differing values on every case of CASES, EDGES, TPB_CASES and WRITE_CASES
"""

DEV = "cuda"


def _generated_cases():
    """One case per reachable instantiation: the smallest grid that reaches the tile shape (G = 4: 16x8 tiles; 16 and 32: 8x16
    and 4x32 tiles, 256-cell tiles where the class takes them; 68 and 164: the same widths on a map that does not divide into
    256-cell tiles, with partial tiles; 5: the two-pass form on a grid side that is no multiple of 4) and one odd, ragged M per count
    of 32-row tiles (32 t - 3, t = 1 .. 16)."""
    seen = {}
    for cls in CLASSES:
        for G in (4, 5, 16, 32, 68, 164):
            for t in range(1, 17):
                B, M = (2 if G <= 16 else 1), 32 * t - 3
                r = route(cls, B, 3, M, G)
                if r is None or route_key(r) in seen:
                    continue
                if G >= 68:
                    C = (1, 3, 5)[t % 3]
                elif G == 32:
                    C = 17 if r["KW"] == 2 else (3, 17)[t % 2]
                else:
                    C = 33 if r["KW"] == 2 else (1, 3, 15, 16, 17, 33)[(t + G) % 6]
                seen[route_key(r)] = (cls, B, C, M, G)
    return list(seen.values())


CASES = _generated_cases()
EDGES = (
    # M > 448: a ragged and a full second slab group, every class, fused and two-pass
    [(cls, 1, 20, M, 8) for cls in CLASSES for M in (449, 480)]
    # the folded last block: C -> 3, fp16 map in and fp32 out, and the fp32 class
    + [(cls, 1, C, 3, G) for cls in ("map_hf", "f32") for C, G in ((24, 16), (73, 12), (417, 8))]
    # M just below, at and just above 32 * MT * NS: seven tiles in one slab, 4 and 5 in two, an odd tile count (9) over two slabs
    + [(cls, 1, 17, M, 4) for cls in ("f32", "op16", "map_fh", "map_hh") for M in (223, 224, 225, 256, 288, 289, 447, 448)]
    # partial tiles at every tile width
    + [(cls, 1, 3, 40, G) for cls in ("f32", "op16", "map_hh") for G in (8, 12, 24, 40, 68, 164)]
    # two K tiles per iteration with a lone last K tile (C = 16, 48, 417: 1, 3, 27 K tiles), wide C
    + [("map_hh", 1, 16, 100, 4), ("map_hh", 1, 48, 100, 8), ("map_hh", 1, 417, 100, 4), ("map_hh", 1, 417, 129, 16), ("map_hh", 1, 48, 129, 32)]
    + [(cls, 1, 417, 417, 16) for cls in ("f32", "op16", "map_fh", "map_hf")]
    # the two-pass form on grids that are no multiple of 4
    + [(cls, 2, 15, 33, G) for cls in ("f32", "op16_2p") for G in (5, 10)])
EXACT = list(enumerate(CASES + EDGES))  # (seed, case)
# section f: one per tile width and class, partial tiles on every side; the two-pass form with its scratch map
WRITE_CASES = ([(cls, 2, 3, 29, G) for cls in ("f32", "op16", "map_fh", "map_hh", "map_hf") for G in (12, 68, 164)]
               + [("f32_2p", 2, 3, 29, 12), ("op16_2p", 2, 3, 29, 10), ("f32_2p", 1, 3, 29, 5)])
# section c: >= 16384 work items, two per workgroup.  An odd item count (the last workgroup has one item); 256-cell tiles on the
# matrix-core depthwise; 4x32 tiles in fp32; two K tiles per iteration; two slab groups
TPB_PERIOD = 5  # distinct maps of a batch: map b is map b % 5, so every pair of neighbours shares a workgroup somewhere
TPB_CASES = [("f32", 16385, 2, 3, 4), ("op16", 16385, 2, 3, 4), ("map_hh", 16385, 2, 3, 16), ("map_fh", 16385, 2, 3, 16),
             ("f32", 2049, 2, 3, 32), ("map_hh", 16385, 17, 100, 4), ("map_hf", 16385, 3, 3, 4), ("f32", 8193, 3, 480, 4)]
# section b: about 30 routes across every class
FLOAT_ROUTES = [
    ("f32", 2, 17, 29, 4), ("f32", 1, 33, 225, 16), ("f32", 1, 3, 61, 32), ("f32", 1, 5, 40, 68), ("f32", 1, 20, 449, 8), ("f32", 1, 24, 3, 12),
    ("f32", 1, 73, 3, 8), ("f32", 1, 417, 3, 4),
    ("f32_2p", 2, 7, 7, 5), ("f32_2p", 1, 16, 100, 8), ("f32_2p", 1, 20, 449, 8),
    ("op16", 1, 17, 29, 16), ("op16", 1, 3, 93, 32), ("op16", 1, 5, 61, 164), ("op16", 2, 33, 161, 4), ("op16", 1, 20, 480, 8),
    ("op16_2p", 1, 15, 33, 10), ("op16_2p", 1, 48, 225, 12),
    ("map_fh", 1, 17, 29, 4), ("map_fh", 1, 33, 100, 16), ("map_fh", 1, 3, 61, 32), ("map_fh", 1, 5, 29, 68),
    ("map_hh", 2, 17, 29, 4), ("map_hh", 1, 33, 100, 8), ("map_hh", 1, 48, 161, 16), ("map_hh", 1, 17, 129, 32), ("map_hh", 1, 15, 61, 16),
    ("map_hh", 1, 3, 93, 164), ("map_hh", 1, 417, 417, 8), ("map_hh", 1, 20, 449, 8),
    ("map_hf", 1, 24, 3, 16), ("map_hf", 1, 73, 3, 8), ("map_hf", 1, 417, 3, 4), ("map_hf", 1, 33, 225, 12), ("map_hf", 1, 17, 29, 32)]


def _id(case):
    case = case[1] if isinstance(case[1], tuple) else case
    return "%s-%dx%dx%dx%d" % case


def pack(p):
    d = {k: (v.to(DEV) if v is not None else None) for k, v in p.items()}
    return ops.conv_block_pack(d["w"], d["cb"], d["alpha"], d["beta"], d["pw"], d["pb"])


def run_block(cls, x, p, out=None, t_scratch=None, pad_is_zero=True):
    """(result as (B, M, G, G) float32, the tensor the kernel wrote), both on the GPU; x (B, C, G, G) float32."""
    kw = CLASSES[cls][0]
    C, M = x.shape[1], p["pw"].shape[0]
    xd, packed = x.to(DEV), pack(p)
    if "variant" in kw:
        raw = ops.conv_block(xd, packed, M, out=out, variant=kw["variant"], t_scratch=t_scratch)
        return raw, raw
    raw = ops.conv_block_half(to_half_map(xd) if kw["x_half"] else xd, packed, C, M, out=out, out_half=kw["out_half"])
    assert out is None or raw.data_ptr() == out.data_ptr()
    if not kw["out_half"]:
        assert raw.dtype == torch.float32
        return raw, raw
    assert raw.dtype == torch.float16 and tuple(raw.shape) == (x.shape[0], (M + 1) // 2, x.shape[2], x.shape[3], 2)
    if M % 2 and pad_is_zero:  # the odd channel past M is written as zero: the next block reads it
        assert float(raw[:, -1, :, :, 1].abs().max()) == 0.0, "odd channel past M of a half map"
    return ops.half_map_to_float(raw, M), raw


def assert_same(got, want, what):
    """got == want value for value (same device), or the count of differing values and the first of them."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if torch.equal(got, want):
        print(f"{what}: 0 of {want.numel()} values differ")
        return
    diff = got != want
    first = tuple(diff.nonzero()[0].tolist())
    raise AssertionError(f"{what}: {int(diff.sum())} of {want.numel()} values differ, first at (b, m, i, j) = {first}: "
                         f"got {float(got[first])}, want {float(want[first])}")


# ---- a. exact data, every route, every class -----------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,case", EXACT, ids=[_id(c) for _, c in EXACT])
def test_exact_every_instantiation(seed, case):
    cls, B, C, M, G = case
    x, p = exact_inputs(B, C, M, G, half_out(cls), seed)
    ref = exact_reference(x, p, half_out(cls))
    got, _ = run_block(cls, x, p)
    assert_same(got.cpu().double(), ref, _id(case))


# ---- c. two items per workgroup ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", TPB_CASES, ids=_id)
def test_exact_two_items_per_workgroup(case):
    cls, B, C, M, G = case
    r = route(cls, B, C, M, G)
    assert r["tpb"] == 2 and r["nwork"] >= 16384
    xs, p = exact_inputs(TPB_PERIOD, C, M, G, half_out(cls), 5)
    ref = exact_reference(xs, p, half_out(cls)).float().to(DEV)
    idx = torch.arange(B, device=DEV) % TPB_PERIOD
    x = xs.to(DEV)[idx]
    got, _ = run_block(cls, x, p)
    want = ref[idx]
    assert_same(got, want, _id(case) + " against float64")
    if "variant" in CLASSES[cls][0]:
        two_pass = ops.conv_block(x, pack(p), M, variant=CLASSES[cls][0]["variant"] | 1)
        assert_same(got, two_pass, _id(case) + " against the two-pass kernels")


# ---- b. float inputs against float64 with derived bounds -------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def float_case(case, family):
    cls, B, C, M, G = case
    x, p = float_inputs(B, C, M, G, family, CLASSES[cls][1])
    return (x, p) + float_preconditions(x, p, CLASSES[cls][1], half_out(cls), family)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("case", FLOAT_ROUTES, ids=_id)
def test_float_families_against_float64(case, family):
    x, p, ref, bound = float_case(case, family)
    got = run_block(case[0], x, p)[0].cpu().double()
    assert torch.isfinite(got).all()
    err = (got - ref).abs()
    ratio = err / bound
    at = tuple(int(v) for v in (ratio == ratio.max()).nonzero()[0])
    print(f"{_id(case)} {family}: err {float(err[at]):.3e} bound {float(bound[at]):.3e} ratio {float(ratio.max()):.3f} "
          f"(max err {float(err.max()):.3e}, max|ref| {float(ref.abs().max()):.3e})")
    assert float(ratio.max()) <= 1.0, (case, family, at, float(err[at]), float(bound[at]))


# ---- f. every element written, nothing else ----------------------------------------------------------------------------------------
GUARD = 4096


def guarded(shape, dtype, sentinel):
    """(buffer, view): the view sits in the middle of the buffer and is filled with NaN, GUARD elements of `sentinel` on both sides."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * GUARD,), sentinel, device=DEV, dtype=dtype)
    view = buf[GUARD:GUARD + n].view(shape)
    view.fill_(float("nan"))
    return buf, view


def assert_guards_untouched(buf, sentinel, what):
    bits = buf.view(torch.int32 if buf.dtype == torch.float32 else torch.int16)
    want = torch.full((1,), sentinel, dtype=buf.dtype, device=DEV).view(bits.dtype)
    assert bool((bits[:GUARD] == want).all()) and bool((bits[-GUARD:] == want).all()), what + ": wrote outside its output"
    assert not bool(torch.isnan(buf[GUARD:-GUARD]).any()), what + ": left an element unwritten"


@pytest.mark.parametrize("k,case", list(enumerate(WRITE_CASES)), ids=[_id(c) for c in WRITE_CASES])
def test_every_element_written_and_nothing_else(k, case):
    cls, B, C, M, G = case
    x, p = exact_inputs(B, C, M, G, half_out(cls), len(EXACT) + k)
    ref = exact_reference(x, p, half_out(cls))
    shape, dtype = ((B, (M + 1) // 2, G, G, 2), torch.float16) if half_out(cls) else ((B, M, G, G), torch.float32)
    buf, view = guarded(shape, dtype, -12345.0)
    tbuf = tview = None
    if not route(cls, B, C, M, G)["fused"]:
        tbuf, tview = guarded((B, C, G, G), torch.float32, -54321.0)
    got, raw = run_block(cls, x, p, out=view, t_scratch=tview)
    assert raw.data_ptr() == view.data_ptr()
    assert_guards_untouched(buf, -12345.0, _id(case))
    if tbuf is not None:
        assert_guards_untouched(tbuf, -54321.0, _id(case) + " t_scratch")
    assert_same(got.cpu().double(), ref, _id(case))


# ---- g. locality of a non-finite input -----------------------------------------------------------------------------------------------
LOCAL_CASES = [(cls, v) for cls in ("f32", "f32_2p", "op16", "map_fh", "map_hh", "map_hf")
               for v in ("inf", "nan", "1e5") if not (cls.startswith("map") and v == "1e5")]  # 1e5 is no fp16 value: the fp32 entry's case


@pytest.mark.parametrize("cls,value", LOCAL_CASES, ids=["%s-%s" % c for c in LOCAL_CASES])
def test_a_non_finite_input_stays_local(cls, value):
    """One bad value at an interior cell and one at a corner of channel 2 of map 1: outside |drow| <= 2 and |dcol| <= 2 (the VALU
    depthwise of the fp32 entry) or |dcol| <= 11 (the banded matrix-core depthwise of the fp16-map entry, include/gfnet_hip.h) of
    either cell, every output keeps the bits of the clean run."""
    maps, value = "variant" not in CLASSES[cls][0], float(value)
    B, C, M = 2, 5, 29
    for G in (32, 40, 48):  # 4x32, 16x8 and 8x16 tiles
        x, p = float_inputs(B, C, M, G, "normal", CLASSES[cls][1])
        cells = [(G // 2 + 1, G // 2 - 3), (0, 0)]
        bad = x.clone()
        for i, j in cells:
            bad[1, 2, i, j] = value
        clean, craw = run_block(cls, x, p)
        got, raw = run_block(cls, bad, p, pad_is_zero=False)
        if raw.dim() == 5:  # a half map: every stored value, the odd channel past M included (0 * inf = NaN is within the envelope too)
            clean, got = ops.half_map_to_float(craw, 2 * craw.shape[1]), ops.half_map_to_float(raw, 2 * raw.shape[1])
        assert torch.isfinite(clean).all()
        rows, cols = torch.arange(G).view(G, 1), torch.arange(G).view(1, G)
        inside = torch.zeros(G, G, dtype=torch.bool)
        for i, j in cells:
            inside |= ((rows - i).abs() <= 2) & ((cols - j).abs() <= (11 if maps else 2))
        same = clean.view(torch.int32) == got.view(torch.int32)
        assert bool(same[0].all()), (cls, G, "the other map of the batch changed")
        changed = (~same[1] & ~inside.to(DEV)).nonzero()
        assert changed.numel() == 0, (cls, G, value, "changed outside the envelope, first (m, i, j):", changed[0].tolist(), len(changed))
        assert not bool(same[1].all()), "the bad value reached no output at all"
        if value == float("inf"):  # (a NaN ends at the ReLU: fmaxf(NaN, 0) = 0, include/gfnet_hip.h)
            assert not bool(torch.isfinite(got[1]).all())


# ---- h. the small-M 1x1 conv -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,M,K,G", [(2, 13, 7, 5), (1, 16, 33, 6), (3, 16, 417, 4), (2, 13, 24, 8)])
def test_pointwise_conv_exact(B, M, K, G):
    g = torch.Generator().manual_seed(M * 1000 + K)
    t = torch.randint(-3, 4, (B, K, G, G), generator=g).float()
    w = torch.randint(-2, 3, (M, K), generator=g).float()
    b = torch.randint(-4, 5, (M,), generator=g).float()
    want = torch.nn.functional.conv2d(t.double(), w.double().view(M, K, 1, 1), b.double())
    assert float(want.abs().max()) < 2 ** 24
    assert_same(ops.pointwise_conv(t.to(DEV), w.to(DEV), b.to(DEV)).cpu().double(), want, f"pointwise {B}x{M}x{K}x{G}")
