"""GPU: the inference conv block on bf16 maps (csrc/conv_stack_bf16.hip = csrc/conv_block_fused.h on the 16-bit element __bf16;
ops.conv_block_bf16, ConvRefiner.conv_precision = "bf16") against float64 of its definition, and the stack against torch's own bf16
autocast of the same modules.

Classes: map_fb (fp32 map in, bf16 map out: a stack's first block), map_bb (bf16 in and out), map_bf (bf16 in, fp32 out: the last
block).  The bf16 entry routes as the fp16-map entry does, so the cases are the map_* rows of the tables of
tests/test_conv_block_routes_gpu.py run in the corresponding bf16 class; tests/test_conv_block_bf16_cpu.py holds the inputs, the
references and the bound, and checks without a GPU that the cases reach every instantiation and that every precondition holds.

Exact data: two integer sets that fit bf16's 8 bits where the output is a bf16 map (dense taps with two 1x1 weights per row, sparse
taps with 17), the fp16 file's set where it is fp32: torch.equal against float64.

Float inputs against float64 on the operands the class rounds (x, taps and W to bf16), bound per output element
  sum_k |W_bf16[m,k]| * (2^-8 * |t64[k,n]| + 4 * E_t) + max(4 * E_pw, 2^-20 * max|ref|)     (+ 2^-8 * |ref[m,n]| into a bf16 map)
with E_t, E_pw the float32-on-the-CPU errors of the two stages (test_conv_block_bf16_cpu.reference_bf16): the fp16 file's bound
with bf16's unit roundoff.  Families: the fp16 file's six and beyond_fp16 (ReLU outputs past 1e5, results past 65504).
"""
import functools

import pytest
import torch

import test_conv_block_routes_gpu as half_gpu
from gfnet_amd import _lib, ops
from gfnet_amd._lib import GfnError
from test_conv_block_bf16_cpu import (BF16_FAMILIES, CLASSES, bf16_out, exact_inputs_bf16, exact_reference_bf16, float_inputs_bf16,
                                      float_preconditions_bf16, route, sets_of, to_bf16_map, twin_cases)
from test_conv_block_routes_cpu import to_half_map
from test_conv_block_routes_gpu import assert_guards_untouched, assert_same, guarded

pytestmark = pytest.mark.gpu

# error / bound on an MI355X, worst element of the worst route per class and family, from the figures every test prints:
MEASURED = """
class     normal  neg_alpha  dead  cancel  large  border  beyond_fp16      (worst route of the class)
map_fb     0.98     0.94     0.97   0.90    0.95   0.93      0.93
map_bb     0.97     0.98     0.98   0.93    0.95   0.93      0.96          worst: 1x3x93x164 neg_alpha, err 3.882e-03, bound 3.951e-03
map_bf     0.87     0.81     0.94   0.82    0.78   0.85      0.78
As in the fp16 file the narrow blocks sit close under 1 by construction: with C = 3 or 5 the bound is a handful of half-ulp roundings
of the ReLU output, and among 10^4 .. 10^6 outputs one has all of them near the half ulp and of one sign.
exact     0 differing values on every case of EXACT_CASES (both sets), TPB_CASES and WRITE_CASES
stack     error against the fp32 modules, bf16 class / torch's bf16 autocast of the modules: 7.8e-4 / 1.8e-3 (C = 24, G = 64),
          8.1e-4 / 1.2e-3 (73, 32), 8.3e-4 / 1.1e-3 (177, 16), 8.3e-4 / 1.2e-3 (417, 8), 7.3e-4 / 9.7e-4 (361, 40)
"""

DEV = "cuda"
EXACT_CASES = twin_cases(half_gpu.CASES + half_gpu.EDGES)
EXACT = list(enumerate(EXACT_CASES))  # (seed, case)
TPB_CASES = twin_cases(half_gpu.TPB_CASES)
TPB_PERIOD = half_gpu.TPB_PERIOD
FLOAT_ROUTES = twin_cases(half_gpu.FLOAT_ROUTES)
WRITE_CASES = twin_cases(half_gpu.WRITE_CASES)


def _id(case):
    case = case[1] if isinstance(case[1], tuple) else case
    return "%s-%dx%dx%dx%d" % case


def pack(p):
    d = {k: (v.to(DEV) if v is not None else None) for k, v in p.items()}
    return ops.conv_block_pack_bf16(d["w"], d["cb"], d["alpha"], d["beta"], d["pw"], d["pb"])


def run_block(cls, x, p, out=None, pad_is_zero=True):
    """(result as (B, M, G, G) float32, the tensor the kernel wrote), both on the GPU; x (B, C, G, G) float32."""
    kw = CLASSES[cls]
    C, M = x.shape[1], p["pw"].shape[0]
    xd = x.to(DEV)
    raw = ops.conv_block_bf16(to_bf16_map(xd) if kw["x_bf16"] else xd, pack(p), C, M, out=out, out_bf16=kw["out_bf16"])
    assert out is None or raw.data_ptr() == out.data_ptr()
    if not kw["out_bf16"]:
        assert raw.dtype == torch.float32 and tuple(raw.shape) == (x.shape[0], M, x.shape[2], x.shape[3])
        return raw, raw
    assert raw.dtype == torch.bfloat16 and tuple(raw.shape) == (x.shape[0], (M + 1) // 2, x.shape[2], x.shape[3], 2)
    if M % 2 and pad_is_zero:  # the odd channel past M is written as zero: the next block reads it
        assert float(raw[:, -1, :, :, 1].abs().max()) == 0.0, "odd channel past M of a bf16 map"
    return ops.bf16_map_to_float(raw, M), raw


# ---- 5. exact data, every instantiation --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,case", EXACT, ids=[_id(c) for _, c in EXACT])
def test_exact_every_instantiation(seed, case):
    cls, B, C, M, G = case
    for which in sets_of(cls):
        x, p = exact_inputs_bf16(B, C, M, G, bf16_out(cls), seed, which)
        ref = exact_reference_bf16(x, p, bf16_out(cls), which)
        got, _ = run_block(cls, x, p)
        assert_same(got.cpu().double(), ref, _id(case) + " " + which)


# ---- 6. two items per workgroup ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", TPB_CASES, ids=_id)
def test_exact_two_items_per_workgroup(case):
    cls, B, C, M, G = case
    r = route(cls, B, C, M, G)
    assert r["tpb"] == 2 and r["nwork"] >= 16384
    idx = torch.arange(B, device=DEV) % TPB_PERIOD
    for which in sets_of(cls):
        xs, p = exact_inputs_bf16(TPB_PERIOD, C, M, G, bf16_out(cls), 5, which)
        ref = exact_reference_bf16(xs, p, bf16_out(cls), which).float().to(DEV)
        got, _ = run_block(cls, xs.to(DEV)[idx], p)
        assert_same(got, ref[idx], _id(case) + " " + which + " against float64")


# ---- 7. float inputs against float64 with the derived bound -----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def float_case(case, family):
    cls, B, C, M, G = case
    x, p = float_inputs_bf16(B, C, M, G, family)
    return (x, p) + float_preconditions_bf16(x, p, bf16_out(cls), family)


@pytest.mark.parametrize("family", BF16_FAMILIES)
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


# ---- 8. every element written, nothing else ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,case", list(enumerate(WRITE_CASES)), ids=[_id(c) for c in WRITE_CASES])
def test_every_element_written_and_nothing_else(k, case):
    cls, B, C, M, G = case
    which = sets_of(cls)[k % len(sets_of(cls))]
    x, p = exact_inputs_bf16(B, C, M, G, bf16_out(cls), len(EXACT) + k, which)
    ref = exact_reference_bf16(x, p, bf16_out(cls), which)
    shape, dtype = ((B, (M + 1) // 2, G, G, 2), torch.bfloat16) if bf16_out(cls) else ((B, M, G, G), torch.float32)
    buf, view = guarded(shape, dtype, -12345.0)
    got, raw = run_block(cls, x, p, out=view)
    assert raw.data_ptr() == view.data_ptr()
    assert_guards_untouched(buf, -12345.0, _id(case))
    assert_same(got.cpu().double(), ref, _id(case))


# ---- 9. locality of a non-finite or huge input ----------------------------------------------------------------------------------------
LOCAL_CASES = [(cls, v) for cls in CLASSES for v in ("inf", "nan", "1e5")]  # 1e5 is a bf16 value: the map classes take it too


@pytest.mark.parametrize("cls,value", LOCAL_CASES, ids=["%s-%s" % c for c in LOCAL_CASES])
def test_a_bad_input_stays_local(cls, value):
    """One bad value at an interior cell and one at a corner of channel 2 of map 1: outside |drow| <= 2, |dcol| <= 11 (the banded
    matrix-core depthwise, include/gfnet_hip.h: the fp16-map entry's envelope) of either cell every output keeps the bits of the clean
    run."""
    value = float(value)
    B, C, M = 2, 5, 29
    for G in (32, 40, 48):  # 4x32, 16x8 and 8x16 tiles
        x, p = float_inputs_bf16(B, C, M, G, "normal")
        cells = [(G // 2 + 1, G // 2 - 3), (0, 0)]
        bad = x.clone()
        for i, j in cells:
            bad[1, 2, i, j] = value
        clean, craw = run_block(cls, x, p)
        got, raw = run_block(cls, bad, p, pad_is_zero=False)
        if raw.dim() == 5:  # a bf16 map: every stored value, the odd channel past M included
            clean, got = ops.bf16_map_to_float(craw, 2 * craw.shape[1]), ops.bf16_map_to_float(raw, 2 * raw.shape[1])
        assert torch.isfinite(clean).all()
        rows, cols = torch.arange(G).view(G, 1), torch.arange(G).view(1, G)
        inside = torch.zeros(G, G, dtype=torch.bool)
        for i, j in cells:
            inside |= ((rows - i).abs() <= 2) & ((cols - j).abs() <= 11)
        same = clean.contiguous().view(torch.int32) == got.contiguous().view(torch.int32)
        assert bool(same[0].all()), (cls, G, "the other map of the batch changed")
        changed = (~same[1] & ~inside.to(DEV)).nonzero()
        assert changed.numel() == 0, (cls, G, value, "changed outside the envelope, first (m, i, j):", changed[0].tolist(), len(changed))
        assert not bool(same[1].all()), "the bad value reached no output at all"
        if value == float("inf"):  # (a NaN ends at the ReLU: fmaxf(NaN, 0) = 0, include/gfnet_hip.h)
            assert not bool(torch.isfinite(got[1]).all())
        elif value == 1e5:         # finite in bf16, and so is everything computed from it
            assert bool(torch.isfinite(got).all())


# ---- 10. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals():
    x, p = float_inputs_bf16(1, 8, 8, 8, "normal")
    packed, xd = pack(p), x.to(DEV)
    xm = to_bf16_map(xd)
    assert ops.conv_block_bf16(xm, packed, 8, 8).dtype == torch.bfloat16
    with pytest.raises(GfnError, match="in-place"):
        ops.conv_block_bf16(xm, packed, 8, 8, out=xm)
    with pytest.raises(ValueError, match="float16 map"):
        ops.conv_block_bf16(to_half_map(xd), packed, 8, 8)
    with pytest.raises(ValueError, match="bf16 map is a contiguous"):
        ops.conv_block_bf16(to_bf16_map(xd[:, :6]), packed, 8, 8)          # a map of another channel count
    with pytest.raises(ValueError, match="packed parameters"):
        ops.conv_block_bf16(xm, packed, 8, 40)
    with pytest.raises(ValueError, match="packed parameters"):
        ops.conv_block_bf16(xm, packed[:-1], 8, 8)
    with pytest.raises(ValueError, match="square"):
        ops.conv_block_bf16(xd[:, :, :4].contiguous(), packed, 8, 8)
    x10, _ = float_inputs_bf16(1, 8, 8, 10, "normal")
    with pytest.raises(GfnError, match="multiple of 4"):
        ops.conv_block_bf16(x10.to(DEV), packed, 8, 8)
    # the C entry point itself: an fp16 map is refused with a message that names the type it takes
    L = _lib.lib()
    out = torch.empty_like(xm)
    half = to_half_map(xd)
    for xa, xt, yt in ((half, _lib.GFN_F16, _lib.GFN_BF16), (xm, _lib.GFN_BF16, _lib.GFN_F16), (xd, _lib.GFN_F32, _lib.GFN_F32)):
        rc = L.gfn_conv_block_bf16_fwd(_lib.ptr(xa), xt, _lib.ptr(packed), _lib.ptr(out), yt, 1, 8, 8, 8, None)
        assert rc != 0 and b"GFN_BF16" in L.gfn_last_error(), (xt, yt, L.gfn_last_error())
    rc = L.gfn_conv_block_half_fwd(_lib.ptr(xm), _lib.GFN_BF16, _lib.ptr(packed), _lib.ptr(out), _lib.GFN_F16, 1, 8, 8, 8, None)
    assert rc != 0                                                          # and the fp16 entry takes no bf16 map


def test_pack_bf16_differs_from_pack_only_in_the_16_bit_sections():
    """The layout and size of gfn_conv_block_pack; every fp32 section (depthwise parameters, fp32 weights, bias, and the conv bias,
    alpha, beta entries of the matrix-core section) bit for bit, the two 16-bit sections the bf16 rounding of what the fp16 pack rounds
    to fp16."""
    C, M = 19, 37
    x, p = float_inputs_bf16(1, C, M, 4, "normal")
    d = {k: (v.to(DEV) if v is not None else None) for k, v in p.items()}
    args = (d["w"], d["cb"], d["alpha"], d["beta"], d["pw"], d["pb"])
    ph, pb = ops.conv_block_pack(*args).cpu(), ops.conv_block_pack_bf16(*args).cpu()
    assert ph.shape == pb.shape and ph.numel() == int(_lib.lib().gfn_conv_block_packed_floats(C, M))
    Kp, Mp = 32, 64
    wt16_off = (Kp // 2) * 64 + Kp * Mp + Mp
    mm_off = wt16_off + Kp * Mp // 2
    assert ph.numel() == mm_off + (Kp // 2) * 96
    assert torch.equal(ph[:wt16_off].view(torch.int32), pb[:wt16_off].view(torch.int32))
    mm_h, mm_b = ph[mm_off:].view(-1, 96), pb[mm_off:].view(-1, 96)
    assert torch.equal(mm_h[:, 80:].view(torch.int32), mm_b[:, 80:].view(torch.int32))
    # 1x1 weights: slot [k half][m][8] of a K tile
    w16_h = ph[wt16_off:mm_off].view(torch.float16).view(Kp // 8, Mp, 8).permute(1, 0, 2).reshape(Mp, Kp)
    w16_b = pb[wt16_off:mm_off].view(torch.bfloat16).view(Kp // 8, Mp, 8).permute(1, 0, 2).reshape(Mp, Kp)
    want = torch.zeros(Mp, Kp)
    want[:M, :C] = p["pw"]
    assert torch.equal(w16_h.float(), want.half().float()) and torch.equal(w16_b.float(), want.bfloat16().float())
    # banded taps: [ch][dy][8] dwords, channel 2p+ch in the low / high half
    taps_b = mm_b[:, :80].contiguous().view(torch.bfloat16).view(-1, 2, 5, 8, 2)
    wantt = torch.zeros(Kp, 5, 5)
    wantt[:C] = p["w"].view(C, 5, 5)
    wantt = wantt.view(Kp // 2, 2, 5, 5)
    for ch in (0, 1):
        assert torch.equal(taps_b[:, ch, :, :5, ch].float(), wantt[:, ch].bfloat16().float())
        assert float(taps_b[:, ch, :, :, 1 - ch].abs().max()) == 0.0 and float(taps_b[:, ch, :, 5:].abs().max()) == 0.0


# ---- 11. the stack ------------------------------------------------------------------------------------------------------------------
def _refiner(feat, disp, r, seed=5):
    from gfnet_amd.model.network import _refiner_for

    torch.manual_seed(seed)
    ref = _refiner_for(feat, disp, r).to(DEV).eval()
    ref.amp = False
    with torch.no_grad():
        for m in ref.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.2)
                m.running_var.uniform_(0.5, 1.5)
                m.weight.uniform_(0.5, 1.5)
                m.bias.normal_(0, 0.2)
    return ref


def _modules(ref, d, dtype=None):
    """out_conv(hidden_blocks(block1(d))) by torch: fp32, or under torch's own autocast to dtype"""
    with torch.no_grad():
        if dtype is None:
            return ref.out_conv(ref.hidden_blocks(ref.block1(d.clone())))
        with torch.autocast("cuda", dtype=dtype):
            h = ref.hidden_blocks(ref.block1(d.clone()))
        return ref.out_conv(h.float())


def _maxerr(a, b):
    return float((a.double() - b.double()).abs().max())


def _stack(ref, d, precision):
    ref.conv_precision = precision
    with torch.no_grad():
        return ref.conv_stack(d)


@pytest.mark.parametrize("feat,disp,r,G,B", [(8, 8, 0, 64, 3), (16, 16, 2, 32, 2), (32, 32, 4, 16, 2), (64, 64, 7, 8, 1), (64, 64, 6, 40, 1)])
def test_conv_stack_bf16_matches_torch_modules(feat, disp, r, G, B):
    """The configurations of test_conv_stack_gpu.test_conv_stack_matches_torch_modules in the bf16 class: as close to the fp32 modules
    as torch's own bf16 autocast of them, with that test's criterion and margin for "amp"; and switching the class on one refiner
    hands each class its own packed blocks."""
    ref = _refiner(feat, disp, r)
    C = ref.block1[0].in_channels
    d = torch.randn(B, C, G, G, generator=torch.Generator().manual_seed(21)).to(DEV)
    want, want_bf16 = _modules(ref, d), _modules(ref, d, torch.bfloat16)
    amp0 = _stack(ref, d, "amp")
    got = _stack(ref, d, "bf16")
    amp1 = _stack(ref, d, "amp")
    got1 = _stack(ref, d, "bf16")
    assert got.dtype == torch.float32 and got.shape == want.shape and torch.isfinite(got).all()
    err, err_torch = _maxerr(got, want), _maxerr(want_bf16, want)
    print(f"C={C} G={G}: bf16 stack err {err:.3e}, torch bf16 autocast err {err_torch:.3e}, amp err {_maxerr(amp0, want):.3e}, "
          f"max|want| {float(want.abs().max()):.3e}")
    assert err <= 2.0 * err_torch + 1e-6, (err, err_torch)
    assert torch.equal(amp0, amp1) and torch.equal(got, got1), "a class was handed the other one's packed blocks"
    assert not torch.equal(got, amp0)


def test_conv_stack_bf16_is_finite_past_the_fp16_range():
    """One channel of one inter-block map scaled past 65504 (the 1x1 row that writes it times s, the depthwise taps that read it
    divided by s: in exact arithmetic the same network): every other value between the blocks stays inside fp16's range, the fp32
    modules are finite, and so is the bf16 class."""
    ref = _refiner(8, 8, 0, seed=9)
    C, G = ref.block1[0].in_channels, 16
    d = torch.randn(2, C, G, G, generator=torch.Generator().manual_seed(22)).to(DEV)
    blocks = [ref.block1] + list(ref.hidden_blocks)
    at, ch = 3, 5

    def maps():
        out, h = [], d
        with torch.no_grad():
            for blk in blocks:
                h = blk(h)
                out.append(h)
        return out

    s = 4e5 / float(maps()[at][:, ch].abs().max())
    with torch.no_grad():
        blocks[at][3].weight[ch] *= s
        blocks[at][3].bias[ch] *= s
        blocks[at + 1][0].weight[ch] /= s
    ms = maps()
    assert len(ms) == 9
    for i, m in enumerate(ms):
        mask = torch.ones(C, dtype=torch.bool, device=DEV)
        if i == at:
            mask[ch] = False
            assert 1e5 < float(m[:, ch].abs().max()) < 1e6
        assert float(m[:, mask].abs().max()) < 65504 / 16, i
    want = _modules(ref, d)
    assert torch.isfinite(want).all()
    got = _stack(ref, d, "bf16")
    assert got.dtype == torch.float32 and torch.isfinite(got).all()
    err, err_torch = _maxerr(got, want), _maxerr(_modules(ref, d, torch.bfloat16), want)
    print(f"err {err:.3e}, torch bf16 autocast err {err_torch:.3e}")
    assert err <= 2.0 * err_torch + 1e-6, (err, err_torch)


def _g4(precision):
    from conftest import load_golden
    from test_network_gpu import _toy_refiner, dev

    g = load_golden("g4_refiner_prefix")
    sd = {k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd.")}
    ref = _toy_refiner(8, 6, int(g["r"]), int(g["hidden_blocks"]), sd)
    if precision == "torch_bf16":  # the modules under torch's own bf16 autocast
        ref.conv_impl, ref.amp, ref.amp_dtype = "torch", True, torch.bfloat16
    else:
        ref.conv_precision = precision
    with torch.no_grad():
        dflow, dcert, lc = ref(int(g["G"]), dev(g["x"]), dev(g["y"]), dev(g["flow"]), scale_factor=float(g["scale_factor"]))
    return g, dflow, dcert, lc


def test_g4_refiner_forward_in_the_bf16_class():
    """The reference's golden G4 (made in fp32 on the CPU) through conv_precision = "bf16": the correlation stays fp32; flow and
    certainty are as close to the golden as torch's bf16 autocast of the same modules is, with the stack test's margin."""
    from conftest import assert_close

    g, dflow, dcert, lc = _g4("bf16")
    _, tflow, tcert, _ = _g4("torch_bf16")
    assert_close(lc.cpu().numpy(), g["local_corr"], 1e-4, "local_corr")
    assert dflow.dtype == torch.float32 and dcert.dtype == torch.float32
    for name, got, via_torch, want in (("delta_flow", dflow, tflow, g["delta_flow"]), ("delta_cert", dcert, tcert, g["delta_cert"])):
        want = torch.from_numpy(want).to(DEV)
        err, err_torch = _maxerr(got, want), _maxerr(via_torch, want)
        print(f"{name}: err {err:.3e}, torch bf16 autocast err {err_torch:.3e}")
        assert tuple(got.shape) == tuple(want.shape) and err <= 2.0 * err_torch + 1e-6, (name, err, err_torch)


def test_grid_10_takes_the_torch_bf16_autocast_path():
    """G % 4 != 0: no fp16 kernel stands in for the missing bf16 one; the modules run under torch's bf16 autocast."""
    ref = _refiner(8, 6, 2, seed=11)
    C = ref.block1[0].in_channels
    d = torch.randn(2, C, 10, 10, generator=torch.Generator().manual_seed(23)).to(DEV)
    got = _stack(ref, d, "bf16")
    assert got.dtype == torch.float32 and torch.equal(got, _modules(ref, d, torch.bfloat16))
    assert not torch.equal(got, _stack(ref, d, "amp"))
    ref.conv_precision = "bf17"
    with pytest.raises(ValueError, match="'bf16'"):
        ref.conv_stack(d)
