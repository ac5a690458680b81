"""The bf16 inference conv block (csrc/conv_stack_bf16.hip: csrc/conv_block_fused.h on the 16-bit element __bf16) without a GPU, and
what tests/test_conv_block_bf16_gpu.py shares with this file: the class table, the two exact-integer input sets that fit bf16, the
float64 reference on the operands the class rounds, and the per-element bound.

The bf16 entry (GFN_CBR_ENTRY_BF16) must route, field for field, as the fp16-map entry does: the two classes share tile shapes on
purpose, so the GPU cases are the fp16-map cases of tests/test_conv_block_routes_gpu.py run in the corresponding bf16 class.

Exact data.  bf16 holds the integers up to 256 (8 significant bits).  The ReLU outputs of test_conv_block_routes_cpu.exact_inputs
(integers <= 114) fit, its half-map outputs (<= 1942) do not, so a case whose output is a bf16 map runs two complementary sets:
  (i)  dense taps   exact_inputs' x, taps and BatchNorm; every 1x1 row has at most 2 non-zero +-1 weights and a bias in [-4, 4]:
                    |out| <= 2 * 114 + 4 = 232.  The non-zeros are placed by a covering rule, so no channel (2M >= C) or at least
                    no 16-channel K tile (2M < C) is left out of every row.
  (ii) wide rows    x in {-1, 0, 1}, at most 3 non-zero +-1 taps per channel, conv bias in [-1, 1], alpha in {+-1, +-2}, beta in
                    [-2, 2]: ReLU outputs <= (3 + 1) * 2 + 2 = 10; up to 17 non-zero +-1 weights per row: |out| <= 174.
A case with fp32 output runs exact_inputs as it is (|out| < 2^24).
"""
import functools

import numpy as np
import torch

from gfnet_amd import _lib, ops
from test_conv_block_routes_cpu import (COL, FAMILIES, NF, SWEEP_C, SWEEP_G, SWEEP_M, exact_inputs, float_inputs, route_key, stage_pw,
                                        stage_t, sweep)
import test_conv_block_routes_cpu as half_cpu

# class name -> arguments of ops.conv_block_route / what ops.conv_block_bf16 is given; the fp16-map class each one is the twin of
CLASSES = {"map_fb": dict(x_bf16=False, out_bf16=True), "map_bb": dict(x_bf16=True, out_bf16=True),
           "map_bf": dict(x_bf16=True, out_bf16=False)}
TWIN = {"map_fh": "map_fb", "map_hh": "map_bb", "map_hf": "map_bf"}
ENTRIES = [(_lib.CBR_ENTRY_BF16, _lib.GFN_F32, _lib.GFN_BF16), (_lib.CBR_ENTRY_BF16, _lib.GFN_BF16, _lib.GFN_BF16),
           (_lib.CBR_ENTRY_BF16, _lib.GFN_BF16, _lib.GFN_F32)]
HALF_ENTRIES = [(_lib.CBR_ENTRY_HALF, _lib.GFN_F32, _lib.GFN_F16), (_lib.CBR_ENTRY_HALF, _lib.GFN_F16, _lib.GFN_F16),
                (_lib.CBR_ENTRY_HALF, _lib.GFN_F16, _lib.GFN_F32)]
BF16_FAMILIES = FAMILIES + ("beyond_fp16",)
U16 = 2.0 ** -8  # unit roundoff of bf16 (8 significant bits, to nearest even)


def route(cls, B, C, M, G):
    return ops.conv_block_route(B, C, M, G, **CLASSES[cls])


def bf16_out(cls):
    return CLASSES[cls]["out_bf16"]


def twin_cases(cases):
    """The rows of a case table of the fp16 file whose class is a half-map class, in the corresponding bf16 class."""
    return [(TWIN[c[0]],) + tuple(c[1:]) for c in cases if c[0] in TWIN]


def is_bf16_exact(v):
    return torch.equal(v.float().bfloat16().float().double(), v.double())


# ---- 1. the route ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sweep_bf16(B, Cs):
    """(shape (n, 4) = entry index, C, M, G; filled; routes (n, NF)) of the three dtype pairs of the bf16 entry, in sweep()'s order."""
    fn = _lib.lib().gfn_conv_block_route
    e, c, g, m = np.meshgrid(np.arange(len(ENTRIES)), Cs, SWEEP_G, SWEEP_M, indexing="ij")
    shape = np.stack([e.ravel(), c.ravel(), m.ravel(), g.ravel()], 1).astype(np.int64)
    routes = np.zeros((len(shape), NF), np.int32)
    ptrs = (routes.ctypes.data + 4 * NF * np.arange(len(shape), dtype=np.int64)).tolist()
    ok = [fn(*ENTRIES[ei], B, ci, mi, gi, p, NF) for (ei, ci, mi, gi), p in zip(shape.tolist(), ptrs)]
    return shape, np.array(ok) == NF, routes


def test_route_equals_the_half_entrys():
    assert half_cpu.ENTRIES[4:] == HALF_ENTRIES
    for B in (1, 16385):
        shape, ok, routes = sweep_bf16(B, (17,))
        hshape, hok, hroutes = sweep(B, (17,))
        rows = hshape[:, 0] >= 4                      # the half entry's three dtype pairs, in the same order
        assert np.array_equal(hshape[rows][:, 1:], shape[:, 1:]) and np.array_equal(hshape[rows][:, 0] - 4, shape[:, 0])
        assert np.array_equal(ok, hok[rows]) and np.array_equal(~ok, shape[:, 3] % 4 != 0)
        assert np.array_equal(routes, hroutes[rows]), "the bf16 entry routes differently from the fp16-map entry"
        assert ok.sum() == 3 * len(SWEEP_M) * sum(g % 4 == 0 for g in SWEEP_G) and (routes[ok][:, COL["F16"]] == 1).all() and (routes[ok][:, COL["MM"]] == 1).all()
    # through ops: the same dict
    for cls_h, cls_b in TWIN.items():
        for B, C, M, G in ((1, 17, 29, 4), (2, 3, 100, 32), (1, 417, 449, 8), (16385, 2, 3, 16)):
            assert route(cls_b, B, C, M, G) == half_cpu.route(cls_h, B, C, M, G) != None  # noqa: E711


def test_route_refuses_the_other_16_bit_type():
    L = _lib.lib()
    buf = (_lib.c_int * NF)()
    for a, b in ((_lib.GFN_F16, _lib.GFN_BF16), (_lib.GFN_BF16, _lib.GFN_F16), (_lib.GFN_F16, _lib.GFN_F16), (_lib.GFN_F16, _lib.GFN_F32)):
        assert L.gfn_conv_block_route(_lib.CBR_ENTRY_BF16, a, b, 1, 8, 8, 8, buf, NF) == 0
        msg = L.gfn_last_error()
        assert b"conv_block_bf16" in msg and b"GFN_BF16" in msg, msg
    for a, b in ((_lib.GFN_BF16, _lib.GFN_BF16), (_lib.GFN_F32, _lib.GFN_BF16), (_lib.GFN_BF16, _lib.GFN_F32)):
        assert L.gfn_conv_block_route(_lib.CBR_ENTRY_HALF, a, b, 1, 8, 8, 8, buf, NF) == 0
        assert L.gfn_conv_block_route(_lib.CBR_ENTRY_BF16, a, b, 1, 8, 8, 8, buf, NF) == NF
    assert L.gfn_conv_block_route(_lib.CBR_ENTRY_BF16, _lib.GFN_F32, _lib.GFN_F32, 1, 8, 8, 8, buf, NF) == 0
    assert route("map_bb", 1, 8, 8, 10) is None and b"multiple of 4" in L.gfn_last_error()
    assert route("map_bb", 1, 1 << 12, 8, 1 << 9) is None and route("map_bb", 0, 8, 8, 8)["nwork"] == 0
    assert _lib.CBR_ENTRY_BF16 == 2 and _lib.CBR_FIELDS == len(ops.CONV_ROUTE_FIELDS)


def test_gpu_cases_reach_every_instantiation_of_the_bf16_entry():
    import test_conv_block_bf16_gpu as gpu

    shape, ok, routes = sweep_bf16(1, SWEEP_C)
    want = half_cpu.keys_of(routes[ok])
    assert 100 <= len(want) <= 300, len(want)
    got = set()
    for cls, B, C, M, G in gpu.EXACT_CASES:
        r = route(cls, B, C, M, G)
        assert r is not None and r["tpb"] == 1 and r["fused"] == 1, (cls, B, C, M, G)
        got.add(route_key(r))
    assert got == want, (sorted(want - got)[:5], sorted(got - want)[:5])
    tp = [(c, route(*c)) for c in gpu.TPB_CASES]
    assert len(tp) == 4 and {c[0] for c, _ in tp} == set(CLASSES)
    for c, r in tp:
        assert r["tpb"] == 2 and r["nwork"] >= 16384 and route_key(dict(r, tpb=1)) in want, c
    assert any(r["KW"] == 2 for _, r in tp) and any(r["NB"] == 2 for _, r in tp)
    assert {route(*c)["TW"] for c in gpu.WRITE_CASES} == {8, 16, 32} and {c[0] for c in gpu.WRITE_CASES} == set(CLASSES)


# ---- 2. exact data ---------------------------------------------------------------------------------------------------------------
def covering_weights(C, M, g):
    """(M, C) of 0 / +-1 with at most 2 non-zeros per row, placed slot by slot (slot s = 2m, 2m+1 of row m): where 2M >= C slot s
    takes channel s % C, so every channel is met; otherwise it takes K tile s % nkt and walks through that tile's channels, so every
    16-channel K tile is met (and, C permitting, many of its channels)."""
    pw = torch.zeros(M, C)
    nkt = (C + 15) // 16
    sign = torch.randint(0, 2, (2 * M,), generator=g).float() * 2 - 1
    for s in range(2 * M):
        if 2 * M >= C:
            k = s % C
        else:
            kt = s % nkt
            k = 16 * kt + (s // nkt) % min(16, C - 16 * kt)
        pw[s // 2, k] = sign[s]
    return pw


def exact_inputs_bf16(B, C, M, G, out_is_bf16, seed, which):
    """(x, p) of set `which` = "dense" (i) or "wide" (ii) of the module docstring; out_is_bf16 False: exact_inputs as it is."""
    if not out_is_bf16:
        return exact_inputs(B, C, M, G, False, seed)
    if which == "dense":
        x, p = exact_inputs(B, C, M, G, True, seed)
        p = dict(p, pw=covering_weights(C, M, torch.Generator().manual_seed(seed + 7919)))
        return x, p
    g = torch.Generator().manual_seed(seed + 104729)

    def ri(lo, hi, *shape):
        return torch.randint(lo, hi + 1, shape, generator=g).float()

    x = ri(-1, 1, B, C, G, G)
    taps = ri(0, 1, C, 25) * 2 - 1
    taps = taps * (torch.rand(C, 25, generator=g).argsort(1).argsort(1) < 3)
    p = dict(w=taps, cb=ri(-1, 1, C) if seed % 2 else None, alpha=torch.tensor([1.0, 2.0, -1.0, -2.0])[torch.randint(0, 4, (C,), generator=g)],
             beta=ri(-2, 2, C), pb=ri(-4, 4, M))
    keep = torch.rand(M, C, generator=g).argsort(1).argsort(1) < min(C, 17)
    p["pw"] = (ri(0, 1, M, C) * 2 - 1) * keep
    return x, p


def exact_reference_bf16(x, p, out_is_bf16, which):
    """float64 result of exact data, the preconditions asserted from float64 alone."""
    C, M = x.shape[1], p["pw"].shape[0]
    t64 = stage_t(x, p, torch.float64)
    ref = stage_pw(t64, p["pw"], p["pb"], torch.float64)
    assert torch.equal(t64, t64.round()) and torch.equal(ref, ref.round())
    for name, v in (("x", x), ("taps", p["w"]), ("relu output", t64)):  # what the class rounds to bf16 on the way
        assert is_bf16_exact(v), name
    nz = (p["pw"] != 0).sum(1)
    if not out_is_bf16:
        assert float(t64.max()) <= 114 and float(ref.abs().max()) <= 2 ** 24 - 1
        return ref
    assert is_bf16_exact(ref) and float(p["pw"].abs().max()) <= 1 and float(p["pb"].abs().max()) <= 4
    if which == "dense":
        assert float(t64.max()) <= 114 and int(nz.max()) <= 2 and float(ref.abs().max()) <= 232
        met = (p["pw"] != 0).any(0)
        if 2 * M >= C:
            assert bool(met.all()), "a channel that no row of the 1x1 weights reads"
        else:
            tiles = torch.nn.functional.pad(met, (0, -C % 16)).view(-1, 16).any(1)
            assert bool(tiles.all()), "a K tile that no row of the 1x1 weights reads"
    else:
        assert float(x.abs().max()) <= 1 and int((p["w"] != 0).sum(1).max()) <= 3 and float(p["beta"].abs().max()) <= 2
        assert float(t64.max()) <= 10 and int(nz.max()) <= 17 and float(ref.abs().max()) <= 174
        assert int(nz.min()) == min(C, 17)
    return ref


def sets_of(cls):
    return ("dense", "wide") if bf16_out(cls) else ("as_is",)


def test_exact_data_preconditions_of_every_case():
    import test_conv_block_bf16_gpu as gpu

    n_dense = 0
    for seed, (cls, B, C, M, G) in gpu.EXACT + list(enumerate(gpu.WRITE_CASES, len(gpu.EXACT))):
        for which in sets_of(cls):
            x, p = exact_inputs_bf16(B, C, M, G, bf16_out(cls), seed, which)
            exact_reference_bf16(x, p, bf16_out(cls), which)
            n_dense += which == "dense" and 2 * M < C
    assert n_dense >= 2  # the K-tile branch of the covering rule is met (C = 417 into M = 100, 129)
    for cls, B, C, M, G in gpu.TPB_CASES:
        for which in sets_of(cls):
            x, p = exact_inputs_bf16(gpu.TPB_PERIOD, C, M, G, bf16_out(cls), 5, which)
            exact_reference_bf16(x, p, bf16_out(cls), which)


# ---- 3. float families -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def float_inputs_bf16(B, C, M, G, family):
    """float_inputs of the fp16-map class; beyond_fp16: its "large" family with x, the conv bias and beta times 64 -- the pre-activation
    and so the ReLU output scale by exactly 64 (a power of two commutes with every rounding), past anything fp16 can hold."""
    if family != "beyond_fp16":
        return float_inputs(B, C, M, G, family, "map16")
    x, p = float_inputs(B, C, M, G, "large", "map16")
    return x * 64.0, dict(p, cb=None if p["cb"] is None else p["cb"] * 64.0, beta=p["beta"] * 64.0)


def rounded_operands_bf16(x, p):
    """x and the parameters as float32 tensors holding what the bf16 class feeds its products: x, the taps and the 1x1 weights rounded."""
    return x.bfloat16().float(), dict(p, w=p["w"].bfloat16().float(), pw=p["pw"].bfloat16().float())


def reference_bf16(x, p, out_is_bf16):
    """(ref float64 (B, M, G, G), bound per element, t64): test_conv_block_routes_cpu.reference for the map16 class with bf16's unit
    roundoff 2^-8 where it has fp16's 2^-11 and .bfloat16() where it has .half()."""
    xr, q = rounded_operands_bf16(x, p)
    t64 = stage_t(xr, q, torch.float64)
    ref = stage_pw(t64, q["pw"], q["pb"], torch.float64)
    rmax = float(ref.abs().max())
    e_t = float((stage_t(xr, q, torch.float32).double() - t64).abs().max())
    t16 = t64.float().bfloat16()
    e_pw = float((stage_pw(t16, q["pw"], q["pb"], torch.float32).double() - stage_pw(t16, q["pw"], q["pb"], torch.float64)).abs().max())
    bound = torch.einsum("mk,bkij->bmij", q["pw"].double().abs(), U16 * t64.abs() + 4 * e_t) + max(4 * e_pw, 2.0 ** -20 * rmax)
    if out_is_bf16:
        bound = bound + U16 * ref.abs()
    return ref, bound, t64


def float_preconditions_bf16(x, p, out_is_bf16, family):
    """What a family promises, from float64 alone; returns (ref, bound)."""
    ref, bound, t64 = reference_bf16(x, p, out_is_bf16)
    assert torch.isfinite(ref).all() and torch.isfinite(t64).all() and torch.isfinite(bound).all() and float(bound.min()) > 0
    assert torch.isfinite(x.bfloat16().float()).all()
    xr, q = rounded_operands_bf16(x, p)
    if family == "neg_alpha":
        assert int((p["alpha"] < 0).sum()) == (x.shape[1] + 1) // 2
    elif family == "dead":
        assert float((t64 == 0).double().mean()) >= 0.9
    elif family == "cancel":
        gross = torch.einsum("mk,bkij->bmij", q["pw"].double().abs(), t64.abs())
        assert float(ref.abs().max()) < 0.05 * float(gross.max()), (float(ref.abs().max()), float(gross.max()))
    elif family == "large":
        assert 1e3 <= float(t64.max()) <= 3e4
    elif family == "border":
        G = x.shape[-1]
        assert G == 4 or float(x[..., 2:G - 2, 2:G - 2].abs().max()) < 0.1
        assert float(x[..., 0, :].abs().mean()) > 10
    elif family == "beyond_fp16":  # nothing of this fits an fp16 map: the ReLU output and the result pass 65504
        assert float(t64.max()) >= 1e5 and float(ref.abs().max()) > 65504, (float(t64.max()), float(ref.abs().max()))
        xl, pl = float_inputs_bf16(x.shape[0], x.shape[1], p["pw"].shape[0], x.shape[-1], "large")
        assert torch.equal(stage_t(*rounded_operands_bf16(xl, pl), torch.float64) * 64.0, t64)  # scaled by exactly 64
    return ref, bound


def test_float_family_preconditions_of_every_route():
    import test_conv_block_bf16_gpu as gpu

    assert len(gpu.FLOAT_ROUTES) == 17 and {c[0] for c in gpu.FLOAT_ROUTES} == set(CLASSES)
    assert len({route_key(route(*c)) for c in gpu.FLOAT_ROUTES}) >= 15
    for cls, B, C, M, G in gpu.FLOAT_ROUTES:
        for family in BF16_FAMILIES:
            x, p = float_inputs_bf16(B, C, M, G, family)
            float_preconditions_bf16(x, p, bf16_out(cls), family)


# ---- 4. the layout -----------------------------------------------------------------------------------------------------------------
def to_bf16_map(x):
    """(B, C, G, G) -> the bf16 map layout (B, ceil(C/2), G, G, 2) bfloat16 (the half map's), the odd channel past C zero."""
    B, C, G, _ = x.shape
    xp = torch.zeros(B, 2 * ((C + 1) // 2), G, G, device=x.device, dtype=torch.bfloat16)
    xp[:, :C] = x.bfloat16()
    return xp.reshape(B, (C + 1) // 2, 2, G, G).permute(0, 1, 3, 4, 2).contiguous()


def test_bf16_map_layout_round_trip():
    g = torch.Generator().manual_seed(3)
    for B, C, G in ((2, 5, 4), (1, 8, 12), (3, 1, 8)):
        x = torch.randn(B, C, G, G, generator=g) * 1e5  # past fp16's range
        m = to_bf16_map(x)
        assert m.dtype == torch.bfloat16 and tuple(m.shape) == (B, (C + 1) // 2, G, G, 2) and m.is_contiguous()
        assert torch.equal(ops.bf16_map_to_float(m, C), x.bfloat16().float())
        assert torch.equal(m[:, 1 if C > 2 else 0, :, :, 0].float(), x[:, 2 if C > 2 else 0].bfloat16().float())  # channel 2p in slot 0
        if C % 2:
            assert float(m[:, -1, :, :, 1].abs().max()) == 0.0
            assert tuple(ops.bf16_map_to_float(m, C + 1).shape) == (B, C + 1, G, G)
