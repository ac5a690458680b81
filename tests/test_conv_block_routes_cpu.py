"""The inference conv block's launch decision (csrc/conv_block_fused.h conv_route, exported as gfn_conv_block_route) without a GPU,
and what tests/test_conv_block_routes_gpu.py shares with this file: the arithmetic classes, the exact-integer and the float input
families, the float64 references on the operands each class rounds, and the per-element bounds.

The sweep asks the route of every shape (C, M, G) below for both entry points, every variant and every dtype pair, at B = 1 -- the
instantiation does not depend on B; B only decides `tpb` (two work items per workgroup from 16384 items on), which the sweep
checks on its own at B = 16385 (nothing but nwork and tpb moves).  The set of distinct instantiations (route_key) is what the GPU
file's case table has to reach, exactly; its tpb = 2 cases are a table of their own (TPB_CASES) whose instantiations must belong
to the set.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from gfnet_amd import _lib, ops

# class name -> (arguments of ops.conv_block_route, arithmetic class)
#   f32    fp32 throughout                                 reference: float64 of the definition on the fp32 inputs
#   op16   fp16 1x1 operands (W and the ReLU output)       reference rounds W
#   map16  fp16 maps: x, depthwise taps and W are rounded  reference rounds x, taps and W; a half-map output is rounded once more
CLASSES = {
    "f32": (dict(variant=0), "f32"), "f32_2p": (dict(variant=1), "f32"),
    "op16": (dict(variant=2), "op16"), "op16_2p": (dict(variant=3), "op16"),
    "map_fh": (dict(x_half=False, out_half=True), "map16"), "map_hh": (dict(x_half=True, out_half=True), "map16"),
    "map_hf": (dict(x_half=True, out_half=False), "map16"),
}
KEY_FIELDS = ("fused", "TW", "MT", "NS", "NB", "KW", "F16", "HIN", "HOUT", "MM", "VEC", "mt", "tpb")


def route(cls, B, C, M, G):
    return ops.conv_block_route(B, C, M, G, **CLASSES[cls][0])


def route_key(r):
    """An instantiation: the route without nwork, ngrp and the tile counts, plus tpb and `more than one slab group / row block`."""
    return tuple(r[f] for f in KEY_FIELDS) + (int(r["ngrp"] > 1 or r["nblk"] > 1),)


def half_out(cls):
    return CLASSES[cls][0].get("out_half", False)


# ---- the sweep -------------------------------------------------------------------------------------------------------------------
SWEEP_C = (1, 3, 15, 16, 17, 33, 417)
SWEEP_M = tuple(range(1, 513))
SWEEP_G = tuple(range(4, 201, 4)) + (1, 5, 10, 30, 67, 161)
ENTRIES = [(_lib.CBR_ENTRY_FWD, v, 0) for v in range(4)] + [(_lib.CBR_ENTRY_HALF, _lib.GFN_F32, _lib.GFN_F16),
                                                             (_lib.CBR_ENTRY_HALF, _lib.GFN_F16, _lib.GFN_F16),
                                                             (_lib.CBR_ENTRY_HALF, _lib.GFN_F16, _lib.GFN_F32)]
NF = _lib.CBR_FIELDS
COL = {f: (_lib.CBR_GEMM_MT if f == "mt" else getattr(_lib, "CBR_" + f.upper())) for f in ops.CONV_ROUTE_FIELDS}


@functools.lru_cache(maxsize=None)
def sweep(B, Cs=SWEEP_C):
    """(shape (n, 4) = entry index, C, M, G; filled (n,) bool; routes (n, NF)) of every shape of the sweep."""
    fn = _lib.lib().gfn_conv_block_route
    e, c, g, m = np.meshgrid(np.arange(len(ENTRIES)), Cs, SWEEP_G, SWEEP_M, indexing="ij")
    shape = np.stack([e.ravel(), c.ravel(), m.ravel(), g.ravel()], 1).astype(np.int64)
    routes = np.zeros((len(shape), NF), np.int32)
    ptrs = (routes.ctypes.data + 4 * NF * np.arange(len(shape), dtype=np.int64)).tolist()
    ok = [fn(*ENTRIES[ei], B, ci, mi, gi, p, NF) for (ei, ci, mi, gi), p in zip(shape.tolist(), ptrs)]
    return shape, np.array(ok) == NF, routes


def keys_of(routes):
    r = {f: routes[:, COL[f]] for f in ops.CONV_ROUTE_FIELDS}
    k = np.stack([r[f] for f in KEY_FIELDS] + [((r["ngrp"] > 1) | (r["nblk"] > 1)).astype(np.int32)], 1)
    return {tuple(int(v) for v in row) for row in np.unique(k, axis=0)}


@functools.lru_cache(maxsize=None)
def reachable():
    shape, ok, routes = sweep(1)
    return keys_of(routes[ok])


def parent_dispatch(entry, a, b, B, M, G):
    """The launch decision as the launchers stated it before conv_route existed (gfn_conv_block_fwd, launch_half, launch_fused,
    launch_fused_mt), restated branch by branch: (fused, TW, MT, NS, NB, KW, F16, HIN, HOUT, MM, ngrp, nwork, tpb, VEC, nblk, mt)."""
    tiles = (M + 31) // 32
    if entry == _lib.CBR_ENTRY_FWD:
        f16, hin, hout, mm, kw = (a & 2) != 0, False, False, False, 1
        if (a & 1) or G % 4:
            nblk = (tiles + 6) // 7
            return (0, 0, 0, 0, 0, 0, int(f16), 0, 0, 0, 0, 0, 0, 4 if G % 4 == 0 else 1, nblk, (tiles + nblk - 1) // nblk)
    else:
        f16, hin, hout, mm = True, a == _lib.GFN_F16, b == _lib.GFN_F16, True
        kw = 2 if hin and hout and M > 96 else 1
    TW = 32 if (G % 32 == 0 or G > 160) else 16 if (G % 16 == 0 or G > 64) else 8
    if f16 and tiles <= 3 and TW >= 16 and G % (256 // TW) == 0:
        MT, NS, NB, kw = tiles, 1, 2, 1
    elif tiles <= 7:
        MT, NS, NB = tiles, 1, 1
        kw = kw if tiles >= 4 else 1
    else:
        grp = (tiles + 13) // 14
        mt = ((tiles + grp - 1) // grp + 1) // 2
        MT, NS, NB = (mt if 4 <= mt <= 6 else 7), 2, 1
    TH = 128 * NB // TW
    tx, ty = (G + TW - 1) // TW, (G + TH - 1) // TH
    ngrp = (M + 32 * MT * NS - 1) // (32 * MT * NS)
    nwork = B * tx * ty * ngrp
    return (1, TW, MT, NS, NB, kw, int(f16), int(hin), int(hout), int(mm), ngrp, nwork, 2 if nwork >= 16384 else 1, 0, 0, 0)


def test_route_equals_the_launchers_former_decision():
    order = ("fused", "TW", "MT", "NS", "NB", "KW", "F16", "HIN", "HOUT", "MM", "ngrp", "nwork", "tpb", "VEC", "nblk", "mt")
    cols = [COL[f] for f in order]
    for B in (1, 16385):
        shape, ok, routes = sweep(B, (17,))
        got = routes[:, cols].tolist()
        for (ei, C, M, G), filled, row in zip(shape.tolist(), ok.tolist(), got):
            entry, a, b = ENTRIES[ei]
            if not filled:
                assert entry == _lib.CBR_ENTRY_HALF and G % 4, (entry, a, b, M, G)
                continue
            assert tuple(row) == parent_dispatch(entry, a, b, B, M, G), (entry, a, b, B, M, G)


def test_shape_invariants_over_the_sweep():
    shape, ok, routes = sweep(1)
    ei, C, M, G = shape.T
    half = np.array([e[0] == _lib.CBR_ENTRY_HALF for e in ENTRIES])[ei]
    variant = np.array([e[1] for e in ENTRIES])[ei]
    assert np.array_equal(~ok, half & (G % 4 != 0))          # refused: the fp16-map entry on a grid side that is no multiple of 4
    r = {f: routes[:, COL[f]].astype(np.int64) for f in ops.CONV_ROUTE_FIELDS}
    fused = ok & (r["fused"] == 1)
    assert np.array_equal(fused, ok & (half | ((variant & 1) == 0) & (G % 4 == 0)))
    f = {k: v[fused] for k, v in r.items()}
    Mf, Gf = M[fused], G[fused]
    TH = 128 * f["NB"] // f["TW"]
    assert np.isin(f["TW"], (8, 16, 32)).all() and (f["MT"] >= 1).all() and (f["MT"] <= 7).all() and np.isin(f["NS"], (1, 2)).all()
    assert (f["tiles_x"] * f["TW"] >= Gf).all() and ((f["tiles_x"] - 1) * f["TW"] < Gf).all()
    assert (f["tiles_y"] * TH >= Gf).all() and ((f["tiles_y"] - 1) * TH < Gf).all()
    slab = f["MT"] * f["NS"] * 32
    assert (slab * f["ngrp"] >= Mf).all() and (slab * (f["ngrp"] - 1) < Mf).all()
    assert (f["MT"][f["NS"] == 2] >= 4).all()
    nb2 = f["NB"] == 2
    assert np.isin(f["NB"], (1, 2)).all() and (Gf[nb2] % (256 // f["TW"][nb2]) == 0).all()
    assert (f["F16"][nb2] == 1).all() and (f["TW"][nb2] >= 16).all() and (f["MT"][nb2] <= 3).all() and (f["NS"][nb2] == 1).all()
    assert np.array_equal(f["KW"] == 2, (f["HIN"] == 1) & (f["HOUT"] == 1) & (Mf > 96)) and np.isin(f["KW"], (1, 2)).all()
    assert np.array_equal(f["MM"] == 1, half[fused]) and (f["F16"][half[fused]] == 1).all()
    assert np.array_equal(f["nwork"], f["tiles_x"] * f["tiles_y"] * f["ngrp"]) and (f["tpb"] == 1).all()
    assert (f["VEC"] == 0).all() and (f["nblk"] == 0).all() and (f["mt"] == 0).all()
    two = ok & ~fused
    t = {k: v[two] for k, v in r.items()}
    assert np.array_equal(t["VEC"] == 4, G[two] % 4 == 0) and np.isin(t["VEC"], (1, 4)).all()
    assert (t["nblk"] * t["mt"] * 32 >= M[two]).all() and (t["mt"] >= 1).all() and (t["mt"] <= 7).all()
    assert ((t["nblk"] - 1) * t["mt"] * 32 < M[two]).all()
    assert np.array_equal(t["F16"], (variant[two] >> 1) & 1)
    for name in ("TW", "MT", "NS", "NB", "KW", "ngrp", "nwork", "tpb", "tiles_x", "tiles_y", "HIN", "HOUT", "MM"):
        assert (t[name] == 0).all(), name
    # B = 16385: every fused launch walks two items per workgroup, and nothing else of the route moves
    shape2, ok2, routes2 = sweep(16385, (17,))
    c17 = C == 17
    assert np.array_equal(shape[c17], shape2) and np.array_equal(ok[c17], ok2)
    same = [COL[n] for n in ops.CONV_ROUTE_FIELDS if n not in ("nwork", "tpb")]
    assert np.array_equal(routes[c17][:, same], routes2[:, same])
    f17 = fused[c17]
    assert np.array_equal(routes2[f17, COL["nwork"]], 16385 * routes[c17][f17, COL["nwork"]]) and (routes2[f17, COL["tpb"]] == 2).all()


def test_route_refuses_what_the_entry_points_refuse():
    assert route("f32", 1, 8, 8, 8) is not None and route("f32", 0, 8, 8, 8)["nwork"] == 0
    assert ops.conv_block_route(1, 8, 8, 8, variant=4) is None and b"variant" in _lib.lib().gfn_last_error()
    assert route("map_hh", 1, 8, 8, 10) is None and route("f32", 1, 0, 8, 8) is None and route("f32", 1, 8, 0, 8) is None
    assert route("f32", 1, 1 << 12, 8, 1 << 9) is None       # a map of 2^30 floats
    assert route("f32_2p", 65536, 1, 8, 8) is None and route("f32", 65536, 1, 8, 8) is not None
    L = _lib.lib()
    few = (_lib.c_int * 4)()
    assert L.gfn_conv_block_route(_lib.CBR_ENTRY_FWD, 0, 0, 1, 8, 8, 8, few, 4) == 0
    assert L.gfn_conv_block_route(7, 0, 0, 1, 8, 8, 8, (_lib.c_int * NF)(), NF) == 0
    assert L.gfn_conv_block_route(_lib.CBR_ENTRY_HALF, _lib.GFN_F32, _lib.GFN_F32, 1, 8, 8, 8, (_lib.c_int * NF)(), NF) == 0


def test_gpu_case_table_reaches_exactly_the_reachable_set():
    import test_conv_block_routes_gpu as gpu

    want = reachable()
    assert 200 <= len(want) <= 400, len(want)
    got = {}
    for case in gpu.CASES + gpu.EDGES:
        cls, B, C, M, G = case
        r = route(cls, B, C, M, G)
        assert r is not None and r["tpb"] == r["fused"], case  # one item per workgroup; the two-pass form has none
        got.setdefault(route_key(r), case)
    assert set(got) == want, (sorted(want - set(got))[:5], sorted(set(got) - want)[:5])
    assert {route_key(route(*c)) for c in gpu.CASES} == want  # the generated table alone: one case per instantiation
    assert len(gpu.CASES) == len(want)
    # the gaps the old table left, by name
    fused_keys = {k[:6] + (k[-1],) for k in got if k[0] == 1}
    for tw in (8, 16, 32):
        assert (1, tw, 7, 1, 1, 1, 0) in fused_keys and (1, tw, 4, 2, 1, 1, 0) in fused_keys and (1, tw, 5, 2, 1, 1, 0) in fused_keys
        assert (1, tw, 4, 2, 1, 1, 1) in fused_keys                                       # M > 448: two slab groups
    assert all((1, tw, mt, 1, 1, 1, 0) in fused_keys and (1, tw, mt, 1, 2, 1, 0) in fused_keys for tw in (16, 32) for mt in (1, 2))
    edges = [(c, route(*c)) for c in gpu.EDGES]
    assert any(r["fused"] and r["NS"] == 2 and ((c[3] + 31) // 32) % 2 == 1 for c, r in edges)        # odd tile count over two slabs
    assert any(r["TW"] == 32 and c[4] % 32 for c, r in edges) and any(r["TW"] == 16 and c[4] % 16 for c, r in edges)  # partial tiles
    assert any(r["KW"] == 2 and ((c[2] + 15) // 16) % 2 == 1 for c, r in edges)                       # a lone last K tile
    # section c: two items per workgroup
    tp = [(c, route(*c)) for c in gpu.TPB_CASES]
    for c, r in tp:
        assert r["tpb"] == 2 and route_key(dict(r, tpb=1)) in want, c
    assert any(r["nwork"] % 2 for _, r in tp) and {r["TW"] for _, r in tp} == {8, 16, 32}
    assert any(r["KW"] == 2 for _, r in tp) and any(r["ngrp"] == 2 for _, r in tp) and any(r["MM"] and r["NB"] == 2 for _, r in tp)


# ---- layouts ---------------------------------------------------------------------------------------------------------------------
def to_half_map(x):
    """(B, C, G, G) -> the half map layout (B, ceil(C/2), G, G, 2) float16, the odd channel past C zero."""
    B, C, G, _ = x.shape
    xp = torch.zeros(B, 2 * ((C + 1) // 2), G, G, device=x.device, dtype=torch.float16)
    xp[:, :C] = x.half()
    return xp.reshape(B, (C + 1) // 2, 2, G, G).permute(0, 1, 3, 4, 2).contiguous()


# ---- the definition --------------------------------------------------------------------------------------------------------------
def stage_t(x, p, dt):
    """relu((dw5x5(x) + conv bias) * alpha + beta) in dtype dt on the CPU."""
    C = x.shape[1]
    u = F.conv2d(x.to(dt), p["w"].to(dt).view(C, 1, 5, 5), None if p["cb"] is None else p["cb"].to(dt), padding=2, groups=C)
    return F.relu(u * p["alpha"].to(dt).view(1, C, 1, 1) + p["beta"].to(dt).view(1, C, 1, 1))


def stage_pw(t, pw, pb, dt):
    return F.conv2d(t.to(dt), pw.to(dt).view(pw.shape[0], pw.shape[1], 1, 1), pb.to(dt))


def rounded_operands(x, p, arith):
    """x and the parameters as float32 tensors holding what the class feeds its products: map16 rounds x and the taps to fp16, op16
    and map16 round the 1x1 weights."""
    q = dict(p)
    if arith == "map16":
        x, q["w"] = x.half().float(), p["w"].half().float()
    if arith in ("op16", "map16"):
        q["pw"] = p["pw"].half().float()
    return x, q


def reference(x, p, arith, out_is_half):
    """(ref float64 (B, M, G, G), bound per element or scalar, t64) for float inputs; the bounds of the module docstring of the GPU file."""
    xr, q = rounded_operands(x, p, arith)
    t64 = stage_t(xr, q, torch.float64)
    ref = stage_pw(t64, q["pw"], q["pb"], torch.float64)
    rmax = float(ref.abs().max())
    if arith == "f32":
        e32 = float((stage_pw(stage_t(xr, q, torch.float32), q["pw"], q["pb"], torch.float32).double() - ref).abs().max())
        return ref, torch.full_like(ref, max(4 * e32, 2.0 ** -20 * rmax)), t64
    e_t = float((stage_t(xr, q, torch.float32).double() - t64).abs().max())
    t16 = t64.float().half()
    e_pw = float((stage_pw(t16, q["pw"], q["pb"], torch.float32).double() - stage_pw(t16, q["pw"], q["pb"], torch.float64)).abs().max())
    absw = q["pw"].double().abs()
    bound = torch.einsum("mk,bkij->bmij", absw, 2.0 ** -11 * t64.abs() + 4 * e_t) + max(4 * e_pw, 2.0 ** -20 * rmax)
    if out_is_half:
        bound = bound + 2.0 ** -11 * ref.abs()
    return ref, bound, t64


# ---- exact data ------------------------------------------------------------------------------------------------------------------
def exact_inputs(B, C, M, G, out_is_half, seed):
    """Small integers all the way: every ReLU output is an integer of magnitude <= (25 * 2 + 3) * 2 + 8 = 114, exact in fp16 and
    fp32 (also through fp16 taps); a row of the 1x1 weights has at most 17 non-zeros where the output is a half map (|out| <= 17 *
    114 + 4 = 1942 <= 2048, the integers fp16 holds exactly) and any number otherwise (|out| <= 417 * 114 + 4 < 2^24)."""
    g = torch.Generator().manual_seed(seed)

    def ri(lo, hi, *shape):
        return torch.randint(lo, hi + 1, shape, generator=g).float()

    x = ri(-2, 2, B, C, G, G)
    p = dict(w=ri(-1, 1, C, 25), cb=ri(-3, 3, C) if seed % 2 else None, alpha=torch.tensor([1.0, 2.0, -1.0, -2.0])[torch.randint(0, 4, (C,), generator=g)],
             beta=ri(-8, 8, C), pb=ri(-4, 4, M))
    pw = ri(-1, 1, M, C)
    rank = torch.rand(M, C, generator=g).argsort(1).argsort(1)
    keep = rank < (min(C, 17) if out_is_half else max(1, (3 * C + 3) // 4))
    p["pw"] = pw * keep
    return x, p


def exact_reference(x, p, out_is_half):
    """float64 result of exact data, with the preconditions asserted from float64 alone."""
    t64 = stage_t(x, p, torch.float64)
    ref = stage_pw(t64, p["pw"], p["pb"], torch.float64)
    assert float(t64.max()) <= 114 and torch.equal(t64, t64.round())
    assert torch.equal(ref, ref.round()) and float(ref.abs().max()) <= (2048 if out_is_half else 2 ** 24 - 1)
    for v in (x, p["w"]):  # what the fp16-map class rounds is exact in fp16
        assert torch.equal(v.half().float(), v)
    return ref


# ---- float families --------------------------------------------------------------------------------------------------------------
FAMILIES = ("normal", "neg_alpha", "dead", "cancel", "large", "border")


@functools.lru_cache(maxsize=None)
def float_inputs(B, C, M, G, family, arith):
    g = torch.Generator().manual_seed(((B * 1009 + C) * 1009 + M) * 1009 + G * 7 + FAMILIES.index(family))
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    x = rn(B, C, G, G)
    p = dict(w=rn(C, 25) * 0.3, cb=rn(C) if C % 2 else None, alpha=torch.rand(C, generator=g) * 1.5 + 0.5, beta=rn(C),
             pw=rn(M, C) * C ** -0.5, pb=rn(M))
    if family == "neg_alpha":
        p["alpha"][::2] *= -1.0
    elif family == "dead":  # per channel, beta moves down to the 94 % quantile of the pre-activation
        xr, q = rounded_operands(x, p, arith)
        z = F.conv2d(xr.double(), q["w"].double().view(C, 1, 5, 5), None if q["cb"] is None else q["cb"].double(), padding=2, groups=C)
        z = z * q["alpha"].double().view(1, C, 1, 1) + q["beta"].double().view(1, C, 1, 1)
        p["beta"] = (p["beta"].double() - torch.quantile(z.permute(1, 0, 2, 3).reshape(C, -1), 0.94, dim=1)).float()
    elif family == "cancel":  # channel 2p+1 carries channel 2p's map and parameters up to 2^-6, and the opposite 1x1 weight
        n2 = C // 2
        x[:, 1:2 * n2:2] = x[:, 0:2 * n2:2] * (1 + 2.0 ** -6 * rn(B, n2, G, G))
        for k in ("w", "alpha", "beta"):
            p[k][1:2 * n2:2] = p[k][0:2 * n2:2]
        if p["cb"] is not None:
            p["cb"][1:2 * n2:2] = p["cb"][0:2 * n2:2]
        p["pw"][:, 1:2 * n2:2] = -p["pw"][:, 0:2 * n2:2]
        p["pw"][:, 2 * n2:] = 0.0
        p["pb"] *= 2.0 ** -6
    elif family == "large":  # ReLU outputs up to 4e3 (inside 1e3 .. 3e4)
        xr, q = rounded_operands(x, p, arith)
        x = x * (4e3 / float(stage_t(xr, q, torch.float64).max()))
        p["beta"] *= 100.0
    elif family == "border":  # O(100) in the two outermost rings, O(0.01) inside
        ring = torch.ones(G, G, dtype=torch.bool)
        ring[2:G - 2, 2:G - 2] = False
        x = torch.where(ring, x * 100.0, x * 0.01)
    return x, p


def float_preconditions(x, p, arith, out_is_half, family):
    """What a family promises, from float64 alone; returns (ref, bound)."""
    ref, bound, t64 = reference(x, p, arith, out_is_half)
    assert torch.isfinite(ref).all() and float(bound.min()) > 0
    xr, q = rounded_operands(x, p, arith)
    if arith == "map16":
        assert float(x.abs().max()) < 65504
    assert float(t64.max()) < 65504 and (not out_is_half or float(ref.abs().max()) < 65504)     # every stored or rounded value is in range
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
        assert G == 4 or float(x[..., 2:G - 2, 2:G - 2].abs().max()) < 0.1  # (a 4x4 map is all ring)
        assert float(x[..., 0, :].abs().mean()) > 10
    return ref, bound


def test_exact_data_preconditions_of_every_case():
    import test_conv_block_routes_gpu as gpu

    for i, (cls, B, C, M, G) in enumerate(gpu.CASES + gpu.EDGES + gpu.WRITE_CASES):
        x, p = exact_inputs(B, C, M, G, half_out(cls), i)
        exact_reference(x, p, half_out(cls))
    for cls, B, C, M, G in gpu.TPB_CASES:
        x, p = exact_inputs(gpu.TPB_PERIOD, C, M, G, half_out(cls), 5)
        exact_reference(x, p, half_out(cls))


def test_float_family_preconditions_of_every_route():
    import test_conv_block_routes_gpu as gpu

    assert 28 <= len(gpu.FLOAT_ROUTES) <= 36 and {c[0] for c in gpu.FLOAT_ROUTES} == set(CLASSES)
    assert len({route_key(route(*c)) for c in gpu.FLOAT_ROUTES}) >= 28
    for cls, B, C, M, G in gpu.FLOAT_ROUTES:
        for family in FAMILIES:
            x, p = float_inputs(B, C, M, G, family, CLASSES[cls][1])
            float_preconditions(x, p, CLASSES[cls][1], half_out(cls), family)
