"""Global correlation and its soft-argmax (csrc/corr_softargmax.hip) on every route of launch_corr, through the C ABI, against the
float64 oracle (pinned to the reference's G2 golden by test_oracle_golden.py) and against flows known in closed form.

launch_corr picks a kernel from the channel count C (k-steps KS = 8 / 16 / 32 / 64), the B-image row width W1 (32..64: row tiles,
else the general tile loop), the workspace (pre-split bf16 images) and whether a volume is written.  Every route meets inputs that
expose masking and indexing (all logits equal, one-hot logits at the tiles' edges, exact ties, all logits far below zero) and random
features at three magnitudes, checked against a bound derived from the operands.  fp16 maps, symmetric virtual batches and the
workspace must reproduce their fp32 / concatenated / in-kernel counterparts bit for bit."""
import numpy as np
import pytest
import torch

import oracle
import synth

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
# Bounds from the operands, per A-position i and B-position j: M_ij = sum_c |f0_ci f1_cj| / sqrt(C), T_i = max_j M_ij.
#   volume: |V_ij - V64_ij| <= K_VOL (C + 4) U M_ij;   flow: |flow_i - flow64_i| <= K_FLOW (C + 4) U T_i + FLOOR.
# K_VOL: (C + 4) U M is the worst case of a length-C fp32 sum plus the rounding of sqrt(C) and of the division by it (split-bf16:
#    the dropped piece products add <= 3 U of each product).
K_VOL = 1.0
# K_FLOW: the flow moves by at most 2 max_j |dlogit_j| (|coordinate| < 1), but the rounding of C / 4 chained matrix steps grows
#    like sqrt(C), not C, and the softmax averages it: a quarter of the worst case keeps every route several times inside (the GPU
#    log prints the margins) and puts the bound under the fixed 1e-4 of test_ops_gpu.py at its inputs.
K_FLOW = 0.25
FLOOR = 4e-6
EXACT = 1e-6          # flows known in closed form (all logits equal, one-hot, ties): a masked or misplaced position moves them ~1e-3
HOT = 40.0            # one-hot amplitude: a hot logit of 1600 / sqrt(C) >= 141, every other weight below e^-141 (0 in fp32)
NEG = 120.0           # all-negative regime: f0 = -NEG, f1 in [0.5, 1.5] -> every logit <= -NEG / 2 * sqrt(C) <= -158

CS = [7, 16, 17, 31, 32, 33, 48, 64, 65, 96, 128]
ROW_W = [32, 33, 35, 40, 48, 63, 64]        # row-tile path (35 / 40 / 48: the 560 / 672 maps)
GEN_W = [16, 28, 31, 65, 80]                # general tile loop
A_MAPS = [(5, 7), (3, 11), (7, 9), (4, 13), (9, 5)]    # 35 / 33 / 63 / 52 / 45 A-positions: never a multiple of 32


def _cases():
    out = []
    for k, C in enumerate(CS):
        H0, W0 = A_MAPS[k % len(A_MAPS)]
        out.append((C, H0, W0, 3 + 2 * (k % 2), ROW_W[k % len(ROW_W)]))
        out.append((C, W0, H0, 5 - 2 * (k % 2), ROW_W[(k + 3) % len(ROW_W)]))
        out.append((C, H0, W0, 7 - 2 * (k % 3), GEN_W[k % len(GEN_W)]))
    # B-maps of at most four positions: the second half-wave's first (and only) tile is all padding
    out += [(16, 5, 7, 2, 2), (65, 3, 11, 1, 3), (7, 4, 13, 1, 1)]
    return out


CASES = _cases()
REGIMES = ["flat", "peaked", "ties", "negative", "mag0.05", "mag1", "mag8"]
STATS = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if STATS:
        print("\ncorr_softargmax: worst err / tol per route")
        for name in sorted(STATS):
            print(f"  {name:48s} {STATS[name]:.3f}")


def _record(name, ratio):
    STATS[name] = max(STATS.get(name, 0.0), float(ratio))


def _ks(C):
    return 8 if C <= 16 else 16 if C <= 32 else 32 if C <= 64 else 64


def fused_route(C, W1, ws_used):
    """launch_corr's choice for a flow-only call"""
    if 32 <= W1 <= 64:
        if _ks(C) == 32:
            return f"row split-bf16 workspace P{2 if W1 > 32 else 1}" if ws_used else "row split-bf16 in-kernel"
        return f"row fp32 KS{_ks(C)}"
    return f"general KS{_ks(C)}"


def centres(n):
    return (np.arange(n) * 2 + 1) / n - 1.0


def fp16_exact(a):
    return np.ascontiguousarray(a, np.float32).astype(np.float16).astype(np.float32)


def hot_candidates(H1, W1):
    """B-positions where masking and indexing go wrong: first / last, x = 31 / 32 (the two parities of a two-part row) / W1 - 1
    (the masked part's edge), the first row's end, the start and middle of the ragged last tile of 32"""
    N1 = H1 * W1
    t0 = (N1 - 1) // 32 * 32
    c = [0, N1 - 1, W1 - 1, t0, (t0 + N1 - 1) // 2]
    for x in (31, 32, W1 - 1):
        if x < W1:
            c += [(H1 - 1) * W1 + x, (H1 // 2) * W1 + x]
    return list(dict.fromkeys(c))


def make_inputs(regime, B, C, H0, W0, H1, W1, seed):
    """(f0, f1, expected flow or None): fp16-exact fp32 maps, so that the fp16 calls see the same values"""
    N0, N1 = H0 * W0, H1 * W1
    gx, gy = centres(W1), centres(H1)
    if regime.startswith("mag"):
        s = np.float32(float(regime[3:]))
        return (fp16_exact(s * synth.lattice_normalish((B, C, H0, W0), seed)),
                fp16_exact(s * synth.lattice_normalish((B, C, H1, W1), seed + 1)), None)
    if regime == "negative":
        f1 = 1.0 + synth.lattice_uniform((B, C, H1, W1), seed) / 2   # [0.5, 1.5] on a 2^-12 lattice ...
        return np.full((B, C, H0, W0), -NEG, np.float32), fp16_exact(np.round(f1 * 1024) / 1024), None   # ... on 2^-10: fp16
    if regime == "flat":
        f1 = fp16_exact(synth.lattice_normalish((B, C, H1, W1), seed))
        exp = np.empty((B, 2, H0, W0))
        exp[:, 0], exp[:, 1] = gx.mean(), gy.mean()
        return np.zeros((B, C, H0, W0), np.float32), f1, exp
    # peaked / ties: A-position i of batch b reads channel c = i % nc only; channel c of batch b is HOT at one B-position (two for
    # ties) and zero elsewhere, every other channel of f1 at that position is zero or hot for another channel -> logit 0
    cand = hot_candidates(H1, W1)
    nc = min(C, N0)
    f0 = np.zeros((B, C, N0), np.float32)
    f1 = np.zeros((B, C, N1), np.float32)
    exp = np.empty((B, 2, N0))
    for b in range(B):
        hots = []
        for c in range(nc):
            k = (b * nc + c) % len(cand)
            js = [cand[k]] if regime == "peaked" else [cand[k], cand[(k + len(cand) // 2) % len(cand)]]
            f1[b, c, js] = HOT
            hots.append(js)
        for i in range(N0):
            js = hots[i % nc]
            f0[b, i % nc, i] = HOT
            exp[b, 0, i] = np.mean([gx[j % W1] for j in js])
            exp[b, 1, i] = np.mean([gy[j // W1] for j in js])
    if B * nc < len(cand):
        raise AssertionError("not every candidate position is hot somewhere")
    return f0.reshape(B, C, H0, W0), f1.reshape(B, C, H1, W1), exp.reshape(B, 2, H0, W0)


def operand_magnitude(f0, f1):
    """sum_c |f0_ci f1_cj| / sqrt(C) as (B, N1, N0), float64"""
    B, C = f0.shape[:2]
    a = np.abs(f0.reshape(B, C, -1).astype(np.float64))
    b = np.abs(f1.reshape(B, C, -1).astype(np.float64))
    return np.einsum("bcj,bci->bji", b, a) / np.sqrt(C)


def flow_tol(f0, f1, mag=None):
    """(B, 2, H0, W0) bound of the fused flow: K_FLOW (C + 4) U T_i + FLOOR"""
    B, C, H0, W0 = f0.shape
    mag = operand_magnitude(f0, f1) if mag is None else mag
    t = K_FLOW * (C + 4) * U * mag.max(axis=1) + FLOOR
    return np.broadcast_to(t.reshape(B, 1, H0, W0), (B, 2, H0, W0))


def check(name, got, ref, tol):
    """|got - ref| <= tol elementwise; records the worst err / tol under the route's name"""
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert np.isfinite(got).all(), f"{name}: non-finite output at {np.argwhere(~np.isfinite(got))[:4].tolist()}"
    err = np.abs(got - ref)
    ratio = err / tol
    _record(name, ratio.max())
    k = np.unravel_index(ratio.argmax(), ratio.shape)
    assert ratio.max() <= 1.0, f"{name}: err {err[k]:.3e} > tol {np.asarray(tol)[k]:.3e} at {k} (got {got[k]:.7f}, want {ref[k]:.7f})"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


# ---- the C-ABI calls ------------------------------------------------------------------------------------------------------------
def _L():
    from gfnet_amd import _lib

    return _lib, _lib.lib()


def call_fwd(a, b, H1, W1, sym=False):
    lib, L = _L()
    B, C, H0, W0 = a.shape
    flow = torch.full((B * (2 if sym else 1), 2, H0, W0), float("nan"), device="cuda")
    lib.check(L.gfn_corr_softargmax_fwd(lib.ptr(a), lib.ptr(b), lib.ptr(flow), flow.shape[0], C, H0, W0, H1, W1, int(sym),
                                        lib.stream_ptr(a.device)), "gfn_corr_softargmax_fwd")
    return host(flow)


def call_dt(a, b, H1, W1, sym=False):
    lib, L = _L()
    B, C, H0, W0 = a.shape
    dt = lib.GFN_F16 if a.dtype == torch.float16 else lib.GFN_F32
    flow = torch.full((B * (2 if sym else 1), 2, H0, W0), float("nan"), device="cuda")
    lib.check(L.gfn_corr_softargmax_fwd_dt(lib.ptr(a), lib.ptr(b), dt, lib.ptr(flow), flow.shape[0], C, H0, W0, H1, W1, int(sym),
                                           lib.stream_ptr(a.device)), "gfn_corr_softargmax_fwd_dt")
    return host(flow)


def call_ws(a, b, H1, W1, use_ws, sym=False):
    """gfn_corr_softargmax_fwd_ws with a workspace of the size it asks for (when it asks for one) or without; -> (flow, ws used)"""
    lib, L = _L()
    B, C, H0, W0 = a.shape
    nb = B * (2 if sym else 1)
    dt = lib.GFN_F16 if a.dtype == torch.float16 else lib.GFN_F32
    need = int(L.gfn_corr_softargmax_ws_bytes(nb, C, H1, W1)) if use_ws else 0
    ws = torch.empty(max(need, 16), device="cuda", dtype=torch.uint8) if use_ws else None
    flow = torch.full((nb, 2, H0, W0), float("nan"), device="cuda")
    lib.check(L.gfn_corr_softargmax_fwd_ws(lib.ptr(a), lib.ptr(b), dt, lib.ptr(flow), nb, C, H0, W0, H1, W1, int(sym), lib.ptr(ws), need,
                                           lib.stream_ptr(a.device)), "gfn_corr_softargmax_fwd_ws")
    return host(flow), need > 0


def call_volume(a, b, H1, W1, with_flow):
    lib, L = _L()
    B, C, H0, W0 = a.shape
    vol = torch.full((B, H1, W1, H0, W0), float("nan"), device="cuda")
    flow = torch.full((B, 2, H0, W0), float("nan"), device="cuda") if with_flow else None
    lib.check(L.gfn_corr_volume_fwd(lib.ptr(a), lib.ptr(b), lib.ptr(vol), lib.ptr(flow), B, C, H0, W0, H1, W1, lib.stream_ptr(a.device)),
              "gfn_corr_volume_fwd")
    return (vol, host(flow)) if with_flow else vol


def call_pos_embed(vol):
    lib, L = _L()
    B, H1, W1, H0, W0 = vol.shape
    flow = torch.full((B, 2, H0, W0), float("nan"), device="cuda")
    lib.check(L.gfn_pos_embed_fwd(lib.ptr(vol), lib.ptr(flow), B, H0, W0, H1, W1, lib.stream_ptr(vol.device)), "gfn_pos_embed_fwd")
    return host(flow)


# ---- 1 + 2 + 3: every route, every input regime, against float64 -----------------------------------------------------------------
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("C,H0,W0,H1,W1", CASES, ids=[f"C{c[0]}-A{c[1]}x{c[2]}-B{c[3]}x{c[4]}" for c in CASES])
def test_every_route_against_float64(C, H0, W0, H1, W1, regime):
    """Every fused entry point (fp32, fp16, with and without a workspace), the volume with and without its flow, and pos_embed on
    that volume, on one shape and input regime"""
    B = 2
    f0, f1, exact = make_inputs(regime, B, C, H0, W0, H1, W1, 1000 + 7 * C + W1 + 131 * H1)
    a32, b32 = dev(f0), dev(f1)
    a16, b16 = a32.half(), b32.half()

    fwd = call_fwd(a32, b32, H1, W1)
    # bit for bit: the dtype entry point, fp16 maps against their widened copy, the workspace against the in-kernel split
    assert np.array_equal(call_dt(a32, b32, H1, W1), fwd, equal_nan=True)
    assert np.array_equal(call_dt(a16, b16, H1, W1), fwd, equal_nan=True)
    ws_none, _ = call_ws(a32, b32, H1, W1, False)
    ws32, used = call_ws(a32, b32, H1, W1, True)
    ws16, used16 = call_ws(a16, b16, H1, W1, True)
    assert used == used16 == (32 < C <= 64 and 32 <= W1 <= 64)
    assert np.array_equal(ws_none, fwd, equal_nan=True) and np.array_equal(ws32, fwd, equal_nan=True)
    assert np.array_equal(ws16, ws32, equal_nan=True)

    vol_t, vflow = call_volume(a32, b32, H1, W1, True)
    vol = host(vol_t)
    assert np.array_equal(host(call_volume(a32, b32, H1, W1, False)), vol, equal_nan=True)
    pflow = call_pos_embed(vol_t)

    mag = operand_magnitude(f0, f1)
    vref = oracle.corr_volume(f0, f1, variant="f64")
    vtol = (K_VOL * (C + 4) * U * mag).reshape(vref.shape)
    check(f"volume KS{_ks(C)}", vol, vref, np.maximum(vtol, np.finfo(np.float64).tiny))
    # pos_embed alone, on the volume the kernel wrote: only the softmax's rounding
    check("pos_embed (own volume)", pflow, oracle.pos_embed(vol), np.full(pflow.shape, FLOOR))
    outs = {fused_route(C, W1, False): fwd, "volume+flow KS%d" % _ks(C): vflow, "pos_embed": pflow}
    if used:
        outs[fused_route(C, W1, True)] = ws32
    if exact is not None:
        for name, got in outs.items():
            check(f"{name} [{regime}]", got, exact, np.full(exact.shape, EXACT))
    else:
        ref = oracle.corr_softargmax(f0, f1, variant="f64")
        tol = flow_tol(f0, f1, mag)
        for name, got in outs.items():
            check(name, got, ref, tol)


# ---- 4: symmetric virtual batches ------------------------------------------------------------------------------------------------
SYM_CASES = [(C, 5, ROW_W[k % len(ROW_W)]) for k, C in enumerate(CS)] + [(C, 3, GEN_W[k % len(GEN_W)]) for k, C in enumerate(CS)]


@pytest.mark.parametrize("C,H,W", SYM_CASES, ids=[f"C{c[0]}-{c[1]}x{c[2]}" for c in SYM_CASES])
def test_symmetric_batch_equals_the_concatenated_batch(C, H, W):
    """symmetric=True reads direction b >= Bh as (f1[b - Bh], f0[b - Bh]) instead of a concatenated copy; two images per side so
    that a wrong image index cannot go unseen"""
    Bh = 2
    f0 = fp16_exact(synth.lattice_normalish((Bh, C, H, W), 500 + C + W))
    f1 = fp16_exact(synth.lattice_normalish((Bh, C, H, W), 600 + C + W))
    a, b = dev(f0), dev(f1)
    ca, cb = torch.cat((a, b)), torch.cat((b, a))
    sym = call_fwd(a, b, H, W, sym=True)
    assert np.array_equal(sym, call_fwd(ca, cb, H, W))
    sym_ws, used = call_ws(a.half(), b.half(), H, W, True, sym=True)
    assert np.array_equal(sym_ws, call_ws(ca.half(), cb.half(), H, W, True)[0])
    assert np.array_equal(sym_ws, sym)          # fp16 == widened fp32; the workspace == the in-kernel split
    assert np.array_equal(call_ws(a, b, H, W, False, sym=True)[0], sym)
    ref = oracle.corr_softargmax(np.concatenate((f0, f1)), np.concatenate((f1, f0)), variant="f64")
    check(fused_route(C, W, False) + " symmetric", sym, ref, flow_tol(np.concatenate((f0, f1)), np.concatenate((f1, f0))))
    if used:
        check(fused_route(C, W, True) + " symmetric", sym_ws, ref, flow_tol(np.concatenate((f0, f1)), np.concatenate((f1, f0))))


def test_derived_bound_is_not_looser_than_the_suites_at_its_inputs():
    """At the moderate inputs test_ops_gpu.py checks with a fixed 1e-4, the operand-derived flow bound is tighter"""
    for C, H0, H1 in [(64, 48, 48), (64, 32, 32), (16, 12, 20), (7, 9, 5), (48, 32, 32)]:
        f0 = 2 * synth.lattice_normalish((1, C, H0, H0), 71)
        f1 = 2 * synth.lattice_normalish((1, C, H1, H1 + 1), 72)
        assert flow_tol(f0, f1).max() < 1e-4, C


# ---- 5: B-maps of close to 2^24 positions ------------------------------------------------------------------------------------------
def test_general_loop_places_b_positions_exactly_up_to_2_pow_24():
    """A flow-only call on a (1, 4, 4096, 4095) B-map: 16 773 120 positions, under check_args' 2^24.  Each channel is hot at one
    position where the general loop's float row quotient, ((float)j + 0.5f) * (1.0f / W1), lands a row too high (x = W1 - 2 / W1 - 1,
    found by emulating it in float32 here), the last of them at j = N1 - 1; each A-position reads one channel, so its flow is that
    position's cell centre."""
    C, H1, W1, N0 = 4, 4096, 4095, 64
    N1 = H1 * W1
    j = np.arange(N1, dtype=np.int32)
    jy = ((j.astype(np.float32) + np.float32(0.5)) * (np.float32(1.0) / np.float32(W1))).astype(np.int32)
    bad = np.nonzero(jy != j // W1)[0]
    assert len(bad) > 0 and bad[-1] == N1 - 1
    hot = [int(bad[0]), int(bad[len(bad) // 2]), int(bad[len(bad) // 2 + 1]), N1 - 1]
    assert {h % W1 for h in hot} == {W1 - 2, W1 - 1}
    f1 = torch.zeros((1, C, N1), device="cuda")
    for c, h in enumerate(hot):
        f1[0, c, h] = 16.0                      # hot logit 16 * 16 / sqrt(4) = 128
    f0 = torch.zeros((1, C, 1, N0), device="cuda")
    for i in range(N0):
        f0[0, i % C, 0, i] = 16.0
    flow = call_fwd(f0, f1.view(1, C, H1, W1), H1, W1)
    gx, gy = centres(W1), centres(H1)
    want = np.empty((1, 2, 1, N0))
    for i in range(N0):
        want[0, 0, 0, i], want[0, 1, 0, i] = gx[hot[i % C] % W1], gy[hot[i % C] // W1]
    check("general KS8, 2^24 - 2^12 B-positions", flow, want, np.full(want.shape, EXACT))
