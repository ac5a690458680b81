"""ops.refiner_input (ConvRefiner's concat tensor d, model/network.py:533-558) on hostile flows, through every route of the local
correlation that fills its last slice (csrc/local_corr.hip lc_route): the lean kernel behind the plan that the refiner-input launch
writes (r <= 4, C-ABI variant bit 8), the round-1 kernel, the matrix-core kernel and the general kernel.

tests/test_local_corr_gpu.py puts these flows through utils.local_correlation, which launches its own plan and never passes
f1_second.  Here the same flows go through refiner_input, in plain and symmetric batches (directions b >= Bh read the other image
through f1_second), with fp32 and fp16 maps, on ragged grids and on grids large enough for the XCD-banded launch of symmetric
batches (>= 8 cell blocks per direction: G >= 46).  Every slice is compared with the oracle (itself checked against a float64
restatement by tests/test_refiner_input_cpu.py), and the fused plan with the unfused one and with a standalone correlation call."""
import numpy as np
import pytest
import torch

import oracle
import synth
from conftest import assert_close
from test_configs_gpu import _bench_flows, _raw_softargmax_flows
from test_refiner_input_cpu import FLOW_KINDS, hard_flows

pytestmark = pytest.mark.gpu
TOL = 1e-4
DD = 8      # displacement embedding width
SF = 1.25   # scale_factor


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _maps(c, h, w, seed, Bh=2):
    return synth.lattice_normalish((Bh, c, h, w), seed), synth.lattice_normalish((Bh, c, h, w), seed + 1)


def _flows(kind, B, G, seed, S=None):
    if kind == "softargmax":  # the raw soft-argmax flows of a synthetic scene's coarsest maps (G = S / 14)
        flow = _raw_softargmax_flows(B, S, seed)
        assert flow.shape == (B, 2, G, G)
        return flow
    return hard_flows(kind, B, G, seed)


def _emb(seed):
    return synth.lattice_uniform((DD, 2, 1, 1), seed), synth.lattice_uniform((DD,), seed + 1)


def _ri(G, x, y, flow, w, bias, r, fuse=True, **kw):
    """ops.refiner_input on device tensors, the fused plan on or off (restored whatever happens)."""
    from gfnet_amd import ops

    keep = ops.FUSE_PLAN
    ops.FUSE_PLAN = fuse
    try:
        return ops.refiner_input(G, x, y, flow, w, bias, r, scale_factor=SF, **kw)
    finally:
        ops.FUSE_PLAN = keep


def _standalone_corr(d, x, y, flow, r, G):
    """The correlation slice as a standalone gfn_local_corr_fwd_dt call (its own plan launch, variant 0) with f0 = d[:, :C] and the
    f1 / f1_second refiner_input passes: y, and x for symmetric batches."""
    from gfnet_amd import _lib

    L = _lib.lib()
    (xc, dt), (yc, _) = _lib.featc(x), _lib.featc(y)
    B, CH = d.shape[:2]
    C, Hs, Ws = xc.shape[1:]
    K = (2 * r + 1) ** 2
    symmetric = B == 2 * xc.shape[0]
    out = torch.full((B, K, G, G), 7.0, device=d.device)
    nscr = int(L.gfn_local_corr_scratch_bytes(B, G))
    scr = _lib.scratch(d.device, nscr)
    _lib.check(L.gfn_local_corr_fwd_dt(_lib.ptr(d), CH * G * G, _lib.ptr(yc), _lib.ptr(xc) if symmetric else None, dt, _lib.ptr(flow),
                                       _lib.c_vp(out.data_ptr()), K * G * G, B, C, G, Hs, Ws, r, 0, Hs, Ws, 0, _lib.ptr(scr), nscr,
                                       _lib.stream_ptr(d.device)), "gfn_local_corr_fwd")
    return out


def _route(c, h, w, G, r, f16):
    """lc_route's choice for this call (csrc/local_corr.hip), restated from the C-ABI's own answers."""
    from gfnet_amd import _lib

    if c % 16:
        return "general"
    if _lib.lib().gfn_local_corr_plans(c, h, w, G, r, 1 if f16 else 0):
        return "lean"
    if r >= 5 and c == 64 and not (f16 and w & 1):
        return "mq"
    return "round1"


def check_case(c, h, w, G, r, a, b, flow, wt, bias, f16, what):
    """Plain (concatenated) and symmetric form of one case: d against the oracle, bit-identical without the fused plan, correlation
    planes bit-identical to a standalone call."""
    if f16:  # the oracle gets the widened fp16 values
        a, b = a.astype(np.float16), b.astype(np.float16)
    ref = oracle.refiner_input(G, np.concatenate((a, b)).astype(np.float32), np.concatenate((b, a)).astype(np.float32), flow, wt, bias, r,
                               scale_factor=SF)
    K0 = 2 * c + DD
    fl, W_, B_ = dev(flow), dev(wt), dev(bias)
    for form, x, y in (("plain", np.concatenate((a, b)), np.concatenate((b, a))), ("symmetric", a, b)):
        x, y = dev(x), dev(y)
        tag = f"{what} {form} {'fp16' if f16 else 'fp32'}"
        d = _ri(G, x, y, fl, W_, B_, r)
        got = host(d)
        assert_close(got, ref, TOL, tag)
        np.testing.assert_array_equal(host(_ri(G, x, y, fl, W_, B_, r, fuse=False)), got, err_msg=f"{tag}: fused vs unfused plan")
        # The fused plan and the standalone plan launch both run plan_tiles on the same flows, and the tile kernels read the same f0
        # (d[:, :C]), f1 and f1_second: the same tiles take the same branches with the same arithmetic.
        np.testing.assert_array_equal(host(_standalone_corr(d, x, y, fl, r, G)), got[:, K0:], err_msg=f"{tag}: fused vs standalone")


# (c, h, w, G, r, S): S is the image side whose raw soft-argmax flows a r = 7 shape also runs (None: no such flows)
LEAN = [(16, 30, 30, 24, 1, None), (32, 56, 56, 46, 2, None), (16, 60, 60, 47, 3, None), (16, 37, 54, 21, 3, None),
        (32, 112, 112, 64, 4, None), (16, 224, 224, 128, 2, None),    # 448, scales 4 and 2
        (32, 140, 140, 80, 4, None), (16, 280, 280, 160, 2, None),    # 560
        (32, 168, 168, 96, 4, None), (16, 336, 336, 192, 2, None),    # 672
        (32, 45, 45, 27, 4, None)]                                    # odd width: fp16 maps take the round-1 kernel
MQ = [(64, 56, 56, 32, 6, None), (64, 70, 70, 40, 6, None), (64, 32, 32, 32, 7, 448), (64, 48, 48, 48, 7, 672),
      (64, 45, 45, 27, 5, None)]                                      # odd width: fp16 maps take the round-1 kernel (narrow stage loads)
ROUND1 = [(48, 56, 56, 32, 2, None), (48, 48, 48, 47, 4, None), (64, 35, 35, 20, 6, None)]
GENERAL = [(24, 40, 40, 24, 2, None), (24, 48, 48, 46, 6, None)]
CASES = [(*s, k) for s in LEAN + MQ + ROUND1 + GENERAL for k in FLOW_KINDS + (["softargmax"] if s[5] else [])]


@pytest.mark.parametrize("c,h,w,G,r,S,kind", CASES)
def test_refiner_input_parity_matrix(c, h, w, G, r, S, kind):
    seed = 20000 + 97 * r + 13 * G + c
    a, b = _maps(c, h, w, seed)
    flow = _flows(kind, 4, G, seed + 2, S)
    wt, bias = _emb(seed + 3)
    routes = set()
    for f16 in (False, True):
        routes.add(_route(c, h, w, G, r, f16))
        check_case(c, h, w, G, r, a, b, flow, wt, bias, f16, f"c{c} {h}x{w} G{G} r{r} {kind}")
    expect = {"lean": r <= 4 and c in (16, 32), "mq": r >= 5 and c == 64, "round1": c == 48 or (w & 1 and c % 16 == 0),
              "general": c % 16 != 0}
    assert routes == {k for k, v in expect.items() if v}, routes


def test_refiner_input_full_batch_bench_flows():
    """configs[1]'s scale 4 at its real batch: 32 pairs = 64 directions, symmetric, bench-like flows."""
    c, hs, G, r = 32, 112, 64, 4
    a, b = _maps(c, hs, hs, 30101, Bh=32)
    flow = _bench_flows(64, G, 448, 30103)
    wt, bias = _emb(30104)
    check_case(c, hs, hs, G, r, a, b, flow, wt, bias, False, "full batch")


def _counters(calls):
    """Header words 3, 5, 7 (tiles left to the second launch, cells redone per tap, tiles staged in halves -- sampled once per 16 tiles
    by the plan, once per 8 by the matrix-core kernel) summed over `calls` (thunks) run under ops.kernel_counters."""
    from gfnet_amd import ops

    ops.kernel_counters = {}
    try:
        for call in calls:
            call()
        tot = np.zeros(3, np.int64)
        for v in ops.kernel_counters.values():
            tot += np.asarray(v, np.int64).sum(axis=0)
        return tot
    finally:
        ops.kernel_counters = None


def _sym_call(c, h, w, G, r, kind, seed, f16=False, S=None):
    a, b = _maps(c, h, w, seed)
    if f16:
        a, b = a.astype(np.float16), b.astype(np.float16)
    flow = _flows(kind, 4, G, seed + 2, S)
    wt, bias = _emb(seed + 3)
    x, y, fl, W_, B_ = dev(a), dev(b), dev(flow), dev(wt), dev(bias)
    return lambda: _ri(G, x, y, fl, W_, B_, r)


WILD = [(np.nan, 0), (np.inf, 0), (-np.inf, 1), (1e30, 0), (-1e9, 1), (50.0, 0)]
# (direction, i, j) of each wild value: both halves of the symmetric batch, next to ordinary cells of the same tile, and at corners
WILD_AT = [[(0, 1, 3), (0, 2, 9), (0, 0, 0), (0, 5, 14), (0, 9, 17), (0, 2, 5)],
           [(2, 3, 2), (3, 1, 6), (2, 23, 23), (3, 10, 10), (2, 1, 7), (3, 6, 1)]]


# lean r = 2 / 4 (fused plan), matrix core, general
WILD_SHAPES = {2: (16, 40, 40, 24), 4: (32, 56, 56, 32), 6: (64, 56, 56, 32), "general": (24, 40, 40, 24)}


def _wild_case(c, h, w, G):
    """Maps, a sane flow, the same flow with the WILD values in, embedding weights, and the mask of the ordinary cells."""
    seed = 43000 + 13 * G + c
    a, b = _maps(c, h, w, seed)
    flow = synth.homography_flow(4, G, seed + 2, scale=1.05)
    wt, bias = _emb(seed + 3)
    good = np.ones((4, G, G), bool)
    wild = flow.copy()
    for at in WILD_AT:
        for (val, comp), (bb, i, j) in zip(WILD, at):
            wild[bb, comp, i, j] = val
            good[bb, i, j] = False
    return a, b, flow, wild, wt, bias, good


@pytest.mark.parametrize("r", [2, 4])
def test_route_coverage_of_the_fused_plan(r):
    """The suite reaches the lean path's rare branches through the fused plan: across the symmetric calls at this radius (the parity
    matrix's flows and the wild-flow case) some tiles go to the second launch, some cells are redone per tap and some tiles are staged
    in halves.  Finite flows flag only cells whose taps straddle a pixel boundary within rounding (a handful per radius); the wild
    flows' non-finite cells are flagged for certain.  At r >= 3 the second launch runs inside the tile kernel, whose workgroups may
    still be adding flagged cells (word 4) when the last worker moves that count to word 5: such cells show in the next call's word 5,
    hence the wild call first and a mild call last."""
    shapes = [s for s in LEAN if s[4] == r and _route(s[0], s[1], s[2], s[3], r, False) == "lean"]
    wc, wh, ww, wG = WILD_SHAPES[r]
    a, b, _, wild, wt, bias, _ = _wild_case(wc, wh, ww, wG)
    wargs = (wG, dev(a), dev(b), dev(wild), dev(wt), dev(bias), r)
    calls = [lambda: _ri(*wargs)]
    calls += [_sym_call(c, h, w, G, r, kind, 40000 + 13 * G + c) for (c, h, w, G, _, _) in shapes for kind in FLOW_KINDS + ["homography"]]
    second, per_tap, halves = _counters(calls)
    print(f"r={r}: second-launch tiles {second}, per-tap cells {per_tap}, halves (sampled) {halves}")
    assert second > 0, "no tile went to the second launch"
    assert per_tap > 0, "no cell was redone per tap"
    assert halves > 0, "no tile was staged in halves"


def test_route_coverage_of_the_matrix_core_second_launch():
    """r = 6 / 7 on 64-channel maps: the matrix-core kernel hands tiles to the second launch under these flows."""
    calls = [_sym_call(c, h, w, G, r, kind, 41000 + 13 * G + r, S=S) for (c, h, w, G, r, S) in MQ if r >= 6
             for kind in FLOW_KINDS + (["softargmax"] if S else [])]
    second, _, in_launch = _counters(calls)
    print(f"matrix core: second-launch tiles {second}, fp32 routine in launch (sampled) {in_launch}")
    assert second > 0, "the matrix-core path sent no tile to the second launch"


def test_scratch_state_across_calls_on_one_stream():
    """The scratch header is zeroed by each call's last workgroup and the tile list is reused: calls that list many tiles (scattered
    flow) followed by calls that list none (mild flow), and the other way round, on one stream without a sync between them, give what
    each gives on its own.  Lean r = 2 (separate second launch) and r = 4 (second launch inside the tile kernel), matrix core, round 1."""
    shapes = [(32, 112, 112, 64, 4), (16, 56, 56, 46, 2), (64, 56, 56, 32, 6), (48, 56, 56, 32, 4)]
    calls = []
    for i, (c, h, w, G, r) in enumerate(shapes):
        for kind in ("random", "homography"):
            calls.append(_sym_call(c, h, w, G, r, kind, 42000 + 100 * i))
    alone = []
    for call in calls:
        torch.cuda.synchronize()
        alone.append(host(call()))
    scattered, mild = list(range(0, len(calls), 2)), list(range(1, len(calls), 2))
    orders = [[k for pair in zip(scattered, mild) for k in pair], [k for pair in zip(mild, scattered) for k in pair],
              scattered + mild + scattered[::-1] + mild[::-1]]
    for order in orders:
        torch.cuda.synchronize()
        outs = [calls[k]() for k in order]  # no sync in between
        torch.cuda.synchronize()
        for k, d in zip(order, outs):
            np.testing.assert_array_equal(host(d), alone[k], err_msg=f"call {k} in order {order}")


@pytest.mark.parametrize("c,h,w,G,r", [(*WILD_SHAPES[2], 2), (*WILD_SHAPES[4], 4), (*WILD_SHAPES[6], 6), (*WILD_SHAPES["general"], 2)])
def test_wild_flows_through_every_route(c, h, w, G, r):
    """NaN, +-inf, 1e30, -1e9 and 50.0 in single cells of both directions of a symmetric batch (lean r = 2 / 4 with the fused plan,
    matrix core, general).  The call succeeds; every other cell -- those sharing a tile with a bad one included, whose staging region
    the plan derives from the tile's flows -- matches the oracle in all four slices; the 50.0 cell (far outside the image) has zero
    x_hat and zero correlation.  Values at the other bad cells are unspecified, as in test_non_finite_and_far_flow_is_memory_safe."""
    a, b, flow, wild, wt, bias, good = _wild_case(c, h, w, G)
    ref = oracle.refiner_input(G, np.concatenate((a, b)), np.concatenate((b, a)), flow, wt, bias, r, scale_factor=SF)  # the sane flow
    d = host(_ri(G, dev(a), dev(b), dev(wild), dev(wt), dev(bias), r))
    for bb in range(4):
        assert_close(d[bb][:, good[bb]], ref[bb][:, good[bb]], TOL, f"direction {bb}: ordinary cells")
    for (bb, i, j) in (at[-1] for at in WILD_AT):  # the 50.0 cells
        assert np.all(d[bb, c:2 * c, i, j] == 0), "x_hat of a cell far outside the image"
        assert np.all(d[bb, 2 * c + DD:, i, j] == 0), "correlation of a cell far outside the image"


@pytest.mark.parametrize("c,h,w,G,r", [(32, 112, 112, 64, 4), (16, 56, 56, 46, 2), (16, 60, 60, 47, 3)])
@pytest.mark.parametrize("f16", [False, True])
def test_reuse_on_hard_flows(c, h, w, G, r, f16):
    """reuse= (the second refiner iteration at a scale keeps the grid_feature planes) on symmetric, banded, fused-plan batches: a
    scattered flow, then a noisy one into the same d, bit-identical to a fresh call with the noisy flow."""
    seed = 44000 + 13 * G + c
    a, b = _maps(c, h, w, seed)
    if f16:
        a, b = a.astype(np.float16), b.astype(np.float16)
    x, y = dev(a), dev(b)
    wt, bias = _emb(seed + 3)
    W_, B_ = dev(wt), dev(bias)
    f_random, f_noisy = dev(hard_flows("random", 4, G, seed + 4)), dev(hard_flows("noisy", 4, G, seed + 5))
    fresh = host(_ri(G, x, y, f_noisy, W_, B_, r))
    d = _ri(G, x, y, f_random, W_, B_, r)
    again = _ri(G, x, y, f_noisy, W_, B_, r, reuse=d)
    assert again.data_ptr() == d.data_ptr()
    np.testing.assert_array_equal(host(again), fresh)


@pytest.mark.parametrize("c,h,w,G,r", [(32, 112, 112, 64, 4), (64, 56, 56, 32, 6)])
def test_mixed_dtypes_widen_on_the_host(c, h, w, G, r):
    """fp16 x with fp32 y (or the other way round) is widened on the host (ops.refiner_input): bit-identical to the all-fp32 call."""
    seed = 45000 + 13 * G + c
    a, b = _maps(c, h, w, seed)
    a16, b16 = dev(a.astype(np.float16)), dev(b.astype(np.float16))
    fl = dev(hard_flows("noisy", 4, G, seed + 2))
    wt, bias = _emb(seed + 3)
    W_, B_ = dev(wt), dev(bias)
    for x, y in ((a16, dev(b)), (dev(a), b16)):
        np.testing.assert_array_equal(host(_ri(G, x, y, fl, W_, B_, r)), host(_ri(G, x.float(), y.float(), fl, W_, B_, r)))
