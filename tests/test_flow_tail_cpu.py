"""The oracle's side of the flow tail (resize between scales, flow update, match_post), pinned to torch on the CPU on the hostile
inputs that tests/test_flow_tail_gpu.py hands to the HIP kernels of gfnet_amd/csrc/grid_ops.hip.  The oracle is the judge there, so
here it is judged first: oracle.interpolate_bilinear against F.interpolate in the same precision, oracle.match_post against a torch
restatement of model/network.py:332-338 + 358-384, oracle.flow_update against tests/test_train_gpu.py's restatement of
model/network.py:262-268 run in float32.  The builders of those inputs live in this file and the GPU file imports them, so both see
the same arrays.  Where a reference holds a NaN the NaN masks are compared for equality and the other values separately
(conftest.assert_close cannot pass on a NaN)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import oracle
import synth
from conftest import assert_close

INF, NAN = float("inf"), float("nan")

# ---- resize ---------------------------------------------------------------------------------------------------------------------
# (H, W) -> (Ho, Wo): a 1 x 1 source and a 1 x 1 target; down, a 3-wide target, the identity; ratio 2; Wo % 4 = 3, 2, 1 (and 0 above);
# a source 64 / 3 times the target
RESIZE_SHAPES = [((1, 1), (3, 5)), ((13, 17), (1, 1)), ((13, 17), (7, 5)), ((13, 17), (40, 3)), ((5, 9), (5, 9)), ((6, 6), (12, 12)),
                 ((9, 7), (18, 15)), ((9, 7), (18, 14)), ((9, 7), (18, 13)), ((64, 64), (3, 3))]
RESIZE_PLANES = (1, 2, 4, 5, 7)  # the kernel serves planes in groups of three: one ragged group, two groups, a ragged second and third
EXACT_SHAPES = [((5, 9), (5, 9)), ((6, 6), (12, 12)), ((9, 7), (18, 14))]  # the identity and ratio 2: weights 0, 1, 0.25, 0.75
PAIR_PLANES = [(1, 1), (4, 2), (2, 4), (3, 3), (6, 1)]


def shape_id(s):
    """(13, 17) -> '13x17', ((13, 17), (7, 5)) -> '13x17to7x5'"""
    return "to".join(shape_id(p) for p in s) if isinstance(s[0], tuple) else "x".join(map(str, s))


@functools.lru_cache(maxsize=None)
def resize_input(BC, hw):
    """(1, BC, H, W) float32, bell-shaped values on a 2^-12 lattice."""
    return synth.lattice_normalish((1, BC) + hw, 1000 * BC + 10 * hw[0] + hw[1])


@functools.lru_cache(maxsize=None)
def resize_exact_input(BC, hw):
    """Small integers that name their plane, row and column: 10000 (plane + 1) + 100 row + column.  With weights that are
    multiples of 1/4 on each axis every product and every sum is exact in fp32, so a swapped plane, row, column or tap is another
    number and not a rounding."""
    H, W = hw
    p, r, c = np.meshgrid(np.arange(BC), np.arange(H), np.arange(W), indexing="ij")
    return (10000.0 * (p + 1) + 100.0 * r + c).astype(np.float32)[None]


NONFINITE_PLANES = 5


@functools.lru_cache(maxsize=None)
def resize_nonfinite_input(hw):
    """Five planes with one non-finite cell each: inf at the first corner, nan on the top edge, -inf in the interior, nan at the last
    corner, inf on the left edge.  A neighbour that reads such a cell with weight 0 turns into nan (0 * inf) as well."""
    H, W = hw
    x = resize_input(NONFINITE_PLANES, hw).copy()
    x[0, 0, 0, 0] = INF
    x[0, 1, 0, W // 2] = NAN
    x[0, 2, H // 2, W // 2] = -INF
    x[0, 3, H - 1, W - 1] = NAN
    x[0, 4, H // 2, 0] = INF
    return x


def finite_max(x):
    x = np.asarray(x, np.float64)
    f = np.isfinite(x)
    return float(np.abs(x[f]).max()) if f.any() else 0.0


@functools.lru_cache(maxsize=None)
def resize_reference(kind, BC, hw, size):
    """(oracle in float64, bound) for one resize case, computed once.  Bound, derived and not tuned, formed as
    tests/test_self_attn_gpu.py forms its fp32 class: E32 = max |oracle f32 - oracle f64| on the same input (over the cells where
    both are finite), times 4 for another order of the four products, plus 2^-22 max|x| (two roundings of a result of the input's
    size)."""
    x = {"plain": resize_input, "exact": resize_exact_input}[kind](BC, hw) if kind != "nonfinite" else resize_nonfinite_input(hw)
    o64 = oracle.interpolate_bilinear(x, size, "f64")
    o32 = oracle.interpolate_bilinear(x, size, "f32").astype(np.float64)
    both = np.isfinite(o64) & np.isfinite(o32)
    e32 = float(np.abs(o32 - o64)[both].max()) if both.any() else 0.0
    return o64, 4 * e32 + 2.0 ** -22 * finite_max(x), e32


def finite_part(got, ref, what):
    """(got, ref) in float64 with the non-finite cells of ref set to 0 in both, after asserting that the NaN masks are equal and the
    infinities are equal, sign included."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, f"{what}: shape {got.shape} vs {ref.shape}"
    gn, rn = np.isnan(got), np.isnan(ref)
    assert np.array_equal(gn, rn), f"{what}: NaN masks differ at {np.argwhere(gn != rn)[:8].tolist()}"
    ri = np.isinf(ref)
    assert np.array_equal(np.isinf(got), ri) and np.array_equal(got[ri], ref[ri]), \
        f"{what}: infinities differ at {np.argwhere((np.isinf(got) != ri) | (ri & (got != ref)))[:8].tolist()}"
    fin = ~rn & ~ri
    return np.where(fin, got, 0.0), np.where(fin, ref, 0.0)


def compare_non_finite(got, ref, bound, what):
    """NaN masks and infinities equal, every other value within `bound` (absolute).  Prints err, bound and their ratio before it
    asserts; returns err."""
    got, ref = finite_part(got, ref, what)
    err = np.abs(got - ref)
    worst = float(err.max()) if err.size else 0.0
    print(f"{what}: err {worst:.3e} bound {bound:.3e} ratio {worst / bound if bound else float(worst > 0):.3f}")
    assert worst <= bound, f"{what}: err {worst:.3e} > bound {bound:.3e} at {np.unravel_index(err.argmax(), err.shape)}"
    return worst


def close_non_finite(got, ref, tol, what):
    """NaN masks and infinities equal, conftest.assert_close on every other value."""
    return assert_close(*finite_part(got, ref, what), tol, what)


def _torch_interp(x, size, dtype):
    return F.interpolate(torch.from_numpy(x).to(dtype), size=size, mode="bilinear", align_corners=False).numpy()


def zero_weight_by_rounding(x, size):
    """(1, BC, Ho, Wo) mask of the outputs on which torch's CPU resize and the oracle may differ in a NaN for no fault of either.
    Where an output's source coordinate (o + 0.5) n_in / n_out - 0.5 is a non-negative integer in exact arithmetic, its second tap
    has weight 0 -- exactly 0 as the oracle and the HIP kernels evaluate it (multiply, then subtract; both are built without
    contraction), one rounding error of the ratio as torch's CPU build evaluates it (a fused multiply-add), and at equal sizes
    torch's CPU path reads the same cell twice (weights 1 and 0) where the general form reads the neighbour.  0 * inf is nan and
    1e-8 * inf is inf, so an output of that kind with a non-finite cell within one cell of its source is left out of the
    comparison with torch.  A weight of 0 from the clamp at the border (f < 0) is 0 for everybody and stays in."""
    _, BC, H, W = x.shape
    Ho, Wo = size
    bad = ~np.isfinite(x[0])
    pad = np.pad(bad, ((0, 0), (1, 1), (1, 1)))
    near = np.zeros_like(bad)
    for dy in range(3):
        for dx in range(3):
            near |= pad[:, dy:dy + H, dx:dx + W]

    def axis(n_in, n_out):
        num = (2 * np.arange(n_out) + 1) * n_in - n_out  # f = num / (2 n_out)
        return (num >= 0) & (num % (2 * n_out) == 0), np.clip(np.floor(np.maximum(num, 0) / (2 * n_out) + 0.5).astype(int), 0, n_in - 1)

    (ey, iy), (ex, ix) = axis(H, Ho), axis(W, Wo)
    return (near[:, iy][:, :, ix] & (ey[:, None] | ex[None, :]))[None]


@pytest.mark.parametrize("shape", RESIZE_SHAPES, ids=shape_id)
@pytest.mark.parametrize("variant,dtype,eps", [("f32", torch.float32, 2.0 ** -24), ("f64", torch.float64, 2.0 ** -53)])
def test_oracle_interpolate_bilinear_is_torchs(shape, variant, dtype, eps):
    """Same precision, same expressions: at most a few roundings of a value of the input's size apart (16 eps max|x|: the source
    coordinate may round to the other side of a cell edge in one of them, where the two forms meet within an ulp of it)."""
    hw, size = shape
    for BC in RESIZE_PLANES:
        x = resize_input(BC, hw)
        got, want = oracle.interpolate_bilinear(x, size, variant), _torch_interp(x, size, dtype)
        assert got.dtype == want.dtype
        compare_non_finite(got, want, 16 * eps * float(np.abs(x).max()), f"{variant} {BC} planes")
    x = resize_nonfinite_input(hw)
    got, want = oracle.interpolate_bilinear(x, size, variant), _torch_interp(x, size, dtype)
    assert not np.isfinite(got).all()
    skip = zero_weight_by_rounding(x, size)
    assert not skip.any() or shape not in EXACT_SHAPES[1:]  # ratio 2 has no such output: every cell is compared
    compare_non_finite(np.where(skip, 0, got), np.where(skip, 0, want), 16 * eps * finite_max(x), f"{variant} non-finite")


@pytest.mark.parametrize("shape", RESIZE_SHAPES, ids=shape_id)
def test_non_finite_cells_spread_alike_in_both_precisions(shape):
    """The GPU test compares the fp32 kernel's NaN mask with the float64 oracle's.  That is a fair demand only where the precision
    does not decide whether a weight is exactly 0: on these inputs the fp32 and the float64 oracle have the same mask."""
    hw, size = shape
    x = resize_nonfinite_input(hw)
    o32, o64 = oracle.interpolate_bilinear(x, size, "f32"), oracle.interpolate_bilinear(x, size, "f64")
    assert np.array_equal(np.isnan(o32), np.isnan(o64))
    assert np.array_equal(np.isinf(o32), np.isinf(o64))


@pytest.mark.parametrize("shape", EXACT_SHAPES, ids=shape_id)
def test_exact_resize_data_is_exact(shape):
    hw, size = shape
    o64, bound, e32 = resize_reference("exact", 7, hw, size)
    assert e32 == 0.0 and np.array_equal(o64, _torch_interp(resize_exact_input(7, hw), size, torch.float64))
    assert np.array_equal(o64.astype(np.float32).astype(np.float64), o64)


# ---- flow update ----------------------------------------------------------------------------------------------------------------
FLOW_B = 3
FLOW_GRIDS = (1, 17)  # 17^2 = 289 cells: a second, ragged 256-thread block
FLOW_SIZES = ((640, 448), (448, 640))  # (W0, H0), never square: dx is divided by 4 W0 and dy by 4 H0
FLOW_SCALES = (1, 2, 4, 8, 16)
REL_STEPS = (0.0, 2.0 ** -22, 4e-6)  # the second and third delta against the one before, per cell: equal, below 1e-6, above it
THRESHOLD_BAND = 2.0 ** -18  # a cell whose rel lies this close (relative) to 1e-6 is decided by the last bit: excluded
MAX_EXCLUDED = 0.01


@functools.lru_cache(maxsize=None)
def flow_chain_inputs(G):
    """flow, certainty and the refiner outputs (B, 3, G, G) of three iterations.  Iteration 2 and 3 repeat the delta before them
    times (1 + step), the step picked per cell from REL_STEPS by the cell's index, so the eval-time zeroing (network.py:264-265)
    fires on two thirds of the cells of iteration 2 and the third iteration meets stored zeros (x / 0), cells that repeat again and
    cells that moved.  One displacement per direction is 0 throughout (0 / 0 in the third iteration) where the grid has room."""
    B = FLOW_B
    flow = synth.lattice_uniform((B, 2, G, G), 201 + G)
    cert = synth.lattice_uniform((B, 1, G, G), 202 + G)
    d1 = 30 * synth.lattice_uniform((B, 3, G, G), 203 + G)
    d1[:, :2][d1[:, :2] == 0] = 0.5  # a zero only where it is placed
    if G > 1:
        d1[:, 0, 2, 3] = 0.0
        d1[:, 1, G - 1, G - 1] = 0.0
    idx = np.arange(B * 2 * G * G).reshape(B, 2, G, G)
    deltas = [d1]
    for pick in (idx % 3, (idx // 3 * 2) % 3):
        d = deltas[-1].copy()
        step = np.asarray(REL_STEPS)[pick]
        d[:, :2] = (d[:, :2].astype(np.float64) * (1.0 + step)).astype(np.float32)
        d[:, 2] = synth.lattice_uniform((B, G, G), 204 + len(deltas))
        deltas.append(d)
    return flow, cert, deltas


def oracle_flow_chain(G, scale, W0, H0):
    """[(flow, certainty, displacement, rel)] of the three iterations, the oracle fed with its own results."""
    flow, cert, deltas = flow_chain_inputs(G)
    prev = np.full(flow.shape, 1e-7, np.float32)  # network.py:256
    out = []
    for d in deltas:
        flow, cert, prev, rel = oracle.flow_update(flow, cert, d[:, :2], d[:, 2:3], prev, scale, W0, H0, return_rel=True)
        out.append((flow, cert, prev, rel))
    return out


def threshold_cells(rel):
    """The cells of the zeroing test that the last bit decides: rel within THRESHOLD_BAND (relative) of 1e-6."""
    with np.errstate(invalid="ignore"):
        return np.abs(np.asarray(rel, np.float64) - 1e-6) <= THRESHOLD_BAND * 1e-6


@functools.lru_cache(maxsize=None)
def flow_hand_inputs():
    """G = 17, B = 3, second-iteration form: every previous displacement is the oracle's first-iteration result except the hand-placed
    cells, one kind per row of direction b, plane b % 2: 0.0, -0.0, +inf, nan, a denormal, exactly the new value, a new
    displacement of 0 against a previous 0, and deltas of inf and nan (against an ordinary previous displacement).
    Returns (flow, cert, delta, prev, cells) with cells = {name: (row, expected outcome)}."""
    G, B, scale, W0, H0 = 17, FLOW_B, 8, 640, 448
    flow, cert, deltas = flow_chain_inputs(G)
    delta = deltas[0].copy()
    delta[:, :2, :12] = np.where(delta[:, :2, :12] == 0, np.float32(0.5), delta[:, :2, :12])
    new = oracle.flow_update(flow, cert, delta[:, :2], delta[:, 2:3], np.full(flow.shape, 1e-7, np.float32), scale, W0, H0)[2]
    prev = (new * np.float32(1.5)).astype(np.float32)
    rows = {"zero": 0, "neg_zero": 1, "inf": 2, "nan": 3, "denormal": 4, "same": 5, "zero_zero": 6, "delta_inf": 7, "delta_nan": 8}
    for b in range(B):
        p = b % 2
        prev[b, p, 0] = 0.0
        prev[b, p, 1] = -0.0
        prev[b, p, 2] = INF
        prev[b, p, 3] = NAN
        prev[b, p, 4] = np.float32(1e-40)
        prev[b, p, 5] = new[b, p, 5]
        prev[b, p, 6] = 0.0
        delta[b, p, 6] = 0.0
        delta[b, p, 7, ::2] = INF
        delta[b, p, 7, 1::2] = -INF
        delta[b, p, 8] = NAN
        delta[b, 2, 9, b] = NAN  # the certainty increment
        delta[b, 2, 10, b] = -INF
    return flow, cert, delta, prev, rows, (scale, W0, H0)


def restated_flow_update(flow, cert, d_flow, d_cert, prev, scale, W0, H0, zero_small):
    from test_train_gpu import restated_flow_update as restated  # model/network.py:262-268

    return restated(flow, cert, d_flow, d_cert, prev, scale, W0, H0, zero_small)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_bits(got, want, what):
    """Bit-equal float32, any NaN counting as equal to any NaN (numpy and torch may pick different payloads)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float32 and want.dtype == np.float32, what
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), f"{what}: NaN masks differ"
    assert np.array_equal(_bits(np.where(gn, 0, got)), _bits(np.where(wn, 0, want))), f"{what}: bits differ"


@pytest.mark.parametrize("G", FLOW_GRIDS)
@pytest.mark.parametrize("W0,H0", FLOW_SIZES)
def test_oracle_flow_update_is_the_restatement_in_float32(G, W0, H0):
    flow, cert, deltas = flow_chain_inputs(G)
    for scale in FLOW_SCALES:
        chain = oracle_flow_chain(G, scale, W0, H0)
        f, c, prev = _t(flow), _t(cert), 1e-7
        for it, (d, (rf, rc, rd, rel)) in enumerate(zip(deltas, chain)):
            f, c, prev = restated_flow_update(f, c, _t(d[:, :2]), _t(d[:, 2:3]), prev, scale, W0, H0, True)
            what = f"G {G} {W0}x{H0} scale {scale} iteration {it + 1}"
            assert np.array_equal(prev.numpy() == 0, rd == 0), f"{what}: zero pattern"
            _same_bits(rd, prev.numpy(), what + " displacement")
            _same_bits(rf, f.numpy(), what + " flow")
            _same_bits(rc, c.numpy(), what + " certainty")
            # the share of cells that the last bit decides stays inside the cap, so the GPU test may exclude them
            assert threshold_cells(rel).mean() <= MAX_EXCLUDED, what
        # the chain is worth its name: iteration 2 zeroes some cells and keeps others, iteration 3 meets stored zeros and does both again
        d2, d3 = chain[1][2], chain[2][2]
        moved2, moved3 = deltas[1][:, :2] != 0, deltas[2][:, :2] != 0
        assert ((d2 == 0) & moved2).any() and ((d2 != 0) & moved2).any()
        stored_zero = (d2 == 0) & moved3
        assert (stored_zero & (d3 != 0)).any(), "x / 0 is never below the threshold"
        assert not (stored_zero & (d3 == 0)).any()
        if G > 1:
            assert ((d2 != 0) & (d3 == 0)).any() and ((d2 != 0) & (d3 != 0)).any()
            assert ((d2 == 0) & ~moved3).any()  # 0 / 0


def test_oracle_flow_update_on_hand_placed_cells():
    flow, cert, delta, prev, rows, (scale, W0, H0) = flow_hand_inputs()
    rf, rc, rd = oracle.flow_update(flow, cert, delta[:, :2], delta[:, 2:3], prev, scale, W0, H0)
    tf, tc, td = restated_flow_update(_t(flow), _t(cert), _t(delta[:, :2]), _t(delta[:, 2:3]), _t(prev), scale, W0, H0, True)
    _same_bits(rd, td.numpy(), "displacement")
    _same_bits(rf, tf.numpy(), "flow")
    _same_bits(rc, tc.numpy(), "certainty")
    new = oracle.flow_update(flow, cert, delta[:, :2], delta[:, 2:3], np.full(flow.shape, 1e-7, np.float32), scale, W0, H0)[2]
    for b in range(FLOW_B):
        p = b % 2
        for name in ("zero", "neg_zero", "inf", "nan", "denormal"):  # never zeroed: rel is inf or nan
            assert np.array_equal(rd[b, p, rows[name]], new[b, p, rows[name]]) and (rd[b, p, rows[name]] != 0).all(), name
        assert (rd[b, p, rows["same"]] == 0).all() and (new[b, p, rows["same"]] != 0).all()
        assert (rd[b, p, rows["zero_zero"]] == 0).all()
        assert np.isinf(rd[b, p, rows["delta_inf"]]).all() and np.isnan(rd[b, p, rows["delta_nan"]]).all()
        assert np.isnan(rf[b, p, rows["delta_nan"]]).all() and np.isnan(rc[b, 0, 9, b]) and rc[b, 0, 10, b] == -INF


# ---- match_post -----------------------------------------------------------------------------------------------------------------
MP_IMAGES, MP_G = 3, 6
MP_GC = (1, 3, MP_G, MP_G + 5)
UP, DOWN = np.nextafter(np.float32(1), np.float32(2)), np.nextafter(np.float32(-1), np.float32(-2))
# (row, column) -> (flow x, flow y): the cells of every direction that sit on the rule's edges (network.py:368-371)
MP_BOUNDARY = {(0, 0): (1.0, 0.25), (0, 1): (-0.5, -1.0), (0, 2): (1.0, -1.0),           # |flow| == 1: certainty kept, warp +-1
               (1, 0): (UP, 0.25), (1, 1): (0.5, DOWN), (1, 2): (DOWN, UP),               # one ulp outside: certainty 0, warp +-1
               (2, 0): (INF, 0.0), (2, 1): (0.25, -INF), (2, 2): (-INF, INF),             # certainty 0, warp +-1
               (3, 0): (NAN, 2.0), (3, 1): (-2.0, NAN)}                                   # out of range beside a NaN: certainty 0
MP_NAN_FLOW = {(4, 0): (NAN, 0.5), (4, 1): (-0.25, NAN), (4, 2): (NAN, NAN), (4, 3): (NAN, 1.0)}  # warp NaN, certainty untouched
MP_LOGITS = {(5, 0): 100.0, (5, 1): -100.0, (5, 2): INF, (5, 3): -INF, (5, 4): NAN}


@functools.lru_cache(maxsize=None)
def match_post_inputs(symmetric, Gc, hostile):
    """(flow (nb,2,G,G), certainty logits (nb,1,G,G), cert16 (nb,1,Gc,Gc) or None); nb = 6 directions of 3 images when symmetric.
    plain: flows over +-1.2, so about a sixth of the components lie outside.  hostile: the cells above in EVERY direction, and a
    cert16 with +inf (0.5 * inf * 0 = nan in network.py:338), -inf and nan in directions 0, 1 and 2 (and again from the far end)."""
    nb, G = MP_IMAGES * (2 if symmetric else 1), MP_G
    seed = 300 + 10 * Gc + symmetric
    flow = (1.2 * synth.lattice_uniform((nb, 2, G, G), seed)).astype(np.float32)
    cert = (3 * synth.lattice_normalish((nb, 1, G, G), seed + 1)).astype(np.float32)
    c16 = None if Gc == 0 else (3 * synth.lattice_normalish((nb, 1, Gc, Gc), seed + 2)).astype(np.float32)
    if hostile:
        flow[:, :, :5, :4] *= np.float32(0.5)  # the hand-placed cells' neighbours stay ordinary
        for (i, j), (fx, fy) in {**MP_BOUNDARY, **MP_NAN_FLOW}.items():
            flow[:, 0, i, j], flow[:, 1, i, j] = fx, fy
        flow[:, :, 5] *= np.float32(0.5)  # in range: the certainty of row 5 is the sigmoid's
        for (i, j), v in MP_LOGITS.items():
            cert[:, 0, i, j] = v
        if c16 is not None:
            for k, v in enumerate((INF, -INF, NAN)):
                c16[k, 0, 0, 0] = v
                c16[nb - 1 - k, 0, Gc - 1, Gc // 2] = v
    return flow, cert, c16


def restated_match_post(flow, certainty, cert16, symmetric):
    """model/network.py:332-338 (the attenuation by the scale-16 certainty) and :358-384, batched=True, on torch tensors"""
    G = flow.shape[-1]
    B = flow.shape[0] // 2 if symmetric else flow.shape[0]
    if cert16 is not None:
        low_res_certainty = F.interpolate(cert16, size=(G, G), align_corners=False, mode="bilinear")  # :333-335
        low_res_certainty = 0.5 * low_res_certainty * (low_res_certainty < 0)                          # :336-338
    flow = flow.permute(0, 2, 3, 1).reshape(-1, G, G, 2)                                               # :359
    certainty = certainty - (low_res_certainty if cert16 is not None else 0)                           # :360
    certainty = certainty.sigmoid()                                                                    # :361
    lin = torch.linspace(-1 + 1 / G, 1 - 1 / G, G)
    grid = torch.stack(torch.meshgrid(lin, lin, indexing="xy"), dim=-1).float().expand(B, G, G, 2)     # :362-367
    if (flow.abs() > 1).any():                                                                         # :368-370
        wrong = (flow.abs() > 1).sum(dim=-1) > 0
        certainty[wrong[:, None]] = 0
    flow = torch.clamp(flow, -1, 1)                                                                    # :371
    if symmetric:                                                                                      # :373-378
        A_to_B, B_to_A = flow.chunk(2)
        q_warp = torch.cat((grid, A_to_B), dim=-1)
        s_warp = torch.cat((B_to_A, grid), dim=-1)
        warp = torch.cat((q_warp, s_warp), dim=2)
        certainty = torch.cat(certainty.chunk(2), dim=3)
    else:
        warp = torch.cat((grid, flow), dim=-1)                                                         # :380
    return warp, certainty[:, 0]                                                                       # :382


MP_WARP_TOL, MP_CERT_TOL = 1e-6, 2e-6  # the project's figures for this op (tests/test_ops_gpu.py::test_g6_golden_match_post)
MP_CASES = [(s, gc) for s in (True, False) for gc in (0,) + MP_GC]


def oracle_match_post(flow, cert, c16, symmetric):
    return oracle.match_post(flow, cert, c16, symmetric=symmetric, attenuate_cert=c16 is not None)


def check_match_post_properties(warp, cert, flow, logits, symmetric, attenuated):
    """What the hand-placed cells must give in EVERY direction, stated without the oracle (warp (B,G,Gw,4), cert (B,G,Gw))."""
    warp, cert = np.asarray(warp), np.asarray(cert)
    B, G = MP_IMAGES, MP_G
    for d in range(flow.shape[0]):
        b, second = d % B, d >= B
        w = warp[b, :, G:] if second else warp[b, :, :G]
        c = cert[b, :, G:] if second else cert[b, :, :G]
        fl = w[..., :2] if second else w[..., 2:]  # the B->A half carries the flow first (network.py:376)
        for (i, j), (fx, fy) in MP_BOUNDARY.items():
            for got, v in zip(fl[i, j], (fx, fy)):
                assert np.isnan(got) if np.isnan(v) else got == np.sign(v) * min(abs(v), 1.0), (d, i, j)
            if i == 0 and not attenuated:
                assert c[i, j] == pytest.approx(1 / (1 + np.exp(-np.float64(logits[d, 0, i, j]))), abs=MP_CERT_TOL), (d, i, j)
            if i == 0:
                assert c[i, j] > 0 or attenuated, (d, i, j)
            else:
                assert c[i, j] == 0, (d, i, j)
        for (i, j), (fx, fy) in MP_NAN_FLOW.items():
            for got, v in zip(fl[i, j], (fx, fy)):
                assert np.isnan(got) if np.isnan(v) else got == np.float32(v), (d, i, j)
            if not attenuated:
                assert c[i, j] == pytest.approx(1 / (1 + np.exp(-np.float64(logits[d, 0, i, j]))), abs=MP_CERT_TOL), (d, i, j)
        if not attenuated:
            got = [c[i, j] for (i, j) in MP_LOGITS]
            assert got[0] == 1 and got[1] == pytest.approx(0, abs=1e-30) and got[2] == 1 and got[3] == 0 and np.isnan(got[4]), d


@pytest.mark.parametrize("symmetric,Gc", MP_CASES)
@pytest.mark.parametrize("hostile", [False, True])
def test_oracle_match_post_is_the_restatement(symmetric, Gc, hostile):
    flow, cert, c16 = match_post_inputs(symmetric, Gc, hostile)
    warp, c = oracle_match_post(flow, cert, c16, symmetric)
    tw, tc = restated_match_post(_t(flow), _t(cert), None if c16 is None else _t(c16), symmetric)
    assert warp.dtype == np.float32 and c.dtype == np.float32 and warp.shape == tuple(tw.shape) and c.shape == tuple(tc.shape)
    close_non_finite(warp, tw.numpy(), MP_WARP_TOL, "warp")
    skip = np.zeros(c.shape, bool)
    if c16 is not None:  # Gc == G with a non-finite cert16: torch's CPU resize copies at equal size (zero_weight_by_rounding)
        s = zero_weight_by_rounding(c16.reshape((1, -1) + c16.shape[2:]), (MP_G, MP_G))[0]
        skip = np.concatenate((s[:MP_IMAGES], s[MP_IMAGES:]), axis=2) if symmetric else s
        assert not skip.any() or (hostile and Gc == MP_G)
    close_non_finite(np.where(skip, 0, c), np.where(skip, 0, tc.numpy()), MP_CERT_TOL, "certainty")
    if hostile:
        assert np.isnan(warp).any() and np.isnan(c).any()
        check_match_post_properties(warp, c, flow, cert, symmetric, c16 is not None)
        check_match_post_properties(tw.numpy(), tc.numpy(), flow, cert, symmetric, c16 is not None)
    else:
        assert np.isfinite(warp).all() and np.isfinite(c).all() and (c == 0).any() and (c > 0).any()


def match_post_large_inputs():
    """One image, G = 1500, symmetric: 1500 x 3000 = 4.5 M cells, more than the 16384 x 256 that one trip of the kernel's grid-stride
    loop serves.  Flow and logits are functions of (direction, row, column) with periods that divide neither the grid row nor the
    launch (4194304 cells), so a cell served by the wrong trip, row or direction carries another value."""
    G, Gc = 1500, 7
    d, i, j = np.meshgrid(np.arange(2), np.arange(G), np.arange(G), indexing="ij")
    n = (d * 1000003 + i * 1009 + j * 7).astype(np.int64)
    flow = np.stack((((n % 4093) - 2046) / 2000.0, (((n * 3 + 17) % 4091) - 2045) / 2000.0), axis=1).astype(np.float32)
    cert = ((((n * 5 + 3) % 4099) - 2049) / 512.0).astype(np.float32)[:, None]
    c16 = (3 * synth.lattice_normalish((2, 1, Gc, Gc), 399)).astype(np.float32)
    return flow, cert, c16


# ---- image resize + normalisation ----------------------------------------------------------------------------------------------
RN_SOURCES = [(1, 9), (9, 1), (2, 2), (37, 53)]  # one pixel high or wide: every bicubic tap of that axis clamps
RN_TARGETS = [(8, 8), (1, 1), (70, 45)]
RN_RANGES = ("unit", "1e4")
RN_B = 2
RN_JUNK = 1e30  # what the two extra channels of the 5-channel source hold


@functools.lru_cache(maxsize=None)
def rn_input(hw, rng, B=RN_B):
    """(B, 5, H, W): three image channels in [0, 1] or [-1e4, 1e4] (batch-dependent), two channels of 1e30 behind them."""
    u = synth.lattice_uniform((B, 3) + hw, 500 + 7 * hw[0] + hw[1])
    x = (0.5 * (u + 1)) if rng == "unit" else (1e4 * u)
    return np.concatenate((x.astype(np.float32), np.full((B, 2) + hw, RN_JUNK, np.float32)), axis=1)


def rn_reference(x5, size, mode):
    """(oracle f64, bound): E32 = max |oracle f32 - oracle f64| on the same input; 4 E32 + 2^-22 max|x| / min(std)."""
    o64 = oracle.resize_normalise(x5, size, mode, "f64")
    e32 = float(np.abs(oracle.resize_normalise(x5, size, mode, "f32").astype(np.float64) - o64).max())
    return o64, 4 * e32 + 2.0 ** -22 * float(np.abs(x5[:, :3]).max()) / min(oracle.IMAGENET_STD)


@pytest.mark.parametrize("hw", RN_SOURCES, ids=shape_id)
@pytest.mark.parametrize("mode", ["bilinear", "bicubic"])
def test_oracle_resize_normalise_is_torchs(hw, mode):
    """In float64, where the order of the sums does not show: F.interpolate(antialias=False) and (x - mean) / std on the first
    three channels; a target of the source's own size leaves the image untouched."""
    mean = torch.tensor(oracle.IMAGENET_MEAN, dtype=torch.float64).view(1, 3, 1, 1)
    std = torch.tensor(oracle.IMAGENET_STD, dtype=torch.float64).view(1, 3, 1, 1)
    for rng in RN_RANGES:
        x5 = rn_input(hw, rng)
        for size in RN_TARGETS + [hw]:
            x = torch.from_numpy(x5[:, :3]).double()
            kw = {} if mode == "bilinear" else {"antialias": False}
            y = x if size == hw else F.interpolate(x, size=size, mode=mode, align_corners=False, **kw)
            want = ((y - mean) / std).numpy()
            got, bound = rn_reference(x5, size, mode)
            err = float(np.abs(got - want).max())
            assert err <= 2.0 ** -40 * float(np.abs(x5[:, :3]).max()) / min(oracle.IMAGENET_STD), (rng, size, err)
            assert np.isfinite(bound) and bound < 1e-2 * max(1.0, float(np.abs(want).max()))  # nothing of the 1e30 in it
