"""The flow tail on the GPU -- the four small kernels of gfnet_amd/csrc/grid_ops.hip through which every result leaves the network --
against the float64 oracle, at the shapes and values where they can go wrong: interp_bilinear[_pair]_kernel (the resize between
scales), flow_update_kernel (displacement scaling, eval-time zeroing, carry), match_post_kernel (attenuation, sigmoid, masking, clamp,
warp assembly) and resize_normalize_kernel (the image resize in front of everything).  The inputs and the oracle's own pinning to
torch are in tests/test_flow_tail_cpu.py.

Bounds.  Resize: 4 E32 + 2^-22 max|x|, E32 = max |oracle f32 - oracle f64| on the same input (derived, not tuned: the fp32 class as
tests/test_self_attn_gpu.py forms it); 0, i.e. equality with the float64 oracle, on the identity and on ratio 2 with small-integer
data.  resize_normalise: 4 E32 + 2^-22 max|x| / min(std).  Flow update: 1e-6 and match_post 1e-6 (warp) / 2e-6 (certainty) through
conftest.assert_close, the project's figures for these ops (tests/test_ops_gpu.py), with identical sets of zeroed cells and identical
NaN masks.  Every comparison prints err, bound and their ratio before it asserts.

Before the clamp of match_post_kernel was changed to carry a NaN through as torch.clamp does (model/network.py:371), the hostile
cases of test_match_post_every_image_and_half failed: fminf(fmaxf(nan, -1), 1) is -1, a confident match at the image corner.
"""
import ctypes

import numpy as np
import pytest
import torch

import oracle
import test_flow_tail_cpu as ft
from conftest import assert_close

pytestmark = pytest.mark.gpu

# error / bound on an MI355X, from the figures the tests print before they assert:
MEASURED = """
error / bound, worst case per family:
resize             0.25 (64x64to3x3, 5 planes: err 1.5e-05, bound 6.0e-05); err 0 on the 1 x 1 source and target, the identity, ratio 2.
                   The kernel evaluates the fp32 oracle's own expressions, so err is E32 itself and the ratio stays under 1/4.
resize, exact      0 of 8379 values differ from the float64 oracle; pair == two single calls and the unaligned output bit for bit
resize, non-finite 0.25 (64x64to3x3); NaN masks and infinities equal on all ten shapes
flow update        0.00: err 0 in all 20 three-iteration chains, on the hand-placed cells and over 65540 directions; 0 cells left out
match_post         warp 0.00 (err 0), certainty 0.03 (err 6.0e-08, one ulp of the sigmoid) in all 20 cases and at G = 1500
resize_normalise   0.25 (bilinear 37x53to70x45 in [-1e4, 1e4]: err 2.6e-01, bound 1.05; in [0, 1]: err 1.3e-05, bound 5.3e-05);
                   past the block cap 0.22 (bilinear) and 0.24 (bicubic)
"""


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- a. resize ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ft.RESIZE_SHAPES, ids=ft.shape_id)
def test_resize_against_float64(shape):
    from gfnet_amd import ops

    hw, size = shape
    for BC in ft.RESIZE_PLANES:
        o64, bound, _ = ft.resize_reference("plain", BC, hw, size)
        got = ops.interpolate_bilinear(dev(ft.resize_input(BC, hw)), size)
        assert tuple(got.shape) == (1, BC) + size
        ft.compare_non_finite(host(got), o64, bound, f"resize {ft.shape_id(shape)} x{BC}")


@pytest.mark.parametrize("shape", ft.EXACT_SHAPES, ids=ft.shape_id)
def test_resize_exact_layout(shape):
    """Integers that name their plane, row and column, weights 0 / 1 / 0.25 / 0.75: the result EQUALS the float64 oracle; a swapped
    plane, tap or weight gives another number.  Singly, and as both halves of a pair."""
    from gfnet_amd import ops

    hw, size = shape
    for BC in ft.RESIZE_PLANES:
        o64, bound, e32 = ft.resize_reference("exact", BC, hw, size)
        assert bound > 0 and e32 == 0.0
        x = dev(ft.resize_exact_input(BC, hw))
        got = host(ops.interpolate_bilinear(x, size)).astype(np.float64)
        wrong = got != o64
        print(f"exact {ft.shape_id(shape)} x{BC}: {int(wrong.sum())} of {wrong.size} values differ")
        assert not wrong.any(), np.argwhere(wrong)[:8].tolist()
        if BC > 1:
            a, b = ops.interpolate_bilinear_pair(x[:, :BC // 2].contiguous(), x[:, BC // 2:].contiguous(), size)
            assert np.array_equal(host(torch.cat((a, b), 1)).astype(np.float64), o64)


@pytest.mark.parametrize("shape", [((9, 7), (18, 14)), ((9, 7), (18, 13)), ((13, 17), (7, 5)), ((1, 1), (3, 5))], ids=ft.shape_id)
def test_resize_pair_is_the_two_single_calls(shape):
    """Plane groups of three that lie in the first tensor, in the second, and across both."""
    from gfnet_amd import ops

    hw, size = shape
    for BCa, BCb in ft.PAIR_PLANES:
        a, b = dev(ft.resize_input(BCa, hw)), dev(2 * ft.resize_input(BCb, hw) + 1)
        oa, ob = ops.interpolate_bilinear_pair(a, b, size)
        assert same_bits(oa, ops.interpolate_bilinear(a, size)) and same_bits(ob, ops.interpolate_bilinear(b, size)), (BCa, BCb)


def test_resize_into_an_output_off_the_16_byte_grid():
    """Wo % 4 == 0 and an output base 4 bytes past a 16-byte boundary (only the C ABI can pass one): the kernel must leave the
    16-byte stores, write the same bits, and nothing on either side."""
    from gfnet_amd import _lib, ops

    (H, W), (Ho, Wo), BC, sentinel = (9, 7), (18, 16), 5, -12345.0
    x = dev(ft.resize_input(BC, (H, W)))
    want = ops.interpolate_bilinear(x, (Ho, Wo))
    o64, bound, _ = ft.resize_reference("plain", BC, (H, W), (Ho, Wo))
    ft.compare_non_finite(host(want), o64, bound, "resize 9x7to18x16 aligned")
    n = BC * Ho * Wo
    buf = torch.full((n + 9,), sentinel, device="cuda")
    assert buf.data_ptr() % 16 == 0 and (n * 4) % 16 == 0
    code = _lib.lib().gfn_interp_bilinear_fwd(_lib.ptr(x), ctypes.c_void_p(buf.data_ptr() + 4), BC, H, W, Ho, Wo, _lib.stream_ptr(x.device))
    torch.cuda.synchronize()
    assert code == 0
    assert same_bits(buf[1:1 + n], want.flatten())
    assert float(buf[0]) == sentinel and bool((buf[1 + n:] == sentinel).all())


def test_resize_plane_loop_second_trip():
    """3 * 65535 + 5 planes of 1 x 1 -> 2 x 2: the launch holds 65535 plane groups, the last two groups come from the loop's second
    trip.  Every output is its plane's value (its number: exact in fp32)."""
    from gfnet_amd import ops

    BC = 3 * 65535 + 5
    x = torch.arange(BC, device="cuda", dtype=torch.float32).view(BC, 1, 1, 1)
    want = x.expand(BC, 1, 2, 2)
    assert torch.equal(ops.interpolate_bilinear(x, 2), want)
    k = 100000  # the pair kernel: the boundary between the tensors in the first trip, the tail in the second
    xv, wv = x.view(1, BC, 1, 1), want.reshape(1, BC, 2, 2)
    a, b = ops.interpolate_bilinear_pair(xv[:, :k], xv[:, k:], (2, 2))
    assert torch.equal(a, wv[:, :k]) and torch.equal(b, wv[:, k:])


@pytest.mark.parametrize("shape", ft.RESIZE_SHAPES, ids=ft.shape_id)
def test_resize_spreads_non_finite_cells_like_the_oracle(shape):
    """inf / nan at a corner, on an edge, in the interior: the same NaN mask as the float64 oracle (the 0 * inf of a neighbour that
    reads the cell with weight 0 included), the same infinities, everything else in bound."""
    from gfnet_amd import ops

    hw, size = shape
    o64, bound, _ = ft.resize_reference("nonfinite", ft.NONFINITE_PLANES, hw, size)
    assert not np.isfinite(o64).all()
    x = dev(ft.resize_nonfinite_input(hw))
    got = ops.interpolate_bilinear(x, size)
    ft.compare_non_finite(host(got), o64, bound, f"resize non-finite {ft.shape_id(shape)}")
    a, b = ops.interpolate_bilinear_pair(x[:, :2].contiguous(), x[:, 2:].contiguous(), size)
    assert same_bits(torch.cat((a, b), 1), got)


# ---- b. flow update -------------------------------------------------------------------------------------------------------------
def _three_routes(flow, cert):
    """State (flow, certainty, disp_prev) of the in-place call, the out-of-place call on channel slices and the one on contiguous
    copies.  disp_prev starts as junk: the first iteration must not read it."""
    return [[dev(flow), dev(cert), torch.full(flow.shape, 7.0, device="cuda")] for _ in range(3)]


def _step(routes, d, scale, W0, H0, first):
    """One iteration on all three routes from the refiner output d (B, 3, G, G), embedded in 5-channel tensors whose other channels
    hold 1e30 (batch stride 5 G^2); returns the in-place route's state after asserting that the others hold the same bits."""
    from gfnet_amd import ops

    B, _, G, _ = d.shape
    junk = np.full((B, 1, G, G), 1e30, np.float32)
    d_front, d_mid = dev(np.concatenate((d, junk, junk), 1)), dev(np.concatenate((junk, d, junk), 1))
    kw = dict(zero_small=True, first_iteration=first)
    r = routes
    ops.flow_update_(r[0][0], r[0][1], d_front, r[0][2], scale, W0, H0, **kw)  # channels 0, 1, 2 of 5
    r[1][0], r[1][1] = ops.flow_update(r[1][0], r[1][1], d_mid[:, 1:3], d_mid[:, 3:4], r[1][2], scale, W0, H0, **kw)
    r[2][0], r[2][1] = ops.flow_update(r[2][0], r[2][1], d_mid[:, 1:3].contiguous(), d_mid[:, 3:4].contiguous(), r[2][2], scale, W0, H0, **kw)
    for other in r[1:]:
        assert all(same_bits(a, b) for a, b in zip(r[0], other))
    return [host(t) for t in r[0]]


@pytest.mark.parametrize("scale", ft.FLOW_SCALES)
@pytest.mark.parametrize("W0,H0", ft.FLOW_SIZES)
@pytest.mark.parametrize("G", ft.FLOW_GRIDS)
def test_flow_update_three_iterations_rectangular(G, W0, H0, scale):
    """W0 != H0 throughout; the second iteration zeroes some cells and keeps others, the third meets the stored zeros."""
    flow, cert, deltas = ft.flow_chain_inputs(G)
    chain = ft.oracle_flow_chain(G, scale, W0, H0)
    routes = _three_routes(flow, cert)
    left_out = np.zeros(flow.shape, bool)  # cells the last bit decided in this or an earlier iteration
    worst = 0.0
    for it, (d, (rf, rc, rd, rel)) in enumerate(zip(deltas, chain)):
        gf, gc, gd = _step(routes, d, scale, W0, H0, it == 0)
        near = ft.threshold_cells(rel)
        assert near.mean() <= ft.MAX_EXCLUDED
        left_out |= near
        what = f"flow_update G {G} {W0}x{H0} scale {scale} iteration {it + 1}"
        assert np.array_equal((gd == 0) | left_out, (rd == 0) | left_out), f"{what}: sets of zeroed cells differ"
        errs = [assert_close(np.where(left_out, r, g), r, 1e-6, f"{what} {name}") for name, g, r in (("flow", gf, rf), ("disp", gd, rd))]
        errs.append(assert_close(gc, rc, 1e-6, f"{what} certainty"))
        worst = max(worst, *errs)
        moved = d[:, :2] != 0
        if it > 0:  # both outcomes of the zeroing test, in what the kernel itself stored
            assert ((gd == 0) & moved).any() and ((gd != 0) & moved).any(), what
    print(f"flow_update G {G} {W0}x{H0} scale {scale}: err {worst:.3e} bound 1.0e-06 ratio {worst / 1e-6:.3f}, {int(left_out.sum())} cells left out")


def test_flow_update_hand_placed_previous_displacements():
    """0.0, -0.0, +inf, nan, a denormal and exactly the new value as the previous displacement, 0 against 0, deltas of inf and nan:
    the oracle's zero pattern, NaN mask and infinities, the rest within 1e-6."""
    flow, cert, delta, prev, rows, (scale, W0, H0) = ft.flow_hand_inputs()
    rf, rc, rd = oracle.flow_update(flow, cert, delta[:, :2], delta[:, 2:3], prev, scale, W0, H0)
    routes = _three_routes(flow, cert)
    for r in routes:
        r[2] = dev(prev)
    gf, gc, gd = _step(routes, delta, scale, W0, H0, False)
    assert np.array_equal(gd == 0, rd == 0)
    errs = [ft.close_non_finite(g, r, 1e-6, name) for name, g, r in (("flow", gf, rf), ("certainty", gc, rc), ("disp", gd, rd))]
    print(f"flow_update hand-placed: err {max(errs):.3e} bound 1.0e-06 ratio {max(errs) / 1e-6:.3f}")
    for b in range(ft.FLOW_B):
        p = b % 2
        assert (gd[b, p, rows["same"]] == 0).all() and (gd[b, p, rows["zero"]] != 0).all() and (gd[b, p, rows["neg_zero"]] != 0).all()


def test_flow_update_direction_loop_second_trip():
    """B = 65535 + 5 directions of 2 x 2 cells (both planes of a direction in one block): the last five come from the loop's second
    trip.  Second-iteration form, every value a function of the direction; in place and out of place."""
    B, G, scale, W0, H0 = 65535 + 5, 2, 4, 448, 640
    n = np.arange(B * 3 * G * G, dtype=np.int64).reshape(B, 3, G, G)
    delta = (((n * 7 + 3) % 1999) - 999.5).astype(np.float32) / np.float32(8)  # never 0
    flow = ((((n[:, :2] * 5 + 1) % 2003) - 1001) / 1024.0).astype(np.float32)
    cert = ((((n[:, :1] * 3 + 2) % 1997) - 998) / 256.0).astype(np.float32)
    new = oracle.flow_update(flow, cert, delta[:, :2], delta[:, 2:3], np.full(flow.shape, 1e-7, np.float32), scale, W0, H0)[2]
    plane = n[:, :2] // (G * G)  # 3 b + channel
    prev = np.where((plane // 3 + plane % 3) % 3 == 0, new, np.float32(1.25) * new).astype(np.float32)  # a third of the planes is zeroed
    rf, rc, rd, rel = oracle.flow_update(flow, cert, delta[:, :2], delta[:, 2:3], prev, scale, W0, H0, return_rel=True)
    assert not ft.threshold_cells(rel).any() and (rd[-5:] == 0).any() and (rd[-5:] != 0).any()
    routes = _three_routes(flow, cert)
    for r in routes:
        r[2] = dev(prev)
    gf, gc, gd = _step(routes, delta, scale, W0, H0, False)
    assert np.array_equal(gd == 0, rd == 0)
    errs = [assert_close(g, r, 1e-6, name) for name, g, r in (("flow", gf, rf), ("certainty", gc, rc), ("disp", gd, rd))]
    print(f"flow_update 65540 directions: err {max(errs):.3e} bound 1.0e-06 ratio {max(errs) / 1e-6:.3f}")


# ---- c. match_post --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hostile", [False, True], ids=["plain", "hostile"])
@pytest.mark.parametrize("symmetric,Gc", ft.MP_CASES)
def test_match_post_every_image_and_half(symmetric, Gc, hostile):
    """Three images, both halves of the symmetric warp, with and without cert16 (Gc = 1, 3, G, G + 5): the whole tensors against
    oracle.match_post.  hostile: |flow| == 1 and one ulp above, +-inf, NaN flows (the warp component is NaN and the certainty is
    left alone: torch.clamp, network.py:371), logits of +-100, +-inf and nan, a cert16 with +-inf and nan."""
    from gfnet_amd import ops

    flow, cert, c16 = ft.match_post_inputs(symmetric, Gc, hostile)
    rw, rc = ft.oracle_match_post(flow, cert, c16, symmetric)
    warp, c = ops.match_post(dev(flow), dev(cert), None if c16 is None else dev(c16), symmetric=symmetric)
    gw, gc = host(warp), host(c)
    what = f"match_post {'symmetric' if symmetric else 'one-way'} Gc {Gc} {'hostile' if hostile else 'plain'}"
    ew = ft.close_non_finite(gw, rw, ft.MP_WARP_TOL, what + " warp")
    ec = ft.close_non_finite(gc, rc, ft.MP_CERT_TOL, what + " certainty")
    print(f"{what}: warp err {ew:.3e} bound {ft.MP_WARP_TOL:.1e} ratio {ew / ft.MP_WARP_TOL:.3f}; "
          f"certainty err {ec:.3e} bound {ft.MP_CERT_TOL:.1e} ratio {ec / ft.MP_CERT_TOL:.3f}")
    if hostile:
        ft.check_match_post_properties(gw, gc, flow, cert, symmetric, c16 is not None)


def test_match_post_grid_stride_second_trip():
    """1500 x 3000 cells, 7 % more than one trip of the 16384 x 256 launch serves; data named by (direction, row, column)."""
    from gfnet_amd import ops

    flow, cert, c16 = ft.match_post_large_inputs()
    rw, rc = ft.oracle_match_post(flow, cert, c16, True)
    warp, c = ops.match_post(dev(flow), dev(cert), dev(c16), symmetric=True)
    assert c.numel() > 16384 * 256 and (rc == 0).any()
    ew, ec = assert_close(host(warp), rw, ft.MP_WARP_TOL, "warp"), assert_close(host(c), rc, ft.MP_CERT_TOL, "certainty")
    print(f"match_post 1500: warp err {ew:.3e} ratio {ew / ft.MP_WARP_TOL:.3f}; certainty err {ec:.3e} ratio {ec / ft.MP_CERT_TOL:.3f}")


# ---- d. image resize + normalisation --------------------------------------------------------------------------------------------
def _resize_normalise_case(x5, size, mode, what):
    from gfnet_amd import ops

    o64, bound = ft.rn_reference(x5, size, mode)
    got = ops.resize_normalise(dev(x5), size, mode)  # batch stride 5 H W
    assert same_bits(got, ops.resize_normalise(dev(x5[:, :3]), size, mode)), f"{what}: the extra channels leak"
    err = float(np.abs(host(got).astype(np.float64) - o64).max())
    print(f"{what}: err {err:.3e} bound {bound:.3e} ratio {err / bound:.3f}")
    assert np.isfinite(host(got)).all() and err <= bound, (what, err, bound)


@pytest.mark.parametrize("mode", ["bilinear", "bicubic"])
@pytest.mark.parametrize("hw", ft.RN_SOURCES, ids=ft.shape_id)
def test_resize_normalise_against_float64(hw, mode):
    for rng in ft.RN_RANGES:
        for size in ft.RN_TARGETS + [hw]:
            _resize_normalise_case(ft.rn_input(hw, rng), size, mode, f"resize_normalise {mode} {rng} {ft.shape_id((hw, size))}")


@pytest.mark.parametrize("mode", ["bilinear", "bicubic"])
def test_resize_normalise_past_the_block_cap(mode):
    """2 x 1500 x 1500 output pixels, 7 % more than 16384 blocks of 256 serve in one trip; the two images differ."""
    x5 = ft.rn_input((8, 8), "unit")
    assert not np.array_equal(x5[0], x5[1]) and ft.RN_B * 1500 * 1500 > 16384 * 256
    _resize_normalise_case(x5, (1500, 1500), mode, f"resize_normalise {mode} 8x8to1500x1500")


# ---- e. refusals ----------------------------------------------------------------------------------------------------------------
def test_host_side_refusals():
    """Argument errors answered on the host, before any launch: GFN_ERR_INVALID_ARG and the check's own text."""
    from gfnet_amd import _lib

    L, p = _lib.lib(), _lib.ptr
    buf = [torch.zeros(4096, device="cuda") for _ in range(6)]  # valid, and larger than any of the small shapes below
    s = _lib.stream_ptr(buf[0].device)
    mean, std, std0 = (ctypes.c_float * 3)(0.5, 0.5, 0.5), (ctypes.c_float * 3)(0.2, 0.2, 0.2), (ctypes.c_float * 3)(0.2, 0.0, 0.2)
    G = 4

    def refused(code, text):
        assert code == _lib.ERR_INVALID_ARG and text in L.gfn_last_error(), (code, L.gfn_last_error())

    refused(L.gfn_interp_bilinear_fwd(p(buf[0]), p(buf[1]), 2, 4, 4, 0, 4, s), b"interp_bilinear: bad argument")
    refused(L.gfn_resize_normalize_fwd(p(buf[0]), 3 * 16, p(buf[1]), 1, 4, 4, 8, 8, 2, mean, std, s), b"mode must be")
    refused(L.gfn_resize_normalize_fwd(p(buf[0]), 3 * 16, p(buf[1]), 1, 4, 4, 8, 8, 1, mean, std0, s), b"zero std")
    refused(L.gfn_match_post_fwd(p(buf[0]), p(buf[1]), p(buf[2]), p(buf[3]), p(buf[4]), 1, G, 0, 1, s), b"match_post: bad argument")
    refused(L.gfn_flow_update_out_fwd(p(buf[0]), p(buf[1]), p(buf[2]), p(buf[3]), p(buf[4]), 2 * G * G, p(buf[5]), G * G, p(None), 1, G, 8,
                                      640, 448, 1, 0, s), b"flow_update_out: bad argument")
    big = 46341  # floor(sqrt(2^31)) + 1: the strides are passed large enough that the size check is the one that answers
    refused(L.gfn_flow_update_out_fwd(p(buf[0]), p(buf[1]), p(buf[2]), p(buf[3]), p(buf[4]), 2 * big * big, p(buf[5]), big * big, p(buf[5]),
                                      1, big, 8, 640, 448, 1, 1, s), b"flow_update_out: grid too large")
    torch.cuda.synchronize()
    assert all(float(b.abs().max()) == 0 for b in buf)  # nothing ran
