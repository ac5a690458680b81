"""The fused last-update-of-a-scale + resize (ops.flow_update_resize, gfn_flow_update_resize_fwd) against what it replaces:
ops.flow_update followed by ops.interpolate_bilinear_pair on the same inputs.  All four outputs and disp_prev must be equal
bit for bit (torch.equal; the non-finite case compares the bit patterns, since nan != nan).  Shapes are the smallest at which
the tiled kernel can go wrong: one ragged tile (5 -> 10), full tiles plus a one-cell-wide tile on an odd pitch without 16-byte
stores (33 -> 66), a multiple of 8 that is no multiple of the 16-cell tile (40 -> 80), and the ratio-1 transition (32 -> 32).
The stand-alone resize kernels are checked against torch's F.interpolate to the tolerance of the existing resize tests (1e-6)
and against each other exactly."""
import pytest
import torch
import torch.nn.functional as F

from conftest import assert_close

pytestmark = pytest.mark.gpu

B, SCALE, W0, H0 = 3, 8, 448, 448
SHAPES = [(5, 10), (33, 66), (40, 80), (32, 32)]


def _inputs(G, seed, sliced):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    flow = torch.rand((B, 2, G, G), device="cuda", generator=gen) * 2 - 1
    cert = torch.randn((B, 1, G, G), device="cuda", generator=gen)
    d = torch.randn((B, 5, G, G), device="cuda", generator=gen) * 30  # displacements of a few hundredths, in normalised units
    if sliced:  # the refiner's outputs as channel slices of one tensor: batch stride 5 G^2, not 2 G^2 / G^2
        return flow, cert, d[:, 1:3], d[:, 3:4]
    return flow, cert, d[:, 1:3].contiguous(), d[:, 3:4].contiguous()


def _disp_prev(d_flow, seed):
    """A previous displacement that sends cells into every branch of the zeroing test: a third equal to the new displacement
    (zeroed), a third 0 (x / 0: never zeroed), the rest unrelated."""
    div = torch.tensor([4.0 * W0, 4.0 * H0], device="cuda").view(1, 2, 1, 1)
    new = float(SCALE) * (d_flow / div)  # network.py:262-263, the kernel's own fp32 expression
    gen = torch.Generator(device="cuda").manual_seed(seed)
    pick = torch.randint(0, 3, new.shape, device="cuda", generator=gen)
    other = torch.randn(new.shape, device="cuda", generator=gen) * 0.01
    return torch.where(pick == 0, new, torch.where(pick == 1, torch.zeros_like(new), other)).contiguous()


def _both(flow, cert, d_flow, d_cert, prev, G_next, zero_small, first):
    from gfnet_amd import ops

    p_ref = None if prev is None else prev.clone()
    p_got = None if prev is None else prev.clone()
    fo, co = ops.flow_update(flow, cert, d_flow, d_cert, p_ref, SCALE, W0, H0, zero_small=zero_small, first_iteration=first)
    fn, cn = ops.interpolate_bilinear_pair(fo, co, G_next)
    got = ops.flow_update_resize(flow, cert, d_flow, d_cert, p_got, SCALE, W0, H0, G_next, zero_small=zero_small, first_iteration=first)
    torch.cuda.synchronize()
    return (fo, co, fn, cn, p_ref), tuple(got) + (p_got,)


NAMES = ("flow", "certainty", "flow_next", "cert_next", "disp_prev")


@pytest.mark.parametrize("G,G_next", SHAPES)
def test_fused_equals_two_launches(G, G_next):
    for sliced in (True, False):
        flow, cert, d_flow, d_cert = _inputs(G, 7 * G + sliced, sliced)
        flow0, cert0 = flow.clone(), cert.clone()
        for zero_small in (True, False):
            cases = [(True, None), (True, _disp_prev(d_flow, G + 1)), (False, _disp_prev(d_flow, G + 2))]
            for first, prev in cases:
                ref, got = _both(flow, cert, d_flow, d_cert, prev, G_next, zero_small, first)
                what = f"G {G}->{G_next} sliced={sliced} zero_small={zero_small} first={first} prev={'no' if prev is None else 'yes'}"
                for name, r, g in zip(NAMES, ref, got):
                    if r is None:
                        assert g is None, what
                        continue
                    assert g.shape == r.shape and torch.equal(g, r), f"{name}: {what}"
                if zero_small and not first:  # the case is worth its name only if both outcomes of the test occur
                    zeroed = (ref[4] == 0) & (d_flow != 0)
                    assert zeroed.any() and not zeroed.all(), what
                    assert not torch.equal(ref[4], prev)
        assert torch.equal(flow, flow0) and torch.equal(cert, cert0)  # inputs untouched


def test_fused_non_finite_cells():
    """inf / nan in single cells: in a tile's last row beside the next tile's first column, in the corner cell that a tile sees
    only as the corner of its ring, in the one-cell-wide tile, at the map's corner.  0 * inf of the interpolation weights must
    spread exactly as it does from the two launches."""
    G, G_next = 33, 66
    flow, cert, d_flow, d_cert = _inputs(G, 99, True)
    flow[0, 0, 15, 16] = float("inf")
    flow[1, 1, 16, 16] = float("nan")
    flow[2, 0, 32, 32] = float("-inf")
    flow[1, 0, 31, 15] = float("nan")
    cert[0, 0, 16, 16] = float("inf")
    d_cert[2, 0, 0, 0] = float("inf")
    d_flow[2, 1, 16, 15] = float("-inf")
    d_flow[0, 0, 0, 32] = float("nan")
    for first, prev in ((True, None), (False, _disp_prev(d_flow, 5))):
        ref, got = _both(flow, cert, d_flow, d_cert, prev, G_next, True, first)
        for name, r, g in zip(NAMES, ref, got):
            if r is None:
                assert g is None
                continue
            assert torch.equal(g.view(torch.int32), r.view(torch.int32)), f"{name} first={first}"
        assert not torch.isfinite(ref[2]).all() and not torch.isfinite(ref[3]).all()
    # ratio 1 reads the ring too (weight 0 on the right / lower neighbour)
    G = 32
    flow, cert, d_flow, d_cert = _inputs(G, 98, False)
    flow[0, 0, 15, 16] = float("inf")
    cert[1, 0, 16, 16] = float("nan")
    ref, got = _both(flow, cert, d_flow, d_cert, None, G, True, True)
    for name, r, g in zip(NAMES[:4], ref, got):
        assert torch.equal(g.view(torch.int32), r.view(torch.int32)), name
    assert torch.isnan(ref[2][0, 0, 15, 15])  # 0 * inf of the neighbour


def test_fused_declines_other_ratios():
    from gfnet_amd import _lib, ops

    G = 8
    flow, cert, d_flow, d_cert = _inputs(G, 3, False)
    fo, co = torch.empty_like(flow), torch.empty_like(cert)
    fn, cn = torch.empty((B, 2, 3 * G, 3 * G), device="cuda"), torch.empty((B, 1, 3 * G, 3 * G), device="cuda")
    p = _lib.ptr
    code = _lib.lib().gfn_flow_update_resize_fwd(p(flow), p(cert), p(fo), p(co), p(d_flow), 2 * G * G, p(d_cert), G * G, p(None), B, G,
                                                 SCALE, W0, H0, 1, 1, p(fn), p(cn), 3 * G, _lib.stream_ptr(flow.device))
    assert code == -1  # GFN_ERR_INVALID_ARG
    assert b"G_next" in _lib.lib().gfn_last_error()
    with pytest.raises(_lib.GfnError):
        ops.flow_update_resize(flow, cert, d_flow, d_cert, None, SCALE, W0, H0, 3 * G)
    # outputs that alias the inputs are refused as well (a ring cell is another workgroup's output)
    code = _lib.lib().gfn_flow_update_resize_fwd(p(flow), p(cert), p(flow), p(cert), p(d_flow), 2 * G * G, p(d_cert), G * G, p(None), B, G,
                                                 SCALE, W0, H0, 1, 1, p(fn), p(cn), 2 * G, _lib.stream_ptr(flow.device))
    assert code == -1


@pytest.mark.parametrize("num_itr", [[1] * 5, [2] * 5])
def test_forward_pyramids_fused_equals_unfused(num_itr):
    """Both passes of the 224 scene (grids 16/16/32/64/128, then 20/40/80/160; 2 pairs, symmetric) with the fused path and with
    ops.FUSE_UPDATE_RESIZE off: every entry of corresps equal.  num_itr 2 is the 672b16 arrangement: only a scale's last
    iteration fuses, with first_iteration=False and a disp_prev."""
    from gfnet_amd import _synthetic, ops

    scene = _synthetic.Scene(224, 2, num_itr, torch.float32, "off", torch.device("cuda"), 0)
    model = scene.model
    model.match_pyramids(scene.pyr[0], scene.pyr[1], scene.pyr_up[0], scene.pyr_up[1])  # sets the refinement pass's grids

    def run():
        with torch.inference_mode():
            first = model.match_first_pass(scene.pyr[0], scene.pyr[1])
            up = model.forward_pyramids(scene.pyr_up[0], scene.pyr_up[1], model.upsample_res, symmetric=True, upsample=True,
                                        scale_factor=1.25, pre_corresps=first["1"][num_itr[-1]])
        torch.cuda.synchronize()
        return first, up

    assert ops.FUSE_UPDATE_RESIZE
    fused = run()
    ops.FUSE_UPDATE_RESIZE = False
    try:
        plain = run()
    finally:
        ops.FUSE_UPDATE_RESIZE = True
    n = 0
    for cf, cp in zip(fused, plain):
        assert cf.keys() == cp.keys()
        for scale in cf:
            assert cf[scale].keys() == cp[scale].keys() and len(cf[scale]) == num_itr[0]
            for itr in cf[scale]:
                for k in ("flow", "certainty"):
                    assert torch.equal(cf[scale][itr][k], cp[scale][itr][k]), f"scale {scale} itr {itr} {k}"
                    n += 1
    assert n == 2 * (5 + 4) * num_itr[0]


def test_forward_pyramids_takes_the_fused_path(monkeypatch):
    """The loop really ends its scales with the fused call: one per scale but the last, none with the switch off or grad on."""
    from gfnet_amd import _synthetic, ops

    scene = _synthetic.Scene(224, 2, [2] * 5, torch.float32, "off", torch.device("cuda"), 0, upsample=False)
    calls = []
    real = ops.flow_update_resize
    monkeypatch.setattr(ops, "flow_update_resize", lambda *a, **k: (calls.append((a[0].shape[-1], a[8], k["first_iteration"])), real(*a, **k))[1])
    scene.model.match_first_pass(scene.pyr[0], scene.pyr[1])
    assert calls == [(16, 16, False), (16, 32, False), (32, 64, False), (64, 128, False)]
    calls.clear()
    monkeypatch.setattr(ops, "FUSE_UPDATE_RESIZE", False)
    scene.model.match_first_pass(scene.pyr[0], scene.pyr[1])
    assert calls == []


@pytest.mark.parametrize("shape,size", [((2, 3, 13, 17), (26, 34)), ((2, 3, 13, 17), (5, 5)), ((3, 2, 33, 33), (66, 66)),
                                        ((64, 3, 32, 32), (5, 5)), ((1, 7, 9, 40), (40, 3)), ((2, 1, 16, 16), (16, 16))])
def test_standalone_resize(shape, size):
    """interpolate_bilinear / interpolate_bilinear_pair (plane groups of three with shared taps; 7 and 1 planes leave a ragged
    group) against F.interpolate at the existing resize tests' 1e-6, and against each other exactly."""
    from gfnet_amd import ops

    gen = torch.Generator(device="cuda").manual_seed(shape[2] * 100 + size[0])
    x = torch.randn(shape, device="cuda", generator=gen)
    want = F.interpolate(x, size=size, mode="bilinear", align_corners=False)
    got = ops.interpolate_bilinear(x, size)
    assert_close(got.cpu().numpy(), want.cpu().numpy(), 1e-6, f"interp {shape} -> {size}")
    k = max(1, shape[1] - 1)
    a, b = ops.interpolate_bilinear_pair(x[:, :k].contiguous(), x[:, k - 1:].contiguous(), size)  # plane k - 1 is in both
    assert torch.equal(a, got[:, :k]) and torch.equal(b, got[:, k - 1:])
