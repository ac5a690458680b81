"""csrc/pair_synth.hip on the GPU against the float64 oracle of gfnet_amd/datasets/generate_random_H_large_size.py.

Tolerance of every comparison with the oracle (the pattern of DESIGN 4.4): the device has to be at least as close to float64 as the
reference's arithmetic class, |got - ref64| <= max(dev32, 2^-21 * max(1, |ref64|)), dev32 the largest deviation over that output
tensor of the SAME oracle run in float32 on the same inputs.  Sources are white noise, so a coordinate error shows in the pixels.
The four-point solve is double on the device and is held to 1e-3 * dev32 against torch.linalg.solve in float64."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def held(what, got, ref64, ref32, factor=1.0, floor=2.0 ** -21):
    """print worst error / bound, then assert it <= 1"""
    got, ref64, ref32 = got.detach().double().cpu(), ref64.double(), ref32.double()
    assert got.shape == ref64.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref64.shape)}"
    dev32 = float((ref32 - ref64).abs().max())
    bound = torch.clamp(floor * ref64.abs().clamp_min(1.0), min=factor * dev32)
    ratio = float(((got - ref64).abs() / bound).max())
    print(f"{what}: worst error / bound {ratio:.3g} (dev32 {dev32:.3g}, worst error {float((got - ref64).abs().max()):.3g})")
    assert math.isfinite(ratio) and ratio <= 1.0, f"{what}: worst error / bound {ratio:.3g}"
    return ratio


def zero_share(img):
    """the share of pixels that are zero in every channel"""
    return float((img == 0).all(dim=-3).double().mean())


# ---- the four-point solve --------------------------------------------------------------------------------------------------------------
def convex_quads(n, gen):
    """n quads with corners on a circle inside [0, 640)^2 (so they are convex), in one orientation"""
    centre = 200 + 240 * torch.rand((n, 1, 2), generator=gen)
    radius = 50 + 140 * torch.rand((n, 1), generator=gen)
    angle = torch.rand((n, 1), generator=gen) * 2 * math.pi + torch.arange(4) * (math.pi / 2) + (torch.rand((n, 4), generator=gen) - 0.5) * (math.pi / 3)
    return (centre + radius[..., None] * torch.stack([torch.cos(angle), torch.sin(angle)], dim=-1)).float()


def solve_reference(src, dst, dtype):
    from gfnet_amd.datasets.generate_random_H_large_size import reference_perspective_transform

    return torch.stack([reference_perspective_transform(s.to(dtype), d.to(dtype)) for s, d in zip(src, dst)])


def test_perspective_from_points():
    from gfnet_amd import ops
    from gfnet_amd.datasets import draw_random_h

    gen = torch.Generator().manual_seed(0)
    src, dst = convex_quads(64, gen), convex_quads(64, gen)
    assert float(src.min()) >= 0 and float(src.max()) < 640
    H, ok = ops.get_perspective_transform(src.cuda(), dst.cuda(), return_ok=True)
    assert H.dtype == torch.float64 and H.shape == (64, 3, 3) and bool((ok == 1).all()) and bool((H[:, 2, 2] == 1).all())
    held("solve, 64 convex quads", H, solve_reference(src, dst, torch.float64), solve_reference(src, dst, torch.float32), factor=1e-3, floor=0.0)
    # the corner sets of draw_random_h samples at crop 80 (deform_area 24), both images: sixteen problems
    draws = draw_random_h(8, 100, 90, 80, 24, generator=gen)
    corners = draws[:, 2:].reshape(16, 4, 2).float()
    tgt = torch.tensor([[12, 12], [67, 12], [67, 67], [12, 67]], dtype=torch.float32).expand(16, 4, 2)
    H, ok = ops.get_perspective_transform(corners.cuda(), tgt.cuda(), return_ok=True)
    assert bool((ok == 1).all())
    held("solve, 16 corner sets", H, solve_reference(corners, tgt, torch.float64), solve_reference(corners, tgt, torch.float32), factor=1e-3, floor=0.0)
    # src == dst: the identity, exactly
    H, ok = ops.get_perspective_transform(src.cuda(), src.cuda(), return_ok=True)
    assert torch.equal(H.cpu(), torch.eye(3, dtype=torch.float64).expand(64, 3, 3)) and bool((ok == 1).all())
    # three source points on a line: ok = 0 and the identity; its neighbours in the batch are solved
    bad = src.clone()
    bad[5] = torch.tensor([[10.0, 10.0], [110.0, 60.0], [210.0, 110.0], [30.0, 300.0]])
    H, ok = ops.get_perspective_transform(bad.cuda(), dst.cuda(), return_ok=True)
    assert ok.cpu().tolist() == [1] * 5 + [0] + [1] * 58
    assert torch.equal(H[5].cpu(), torch.eye(3, dtype=torch.float64))
    assert ops.get_perspective_transform(src[0].cuda(), dst[0].cuda()).shape == (1, 3, 3)


# ---- the warp ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def source():
    return torch.rand((3, 3, 37, 53), generator=torch.Generator().manual_seed(1))


def test_warp_exact_cases(source):
    from gfnet_amd import ops

    src = source.cuda()
    eye = torch.eye(3).expand(3, 3, 3)
    out = ops.warp_perspective(src, eye.cuda(), (29, 41))
    assert out.dtype == torch.float32 and torch.equal(out.cpu(), source[:, :, :29, :41])
    shift = torch.tensor([[1.0, 0, -5], [0, 1, 4], [0, 0, 1]]).expand(3, 3, 3)
    out = ops.warp_perspective(src, shift.cuda(), (29, 41)).cpu()
    assert torch.equal(out[:, :, 4:, :], source[:, :, :25, 5:46]) and bool((out[:, :, :4, :] == 0).all())
    out = ops.warp_perspective(src, eye.double().cuda(), (1, 1))
    assert torch.equal(out.cpu(), source[:, :, :1, :1])
    out = ops.warp_perspective(list(src), eye.cuda(), (37, 56)).cpu()                                   # wider than the source: zeros past it
    assert torch.equal(out[..., :53], source) and bool((out[..., 53:] == 0).all())


@pytest.fixture(scope="module")
def projective_case(source):
    """three samples, the third a view with batch and channel strides larger than its planes (and an odd element offset)"""
    from gfnet_amd.datasets.generate_random_H_large_size import reference_warp

    base = torch.tensor([[0.9, -0.25, 14], [0.2, 1.1, -9], [1.5e-3, -2e-3, 1]], dtype=torch.float64)
    H = torch.stack([base, base.clone(), base.clone()])
    H[1, 0, 2], H[1, 1, 2] = 18, -11
    H[2, 0, 2], H[2, 1, 2] = 3, 5
    ref = {}
    for wo in (41, 40):
        ref[wo] = {dt: torch.stack([reference_warp(source[b].to(dt), H[b].to(dt), (29, wo)) for b in range(3)]) for dt in (torch.float64, torch.float32)}
    return H, ref


@pytest.mark.parametrize("wo", [41, 40])
@pytest.mark.parametrize("normalise", [False, True])
def test_warp_projective_with_padding(source, projective_case, wo, normalise):
    from gfnet_amd import ops

    H, ref = projective_case
    ref64, ref32 = ref[wo][torch.float64], ref[wo][torch.float32]
    shares = [zero_share(ref64[b]) for b in range(3)]
    print("all-zero share of the oracle's output pixels:", shares)
    assert 0.10 <= shares[0] <= 0.60 and 0.10 <= shares[1] <= 0.60
    buf = torch.zeros(3 * (37 * 53 + 17) + 5).cuda()
    view = buf.as_strided((3, 37, 53), (37 * 53 + 17, 53, 1), 5)
    view.copy_(source[2])
    imgs = [source[0].cuda(), source[1].cuda(), view]
    got = ops.warp_perspective(imgs, H.cuda(), (29, wo), MEAN if normalise else None, STD if normalise else None)
    if normalise:
        m64, s64 = torch.tensor(MEAN, dtype=torch.float64)[:, None, None], torch.tensor(STD, dtype=torch.float64)[:, None, None]
        ref64, ref32 = (ref64 - m64) / s64, (ref32 - m64.float()) / s64.float()
    held(f"warp Wo={wo} normalise={normalise}", got, ref64, ref32)
    assert torch.equal(got, ops.warp_perspective(imgs, H.cuda(), (29, wo), MEAN if normalise else None, STD if normalise else None))


# ---- the synthesis -------------------------------------------------------------------------------------------------------------------------
def images(sizes, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.rand((3, h, w), generator=g) for h, w in sizes], [torch.rand((3, h, w), generator=g) for h, w in sizes]


def synth_case(sizes, crop, res, bi, normalize, seed):
    """the device batch and the oracle's (float64, float32) for the same draws; computed once per case"""
    from gfnet_amd import ops
    from gfnet_amd.datasets import draw_random_h, reference_random_h
    from gfnet_amd.datasets.generate_random_H_large_size import pre_resize, pre_resize_size

    a, b = images(sizes, seed)
    da, db = [pre_resize(t.cuda(), crop) for t in a], [pre_resize(t.cuda(), crop) for t in b]
    after = [pre_resize_size(h, w, crop) or (h, w) for h, w in sizes]
    assert [tuple(t.shape[1:]) for t in da] == [tuple(s) for s in after]
    draws = draw_random_h(len(a), [w for _, w in after], [h for h, _ in after], crop, int(crop * 0.3), generator=torch.Generator().manual_seed(seed + 1))
    run = lambda: ops.random_h_batch(da, db, draws, crop, (res, res), 0.3, bi, normalize=normalize, return_warped=True)  # noqa: E731
    refs = {dt: [reference_random_h(a[i], b[i], draws[i], crop, (res, res), 0.3, bi=bi, dtype=dt, normalize=normalize) for i in range(len(a))]
            for dt in (torch.float64, torch.float32)}
    return run, refs, draws, (da, db)


def compare_batch(what, got, refs):
    assert bool((got["ok"] == 1).all())
    assert got["H_s2t"].dtype == torch.float32 and got["im_A"].dtype == torch.float32 and got["H_s2t64"].dtype == torch.float64
    ratios = {}
    for key in ("im_A", "im_B", "H_s2t", "warped_img1", "M_A", "M_B"):
        r64, r32 = (torch.stack([r[key] for r in refs[dt]]) for dt in (torch.float64, torch.float32))
        ratios[key] = held(f"{what} {key}", got[key], r64, r32)
    held(f"{what} H_s2t64", got["H_s2t64"], torch.stack([r["H_s2t"] for r in refs[torch.float64]]), torch.stack([r["H_s2t"] for r in refs[torch.float32]]))
    return ratios


def test_synthesis_without_final_resize():
    """res 56: crop 80, deform_area 24, centre crop 56; the third source takes the pre-resize; normalised in the warp launch"""
    run, refs, _, _ = synth_case([(90, 100), (81, 130), (70, 95)], 80, 56, True, True, 10)
    got = run()
    assert got["im_A"].shape == got["im_B"].shape == got["warped_img1"].shape == (3, 3, 56, 56)
    compare_batch("res 56", got, refs)
    assert zero_share(got["warped_img1"]) > 0                                                           # the padding path ran
    again = run()                                                                                       # determinism: equal bits
    for key in ("im_A", "im_B", "H_s2t", "H_s2t64", "M_A", "M_B", "warped_img1"):
        assert torch.equal(got[key], again[key]), key


def test_synthesis_with_final_resize():
    """res 32: crop 45, deform_area 13, centre crop 33 x 33, bicubic to 32 x 32; H_s2t carries the rescale"""
    run, refs, _, _ = synth_case([(60, 70), (50, 64)], 45, 32, True, True, 20)
    got = run()
    assert got["im_A"].shape == got["warped_img1"].shape == (2, 3, 32, 32)
    compare_batch("res 32", got, refs)
    assert zero_share(got["warped_img1"]) > 0


def test_synthesis_one_way():
    """bi=False: H_2t is the identity and im_B the plain centre crop of the crop window, bit for bit"""
    run, refs, draws, (_, db) = synth_case([(90, 100), (81, 130)], 80, 56, False, False, 30)
    got = run()
    compare_batch("res 56 bi=False", got, refs)
    for i in range(2):
        cx, cy = int(draws[i, 0]), int(draws[i, 1])
        assert torch.equal(got["im_B"][i], db[i][:, cy + 12:cy + 68, cx + 12:cx + 68])
        assert torch.equal(got["M_B"][i].cpu(), torch.tensor([[1, 0, cx + 12.0], [0, 1, cy + 12.0], [0, 0, 1]], dtype=torch.float64))


def test_random_h_keeps_the_reference_order():
    """randomH returns (img2, img1, H_s2t, warped_src): the image warped by H_1t is the SECOND value"""
    from gfnet_amd.datasets import draw_random_h, randomH, reference_random_h

    (a,), (b,) = images([(81, 130)], 40)
    gen = torch.Generator().manual_seed(41)
    second, first, H, warped = randomH(a.cuda(), b.cuda(), 80, (56, 56), deformation_ratio=0.3, bi=True, generator=gen)
    draws = draw_random_h(1, 130, 81, 80, 24, generator=torch.Generator().manual_seed(41))[0]
    r64, r32 = (reference_random_h(a, b, draws, 80, (56, 56), 0.3, dtype=dt) for dt in (torch.float64, torch.float32))
    held("randomH img1 (second value)", first, r64["im_A"], r32["im_A"])
    held("randomH img2 (first value)", second, r64["im_B"], r32["im_B"])
    held("randomH H_s2t", H, r64["H_s2t"], r32["H_s2t"])
    held("randomH warped_src", warped, r64["warped_img1"], r32["warped_img1"])


def test_val_pair():
    import torch.nn.functional as F

    from gfnet_amd.datasets import val_pair
    from gfnet_amd.datasets.generate_random_H_large_size import reference_warp_by_map

    (img0,), (img1,) = images([(40, 50)], 50)
    H = torch.tensor([[1.05, 0.08, -3.0], [-0.06, 0.97, 2.5], [4e-4, -3e-4, 1.0]], dtype=torch.float64)
    got = val_pair(img0.cuda(), img1.cuda(), H, 32)
    ref = {}
    for dt in (torch.float64, torch.float32):
        r0, r1 = (F.interpolate(t.to(dt)[None], size=(32, 32), mode="bicubic", align_corners=False)[0] for t in (img0, img1))
        Hs = torch.diag(torch.tensor([32 / 50, 32 / 40, 1.0], dtype=dt)) @ H.to(dt) @ torch.diag(torch.tensor([32 / 50, 32 / 40, 1.0], dtype=dt)).inverse()
        ref[dt] = {"im_A": r1, "im_B": r0, "H_s2t": Hs, "warped_img1": reference_warp_by_map(r0, Hs, (32, 32))}
    for key in ("im_A", "im_B", "H_s2t", "warped_img1"):
        held(f"val_pair {key}", got[key], ref[torch.float64][key], ref[torch.float32][key])
    assert got["H_s2t"].dtype == torch.float32 and 0 < zero_share(got["warped_img1"]) < 0.5


def test_batch_goes_into_the_loss():
    from gfnet_amd.datasets import PairSynthesizer
    from gfnet_amd.losses import RobustLosses

    a, b = images([(90, 100), (70, 95)], 60)
    synth = PairSynthesizer(56, deformation_ratio=[0.3], generator=torch.Generator().manual_seed(61))
    batch = synth(a, b)
    assert set(batch) == {"im_A", "im_B", "H_s2t"} and batch["im_A"].is_cuda
    assert batch["im_A"].shape == batch["im_B"].shape == (2, 3, 56, 56) and batch["H_s2t"].shape == (2, 3, 3) and batch["H_s2t"].dtype == torch.float32
    gen = torch.Generator().manual_seed(62)
    corresps = {"gm": {1: {"flow": (torch.rand((2, 2, 4, 4), generator=gen) * 2 - 1).cuda().requires_grad_(),
                           "certainty": torch.randn((2, 1, 4, 4), generator=gen).cuda().requires_grad_()}},
                8: {1: {"flow": (torch.rand((2, 2, 8, 8), generator=gen) * 2 - 1).cuda().requires_grad_(),
                        "certainty": torch.randn((2, 1, 8, 8), generator=gen).cuda().requires_grad_()}}}
    loss = RobustLosses(ce_weight=0.01, local_dist={8: 8}, local_largest_scale=8, alpha=0.5, c=1e-4, iteration_base=1)(corresps, batch)
    assert loss.dim() == 0 and bool(torch.isfinite(loss))
