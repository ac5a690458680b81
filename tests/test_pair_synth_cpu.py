"""Pair synthesis without a GPU: the order of the random draws, the geometry of the float64 oracle (gfnet_amd.datasets.reference_random_h)
and the three new symbols of the C ABI."""
import ctypes

import torch

RES56 = dict(crop_size=80, input_size=(56, 56), deformation_ratio=0.3)      # deform_area 24, centre crop 56: no final resize


def _reference_sequence(w1, h1, crop_size, deform_area):
    """One randomH's torch.randint(lo, hi, size=(1,)) calls as (lo, hi) pairs in call order: the crop origin
    (generate_random_H_large_size.py:50-51), then random_four_points' eight (:7-22) for image 1 (:59) and again for image 2 (:60)."""
    c, d = crop_size, deform_area
    four_points = [(0, d), (0, d),              # top left x, y
                   (c - d, c), (0, d),          # top right
                   (c - d, c), (c - d, c),      # bottom right
                   (0, d), (c - d, c)]          # bottom left
    ranges = [(0, w1 - c), (0, h1 - c)] + four_points + four_points
    return [int(torch.randint(lo, hi, size=(1,))) for lo, hi in ranges]


def test_draws_consume_the_generator_as_the_reference_does():
    from gfnet_amd.datasets import draw_random_h

    for seed in (0, 7):
        torch.manual_seed(seed)
        got = draw_random_h(1, 130, 81, 80, 24)
        after = torch.rand(1)
        torch.manual_seed(seed)
        want = _reference_sequence(130, 81, 80, 24)
        assert got.dtype == torch.int32 and got.shape == (1, 18) and got[0].tolist() == want
        assert torch.equal(after, torch.rand(1))                            # the generator is left where the reference leaves it
    sizes = [(100, 90), (130, 81), (122, 90)]
    torch.manual_seed(3)
    got = draw_random_h(3, [w for w, _ in sizes], [h for _, h in sizes], 80, 24)
    torch.manual_seed(3)
    assert got.tolist() == [_reference_sequence(w, h, 80, 24) for w, h in sizes]
    gen = torch.Generator().manual_seed(11)                                 # an explicit generator leaves the global one alone
    torch.manual_seed(5)
    draw_random_h(2, 100, 90, 80, 24, generator=gen)
    after = torch.rand(1)
    torch.manual_seed(5)
    assert torch.equal(after, torch.rand(1))
    lo = torch.tensor([0, 0] + [0, 0, 56, 0, 56, 56, 0, 56] * 2)
    hi = torch.tensor([50, 1] + [24, 24, 80, 24, 80, 80, 24, 80] * 2)
    many = draw_random_h(40, 130, 81, 80, 24)
    assert bool(((many >= lo) & (many < hi)).all())


def _pair(h, w, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand((3, h, w), generator=g), torch.rand((3, h, w), generator=g)


def test_h_s2t_is_the_composition_of_the_two_pixel_maps():
    from gfnet_amd.datasets import draw_random_h, reference_random_h

    img1, img2 = _pair(81, 130, 1)
    gen = torch.Generator().manual_seed(2)
    for draws in draw_random_h(4, 130, 81, 80, 24, generator=gen):
        ref = reference_random_h(img1, img2, draws, **RES56, bi=True, dtype=torch.float64)
        assert ref["im_A"].shape == ref["im_B"].shape == ref["warped_img1"].shape == (3, 56, 56) and ref["H_s2t"].dtype == torch.float64
        comp = torch.linalg.inv(ref["M_B"]) @ ref["M_A"]
        comp = comp / comp[2, 2]
        rel = float(((comp - ref["H_s2t"]).abs() / ref["H_s2t"].abs().clamp_min(1.0)).max())
        assert rel <= 1e-12, rel
        assert ref["H_s2t"][2, 2] == 1.0


def test_rescale_is_applied_as_the_reference_writes_it():
    from gfnet_amd.datasets import draw_random_h, reference_random_h

    img1, img2 = _pair(60, 70, 3)
    draws = draw_random_h(1, 70, 60, 45, 13, generator=torch.Generator().manual_seed(4))[0]
    plain = reference_random_h(img1, img2, draws, 45, (33, 33), 0.3, dtype=torch.float64)["H_s2t"]      # the centre crop's own size
    for h_in, w_in in ((32, 32), (32, 40)):
        ref = reference_random_h(img1, img2, draws, 45, (h_in, w_in), 0.3, dtype=torch.float64)
        assert ref["im_A"].shape == (3, h_in, w_in) and ref["warped_img1"].shape == (3, h_in, w_in)
        # :77-79 -- the HEIGHT ratio on both axes on the left, the WIDTH ratio on both axes (inverted) on the right
        left = torch.diag(torch.tensor([h_in / 33, h_in / 33, 1.0], dtype=torch.float64))
        right = torch.diag(torch.tensor([w_in / 33, w_in / 33, 1.0], dtype=torch.float64)).inverse()
        want = left @ plain @ right
        assert float(((ref["H_s2t"] - want).abs() / want.abs().clamp_min(1.0)).max()) <= 1e-15
    assert float((reference_random_h(img1, img2, draws, 45, (32, 40), 0.3)["H_s2t"] - plain).abs().max()) > 1e-3


def test_one_way_pairs_keep_the_second_image():
    from gfnet_amd.datasets import draw_random_h, reference_random_h

    img1, img2 = _pair(81, 130, 5)
    draws = draw_random_h(1, 130, 81, 80, 24, generator=torch.Generator().manual_seed(6))[0]
    ref = reference_random_h(img1, img2, draws, **RES56, bi=False, dtype=torch.float32)
    cx, cy = int(draws[0]), int(draws[1])
    assert ref["im_B"].dtype == torch.float32
    assert torch.equal(ref["im_B"], img2[:, cy + 12:cy + 68, cx + 12:cx + 68])                           # bit for bit
    assert torch.equal(ref["M_B"], torch.tensor([[1, 0, cx + 12.0], [0, 1, cy + 12.0], [0, 0, 1]]))
    assert not torch.equal(ref["im_A"], img1[:, cy + 12:cy + 68, cx + 12:cx + 68])


def test_library_exports_and_binds_the_pair_synthesis_symbols():
    from gfnet_amd import _lib
    from gfnet_amd._lib import c_i64, c_int, c_vp

    assert _lib.PROTOTYPES["gfn_perspective_from_points"] == (c_int, [c_vp, c_vp, c_vp, c_vp, c_int, c_vp])
    assert _lib.PROTOTYPES["gfn_random_h_params"] == (c_int, [c_vp] + [c_int] * 7 + [c_vp] * 6)
    assert _lib.PROTOTYPES["gfn_warp_perspective_fwd"] == (c_int, [c_vp, c_vp, c_vp, c_int, c_vp, c_i64] + [c_int] * 4 + [c_vp] * 3)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    names = ("gfn_perspective_from_points", "gfn_random_h_params", "gfn_warp_perspective_fwd")
    for name in names:
        assert getattr(raw, name) is not None and name in _lib.STATUS_FUNCS
    L = _lib.lib()
    assert L.gfn_abi_version() == 1
    # argument errors and empty batches are answered on the host
    assert L.gfn_perspective_from_points(None, None, None, None, 0, None) == 0
    assert L.gfn_perspective_from_points(None, None, None, None, 1, None) == _lib.ERR_INVALID_ARG
    assert L.gfn_random_h_params(None, 0, 80, 24, 56, 56, 56, 56, None, None, None, None, None, None) == 0
    assert L.gfn_random_h_params(None, 0, 80, 24, 57, 56, 56, 56, None, None, None, None, None, None) == _lib.ERR_INVALID_ARG
    assert b"centre crop" in L.gfn_last_error()
    assert L.gfn_warp_perspective_fwd(None, None, None, 0, None, 0, 0, 3, 8, 8, None, None, None) == 0
    assert L.gfn_warp_perspective_fwd(None, None, None, 0, None, 0, 1, 3, 8, 8, None, None, None) == _lib.ERR_INVALID_ARG
