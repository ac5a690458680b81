"""Photometric augmentation on the GPU against Pillow's results (tests/golden/photometric_*.npz, written by make_golden_photometric.py).

The kernels restate Pillow's arithmetic term by term -- the float / double mix of Convert.c's rgb2hsv and hsv2rgb and the fixed-point
box blur of BoxBlur.c included; a numpy restatement of the same terms agrees with Pillow 12.2.0 on all 2^24 RGB and HSV triples and
on every blur radius tried.  So blur and hue are held to equality here, which implies the looser conditions an all-float32
restatement would need (blur: no value off by more than one level and at most 0.1 % off at all; hue: at most 1 % of the pixels, each
Pillow's RGB of H +- 1)."""
import json
import random

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

OFF = {"order": [0, 1, 2, 3], "brightness": None, "contrast": None, "saturation": None, "hue": None, "grayscale": False,
       "blur_radius": None}


@pytest.fixture(scope="module")
def stages():
    g = load_golden("photometric_stages")
    return g, [torch.from_numpy(g[f"image_{i}"]).cuda() for i in range(4)], json.loads(str(g["cases"]))


@pytest.fixture(scope="module")
def chains():
    g = load_golden("photometric_chains")
    return g, [torch.from_numpy(g[f"image_{i}"]).cuda() for i in range(4)]


def _same(got, want, what):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.shape} {got.dtype} vs {want.shape} {want.dtype}"
    diff = got.astype(np.int32) - want.astype(np.int32)
    assert not diff.any(), f"{what}: {np.count_nonzero(diff)} of {diff.size} values differ, by up to {np.abs(diff).max()}"


def _stage_names(prefix):
    return [n for n in json.loads(str(load_golden("photometric_stages")["cases"])) if n.startswith(prefix)]


@pytest.mark.parametrize("name", ["none", "grey"] + _stage_names("brightness") + _stage_names("contrast") + _stage_names("saturation")
                         + _stage_names("blur") + _stage_names("hue"))
def test_one_stage_is_pillows(stages, name):
    from gfnet_amd import ops

    g, images, cases = stages
    got = ops.photo_augment(images, [cases[name]] * 4, out="uint8")          # one batch: 70 x 45, 41 x 83, 5 x 3, 1 x 9
    for i in range(4):
        _same(got[i], g[f"{name}/{i}"], f"{name} on image {i}")


def test_float_output_is_u8_over_255(stages):
    from gfnet_amd import ops

    g, images, cases = stages
    for name in ("none", "blur_1.5"):
        got = ops.photo_augment(images, [cases[name]] * 4)
        for i in range(4):
            want = torch.from_numpy(g[f"{name}/{i}"]).permute(2, 0, 1).float().div(255)
            assert got[i].dtype == torch.float32 and got[i].shape == want.shape and got[i].is_contiguous()
            assert torch.equal(got[i].cpu(), want), (name, i)
    one = ops.photo_augment(torch.stack([images[0], images[0]]), [cases["grey"], cases["none"]])    # an (N,h,w,3) tensor
    assert torch.equal(one[1].cpu(), torch.from_numpy(g["none/0"]).permute(2, 0, 1).float().div(255))
    assert torch.equal(one[0].cpu(), torch.from_numpy(g["grey/0"]).permute(2, 0, 1).float().div(255))


def test_resize_is_pillows(stages):
    from gfnet_amd import ops

    rz = load_golden("photometric_resize")
    big = torch.from_numpy(rz["image"]).cuda()                              # 97 x 131
    for size in rz["sizes"]:
        (got,) = ops.photo_resize([big], int(size))
        _same(got, rz[f"resize_{size}"], f"resize to {size}")
    assert ops.photo_resize([big], 97)[0] is big                            # the short side already is 97: the image itself
    _, images, _ = stages
    for size, key in ((4, "small"), (12, "small_up")):                      # one batch of four sizes, down and up
        got = ops.photo_resize(images, size)
        for i in range(4):
            _same(got[i], rz[f"{key}_{i}"], f"{key} image {i}")
    mixed = ops.photo_resize([big, images[0], big[:, :97]], 97)              # resized and untouched images in one batch
    _same(mixed[1], ops.photo_resize([images[0]], 97)[0].cpu().numpy(), "mixed batch")
    assert mixed[0] is big and mixed[2].shape == (97, 97, 3) and torch.equal(mixed[2], big[:, :97])
    _same(ops.photo_resize([big.permute(1, 0, 2)], 48)[0], ops.photo_resize([big.permute(1, 0, 2).contiguous()], 48)[0].cpu().numpy(),
          "a strided view")


@pytest.mark.parametrize("batch", range(6))
def test_chains_without_hue_are_pillows(chains, batch):
    """All six orders of brightness / contrast / saturation; the four images of a batch differ in size, factors, grey and blur, so
    contrast's mean is taken after zero, one and two recomputed ops and with every combination of grey and blur."""
    from gfnet_amd import ops

    g, images = chains
    params = json.loads(str(g["batches"]))[batch]
    got = ops.photo_augment(images, params, out="uint8")
    for i in range(4):
        _same(got[i], g[f"chain_{batch}/{i}"], f"order {params[i]['order']} on image {i}")


def test_presets_with_hue_are_pillows(chains):
    from gfnet_amd import ops

    g, images = chains
    for name, size, params in json.loads(str(g["presets"])):
        got = ops.photo_augment(images, params, out="uint8", resize=size)
        for i in range(4):
            _same(got[i], g[f"{name}/{i}"], f"{name} preset on image {i}")


def test_fused_chain_with_hue_equals_the_ops_one_at_a_time(stages):
    from gfnet_amd import ops

    _, images, _ = stages
    orders = ([3, 1, 0, 2], [1, 3, 2, 0], [0, 2, 3, 1], [2, 0, 1, 3])
    params = [{"order": o, "brightness": 0.7 + 0.2 * i, "contrast": 1.4 - 0.3 * i, "saturation": 0.5 + 0.4 * i, "hue": 0.31 - 0.2 * i,
               "grayscale": i == 2, "blur_radius": (1.8, None, 0.4, 1.1)[i]} for i, o in enumerate(orders)]
    fused = ops.photo_augment(images, params, out="uint8")
    again = ops.photo_augment(images, params, out="uint8")
    step = list(images)
    names = ("brightness", "contrast", "saturation", "hue")
    for k in range(4):
        step = ops.photo_augment(step, [dict(OFF, **{names[p["order"][k]]: p[names[p["order"][k]]]}) for p in params], out="uint8")
    step = ops.photo_augment(step, [dict(OFF, grayscale=p["grayscale"]) for p in params], out="uint8")
    step = ops.photo_augment(step, [dict(OFF, blur_radius=p["blur_radius"]) for p in params], out="uint8")
    for i in range(4):
        assert torch.equal(fused[i], again[i]), i                           # identical calls, identical bits
        _same(fused[i], step[i].cpu().numpy(), f"fused chain {orders[i]} on image {i}")


def test_photometric_augment_is_seeded_and_equals_its_draws(stages):
    from gfnet_amd import ops
    from gfnet_amd.datasets import PhotometricAugment, draw_photometric

    _, images, _ = stages
    kw = dict(brightness=0.6, contrast=0.6, saturation=0.6, hue=0.2, grayscale_p=0.2)
    runs = []
    for _ in range(2):
        aug = PhotometricAugment(resize=24, generator=torch.Generator().manual_seed(8), rng=random.Random(9), **kw)
        runs.append(aug([t.cpu() for t in images] + images))                # host and device images alike
    draws = draw_photometric(8, generator=torch.Generator().manual_seed(8), rng=random.Random(9), **kw)
    want = ops.photo_augment(images + images, draws, resize=24)
    assert [tuple(t.shape) for t in runs[0]] == [(3, 37, 24), (3, 24, 48), (3, 40, 24), (3, 24, 216)] * 2
    for a, b, c in zip(runs[0], runs[1], want):
        assert a.is_cuda and a.dtype == torch.float32 and torch.equal(a, b) and torch.equal(a, c)
        assert float(a.min()) >= 0.0 and float(a.max()) <= 1.0
    assert PhotometricAugment(resize=None, generator=torch.Generator().manual_seed(1))(images[:1])[0].shape == (3, 70, 45)


def test_pair_synthesizer_takes_uint8_images_through_the_augmentation():
    from gfnet_amd.datasets import PairSynthesizer, PhotometricAugment

    g = torch.Generator().manual_seed(3)
    sizes = ((90, 120), (130, 100), (96, 96))
    u0 = [torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8).cuda() for h, w in sizes]
    u1 = [torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8).cuda() for h, w in sizes]

    def aug():
        return PhotometricAugment(resize=88, generator=torch.Generator().manual_seed(5), rng=random.Random(6))

    random.seed(1)
    got = PairSynthesizer(56, generator=torch.Generator().manual_seed(7), photometric=aug())(u0, u1)
    both = aug()([t for pair in zip(u0, u1) for t in pair])                 # imgs0[0], imgs1[0], imgs0[1], ...
    random.seed(1)
    want = PairSynthesizer(56, generator=torch.Generator().manual_seed(7))(both[0::2], both[1::2])
    assert got["im_A"].shape == (3, 3, 56, 56)
    for key in ("im_A", "im_B", "H_s2t"):
        assert torch.equal(got[key], want[key]), key


def test_row_strided_views_are_read_with_their_own_stride(chains):
    """A column crop of a larger image is read in place (its rows are 3 * 131 bytes apart, not 3 * w): without a resize it is the
    stats and the jitter + blur kernels that read it, with contrast's mean taken over the crop alone."""
    from gfnet_amd import ops

    big = torch.from_numpy(load_golden("photometric_resize")["image"]).cuda()       # 97 x 131
    _, images = chains
    views = [big[:, 20:117], big[5:80, 3:50], big[:, :97]]
    assert all(not v.is_contiguous() for v in views)
    params = [dict(OFF, order=[2, 1, 0, 3], contrast=1.5, saturation=0.6, blur_radius=1.7),
              dict(OFF, brightness=1.3, hue=-0.2),
              dict(OFF, order=[0, 1, 2, 3], brightness=0.7, contrast=0.5, grayscale=True)]
    dense = [v.contiguous() for v in views]
    for out in ("uint8", "float"):
        got = ops.photo_augment(views + [images[0]], params + [params[0]], out=out)
        want = ops.photo_augment(dense + [images[0]], params + [params[0]], out=out)
        for i, (a, b) in enumerate(zip(got, want)):
            assert torch.equal(a, b), (out, i)
    # the same with a resize in the call: to 97, which two of the views already have (they are not resized), and to 60
    for size in (97, 60):
        a = ops.photo_augment(views, params, out="uint8", resize=size)
        b = ops.photo_augment(dense, params, out="uint8", resize=size)
        for i in range(3):
            assert torch.equal(a[i], b[i]), (size, i)
    assert ops.photo_resize(views[:1], 97)[0] is views[0]                           # nothing to do: the view itself, no launch
