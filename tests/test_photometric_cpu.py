"""Photometric augmentation without a GPU: the order of the random draws, the goldens against Pillow (where it is installed), the
resize tables against the goldens, and the three new symbols of the C ABI."""
import ctypes
import json
import random

import numpy as np
import pytest
import torch

from conftest import load_golden


def _restated_draws(n, ranges, grayscale_p, blur_p, blur_radius, rng):
    """The reference's draws, restated: per image ColorJitter.get_params (randperm(4), then one uniform_ per enabled op in the order
    brightness, contrast, saturation, hue), RandomGrayscale's rand(1) when its p > 0, RandomGaussianBlur's random() and uniform()."""
    out = []
    for _ in range(n):
        p = {"order": torch.randperm(4).tolist()}
        for name in ("brightness", "contrast", "saturation", "hue"):
            p[name] = None if ranges[name] is None else float(torch.empty(1).uniform_(*ranges[name]))
        p["grayscale"] = bool(torch.rand(1) < grayscale_p) if grayscale_p > 0 else False
        p["blur_radius"] = None
        if rng.random() < blur_p:
            p["blur_radius"] = rng.uniform(*blur_radius)
        out.append(p)
    return out


def test_draws_follow_the_reference_order():
    from gfnet_amd.datasets import draw_photometric

    online = {"brightness": (0.8, 1.2), "contrast": (0.8, 1.2), "saturation": (0.8, 1.2), "hue": (-0.2, 0.2)}
    glunet = {"brightness": (0.4, 1.6), "contrast": (0.4, 1.6), "saturation": (0.4, 1.6), "hue": (-0.2, 0.2)}
    for seed in (0, 9):
        torch.manual_seed(seed)
        got = draw_photometric(5, rng=random.Random(seed))
        after = torch.rand(1)
        torch.manual_seed(seed)
        assert got == _restated_draws(5, online, 0.0, 0.5, (0.1, 2.0), random.Random(seed))
        assert torch.equal(after, torch.rand(1))                            # the generator is left where the reference leaves it
        torch.manual_seed(seed)
        got = draw_photometric(5, 0.6, 0.6, 0.6, 0.2, grayscale_p=0.2, rng=random.Random(seed))
        torch.manual_seed(seed)
        assert got == _restated_draws(5, glunet, 0.2, 0.5, (0.1, 2.0), random.Random(seed))
    assert any(p["blur_radius"] is None for p in got) and any(p["blur_radius"] is not None for p in got)
    for p in draw_photometric(40, 0.6, 0.6, 0.6, 0.2, rng=random.Random(1)):
        assert sorted(p["order"]) == [0, 1, 2, 3] and 0.4 <= p["brightness"] <= 1.6 and -0.2 <= p["hue"] <= 0.2
        assert p["blur_radius"] is None or 0.1 <= p["blur_radius"] <= 2.0
    # an explicit generator leaves the global one alone; the module-level random serves when rng is None
    torch.manual_seed(5)
    random.seed(3)
    a = draw_photometric(3, generator=torch.Generator().manual_seed(11))
    after = torch.rand(1)
    torch.manual_seed(5)
    assert torch.equal(after, torch.rand(1))
    assert [p["blur_radius"] for p in a] == [p["blur_radius"] for p in draw_photometric(3, generator=torch.Generator().manual_seed(2),
                                                                                        rng=random.Random(3))]


def test_disabled_ops_draw_nothing():
    from gfnet_amd.datasets import draw_photometric

    torch.manual_seed(4)
    rng = random.Random(4)
    got = draw_photometric(3, brightness=0, contrast=None, saturation=(1.0, 1.0), hue=0.0, grayscale_p=0.0, blur_p=0.0, rng=rng)
    after, after_rng = torch.rand(1), rng.random()
    torch.manual_seed(4)
    rng = random.Random(4)
    orders = []
    for _ in range(3):
        orders.append(torch.randperm(4).tolist())
        rng.random()                                                        # the blur's coin is always tossed; nothing else is drawn
    assert torch.equal(after, torch.rand(1)) and after_rng == rng.random()
    assert got == [{"order": o, "brightness": None, "contrast": None, "saturation": None, "hue": None, "grayscale": False,
                    "blur_radius": None} for o in orders]
    torch.manual_seed(4)
    only = draw_photometric(2, brightness=0, contrast=0.3, saturation=0, hue=0, blur_p=0.0)
    torch.manual_seed(4)
    for p in only:
        assert p["order"] == torch.randperm(4).tolist() and p["contrast"] == float(torch.empty(1).uniform_(0.7, 1.3))


def test_goldens_reproduce_from_pillow():
    pytest.importorskip("PIL")
    from gfnet_amd.datasets import reference_photometric

    st = load_golden("photometric_stages")
    images = [st[f"image_{i}"] for i in range(4)]
    for name, p in json.loads(str(st["cases"])).items():
        for i, im in enumerate(images):
            assert np.array_equal(reference_photometric(im, p), st[f"{name}/{i}"]), (name, i)
    ch = load_golden("photometric_chains")
    for b, batch in enumerate(json.loads(str(ch["batches"]))):
        for i, p in enumerate(batch):
            assert np.array_equal(reference_photometric(images[i], p), ch[f"chain_{b}/{i}"]), (b, i)
    for name, size, batch in json.loads(str(ch["presets"])):
        for i, p in enumerate(batch):
            assert np.array_equal(reference_photometric(torch.from_numpy(images[i]), p, size), ch[f"{name}/{i}"]), (name, i)
    rz = load_golden("photometric_resize")
    off = {"order": [0, 1, 2, 3]}
    for size in rz["sizes"]:
        assert np.array_equal(reference_photometric(rz["image"], off, int(size)), rz[f"resize_{size}"])


def _resize_by_table(img, size):
    """Image.resize(BILINEAR) from ops.resize_axis_table alone: what gfn_photo_resize_u8 computes, in numpy"""
    from gfnet_amd import ops

    def axis(x, n_out):
        table, taps = ops.resize_axis_table(x.shape[1], n_out)
        bounds, k = table[:2 * n_out].reshape(n_out, 2), table[2 * n_out:].reshape(n_out, taps).astype(np.int64)
        out = np.zeros((x.shape[0], n_out, 3), np.uint8)
        for o, (lo, count) in enumerate(bounds):
            assert 0 <= lo and 1 <= count <= taps and lo + count <= x.shape[1]
            out[:, o] = np.clip(((x[:, lo:lo + count].astype(np.int64) * k[o, :count, None]).sum(1) + (1 << 21)) >> 22, 0, 255)
        return out

    h, w = ops.resize_output_size(img.shape[0], img.shape[1], size)
    if (h, w) == img.shape[:2]:
        return img
    return axis(axis(img, w).transpose(1, 0, 2), h).transpose(1, 0, 2)


def test_resize_tables_give_pillows_pixels():
    from gfnet_amd import ops

    assert ops.resize_output_size(97, 131, 48) == (48, 64) and ops.resize_output_size(131, 97, 150) == (202, 150)
    assert ops.resize_output_size(97, 131, 97) == (97, 131) and ops.resize_output_size(853, 1137, 640) == (640, 853)
    rz, st = load_golden("photometric_resize"), load_golden("photometric_stages")
    for size in rz["sizes"]:
        assert np.array_equal(_resize_by_table(rz["image"], int(size)), rz[f"resize_{size}"]), size
    for i in range(4):
        assert np.array_equal(_resize_by_table(st[f"image_{i}"], 4), rz[f"small_{i}"])
        assert np.array_equal(_resize_by_table(st[f"image_{i}"], 12), rz[f"small_up_{i}"])
    # GaussianBlur's box radius: 2.0 -> l = 1, a = 0.375 exactly; the kernels' halo holds R < 2
    assert ops.box_blur_radius(2.0) == 1.375 and 0.0 < ops.box_blur_radius(0.1) < 0.002 and ops.box_blur_radius(1.5) > 1.0


def test_parameter_records():
    from gfnet_amd import _lib, ops

    rec = ops._photo_records([{"order": [3, 1, 0, 2], "brightness": 1.2, "contrast": None, "saturation": 0.5, "hue": -0.2,
                               "grayscale": True, "blur_radius": 2.0}, {}], 2)
    assert rec.shape == (2, _lib.PHOTO_REC) and rec.dtype == np.int32
    assert rec[0, :4].tolist() == [3, 1, 0, 2] and rec[0, 7] == (-51 & 255) and rec[0, 8] == 1 and rec[0, 10] == 0b1101
    assert rec[0].view(np.float32)[[4, 6, 9]].tolist() == [np.float32(1.2), 0.5, 1.375]
    assert rec[1].tolist() == [0, 1, 2, 3] + [0] * 8
    for bad in ({"order": [0, 1, 2, 2]}, {"brightness": -0.1}, {"hue": 0.6}, {"blur_radius": 4.0}):
        with pytest.raises(ValueError):
            ops._photo_records([bad], 1)


def test_library_exports_and_binds_the_photometric_symbols():
    from gfnet_amd import _lib
    from gfnet_amd._lib import c_int, c_vp

    assert _lib.PROTOTYPES["gfn_photo_resize_u8"] == (c_int, [c_vp] * 5 + [c_int] * 3 + [c_vp])
    assert _lib.PROTOTYPES["gfn_photo_stats"] == (c_int, [c_vp] * 4 + [c_int] * 3 + [c_vp])
    assert _lib.PROTOTYPES["gfn_photo_jitter_blur"] == (c_int, [c_vp] * 5 + [c_int] * 4 + [c_vp])
    assert (_lib.PHOTO_BRIGHTNESS, _lib.PHOTO_CONTRAST, _lib.PHOTO_SATURATION, _lib.PHOTO_HUE) == (0, 1, 2, 3)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("gfn_photo_resize_u8", "gfn_photo_stats", "gfn_photo_jitter_blur"):
        assert getattr(raw, name) is not None and name in _lib.STATUS_FUNCS
    L = _lib.lib()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.c_void_p(ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 8)
    odd = ctypes.c_void_p(p.value + 2)
    # empty batches are answered on the host without a launch, NULL, negative sizes and misaligned tables refused there
    assert L.gfn_photo_resize_u8(None, None, None, None, None, 0, 8, 8, None) == 0
    assert L.gfn_photo_resize_u8(None, None, None, None, None, 1, 8, 8, None) == _lib.ERR_INVALID_ARG
    assert b"null" in L.gfn_last_error()
    assert L.gfn_photo_resize_u8(p, p, p, p, p, -1, 8, 8, None) == _lib.ERR_INVALID_ARG
    assert L.gfn_photo_resize_u8(p, p, p, p, p, 1, -8, 8, None) == _lib.ERR_INVALID_ARG
    assert L.gfn_photo_resize_u8(odd, p, p, p, p, 1, 8, 8, None) == _lib.ERR_INVALID_ARG
    assert b"misaligned" in L.gfn_last_error()
    assert L.gfn_photo_stats(None, None, None, None, 0, 8, 8, None) == 0
    assert L.gfn_photo_stats(p, p, p, None, 1, 8, 8, None) == _lib.ERR_INVALID_ARG
    assert L.gfn_photo_stats(p, p, p, p, 1, 8, -1, None) == _lib.ERR_INVALID_ARG
    assert L.gfn_photo_stats(p, p, p, odd, 1, 8, 8, None) == _lib.ERR_INVALID_ARG
    assert L.gfn_photo_jitter_blur(None, None, None, None, None, 0, 0, 8, 8, None) == 0
    assert L.gfn_photo_jitter_blur(p, p, p, p, p, 0, 3, 0, 8, None) == 0
    assert L.gfn_photo_jitter_blur(p, p, p, p, None, 0, 1, 8, 8, None) == _lib.ERR_INVALID_ARG
    assert L.gfn_photo_jitter_blur(p, p, p, p, p, 0, 70000, 8, 8, None) == _lib.ERR_INVALID_ARG
    assert L.gfn_photo_jitter_blur(p, odd, p, p, p, 1, 1, 8, 8, None) == _lib.ERR_INVALID_ARG


def _rgb2hsv_terms(rgb):
    """csrc/photometric.hip's rgb2hsv, term by term in numpy: float32 variables, double constants"""
    f32, f64 = np.float32, np.float64
    r, g, b = (rgb[..., k].astype(np.int32) for k in range(3))
    mx, mn = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    with np.errstate(all="ignore"):
        cr = (mx - mn).astype(f32)
        s = cr / mx.astype(f32)
        rc, gc, bc = ((mx - c).astype(f32) / cr for c in (r, g, b))
        h = np.where(r == mx, (bc - gc).astype(f64), np.where(g == mx, (2.0 + rc.astype(f64)) - bc.astype(f64),
                                                              (4.0 + gc.astype(f64)) - rc.astype(f64))).astype(f32)
        t = h.astype(f64) / 6.0 + 1.0
        h = (t - np.floor(t)).astype(f32)
        uh = np.minimum((h.astype(f64) * 255.0).astype(np.int32), 255)
        us = np.minimum((s.astype(f64) * 255.0).astype(np.int32), 255)
    grey = mx == mn
    return np.stack([np.where(grey, 0, uh), np.where(grey, 0, us), mx], -1).astype(np.uint8)


def _hsv2rgb_terms(hsv):
    """csrc/photometric.hip's hsv2rgb: double arithmetic on f and s / 255 rounded to float32, rounding as floor(x + 0.5)"""
    f32, f64 = np.float32, np.float64
    h, s, v = (hsv[..., k] for k in range(3))
    hf = h.astype(f32).astype(f64) * 6.0 / 255.0
    fl = np.floor(hf)
    f = (hf - fl).astype(f32).astype(f64)
    fs = (s.astype(f32).astype(f64) / 255.0).astype(f32).astype(f64)
    vv = v.astype(f64)
    p, q, t = (np.clip(np.floor(vv * x + 0.5), 0, 255) for x in (1.0 - fs, 1.0 - fs * f, 1.0 - fs * (1.0 - f)))
    i = fl.astype(np.int32) % 6
    out = np.stack([np.choose(i, [vv, q, p, p, t, vv]), np.choose(i, [t, vv, vv, q, p, p]), np.choose(i, [p, p, t, vv, vv, q])], -1)
    return np.where((s == 0)[..., None], vv[..., None], out).astype(np.uint8)


def test_hsv_terms_are_pillows_on_every_triple():
    """The kernels' HSV arithmetic, restated, against Pillow's convert("HSV") / convert("RGB") on all 2^24 RGB and all 2^24 HSV triples"""
    Image = pytest.importorskip("PIL.Image")
    b, c = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    for lo in range(0, 256, 32):
        cube = np.stack([np.broadcast_to(np.arange(lo, lo + 32, dtype=np.uint8)[:, None, None], (32, 256, 256)),
                         np.broadcast_to(b, (32, 256, 256)), np.broadcast_to(c, (32, 256, 256))], -1).reshape(32 * 256, 256, 3)
        cube = np.ascontiguousarray(cube)
        assert np.array_equal(_rgb2hsv_terms(cube), np.asarray(Image.fromarray(cube).convert("HSV"))), lo
        hsv = Image.merge("HSV", [Image.fromarray(np.ascontiguousarray(cube[..., k])) for k in range(3)])
        assert np.array_equal(_hsv2rgb_terms(cube), np.asarray(hsv.convert("RGB"))), lo
