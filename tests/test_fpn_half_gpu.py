"""The fp16 class of the native FPN on the GPU (csrc/fpn_conv_half.hip, ops.conv2d_bn_act_half, conv_precision / fpn_precision
"fp16"): every layer as an op, every kernel variant across tile boundaries, edge channel counts, tiny maps, determinism, aliasing,
64-bit batch offsets and overflow against the class's oracle -- float64 on the rounded operands -- within the bound derived in
tests/test_fpn_half_cpu.py; the whole module against the reference's own maps beside torch's fp16 autocast; the backbone handing
fp16 pyramids to the matcher.

Worst error / bound as measured on an MI355X is recorded in DESIGN 4.8."""
import functools

import numpy as np
import pytest
import torch

import fpn_fixture
import synth
from conftest import load_golden
from gfnet_amd import ops
from test_fpn_cpu import build_modules, run_modules
from test_fpn_gpu import LAYERS, StubVit
from test_fpn_half_cpu import CONF, CONFIGS, EDGE, half_case, shape_of

pytestmark = pytest.mark.gpu


def run_op(name, args):
    K, stride, C0, C1, Cout, up0, res, act = CONFIGS[name]
    x0, x1, w, scale, shift, _ = (None if t is None else t.cuda() for t in args)
    residual = {"x0": x0, "x1": x1, None: None}[res]
    return ops.conv2d_bn_act_half(x0, w, scale, shift, x1=x1, up0=up0, residual=residual, stride=stride, act=act, slope=0.1)


def check_case(name, B, Ho, Wo):
    args, ref, bound, _ = half_case(name, B, Ho, Wo)
    out = run_op(name, args)
    assert out.shape == ref.shape and out.dtype == torch.float16
    got = out.cpu().double()
    assert bool(torch.isfinite(got).all())
    ratio = float(((got - ref).abs() / bound).max())
    print(f"{name} {B}x{Ho}x{Wo}: worst error / bound {ratio:.3f} (max err {float((got - ref).abs().max()):.3e})")
    assert ratio <= 1.0, (name, ratio)
    return out


@pytest.mark.parametrize("name", list(LAYERS))
def test_every_layer_of_the_fpn_as_an_op(name):
    """B = 2, output 13 x 19 (the up0 layers: 14 x 22 from a 7 x 11 map; stride 2: from 25 x 37)."""
    check_case(name, *shape_of(name))


@pytest.mark.parametrize("name", ["conv00", "conv01", "conv10", "out3", "inner3", "downsample1", "downsample2", "downsample3", "conv30",
                                  "merge_layer", "inner1", "out0"])
def test_every_kernel_variant_across_tile_boundaries(name):
    """B = 1, output 72 x 136: more than one 16 x 32 tile in both directions with a tail in each; every K, both strides, up0 and x1,
    the 16-wide instruction (Cout 8 and 16) and the 32-wide one (Cout 32 and 64, one and two column tiles per workgroup)."""
    check_case(name, 1, 72, 136)


@pytest.mark.parametrize("name", list(EDGE))
def test_edge_channel_counts(name):
    """Cout 24 and 40 (padding inside a 16- or 32-wide instruction), Cin 3, 5 and 13 (a k-step that ends mid-tap) at a 9 x 35
    output (up0: 10 x 36)."""
    up0 = EDGE[name][5]
    check_case(name, 2, 10 if up0 else 9, 36 if up0 else 35)


@pytest.mark.parametrize("name", ["conv00", "conv01", "downsample1", "conv10", "out3", "downsample3", "conv30", "out0", "edge_k7_cout40"])
def test_tiny_maps(name):
    """1 x 1, 1 x 2 and 2 x 3 outputs with every K on both instructions: maps smaller than the kernel, most taps padding."""
    for Ho, Wo in ((1, 1), (1, 2), (2, 3)):
        check_case(name, 3, Ho, Wo)


@pytest.mark.parametrize("name", ["conv01", "inner2", "merge_layer", "downsample2"])
def test_identical_calls_give_identical_bits(name):
    args, _, _, _ = half_case(name, 2, 14, 22)
    assert torch.equal(run_op(name, args), run_op(name, args))


@pytest.mark.parametrize("name", ["inner1", "merge_layer", "edge_cin13_cout8"])
def test_residual_may_alias_an_input(name):
    """residual IS x1 (x0 for the merge layer) in run_op; a copy of it gives the same bits."""
    K, stride, C0, C1, Cout, up0, res, act = CONFIGS[name]
    args, _, _, _ = half_case(name, 2, 14, 22)
    x0, x1, w, scale, shift, _ = (None if t is None else t.cuda() for t in args)
    aliased = run_op(name, args)
    copied = ops.conv2d_bn_act_half(x0, w, scale, shift, x1=x1, up0=up0, residual=(x0 if res == "x0" else x1).clone(), stride=stride, act=act)
    assert torch.equal(aliased, copied)


def test_batch_offsets_are_64_bit():
    """17 images of 8 x 4096 x 4096 in fp16: 2.28e9 elements (4.6 GB) in and out, every image below 2^31 bytes.  The last image's
    result, whose offset is past 2^31 elements, equals a launch on that image alone."""
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.empty((17, 8, 4096, 4096), device="cuda", dtype=torch.float16)
    x[0] = torch.rand((8, 4096, 4096), device="cuda", generator=g) * 2 - 1
    x[1:-1] = x[0]
    x[-1] = torch.rand((8, 4096, 4096), device="cuda", generator=g) * 2 - 1
    w = torch.randn((8, 8, 1, 1), device="cuda", generator=g) * 0.35
    scale, shift = torch.rand(8, device="cuda", generator=g) + 0.5, torch.rand(8, device="cuda", generator=g) - 0.5
    out = ops.conv2d_bn_act_half(x, w, scale, shift, residual=x, act="swish")
    for i in (0, 16):
        assert torch.equal(out[i:i + 1], ops.conv2d_bn_act_half(x[i:i + 1], w, scale, shift, residual=x[i:i + 1], act="swish"))
    assert not torch.equal(out[16], out[0]) and torch.equal(out[7], out[0])
    del out, x
    torch.cuda.empty_cache()


@pytest.mark.parametrize("name", ["conv10", "out0"])
def test_overflow_is_stored_as_inf_and_nothing_is_clamped(name):
    """A scale of some 5e4 pushes part of the outputs past fp16's range.  The value before the store is within the bound's other
    terms of float64, and the store rounds to inf from 65520 on: so +-inf exactly where float64 exceeds 65520 by that margin, finite
    where it stays below by it, and no NaN anywhere."""
    args, ref, _, before_store = half_case(name, 2, 13, 19, scale_by=5e4)
    got = run_op(name, args).cpu().double()
    assert not bool(torch.isnan(got).any())
    over, under = ref.abs() > 65520 + before_store, ref.abs() < 65520 - before_store
    assert int(over.sum()) > 20 and int(under.sum()) > 20 and int((~over & ~under).sum()) < 20
    assert bool(torch.isinf(got[over]).all()) and bool((torch.sign(got[over]) == torch.sign(ref[over])).all())
    assert bool(torch.isfinite(got[under]).all())
    assert float(got[under].abs().max()) > 3e4  # large finite values beside them


def test_op_refuses_what_it_cannot_run():
    x, w, s = torch.zeros(1, 3, 8, 8, device="cuda").half(), torch.zeros(8, 3, 3, 3, device="cuda"), torch.zeros(8, device="cuda")
    with pytest.raises(TypeError, match="float16"):
        ops.conv2d_bn_act_half(x.float(), w, s, s)
    with pytest.raises(TypeError, match="float32"):
        ops.conv2d_bn_act_half(x, w, s.half(), s)
    with pytest.raises(ValueError, match="channels"):
        ops.conv2d_bn_act_half(x, w, s, s, x1=x)
    with pytest.raises(ValueError, match="residual"):
        ops.conv2d_bn_act_half(x, w, s, s, residual=x)
    with pytest.raises(Exception, match="kernel size 2"):
        ops.conv2d_bn_act_half(x, torch.zeros(8, 3, 2, 2, device="cuda"), s, s)
    with pytest.raises(Exception, match="multiple of 8"):
        ops.conv2d_bn_act_half(x, torch.zeros(12, 3, 3, 3, device="cuda"), torch.zeros(12, device="cuda"), torch.zeros(12, device="cuda"))
    from gfnet_amd.model import fpn

    layer = fpn.Conv2d(3, 12, 3, padding=1, conv_precision="fp16").cuda().train(False)
    with pytest.raises(NotImplementedError, match=r"Conv2d\(3, 12"):
        layer(x.float())


@functools.lru_cache(maxsize=None)
def module_runs(shape_name):
    """(fp16 class, torch path under fp16 autocast) maps of the whole module on the GPU for one fixture shape."""
    mods, _ = build_modules()
    images, side = (t.cuda() for t in fpn_fixture.inputs(shape_name))
    for m in mods.values():
        m.cuda()
        m.conv_precision = "fp16"
    with torch.no_grad():
        hip = run_modules(mods, images, side)
        for m in mods.values():
            m.conv_impl = "torch"
        with torch.autocast("cuda", dtype=torch.float16):
            ref = run_modules(mods, images, side)
    return hip, ref


@pytest.mark.parametrize("shape_name", [s[0] for s in fpn_fixture.SHAPES])
def test_whole_module_against_the_reference_modules_maps_beside_fp16_autocast(shape_name):
    """Every map fp16, and its error against the reference's own maps at most 2 x the error of the module's torch path under
    torch.autocast("cuda", dtype=torch.float16) on the same GPU against the same maps: the comparison and the margin of
    tests/test_vit_gpu.py for its 16-bit classes."""
    g = load_golden("g15_fpn")
    hip, ref = module_runs(shape_name)
    for k in fpn_fixture.MAPS:
        want = g[f"{shape_name}/{k}"]
        assert hip[k].dtype == torch.float16 and tuple(hip[k].shape) == tuple(g[f"{shape_name}/{k}/shape"])
        e_hip = float(np.abs(fpn_fixture.stored(k, hip[k]).cpu().numpy().astype(np.float64) - want).max())
        e_tor = float(np.abs(fpn_fixture.stored(k, ref[k]).cpu().numpy().astype(np.float64) - want).max())
        print(f"{shape_name}/{k}: fp16 class err {e_hip:.3e}  torch fp16 autocast err {e_tor:.3e}  margin {2 * e_tor:.3e}")
        assert e_hip <= 2 * e_tor, (shape_name, k, e_hip, e_tor)


def test_module_keeps_fp32_in_training_mode_and_on_the_torch_path():
    mods, _ = build_modules()
    enc = mods["encoder"].cuda()
    enc.conv_precision = "fp16"
    images = fpn_fixture.inputs("b")[0].cuda()
    with torch.no_grad():
        assert enc(images)[3].dtype == torch.float16
        enc.conv_impl = "torch"
        assert enc(images)[3].dtype == torch.float32
    enc.conv_impl = "hip"
    enc.train(True)
    out = enc(images)[3]
    assert out.dtype == torch.float32 and out.requires_grad


def test_backbone_hands_fp16_pyramids_to_the_matcher():
    """Five fp16 levels of the right shapes, no widened copy; match_batch on them gives bit for bit the warp of the same pyramids
    widened to fp32 -- the post-backbone path's own statement about fp16 maps (tests/test_configs_gpu.py: all arithmetic stays fp32,
    so reading fp16 maps as stored equals reading their widened copy)."""
    from gfnet_amd.model.network import GFNet
    from gfnet_amd.reference_backbone import ReferenceBackbone

    torch.manual_seed(0)
    bb = ReferenceBackbone(CONF, vit=StubVit(), decoder="hip", fpn="hip", fpn_precision="fp16").cuda()
    fpn_fixture.fill({"encoder": bb.encoder, "decoder": bb.decoder, "merge_layer": bb.merge_layer})
    bb.train(False)
    images = torch.from_numpy(synth.lattice_uniform((2, 3, 448, 448), 77)).cuda()
    with torch.no_grad():
        pa, pb = bb(images)
    want = {"16": (1, 64, 32, 32), "8": (1, 64, 56, 56), "4": (1, 32, 112, 112), "2": (1, 16, 224, 224), "1": (1, 8, 448, 448)}
    for p in (pa, pb):
        assert {k: tuple(v.shape) for k, v in p.items()} == want
        assert all(v.dtype == torch.float16 and v.is_contiguous() and bool(torch.isfinite(v).all()) for v in p.values())
    model = GFNet(CONF, backbone=bb, upsample_preds=False).cuda()
    model.train(False)
    with torch.no_grad():
        warp, cert = model.match_batch(images[:1] * 0.5 + 0.5, images[1:] * 0.5 + 0.5)  # the backbone inside, fp16 levels, no cast pass
        warp16, cert16 = model.match_pyramids(pa, pb, batched=True)
        warp32, cert32 = model.match_pyramids({k: v.float() for k, v in pa.items()}, {k: v.float() for k, v in pb.items()}, batched=True)
    assert warp.shape == warp16.shape and bool(torch.isfinite(warp).all()) and bool(torch.isfinite(cert).all())
    assert torch.equal(warp16, warp32) and torch.equal(cert16, cert32)
