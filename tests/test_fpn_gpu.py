"""The fused FPN convolution (csrc/fpn_conv.hip) and the native pyramid on the GPU: every layer of the FPN as an op and every kernel
variant across a tile boundary against the definition in float64, the whole module against the reference's own maps
(tests/golden/g15_fpn.npz) and against its torch path, determinism, aliasing, 64-bit batch offsets and the backbone assembly.

The unit of the per-layer bound is e32: the error of the SAME definition evaluated in fp32 by torch on the CPU against float64, over
the whole tensor; the kernel may take 4 x e32."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fpn_fixture
import synth
from conftest import load_golden
from gfnet_amd import ops
from test_fpn_cpu import build_modules, check_against_golden, run_modules

pytestmark = pytest.mark.gpu

# name: (K, stride, C0, C1, Cout, up0, residual ("x0", "x1" or None), act): the 19 layers of the shipped FPN (feat_chs 8, 16, 32, 64)
LAYERS = {
    "conv00": (7, 1, 3, 0, 8, False, None, "leaky_relu"), "conv01": (5, 1, 8, 0, 8, False, None, "leaky_relu"),
    "downsample1": (5, 2, 8, 0, 16, False, None, "leaky_relu"), "conv10": (3, 1, 16, 0, 16, False, None, "leaky_relu"),
    "conv11": (3, 1, 16, 0, 16, False, None, "leaky_relu"), "downsample2": (5, 2, 16, 0, 32, False, None, "leaky_relu"),
    "conv20": (3, 1, 32, 0, 32, False, None, "leaky_relu"), "conv21": (3, 1, 32, 0, 32, False, None, "leaky_relu"),
    "downsample3": (3, 2, 32, 0, 64, False, None, "leaky_relu"), "conv30": (3, 1, 64, 0, 64, False, None, "leaky_relu"),
    "conv31": (3, 1, 64, 0, 64, False, None, "leaky_relu"), "merge_layer": (3, 1, 64, 64, 64, False, "x0", "swish"),
    "out0": (1, 1, 64, 0, 64, False, None, "swish"), "inner1": (3, 1, 64, 32, 32, True, "x1", "swish"),
    "out1": (1, 1, 32, 0, 32, False, None, "swish"), "inner2": (3, 1, 32, 16, 16, True, "x1", "swish"),
    "out2": (1, 1, 16, 0, 16, False, None, "swish"), "inner3": (3, 1, 16, 8, 8, True, "x1", "swish"),
    "out3": (1, 1, 8, 0, 8, False, None, "swish"),
}
# outside the FPN: Cout no multiple of 8 takes the general kernel
GENERAL = {
    "general_s2": (3, 2, 5, 0, 3, False, None, "leaky_relu"), "general_up": (5, 1, 3, 5, 5, True, "x1", "swish"),
    "general_k7": (7, 1, 2, 0, 1, False, None, None),
}
CONFIGS = {**LAYERS, **GENERAL}


def definition(x0, x1, w, scale, shift, residual, stride, up0, act):
    """out = act(conv(cat(x0', x1), w) * scale + shift) + residual in the dtype of the arguments."""
    if up0:
        x0 = F.interpolate(x0, scale_factor=2, mode="bilinear", align_corners=False)
    x = x0 if x1 is None else torch.cat((x0, x1), dim=1)
    y = F.conv2d(x, w, stride=stride, padding=w.shape[-1] // 2) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
    if act == "leaky_relu":
        y = F.leaky_relu(y, 0.1)
    elif act == "swish":
        y = y * torch.sigmoid(y)
    return y if residual is None else y + residual


@functools.lru_cache(maxsize=None)
def case(name, B, Ho, Wo):
    """Inputs of layer `name` for an output of (B, Cout, Ho, Wo), the float64 result and e32.  Computed once, never modified."""
    K, stride, C0, C1, Cout, up0, res, act = CONFIGS[name]
    seed = 100 + 11 * sorted(CONFIGS).index(name)
    H, W = (Ho, Wo) if stride == 1 else (2 * Ho - 1, 2 * Wo - 1)  # odd inputs under stride 2
    x0 = torch.from_numpy(synth.lattice_normalish((B, C0, H // 2, W // 2) if up0 else (B, C0, H, W), seed))
    x1 = torch.from_numpy(synth.lattice_normalish((B, C1, H, W), seed + 1)) if C1 else None
    w = torch.from_numpy(synth.lattice_normalish((Cout, C0 + C1, K, K), seed + 2) * np.float32(0.87 / np.sqrt((C0 + C1) * K * K)))
    scale = torch.from_numpy(np.float32(0.9) + np.float32(0.5) * synth.lattice_uniform((Cout,), seed + 3))
    shift = torch.from_numpy(np.float32(0.4) * synth.lattice_uniform((Cout,), seed + 4))
    residual = {"x0": x0, "x1": x1, None: None}[res]
    args = (x0, x1, w, scale, shift, residual)
    ref = definition(*(None if t is None else t.double() for t in args), stride, up0, act)
    e32 = float((definition(*args, stride, up0, act).double() - ref).abs().max())
    assert tuple(ref.shape) == (B, Cout, Ho, Wo) and e32 < 1e-5, (name, tuple(ref.shape), e32)
    return args, ref, e32


def run_op(name, args):
    K, stride, C0, C1, Cout, up0, res, act = CONFIGS[name]
    x0, x1, w, scale, shift, _ = (None if t is None else t.cuda() for t in args)
    residual = {"x0": x0, "x1": x1, None: None}[res]
    return ops.conv2d_bn_act(x0, w, scale, shift, x1=x1, up0=up0, residual=residual, stride=stride, act=act, slope=0.1)


def check_case(name, B, Ho, Wo, floor=False):
    """floor: for maps of a handful of values, where e32 can be zero by luck, the unit is at least one rounding of the largest output."""
    args, ref, e32 = case(name, B, Ho, Wo)
    if floor:
        e32 = max(e32, 2.0 ** -24 * float(ref.abs().max()))
    assert floor or e32 > 1e-8, (name, e32)
    out = run_op(name, args)
    assert out.shape == ref.shape and out.dtype == torch.float32
    err = float((out.cpu().double() - ref).abs().max())
    print(f"{name} {B}x{Ho}x{Wo}: max err {err:.3e}, e32 {e32:.3e}, ratio {err / e32:.2f}")
    assert err <= 4 * e32, (name, err, e32)
    return out


@pytest.mark.parametrize("name", list(LAYERS))
def test_every_layer_of_the_fpn_as_an_op(name):
    """B = 2, output 13 x 19 (the up0 layers: 14 x 22 from a 7 x 11 map; stride 2: from 25 x 37)."""
    up0 = LAYERS[name][5]
    check_case(name, 2, 14 if up0 else 13, 22 if up0 else 19)


@pytest.mark.parametrize("name", ["conv00", "conv01", "inner3", "out3", "conv30", "merge_layer", "downsample1", "downsample3", "general_s2"])
def test_every_kernel_variant_across_a_tile_boundary(name):
    """B = 1, output 72 x 136: more than one tile (32 wide, 64 high for 8 output channels, 32 high otherwise) in both directions
    with a tail, the 8- and 16-channel instantiations, both strides, the Cout = 64 layers (four channel groups per tile, the sum
    split by stage) and the general kernel."""
    check_case(name, 1, 72, 136)


@pytest.mark.parametrize("name", list(GENERAL))
def test_general_kernel_on_small_shapes(name):
    up0 = GENERAL[name][5]
    check_case(name, 2, 14 if up0 else 13, 22 if up0 else 19)


def test_tiny_maps_and_single_pixels():
    """H = W = 1 and maps smaller than the kernel: every tap but the centre is padding."""
    for name in ("conv00", "downsample1", "out3", "general_k7"):
        check_case(name, 1, 1, 1, floor=True)
        check_case(name, 3, 2, 3, floor=True)
    check_case("inner3", 1, 2, 2, floor=True)


@pytest.mark.parametrize("name", ["conv01", "inner2", "merge_layer", "downsample2", "general_up"])
def test_identical_calls_give_identical_bits(name):
    args, _, _ = case(name, 2, 14, 22)
    assert torch.equal(run_op(name, args), run_op(name, args))


@pytest.mark.parametrize("name", ["inner1", "merge_layer", "general_up"])
def test_residual_may_alias_an_input(name):
    """residual IS x1 (x0 for the merge layer) in run_op; a copy of it gives the same bits."""
    K, stride, C0, C1, Cout, up0, res, act = CONFIGS[name]
    args, _, _ = case(name, 2, 14, 22)
    x0, x1, w, scale, shift, _ = (None if t is None else t.cuda() for t in args)
    aliased = ops.conv2d_bn_act(x0, w, scale, shift, x1=x1, up0=up0, residual=x0 if res == "x0" else x1, stride=stride, act=act)
    copied = ops.conv2d_bn_act(x0, w, scale, shift, x1=x1, up0=up0, residual=(x0 if res == "x0" else x1).clone(), stride=stride, act=act)
    assert torch.equal(aliased, copied)


def test_batch_offsets_are_64_bit():
    """17 images of 8 x 4096 x 4096: 2.28e9 elements (9.1 GB) in and out, every image below 2^31 bytes.  The last image's result,
    whose offset is past 2^31 elements, equals a launch on that image alone."""
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.empty((17, 8, 4096, 4096), device="cuda", dtype=torch.float32)
    x[0].uniform_(-1, 1, generator=g)
    x[1:-1] = x[0]
    x[-1].uniform_(-1, 1, generator=g)
    w = torch.randn((8, 8, 1, 1), device="cuda", generator=g) * 0.35
    scale, shift = torch.rand(8, device="cuda", generator=g) + 0.5, torch.rand(8, device="cuda", generator=g) - 0.5
    out = ops.conv2d_bn_act(x, w, scale, shift, residual=x, act="swish")
    for i in (0, 16):
        assert torch.equal(out[i:i + 1], ops.conv2d_bn_act(x[i:i + 1], w, scale, shift, residual=x[i:i + 1], act="swish"))
    assert not torch.equal(out[16], out[0]) and torch.equal(out[7], out[0])
    del out, x
    torch.cuda.empty_cache()


def test_op_refuses_what_it_cannot_run():
    x, w, s = torch.zeros(1, 3, 8, 8, device="cuda"), torch.zeros(8, 3, 3, 3, device="cuda"), torch.zeros(8, device="cuda")
    with pytest.raises(TypeError, match="float32"):
        ops.conv2d_bn_act(x.half(), w, s, s)
    with pytest.raises(TypeError, match="contiguous"):
        ops.conv2d_bn_act(x.permute(0, 1, 3, 2)[:, :, :, ::2], w, s, s)
    with pytest.raises(ValueError, match="channels"):
        ops.conv2d_bn_act(x, w, s, s, x1=x)
    with pytest.raises(ValueError, match="residual"):
        ops.conv2d_bn_act(x, w, s, s, residual=x)
    with pytest.raises(Exception, match="kernel size 2"):
        ops.conv2d_bn_act(x, torch.zeros(8, 3, 2, 2, device="cuda"), s, s)


@functools.lru_cache(maxsize=None)
def module_runs(shape_name):
    """(HIP path, torch path) maps of the whole module on the GPU for one fixture shape."""
    mods, _ = build_modules()
    images, side = (t.cuda() for t in fpn_fixture.inputs(shape_name))
    for m in mods.values():
        m.cuda()
    with torch.no_grad():
        hip = run_modules(mods, images, side)
        for m in mods.values():
            m.conv_impl = "torch"
        ref = run_modules(mods, images, side)
    return hip, ref


@pytest.mark.parametrize("shape_name", [s[0] for s in fpn_fixture.SHAPES])
def test_whole_module_on_the_hip_path_against_the_reference_modules_maps(shape_name):
    check_against_golden(module_runs(shape_name)[0], shape_name, load_golden("g15_fpn"))


@pytest.mark.parametrize("shape_name", [s[0] for s in fpn_fixture.SHAPES])
def test_hip_path_against_the_modules_own_torch_path(shape_name):
    g = load_golden("g15_fpn")
    hip, ref = module_runs(shape_name)
    for k in fpn_fixture.MAPS:
        bound = 4 * float(g[f"{shape_name}/{k}/fp32_vs_fp64"])
        err = float((hip[k] - ref[k]).abs().max())
        print(f"{shape_name}/{k}: hip vs torch {err:.3e}, bound {bound:.3e}")
        assert hip[k].shape == ref[k].shape and err <= bound, (k, err, bound)


def test_module_takes_the_torch_path_in_training_mode_and_the_fold_follows_load_state_dict():
    mods, _ = build_modules()
    enc = mods["encoder"].cuda()
    images = fpn_fixture.inputs("b")[0].cuda()
    with torch.no_grad():
        first = enc(images)[3]
        state = {k: (v * 2 if k.endswith("running_var") else v) for k, v in enc.state_dict().items()}
        enc.load_state_dict(state, strict=True)
        second = enc(images)[3]
        enc.conv_impl = "torch"
        want = enc(images)[3]
    assert not torch.equal(first, second)
    assert float((second - want).abs().max()) <= 4 * float(load_golden("g15_fpn")["b/enc8/fp32_vs_fp64"])
    enc.conv_impl = "hip"
    enc.train(True)
    out = enc(images)[3]
    assert out.requires_grad  # batch statistics through torch ops: differentiable


class StubVit(torch.nn.Module):
    """A 14 x 14 patch embedding to 32-dim tokens: what ReferenceBackbone needs of a ViT."""

    def __init__(self):
        super().__init__()
        self.embed = torch.nn.Conv2d(3, 32, 14, stride=14)

    def forward_features(self, x):
        return {"x_norm_patchtokens": self.embed(x).flatten(2).transpose(1, 2)}


def test_backbone_with_native_fpn_and_decoder_feeds_the_matcher():
    from gfnet_amd.model.network import GFNet
    from gfnet_amd.reference_backbone import ReferenceBackbone

    conf = {"dino_cfg": {"d_model": 32,
                         "decoder_cfg": {"num_cross_attn": 2, "init_values": 1.0, "prev_values": 0.5, "nhead": 8, "attention_type": "FLASH2",
                                         "ffn_type": "ffn", "softmax_scale": "entropy_invariance", "train_avg_length": 1024,
                                         "self_cross_types": None, "post_norm": False, "pre_norm_query": True, "no_combine_norm": False}},
            "encoder_cfg": {"feat_chs": [64, 32, 16, 8]},
            "matcher": {"num_grid": [32, 32, 64, 128, 256], "radius": [7, 6, 4, 2, 0], "displacement_dim": [64, 64, 32, 16, 8],
                        "num_itr": [1, 1, 1, 1, 1]}}
    torch.manual_seed(0)
    bb = ReferenceBackbone(conf, vit=StubVit(), decoder="hip", fpn="hip").cuda()
    fpn_fixture.fill({"encoder": bb.encoder, "decoder": bb.decoder, "merge_layer": bb.merge_layer})
    bb.train(False)
    images = torch.from_numpy(synth.lattice_uniform((2, 3, 448, 448), 77)).cuda()
    with torch.no_grad():
        pa, pb = bb(images)
        for m in (bb.encoder, bb.decoder, bb.merge_layer):
            m.conv_impl = "torch"
        ta, tb = bb(images)
        for m in (bb.encoder, bb.decoder, bb.merge_layer):
            m.conv_impl = "hip"
    want = {"16": (1, 64, 32, 32), "8": (1, 64, 56, 56), "4": (1, 32, 112, 112), "2": (1, 16, 224, 224), "1": (1, 8, 448, 448)}
    g = load_golden("g15_fpn")
    for got, ref in ((pa, ta), (pb, tb)):
        assert {k: tuple(v.shape) for k, v in got.items()} == want
        for k, m in (("8", "dec8"), ("4", "dec4"), ("2", "dec2"), ("1", "dec1")):
            bound = 4 * max(float(g[f"{s}/{m}/fp32_vs_fp64"]) for s in "ab")
            err = float((got[k] - ref[k]).abs().max())
            print(f"pyramid {k}: hip vs torch {err:.3e}, bound {bound:.3e}")
            assert err <= bound, (k, err, bound)
    model = GFNet(conf, backbone=bb).cuda()
    model.train(False)
    with torch.no_grad():
        corresps = model({"im_A": images[:1], "im_B": images[1:]})
    last = corresps["1"][1]
    assert tuple(last["flow"].shape) == (1, 2, 256, 256) and bool(torch.isfinite(last["flow"]).all())
