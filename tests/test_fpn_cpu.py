"""The native FPN pyramid as far as it goes without a GPU: the module's torch path against the reference's own modules
(tests/golden/g15_fpn.npz, made by tests/golden/make_golden_fpn.py), its training mode, the opt-in wiring into the reference backbone
and the C ABI's refusals."""
import ctypes
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

import fpn_fixture
from conftest import ROOT, load_golden
from gfnet_amd import _lib
from gfnet_amd.model import fpn


def build_modules(conv_impl="hip"):
    """The three modules with the fixture's parameters, in eval mode, and the sorted key list."""
    chs = fpn_fixture.FEAT_CHS
    mods = {"encoder": fpn.FPNEncoder(chs, conv_impl=conv_impl), "decoder": fpn.FPNDecoder_concat(chs, conv_impl=conv_impl),
            "merge_layer": fpn.merge_layer(chs[-1], conv_impl=conv_impl)}
    keys = fpn_fixture.fill(mods)
    for m in mods.values():
        m.train(False)
    return mods, keys


def run_modules(mods, images, side):
    c0, c1, c2, c3 = mods["encoder"](images)
    c3 = mods["merge_layer"](c3, side)
    return dict(zip(fpn_fixture.MAPS, [c0, c1, c2, c3] + list(mods["decoder"](c0, c1, c2, c3))))


def check_against_golden(got, shape_name, g, factor=4):
    """Every map within factor x the reference's own fp32-vs-float64 difference of the recorded reference map."""
    for k in fpn_fixture.MAPS:
        want, e32 = g[f"{shape_name}/{k}"], float(g[f"{shape_name}/{k}/fp32_vs_fp64"])
        assert 1e-7 < e32 < 1e-5, (k, e32)  # a unit of fp32 rounding on these maps, not zero and not a blunder
        assert tuple(got[k].shape) == tuple(g[f"{shape_name}/{k}/shape"])
        err = float(np.abs(fpn_fixture.stored(k, got[k]).cpu().numpy().astype(np.float64) - want).max())
        print(f"{shape_name}/{k}: max err {err:.3e}, bound {factor * e32:.3e}")
        assert err <= factor * e32, (shape_name, k, err, factor * e32)


def test_state_dict_keys_are_the_references():
    g = load_golden("g15_fpn")
    mods, keys = build_modules()
    assert keys == [str(k) for k in g["keys"]]
    for want in ("encoder.conv00.conv.weight", "encoder.conv00.bn.running_mean", "decoder.out0.0.weight", "decoder.out0.0.bias",
                 "decoder.out0.1.running_var", "decoder.inner1.0.weight", "merge_layer.0.bias", "merge_layer.1.weight"):
        assert want in keys
    assert "encoder.conv00.conv.bias" not in keys  # FPN.py:113: no conv bias in front of a BatchNorm
    assert tuple(mods["decoder"].inner3[0].weight.shape) == (8, 24, 3, 3) and tuple(mods["merge_layer"][0].weight.shape) == (64, 128, 3, 3)


@pytest.mark.parametrize("shape_name", [s[0] for s in fpn_fixture.SHAPES])
def test_torch_path_reproduces_the_reference_modules_maps(shape_name):
    """fp32 on the CPU (where the module takes its torch path whatever conv_impl says) against the reference's fp32 maps: all eight
    within 4 x the reference's own fp32-vs-float64 difference, the convention of test_cross_attn_cpu.py."""
    g = load_golden("g15_fpn")
    mods, _ = build_modules()
    images, side = fpn_fixture.inputs(shape_name)
    with torch.no_grad():
        got = run_modules(mods, images, side)
    check_against_golden(got, shape_name, g)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "g15_fpn.npz")) <= 400 * 1024


def test_fold_is_the_eval_batchnorm_and_follows_load_state_dict():
    """scale / shift of the HIP path, applied by hand in float64, give the module's own eval output -- also after new statistics are
    loaded (nothing cached)."""
    mods, _ = build_modules()
    images, _ = fpn_fixture.inputs("b")
    layer, head = mods["encoder"].conv00, mods["decoder"].out3
    x8 = torch.from_numpy(fpn_fixture.synth.lattice_uniform((1, 8, 6, 5), 3))
    for _ in range(2):
        with torch.no_grad():
            s, b = fpn._fold(layer.conv, layer.bn)
            want = layer.bn(layer.conv(images))
            got = torch.nn.functional.conv2d(images.double(), layer.conv.weight.double(), padding=3) * s.double().view(1, -1, 1, 1) + b.double().view(1, -1, 1, 1)
            assert float((got - want).abs().max()) < 5e-6
            s, b = fpn._fold(head[0], head[1])  # with a conv bias
            want = head[1](head[0](x8))
            got = torch.nn.functional.conv2d(x8.double(), head[0].weight.double()) * s.double().view(1, -1, 1, 1) + b.double().view(1, -1, 1, 1)
            assert float((got - want).abs().max()) < 5e-6
        state = {k: (v * 1.5 if k.endswith("running_var") else v) for k, v in mods["encoder"].state_dict().items()}
        mods["encoder"].load_state_dict(state, strict=True)
        state = {k: (v + 0.25 if k.endswith("running_mean") or k.endswith("0.bias") else v) for k, v in mods["decoder"].state_dict().items()}
        mods["decoder"].load_state_dict(state, strict=True)


def test_training_mode_has_gradients_for_every_parameter_and_moves_the_buffers():
    mods, _ = build_modules()
    for m in mods.values():
        m.train(True)
    before = {f"{top}.{k}": v.clone() for top, m in mods.items() for k, v in m.named_buffers()}
    images, side = fpn_fixture.inputs("b")
    out = run_modules(mods, images, side)
    sum(v.square().mean() for v in out.values()).backward()
    for top, m in mods.items():
        for k, p in m.named_parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all(), (top, k)
            # (a conv bias in front of a batch-statistics BatchNorm cancels in the mean: its gradient is rounding noise around 0)
            assert k.endswith("0.bias") or float(p.grad.abs().max()) > 1e-6, (top, k)
    after = {f"{top}.{k}": v for top, m in mods.items() for k, v in m.named_buffers()}
    assert len(after) == 3 * 19
    for k, v in after.items():
        assert not torch.equal(v, before[k]), k  # running_mean, running_var and num_batches_tracked of all 19 BatchNorms
    assert float(mods["encoder"].conv00.bn.momentum) == 0.1


def test_sizes_and_settings_that_are_refused():
    mods, _ = build_modules()
    for shape in ((1, 3, 40, 60), (1, 3, 36, 56), (1, 3, 7, 8)):
        with pytest.raises(ValueError, match=str(shape[2]) + ", " + str(shape[3])):
            mods["encoder"](torch.zeros(shape))
    with pytest.raises(ValueError, match="double"):
        mods["decoder"](torch.zeros(1, 8, 40, 56), torch.zeros(1, 16, 20, 28), torch.zeros(1, 32, 10, 14), torch.zeros(1, 64, 5, 8))
    with pytest.raises(NotImplementedError, match="norm_type"):
        fpn.FPNEncoder(fpn_fixture.FEAT_CHS, norm_type="IN")
    with pytest.raises(NotImplementedError, match="norm_type"):
        fpn.Conv2d(3, 8, 3, norm_type="IN")
    with pytest.raises(ValueError, match="conv_impl"):
        fpn.FPNDecoder_concat(fpn_fixture.FEAT_CHS, conv_impl="miopen")


def test_abi_declares_the_entry_point_and_refuses_bad_arguments_before_any_launch():
    """Argument errors return before any HIP call, so this runs without a GPU; the dummy pointers are never read."""
    vp, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert _lib.PROTOTYPES["gfn_conv2d_bn_act_fwd"] == (i, [vp, i, i, vp, i, vp, vp, vp, vp, vp, i, i, i, i, i, i, i, f, vp])
    assert "gfn_conv2d_bn_act_fwd" in _lib.STATUS_FUNCS
    L = _lib.lib()
    assert L.gfn_abi_version() == 1
    buf = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p(ctypes.addressof(buf))

    def call(x0=p, C0=3, up0=0, x1=None, C1=0, weight=p, scale=p, shift=p, residual=None, out=p, B=1, H=8, W=8, Cout=8, K=3, stride=1,
             act=1):
        return L.gfn_conv2d_bn_act_fwd(x0, C0, up0, x1, C1, weight, scale, shift, residual, out, B, H, W, Cout, K, stride, act, 0.1, None)

    bad = [(dict(x0=None), "null"), (dict(weight=None), "null"), (dict(scale=None), "null"), (dict(shift=None), "null"),
           (dict(out=None), "null"), (dict(C1=4), "null"),                    # x1 missing although C1 > 0
           (dict(K=2), "kernel size 2"), (dict(K=9), "kernel size 9"), (dict(stride=3), "stride 3"), (dict(stride=0), "stride 0"),
           (dict(act=3), "act 3"), (dict(act=-1), "act -1"),
           (dict(up0=1, H=7), "even"), (dict(up0=1, W=9), "even"),
           (dict(C0=1, H=32768, W=16384), "2^31"),                           # x0 of exactly 2^31 bytes per image
           (dict(C0=1, Cout=256, H=2048, W=1024), "2^31"),                   # the output map
           (dict(C1=64, x1=p, H=4096, W=2048), "2^31"),                      # x1
           (dict(Cout=0), "Cout"), (dict(Cout=257), "Cout"), (dict(C0=0), "C0"), (dict(H=0), "H=0")]
    for kwargs, text in bad:
        assert call(**kwargs) == _lib.ERR_INVALID_ARG == -1, kwargs
        assert text in L.gfn_last_error().decode(), (kwargs, L.gfn_last_error().decode())
    assert call(B=0) == _lib.OK == 0
    assert call(B=0, x0=None, out=None) == 0  # an empty batch reads nothing
    with pytest.raises(_lib.GfnError, match="gfn_conv2d_bn_act_fwd failed"):
        _lib.checked().gfn_conv2d_bn_act_fwd(p, 3, 0, None, 0, p, p, p, None, p, 1, 8, 8, 8, 4, 1, 0, 0.1, None)


def test_op_refuses_cpu_tensors_and_wrong_shapes():
    from gfnet_amd import ops

    x, w, s = torch.zeros(1, 3, 8, 8), torch.zeros(8, 3, 3, 3), torch.zeros(8)
    with pytest.raises(_lib.GfnError, match="no CPU path"):
        ops.conv2d_bn_act(x, w, s, s)
    with pytest.raises(ValueError, match="act"):
        ops.conv2d_bn_act(x, w, s, s, act="relu")


# a stand-in checkout written here WITHOUT model/FPN.py and without the decoder module: with decoder="hip", fpn="hip" nothing of it
# is needed
STANDIN = {"model/__init__.py": ""}

CHILD = """
import os, sys
import numpy as np
import torch
sys.path.insert(0, os.environ["GFNET_TEST_GOLDEN_DIR"])
import fpn_fixture
keys = [str(k) for k in np.load(os.path.join(os.environ["GFNET_TEST_GOLDEN_DIR"], "g15_fpn.npz"))["keys"]]
conf = {"dino_cfg": {"d_model": 32,
                     "decoder_cfg": {"num_cross_attn": 2, "init_values": 1.0, "prev_values": 0.5, "nhead": 8, "attention_type": "FLASH2",
                                     "ffn_type": "ffn", "softmax_scale": "entropy_invariance", "train_avg_length": 1024,
                                     "self_cross_types": None, "post_norm": False, "pre_norm_query": True, "no_combine_norm": False}},
        "encoder_cfg": {"feat_chs": [64, 32, 16, 8]},
        "matcher": {"num_grid": [32, 32, 64, 128, 256], "radius": [7, 6, 4, 2, 0], "displacement_dim": [64, 64, 32, 16, 8],
                    "num_itr": [1, 1, 1, 1, 1]}}
vit = torch.nn.Linear(1, 1)
import compat
from gfnet_amd.model import fpn
from gfnet_amd.model.crossview_decoder import CrossViewDecoder
assert compat.FPNEncoder is fpn.FPNEncoder and compat.FPNDecoder_concat is fpn.FPNDecoder_concat and compat.merge_layer is fpn.merge_layer
assert compat.Swish is fpn.Swish and compat.Conv2d is fpn.Conv2d
"""


def _child(code, tmp_path, env=None):
    root = tmp_path / "checkout"
    for rel, text in STANDIN.items():
        f = root / rel
        f.parent.mkdir(parents=True, exist_ok=True)
        f.write_text(text)
    e = dict(os.environ)
    for k in ("GFNET_COMPAT_BACKBONE", "GFNET_COMPAT_DECODER", "GFNET_COMPAT_FPN"):
        e.pop(k, None)
    e["PYTHONPATH"] = os.pathsep.join([os.path.join(ROOT, "compat"), ROOT, str(root)])
    e["GFNET_TEST_GOLDEN_DIR"] = os.path.join(ROOT, "tests", "golden")
    e.update(env or {})
    script = tmp_path / "child.py"
    script.write_text(CHILD + textwrap.dedent(code))
    r = subprocess.run([sys.executable, str(script)], env=e, capture_output=True, text=True, cwd="/", timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip().endswith("ok")


def test_wiring_fpn_hip_builds_the_native_pyramid_without_a_checkouts_fpn(tmp_path):
    _child("""
    assert compat.checkout_available("hip", "hip") and compat.checkout_available(decoder="hip", fpn="hip")
    assert not compat.checkout_available("hip") and not compat.checkout_available("hip", "checkout") and not compat.checkout_available()
    bb = compat.reference_backbone(conf, vit=vit, decoder="hip", fpn="hip")
    assert type(bb.encoder) is fpn.FPNEncoder and type(bb.decoder) is fpn.FPNDecoder_concat and type(bb.merge_layer) is fpn.merge_layer
    assert type(bb.dino_decoder) is CrossViewDecoder
    assert bb.encoder.conv_impl == bb.decoder.conv_impl == bb.merge_layer.conv_impl == "hip"
    assert "model.FPN" not in sys.modules and "model.crossview_decoder_light" not in sys.modules
    own = sorted(k for k in bb.state_dict() if not k.startswith("dino_decoder."))
    assert own == keys, set(own) ^ set(keys)
    # a state dict under the reference's names loads strictly (the decoder's entries are the module's own)
    src = {"encoder": fpn.FPNEncoder(fpn_fixture.FEAT_CHS), "decoder": fpn.FPNDecoder_concat(fpn_fixture.FEAT_CHS),
           "merge_layer": fpn.merge_layer(64)}
    fpn_fixture.fill(src)
    state = {f"{top}.{k}": v for top, m in src.items() for k, v in m.state_dict().items()}
    state.update({k: v for k, v in bb.state_dict().items() if k.startswith("dino_decoder.")})
    res = bb.load_state_dict(state, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert torch.equal(bb.encoder.conv00.bn.running_var, src["encoder"].conv00.bn.running_var)
    assert torch.equal(bb.merge_layer[0].bias, src["merge_layer"][0].bias)
    # the assembly runs end to end on the CPU (torch path) and hands out the five levels
    class Vit(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.zeros(1))
        def forward_features(self, x):
            B, _, H, W = x.shape
            return {"x_norm_patchtokens": torch.ones(B, (H // 14) * (W // 14), 32) * x.mean()}
    bb2 = compat.ReferenceBackbone(conf, vit=Vit(), decoder="hip", fpn="hip", amp=False)
    bb2.dino_decoder.attn_impl = "torch"
    for blk in bb2.dino_decoder.cross_attn_blocks:
        blk.attn.attn_impl = "torch"
    bb2.train(False)
    with torch.no_grad():
        pa, pb = bb2(torch.rand(2, 3, 56, 56))
    assert {k: tuple(v.shape) for k, v in pa.items()} == {"16": (1, 64, 4, 4), "8": (1, 64, 7, 7), "4": (1, 32, 14, 14),
                                                          "2": (1, 16, 28, 28), "1": (1, 8, 56, 56)}
    try:
        compat.reference_backbone(conf, vit=vit, decoder="hip", fpn="checkout")
    except ImportError as e:
        assert "FPN" in str(e)
    else:
        raise AssertionError("fpn='checkout' must ask for the checkout's model.FPN")
    try:
        compat.reference_backbone(conf, vit=vit, decoder="hip")  # the default is the checkout's FPN, as before
    except ImportError as e:
        assert "FPN" in str(e)
    else:
        raise AssertionError("the default must still ask for the checkout's model.FPN")
    for make in (compat.reference_backbone, compat.ReferenceBackbone):
        try:
            make(conf, vit=vit, decoder="hip", fpn="x")
        except ValueError as e:
            assert "fpn" in str(e)
        else:
            raise AssertionError("unknown fpn accepted")
    print("ok")
    """, tmp_path)


def test_wiring_environment_switch_on_the_reference_constructor_path(tmp_path):
    _child("""
    import gfnet_amd.reference_backbone as rb
    rb._build_vit = lambda w: vit
    from model.network import GFNet
    model = GFNet(conf=conf)
    assert type(model.backbone.encoder) is fpn.FPNEncoder and type(model.backbone.decoder) is fpn.FPNDecoder_concat
    assert type(model.backbone.merge_layer) is fpn.merge_layer and type(model.backbone.dino_decoder) is CrossViewDecoder
    assert "model.FPN" not in sys.modules
    print("ok")
    """, tmp_path, env={"GFNET_COMPAT_BACKBONE": "reference", "GFNET_COMPAT_DECODER": "hip", "GFNET_COMPAT_FPN": "hip"})
    # without the switch the same constructor still asks for the checkout's FPN
    _child("""
    import gfnet_amd.reference_backbone as rb
    rb._build_vit = lambda w: vit
    from model.network import GFNet
    try:
        GFNet(conf=conf)
    except ImportError as e:
        assert "FPN" in str(e)
    else:
        raise AssertionError("GFNET_COMPAT_FPN unset must keep the checkout's FPN")
    print("ok")
    """, tmp_path, env={"GFNET_COMPAT_BACKBONE": "reference", "GFNET_COMPAT_DECODER": "hip"})
