"""The FPN in training mode on the GPU (csrc/fpn_conv_train.hip): every layer as an op -- forward, statistics, running buffers and
every gradient -- against the definition in float64 (F.conv2d -> F.batch_norm(training=True) -> activation -> + residual, with
autograd), across tile boundaries, on tiny maps, the need mask, determinism, aliasing, train() under no_grad, and the three
modules with train_conv_impl = "hip" against the same modules in float64 on the CPU, against their own torch path and against the
reference's own modules' step (tests/golden/g17_fpn_train.npz), and one training step of a whole model.

The unit of every bound is tests/test_fpn_gpu.py's e32: the error of the SAME definition evaluated in fp32 by torch on the CPU
against float64, over the whole tensor; the kernels may take 4 x e32.  For tensors of a handful of values -- the per-channel
vectors (mean, invstd, running buffers, BatchNorm's gradients) and everything on the tiny maps -- e32 can be zero by luck, so there the
unit is at least `floor`, one fp32 rounding of the tensor's largest magnitude.  The conv-bias gradient is asserted to be exact zeros.

Largest ratios measured (MI355X): see DESIGN 4.8."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fpn_fixture
import synth
from conftest import ROOT, load_golden
from gfnet_amd import _lib, ops
from make_golden_fpn_train import MAX_BYTES, SHAPE, stored, train_step
from test_fpn_cpu import run_modules
from test_fpn_gpu import GENERAL, LAYERS

pytestmark = pytest.mark.gpu

CONFIGS = {**LAYERS, **GENERAL}
MOMENTUM, EPS = 0.1, 1e-5
VECTORS = ("mean", "invstd", "running_mean", "running_var", "d_bn_w", "d_bn_b")  # a handful of values each: the floor applies
NAMES = ("out", "u") + VECTORS[:4] + ("gx0", "gx1", "g_residual", "d_weight") + VECTORS[4:]


def act_fn(y, act):
    if act == "leaky_relu":
        return F.leaky_relu(y, 0.1)
    return y * torch.sigmoid(y) if act == "swish" else y


def definition(t, stride, act):
    """Everything the op returns and every gradient of sum(out * lw), in the dtype of the tensors of `t` (fresh leaves)."""
    leaf = {k: (None if v is None else v.clone().requires_grad_(k in ("x0", "x1", "w", "cb", "g", "b", "res"))) for k, v in t.items()}
    x = leaf["x0"] if leaf["x1"] is None else torch.cat((leaf["x0"], leaf["x1"]), dim=1)
    u = F.conv2d(x, leaf["w"], stride=stride, padding=leaf["w"].shape[-1] // 2)
    rm, rv = leaf["rm"], leaf["rv"]
    y = F.batch_norm(u if leaf["cb"] is None else u + leaf["cb"].view(1, -1, 1, 1), rm, rv, leaf["g"], leaf["b"], True, MOMENTUM, EPS)
    out = act_fn(y, act)
    if leaf["res"] is not None:
        out = out + leaf["res"]
    wanted = [k for k in ("x0", "x1", "res", "w", "g", "b", "cb") if leaf[k] is not None]
    grads = dict(zip(wanted, torch.autograd.grad((out * leaf["lw"]).sum(), [leaf[k] for k in wanted])))
    ud = u.detach()
    res = {"out": out.detach(), "u": ud, "mean": ud.mean((0, 2, 3)), "invstd": (ud.var((0, 2, 3), unbiased=False) + EPS).rsqrt(),
           "running_mean": rm, "running_var": rv, "gx0": grads["x0"], "gx1": grads.get("x1"), "g_residual": grads.get("res"),
           "d_weight": grads["w"], "d_bn_w": grads["g"], "d_bn_b": grads["b"]}
    return res


@functools.lru_cache(maxsize=None)
def case(name, B, Ho, Wo):
    """Inputs of layer `name` for an output of (B, Cout, Ho, Wo), the float64 results and every tensor's e32.  Computed once, never
    modified.  The up0 layers get x0 already doubled; a layer with a residual gets it as a tensor of its own (a copy of x0 / x1), so that
    its gradient is told apart; the decoder's heads (swish) have a conv bias, the encoder's layers none."""
    K, stride, C0, C1, Cout, _, res, act = CONFIGS[name]
    seed = 4100 + 13 * sorted(CONFIGS).index(name)
    H, W = (Ho, Wo) if stride == 1 else (2 * Ho - 1, 2 * Wo - 1)

    def lat(shape, s, uniform=False):
        return torch.from_numpy((synth.lattice_uniform if uniform else synth.lattice_normalish)(shape, seed + s))

    t = {"x0": lat((B, C0, H, W), 0), "x1": lat((B, C1, H, W), 1) if C1 else None,
         "w": lat((Cout, C0 + C1, K, K), 2) * np.float32(0.87 / np.sqrt((C0 + C1) * K * K)),
         "cb": np.float32(0.3) * lat((Cout,), 3, True) if act == "swish" else None,
         "g": np.float32(0.9) + np.float32(0.5) * lat((Cout,), 4, True), "b": np.float32(0.4) * lat((Cout,), 5, True),
         "rm": np.float32(0.5) * lat((Cout,), 6, True), "rv": np.float32(1.0) + np.float32(0.75) * lat((Cout,), 7, True),
         "lw": lat((B, Cout, Ho, Wo), 8)}
    t["res"] = {"x0": t["x0"], "x1": t["x1"], None: None}[res]
    t["res"] = None if t["res"] is None else t["res"].clone()
    ref = definition({k: (None if v is None else v.double()) for k, v in t.items()}, stride, act)
    r32 = definition(t, stride, act)
    e32 = {k: (None if ref[k] is None else float((r32[k].double() - ref[k]).abs().max())) for k in NAMES}
    assert tuple(ref["out"].shape) == (B, Cout, Ho, Wo)
    return t, ref, e32


def run_op(name, t, residual="own", requires=("x0", "x1", "w", "g", "b", "res", "cb")):
    """The op and its backward on the GPU: the same dict as `definition`, plus d_conv_bias.  residual: "own" (a leaf of its own),
    or "alias" (the very tensor x0 / x1)."""
    K, stride, C0, C1, Cout, _, res, act = CONFIGS[name]
    d = {k: (None if v is None else v.cuda().requires_grad_(k in requires)) for k, v in t.items()}
    if residual == "alias" and res is not None:
        d["res"] = d[res]
    nbt = torch.zeros((), dtype=torch.long, device="cuda")
    out = ops.conv2d_bn_act_train(d["x0"], d["w"], d["cb"], d["g"], d["b"], d["rm"], d["rv"], nbt, MOMENTUM, EPS, x1=d["x1"],
                                  residual=d["res"], stride=stride, act=act, slope=0.1)
    assert int(nbt) == 1
    got = {"out": out.detach(), "running_mean": d["rm"], "running_var": d["rv"]}
    if out.requires_grad:
        (out * d["lw"]).sum().backward()
        got.update(gx0=d["x0"].grad, gx1=None if d["x1"] is None else d["x1"].grad, d_weight=d["w"].grad, d_bn_w=d["g"].grad,
                   d_bn_b=d["b"].grad, g_residual=None if d["res"] is None else d["res"].grad,
                   d_conv_bias=None if d["cb"] is None else d["cb"].grad)
    return got


def saved(name, t):
    """(u, mean, invstd) of the forward, from the thin wrapper."""
    K, stride, C0, C1, Cout, _, res, act = CONFIGS[name]
    d = {k: (None if v is None else v.cuda()) for k, v in t.items()}
    out, u, mean, invstd = ops.conv2d_bn_act_train_fwd(d["x0"], d["w"], d["cb"], d["g"], d["b"], d["rm"], d["rv"], MOMENTUM, EPS,
                                                       x1=d["x1"], residual=d["res"], stride=stride, act=act, slope=0.1)
    return d, out, u, mean, invstd


def check_case(name, B, Ho, Wo, floor=False):
    t, ref, e32 = case(name, B, Ho, Wo)
    got = run_op(name, t)
    _, out, u, mean, invstd = saved(name, t)
    assert torch.equal(out, got["out"])  # the wrapper and the autograd function run the same launches
    got.update(u=u, mean=mean, invstd=invstd)
    worst = 0.0
    for k in NAMES:
        if ref[k] is None:
            assert got.get(k) is None, k
            continue
        if k == "g_residual":  # gy itself
            assert torch.equal(got[k].cpu().double(), ref[k]), k
            continue
        unit = e32[k]
        if floor or k in VECTORS:
            unit = max(unit, 2.0 ** -24 * float(ref[k].abs().max()))
        assert unit > 0.0, (name, k)
        assert got[k].shape == ref[k].shape and got[k].dtype == torch.float32, k
        err = float((got[k].detach().cpu().double() - ref[k]).abs().max())
        worst = max(worst, err / unit)
        print(f"{name} {B}x{Ho}x{Wo} {k}: max err {err:.3e}, unit {unit:.3e}, ratio {err / unit:.2f}")
    print(f"{name} {B}x{Ho}x{Wo}: largest ratio {worst:.2f}")
    for k in NAMES:
        if ref[k] is not None and k != "g_residual":
            unit = max(e32[k], 2.0 ** -24 * float(ref[k].abs().max())) if floor or k in VECTORS else e32[k]
            err = float((got[k].detach().cpu().double() - ref[k]).abs().max())
            assert err <= 4 * unit, (name, k, err, unit)
    if t["cb"] is not None:
        assert got["d_conv_bias"] is not None and not bool(got["d_conv_bias"].any()), "the conv bias's gradient is exactly zero"


@pytest.mark.parametrize("name", list(CONFIGS))
def test_every_layer_as_an_op(name):
    """B = 2, output 13 x 19 (stride 2: from 25 x 37); the up0 layers take a pre-doubled 14 x 22 x0."""
    up0 = CONFIGS[name][5]
    check_case(name, 2, 14 if up0 else 13, 22 if up0 else 19)


@pytest.mark.parametrize("name", ["conv00", "conv01", "downsample1", "downsample3", "conv30", "merge_layer", "inner3", "out3", "general_s2"])
def test_across_a_tile_boundary(name):
    """B = 1, output 72 x 136: both strides, the 8 / 16 / 64-channel instantiations, more than one partial per channel in every
    reduction (9792 values per plane: three chunks of 4096; 45 weight-gradient tiles) and the tails."""
    check_case(name, 1, 72, 136)


@pytest.mark.parametrize("name", ["conv00", "downsample1", "out3", "general_k7", "inner3"])
def test_tiny_maps(name):
    check_case(name, 3, 2, 3, floor=True)


def test_a_single_value_per_channel_is_refused():
    x, w, v = torch.zeros(1, 3, 1, 1, device="cuda"), torch.zeros(8, 3, 3, 3, device="cuda"), torch.ones(8, device="cuda")
    with pytest.raises(_lib.GfnError, match="more than one value per channel"):
        ops.conv2d_bn_act_train(x, w, None, v, v, v.clone(), v.clone(), None, 0.1, 1e-5)
    with pytest.raises(ValueError, match="momentum"):
        ops.conv2d_bn_act_train(x, w, None, v, v, v.clone(), v.clone(), None, None, 1e-5)


def test_op_refuses_what_it_cannot_run():
    x, w, s = torch.zeros(1, 3, 8, 8, device="cuda"), torch.zeros(8, 3, 3, 3, device="cuda"), torch.ones(8, device="cuda")
    with pytest.raises(TypeError, match="float32"):
        ops.conv2d_bn_act_train(x.half(), w, None, s, s, s.clone(), s.clone(), None, 0.1, 1e-5)
    with pytest.raises(TypeError, match="contiguous"):
        ops.conv2d_bn_act_train(x.permute(0, 1, 3, 2)[:, :, :, ::2], w, None, s, s, s.clone(), s.clone(), None, 0.1, 1e-5)
    with pytest.raises(ValueError, match="channels"):
        ops.conv2d_bn_act_train(x, w, None, s, s, s.clone(), s.clone(), None, 0.1, 1e-5, x1=x)
    with pytest.raises(ValueError, match="residual"):
        ops.conv2d_bn_act_train(x, w, None, s, s, s.clone(), s.clone(), None, 0.1, 1e-5, residual=x)
    with pytest.raises(Exception, match="kernel size 2"):
        ops.conv2d_bn_act_train(x, torch.zeros(8, 3, 2, 2, device="cuda"), None, s, s, s.clone(), s.clone(), None, 0.1, 1e-5)


def bwd(name, d, u, mean, invstd, need, buffers=None):
    K, stride, C0, C1, Cout, _, res, act = CONFIGS[name]
    return ops.conv2d_bn_act_train_bwd(d["lw"], d["x0"], d["w"], d["g"], d["b"], u, mean, invstd, x1=d["x1"], stride=stride, act=act, slope=0.1,
                                       need=need, buffers=buffers)


@pytest.mark.parametrize("name", ["conv01", "downsample2", "merge_layer"])
def test_need_mask(name):
    """x0 without requires_grad: nothing is computed for gx0 -- a poisoned buffer handed to the backward comes back untouched -- and
    each single need bit gives the bits of the full call."""
    t, _, _ = case(name, 2, 13, 19)
    d, _, u, mean, invstd = saved(name, t)
    full = bwd(name, d, u, mean, invstd, (True, True, True))
    poison = {"gx0": torch.full_like(d["x0"], 7.25), "gx1": None if d["x1"] is None else torch.full_like(d["x1"], 7.25)}
    partial = bwd(name, d, u, mean, invstd, (False, True, True), buffers=dict(poison))
    assert partial[0] is None and partial[1] is None
    assert bool((poison["gx0"] == 7.25).all()) and (poison["gx1"] is None or bool((poison["gx1"] == 7.25).all()))
    assert torch.equal(partial[2], full[2]) and torch.equal(partial[3], full[3]) and torch.equal(partial[4], full[4])
    only_x, only_w, only_bn = (bwd(name, d, u, mean, invstd, tuple(i == j for j in range(3))) for i in range(3))
    assert torch.equal(only_x[0], full[0]) and (full[1] is None or torch.equal(only_x[1], full[1])) and only_x[2] is None and only_x[3] is None
    assert torch.equal(only_w[2], full[2]) and only_w[0] is None and only_w[3] is None
    assert torch.equal(only_bn[3], full[3]) and torch.equal(only_bn[4], full[4]) and only_bn[0] is None and only_bn[2] is None
    assert all(g is None for g in bwd(name, d, u, mean, invstd, (False, False, False)))
    # through autograd: no gradient for an input that does not ask for one, the others unchanged
    frozen = run_op(name, t, requires=("w", "g", "b"))
    everything = run_op(name, t)
    assert frozen["gx0"] is None and torch.equal(frozen["d_weight"], everything["d_weight"]) and torch.equal(frozen["d_bn_w"], everything["d_bn_w"])


@pytest.mark.parametrize("name", ["conv01", "downsample2", "merge_layer", "inner2"])
def test_identical_calls_give_identical_bits(name):
    t, _, _ = case(name, 2, 14, 22)
    a, b = run_op(name, t), run_op(name, t)
    for k, v in a.items():
        assert (v is None and b[k] is None) or torch.equal(v, b[k]), k


@pytest.mark.parametrize("name", ["inner1", "merge_layer", "general_up"])
def test_residual_may_alias_an_input(name):
    """residual IS x1 (x0 for the merge layer): the same bits as with a copy, and its gradient arrives summed on the aliased leaf."""
    res = CONFIGS[name][6]
    t, _, _ = case(name, 2, 14, 22)
    own, aliased = run_op(name, t), run_op(name, t, residual="alias")
    for k in ("out", "running_mean", "running_var", "d_weight", "d_bn_w", "d_bn_b"):
        assert torch.equal(own[k], aliased[k]), k
    key = "g" + res
    assert torch.equal(aliased[key], own[key] + own["g_residual"])
    other = "gx1" if res == "x0" else "gx0"
    assert torch.equal(aliased[other], own[other])


@pytest.mark.parametrize("name", ["conv01", "inner2"])
def test_train_under_no_grad(name):
    """Buffers move, num_batches_tracked goes up by one (run_op asserts it), out equals the grad-mode call bit for bit, nothing is
    differentiable."""
    t, _, _ = case(name, 2, 14, 22)
    graded = run_op(name, t)
    with torch.no_grad():
        plain = run_op(name, t)
    assert "gx0" not in plain and torch.equal(plain["out"], graded["out"])
    for k in ("running_mean", "running_var"):
        assert torch.equal(plain[k], graded[k]) and not torch.equal(plain[k].cpu(), t["rm" if k == "running_mean" else "rv"])


# ---- the three modules ---------------------------------------------------------------------------------------------------------------
def build(dtype, device, train_conv_impl="torch"):
    from gfnet_amd.model import fpn

    chs = fpn_fixture.FEAT_CHS
    mods = {"encoder": fpn.FPNEncoder(chs, train_conv_impl=train_conv_impl), "decoder": fpn.FPNDecoder_concat(chs, train_conv_impl=train_conv_impl),
            "merge_layer": fpn.merge_layer(chs[-1], train_conv_impl=train_conv_impl)}
    fpn_fixture.fill(mods)
    for m in mods.values():
        m.to(device=device, dtype=dtype).train(True)
    return mods


def module_step(shape_name, dtype, device, train_conv_impl="torch"):
    """make_golden_fpn_train.train_step -- one forward and backward of the three modules in train(): the eight maps, the 57 buffers
    after it and every gradient, the loss sum_k (map_k * w_k).sum() / sqrt(numel of one image's map) with lattice weights seeded
    9000 + k -- as float64 CPU tensors."""
    mods = build(dtype, device, train_conv_impl)
    images, side = (t.to(device=device, dtype=dtype) for t in fpn_fixture.inputs(shape_name))
    return train_step(mods, run_modules, images, side)


@functools.lru_cache(maxsize=None)
def module_reference(shape_name):
    ref = module_step(shape_name, torch.float64, "cpu")
    r32 = module_step(shape_name, torch.float32, "cpu")
    return ref, {k: float((r32[k] - ref[k]).abs().max()) for k in ref}


@functools.lru_cache(maxsize=None)
def module_on_gpu(shape_name, train_conv_impl):
    return module_step(shape_name, torch.float32, "cuda", train_conv_impl)


def compare_modules(label, got, ref, e32):
    assert set(got) == set(ref) and sum(k.startswith("buf/") for k in ref) == 57
    worst, failed = 0.0, []
    for k in sorted(ref):
        if k.endswith("num_batches_tracked"):
            assert float(got[k]) == float(ref[k]) == 1.0
            continue
        if k.startswith("grad/") and k.endswith(".0.bias"):  # a conv bias in front of batch statistics
            continue
        unit = e32[k]
        if ref[k].dim() <= 1:  # a handful of values
            unit = max(unit, 2.0 ** -24 * float(ref[k].abs().max()))
        assert unit > 0.0, k
        err = float((got[k] - ref[k]).abs().max())
        worst = max(worst, err / unit)
        print(f"{label} {k}: max err {err:.3e}, unit {unit:.3e}, ratio {err / unit:.2f}")
        if err > 4 * unit:
            failed.append((k, err, unit))
    print(f"{label}: largest ratio {worst:.2f}")
    assert not failed, failed


@pytest.mark.parametrize("shape_name", [s[0] for s in fpn_fixture.SHAPES])
def test_whole_module_in_training_mode_against_float64(shape_name):
    ref, e32 = module_reference(shape_name)
    got = module_on_gpu(shape_name, "hip")
    compare_modules(f"{shape_name} hip vs float64", got, ref, e32)
    for k, v in got.items():
        if k.startswith("grad/") and k.endswith(".0.bias"):
            assert not bool(v.any()), k  # exact zeros


@pytest.mark.parametrize("shape_name", [s[0] for s in fpn_fixture.SHAPES])
def test_hip_training_path_against_the_modules_own_torch_path(shape_name):
    _, e32 = module_reference(shape_name)
    compare_modules(f"{shape_name} hip vs torch", module_on_gpu(shape_name, "hip"), module_on_gpu(shape_name, "torch"), e32)


def compare_to_golden(label, got, g, factor=4):
    """Every recorded tensor of G17 (the reference's own modules in train(), fp32) within factor x the reference's own fp32-vs-float64
    difference; conv-bias gradients, which are rounding noise in the reference, apart."""
    names = [str(n) for n in g["names"]]
    assert sorted(got) == names and sum(n.startswith("buf/") for n in names) == 57
    worst, failed = 0.0, []
    for k in names:
        want = torch.from_numpy(g[k]).double()
        have = stored(k, got[k])
        assert have.shape == want.shape, k
        if k.endswith("num_batches_tracked"):
            assert torch.equal(have, want)
            continue
        if k.startswith("grad/") and k.endswith(".0.bias"):
            assert float(have.abs().max()) < 1e-6 and float(want.abs().max()) < 1e-6, k  # zero, or noise around it
            continue
        unit = float(g[k + "/e32"])
        if got[k].dim() <= 1:  # a handful of values
            unit = max(unit, 2.0 ** -24 * float(want.abs().max()))
        assert unit > 0.0, k
        err = float((have - want).abs().max())
        worst = max(worst, err / unit)
        print(f"{label} {k}: max err {err:.3e}, unit {unit:.3e}, ratio {err / unit:.2f}")
        if err > factor * unit:
            failed.append((k, err, unit))
    print(f"{label}: largest ratio {worst:.2f}")
    assert not failed, failed
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "g17_fpn_train.npz")) <= MAX_BYTES


def test_hip_training_path_against_the_reference_modules_own_step():
    compare_to_golden("hip vs the reference's modules", module_on_gpu(SHAPE, "hip"), load_golden("g17_fpn_train"))


def test_module_runs_the_hip_training_op_only_when_asked(monkeypatch):
    calls = []
    orig = ops.conv2d_bn_act_train
    monkeypatch.setattr(ops, "conv2d_bn_act_train", lambda *a, **k: (calls.append(1), orig(*a, **k))[1])
    mods = build(torch.float32, "cuda", "hip")
    images, side = (t.cuda() for t in fpn_fixture.inputs("b"))
    out = run_modules(mods, images, side)
    assert len(calls) == 19 and all(v.requires_grad for v in out.values())
    for m in mods.values():
        m.train_conv_impl = "torch"
    run_modules(mods, images, side)
    assert len(calls) == 19
    mods["encoder"].train_conv_impl = "hip"  # the top-level module's value governs its children
    mods["encoder"](images)
    assert len(calls) == 19 + 11
    mods["encoder"].train(False)
    with torch.no_grad():
        mods["encoder"](images)  # eval() takes the inference launches
    assert len(calls) == 19 + 11


# the conf of test_fpn_gpu.py's test_backbone_with_native_fpn_and_decoder_feeds_the_matcher
E2E_CONF = {"dino_cfg": {"d_model": 32,
                         "decoder_cfg": {"num_cross_attn": 2, "init_values": 1.0, "prev_values": 0.5, "nhead": 8, "attention_type": "FLASH2",
                                         "ffn_type": "ffn", "softmax_scale": "entropy_invariance", "train_avg_length": 1024,
                                         "self_cross_types": None, "post_norm": False, "pre_norm_query": True, "no_combine_norm": False}},
            "encoder_cfg": {"feat_chs": [64, 32, 16, 8]},
            "matcher": {"num_grid": [32, 32, 64, 128, 256], "radius": [7, 6, 4, 2, 0], "displacement_dim": [64, 64, 32, 16, 8],
                        "num_itr": [1, 1, 1, 1, 1]}}


def one_training_step(impl):
    """model.train() and one trainer.train_step on 2 pairs of 448 x 448 with the FPN's training path `impl`: the loss, after checking
    that every FPN parameter has a finite gradient and that the FPN took the path it was asked for.  The library convolutions of the
    torch path are asked to be deterministic, so that both losses are reproducible."""
    from gfnet_amd.model.network import GFNet
    from gfnet_amd.reference_backbone import ReferenceBackbone
    from gfnet_amd.trainer import FusedAdamWStep, train_step as trainer_step
    from test_fpn_gpu import StubVit

    images = torch.from_numpy(synth.lattice_uniform((4, 3, 448, 448), 78)).cuda()
    batch = {"im_A": images[:2], "im_B": images[2:]}

    def objective(out, _):
        loss = torch.zeros((), device="cuda")
        for scale in out.values():
            for d in scale.values():
                loss = loss + d["flow"].float().square().mean() + d["certainty"].float().square().mean()
        return loss

    calls, orig = [], ops.conv2d_bn_act_train
    ops.conv2d_bn_act_train = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
    flags = (torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark)
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    try:
        torch.manual_seed(0)
        bb = ReferenceBackbone(E2E_CONF, vit=StubVit(), decoder="hip", fpn="hip", fpn_train_impl=impl).cuda()
        fpn_fixture.fill({"encoder": bb.encoder, "decoder": bb.decoder, "merge_layer": bb.merge_layer})
        model = GFNet(E2E_CONF, backbone=bb).cuda()
        model.train()
        stepper = FusedAdamWStep([p for p in model.parameters() if p.requires_grad], lr=1e-4, init_scale=1.0, zero_grads=False)
        res = trainer_step(batch, model, objective, stepper)
    finally:
        ops.conv2d_bn_act_train = orig
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = flags
    for top in (bb.encoder, bb.decoder, bb.merge_layer):
        for k, p in top.named_parameters():
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), (impl, k)
            assert k.endswith("0.bias") or float(p.grad.abs().max()) > 0.0, (impl, k)
    assert len(calls) == (19 if impl == "hip" else 0), "the FPN did not take the path it was asked for"
    return float(res["train_loss"])


def test_one_training_step_end_to_end():
    """The backbone assembly of test_fpn_gpu.py's test_backbone_with_native_fpn_and_decoder_feeds_the_matcher -- its conf and StubVit,
    unchanged -- with fpn_train_impl = "hip" inside GFNet, model.train() and one trainer.train_step on 2 pairs: every FPN parameter gets
    a finite gradient, and the loss equals the fpn_train_impl = "torch" run within the whole-model tolerance of
    tests/test_conv_train_gpu.py (1e-4 of max(1, |loss|)).

    The images are 448 x 448, the size that conf is written for and that test runs: its matcher wants 32 x 32 ViT tokens, and on
    64 x 64 images (4 x 4 tokens) the model refuses to run.  Measured: 0.67593092 (HIP) against 0.67588842 (torch), 4.3e-5 apart, both
    the same on every run.  With the matcher's grids divided by 8 to fit 64 x 64 images the two losses were 0.94369680 and 0.94402176,
    3.2e-4 apart, although the FPN maps of the two paths differed by at most 8.6e-6 there (1.4e-5 at 448): on 4 x 4 to 32 x 32 grids
    the randomly initialised matcher's certainty amplifies rounding-level differences of its input about a thousandfold."""
    hip, ref = one_training_step("hip"), one_training_step("torch")
    print(f"one training step: loss {hip:.9e} (hip) vs {ref:.9e} (torch)")
    assert np.isfinite(hip) and abs(hip - ref) <= 1e-4 * max(1.0, abs(ref))
