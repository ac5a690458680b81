"""Two training steps from the same seeds under torch.use_deterministic_algorithms(True) give the same bits.

T1: everything after the backbone -- GFNet.forward_pyramids in train() on random pyramids that require a gradient (the toy
configuration of tests/test_train_gpu.py, refiners on train_conv_impl = "hip"), RobustLosses, backward, FusedAdamWStep.step():
every pyramid gradient, parameter, parameter gradient and moment.  The pyramid gradients are where the refiner input's dy arrives,
the one gradient of the package that varied between runs.
T2: the backbone -- ReferenceBackbone with the native decoder and FPN on their HIP training paths, a stand-in ViT, 112 x 112 images
(8 x 8 tokens, resized to the 14 x 14 stride-8 grid by ops.resize_bilinear under the flag): every backbone parameter gradient."""
import pytest
import torch
import torch.nn as nn

from conftest import load_golden
from test_train_cpu import SCALES, g12_refiners

pytestmark = pytest.mark.gpu


@pytest.fixture
def deterministic_flag():
    was, warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True)
    yield
    torch.use_deterministic_algorithms(was, warn_only=warn)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))


def assert_same(first, second, what):
    assert first.keys() == second.keys()
    for k in first:
        assert same_bits(first[k], second[k]), f"{what}: {k} differs between the two runs"


def post_backbone_step():
    from gfnet_amd import ops
    from gfnet_amd.losses import RobustLosses
    from gfnet_amd.model.network import GFNet
    from gfnet_amd.trainer import FusedAdamWStep

    g = load_golden("g12_train_grads")
    torch.manual_seed(0)
    refiners = g12_refiners(g, "cuda")
    for ref in refiners.values():
        ref.train_conv_impl = "hip"
    conf = {"matcher": {"num_grid": [int(v) for v in g["num_grid"]], "radius": [int(v) for v in g["radius"]],
                        "num_itr": [int(v) for v in g["num_itr"]]}}
    model = GFNet(conf, conv_refiner=nn.ModuleDict(refiners)).cuda().train()
    gen = torch.Generator().manual_seed(11)
    pyrs = tuple({s: torch.randn(g[f"{p}.{s}"].shape, generator=gen).cuda().requires_grad_() for s in SCALES} for p in ("pyr0", "pyr1"))
    H, W = (int(v) for v in g["image_hw"])
    B = pyrs[0]["16"].shape[0]
    seen = []
    orig = ops.refiner_input_bwd
    ops.refiner_input_bwd = lambda *a, **k: (seen.append(k.get("deterministic")), orig(*a, **k))[1]
    try:
        corresps = model.forward_pyramids(pyrs[0], pyrs[1], (H, W))
        batch = {"H_s2t": torch.tensor([[1.02, 0.03, 1.5], [-0.02, 0.98, -1.0], [1e-4, -5e-5, 1.0]]).repeat(B, 1, 1).cuda(),
                 "im_A": torch.zeros(B, 3, H, W, device="cuda"), "im_B": torch.zeros(B, 3, H, W, device="cuda")}
        loss = RobustLosses(ce_weight=0.01, local_dist={1: 4, 2: 4, 4: 8, 8: 8}, local_largest_scale=8, alpha=0.5, c=1e-4,
                            iteration_base=1)(corresps, batch)
        stepper = FusedAdamWStep(list(model.named_parameters()), lr=1e-3, init_scale=16.0, zero_grads=False)
        stepper.scale_loss(loss).backward()
    finally:
        ops.refiner_input_bwd = orig
    stepper.step()
    torch.cuda.synchronize()
    assert seen and all(d is True for d in seen), "a refiner input's backward did not take the deterministic route"
    assert bool(torch.isfinite(loss)) and float(stepper.last_stats["found_inf"]) == 0.0
    out = {"loss": loss.detach()}
    for i, pyr in enumerate(pyrs):
        for s, t in pyr.items():
            assert t.grad is not None and float(t.grad.abs().max()) > 0, (i, s)
            out[f"pyr{i}.{s}.grad"] = t.grad
    for k, p in model.named_parameters():
        assert p.grad is not None, k
        out[f"{k}"] = p.detach()
        out[f"{k}.grad"] = p.grad
        out[f"{k}.exp_avg"] = stepper.state[p]["exp_avg"]
        out[f"{k}.exp_avg_sq"] = stepper.state[p]["exp_avg_sq"]
    return {k: v.clone() for k, v in out.items()}


def test_t1_post_backbone_training_step_is_bit_reproducible(deterministic_flag):
    first, second = post_backbone_step(), post_backbone_step()
    assert_same(first, second, "post-backbone step")
    print(f"T1: {len(first)} tensors bit-equal between two runs, loss {float(first['loss']):.9e}")


def backbone_gradients():
    import fpn_fixture
    import synth
    from gfnet_amd import ops
    from gfnet_amd.reference_backbone import ReferenceBackbone
    from test_fpn_gpu import StubVit
    from test_fpn_train_gpu import E2E_CONF

    torch.manual_seed(0)
    bb = ReferenceBackbone(E2E_CONF, vit=StubVit(), decoder="hip_fused", fpn="hip", fpn_train_impl="hip_fused", decoder_train_impl="hip").cuda()
    fpn_fixture.fill({"encoder": bb.encoder, "decoder": bb.decoder, "merge_layer": bb.merge_layer})
    bb.train()
    images = torch.from_numpy(synth.lattice_uniform((4, 3, 112, 112), 78)).cuda()
    seen = []
    orig = ops.resize_bilinear
    ops.resize_bilinear = lambda x, size: (seen.append((tuple(x.shape[2:]), tuple(size))), orig(x, size))[1]
    try:
        pa, pb = bb(images)
    finally:
        ops.resize_bilinear = orig
    assert seen == [((8, 8), (14, 14))], "the ViT map's resize did not go through ops.resize_bilinear"
    gen = torch.Generator().manual_seed(5)
    loss = torch.zeros((), device="cuda")
    for pyr in (pa, pb):
        for s in ("16", "8", "4", "2", "1"):
            loss = loss + (pyr[s] * torch.randn(pyr[s].shape, generator=gen).cuda()).sum()
    loss.backward()
    torch.cuda.synchronize()
    out = {}
    for k, p in bb.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
        out[k] = p.grad.clone()
    assert any(float(v.abs().max()) > 0 for k, v in out.items() if k.startswith("dino_decoder"))
    return out


def test_t2_backbone_gradients_are_bit_reproducible(deterministic_flag):
    first, second = backbone_gradients(), backbone_gradients()
    assert_same(first, second, "backbone")
    print(f"T2: {len(first)} backbone parameter gradients bit-equal between two runs")
