"""GPU: training mode end to end.  GFNet.forward_pyramids in train() against one training step of the reference (fixture G12, made by
tests/golden/make_golden_train.py), and the backward of the flow update (ops.flow_update) against a float64 restatement of
model/network.py:257-268."""
import pytest
import torch
import torch.nn as nn

from conftest import load_golden
from test_train_cpu import SCALES, compare_to_g12, g12_pyramids, g12_refiners, weighted_loss

pytestmark = pytest.mark.gpu


def g12_model(g):
    from gfnet_amd.model.network import GFNet

    conf = {"matcher": {"num_grid": [int(v) for v in g["num_grid"]], "radius": [int(v) for v in g["radius"]],
                        "num_itr": [int(v) for v in g["num_itr"]]}}
    return GFNet(conf, conv_refiner=nn.ModuleDict(g12_refiners(g, "cuda"))).cuda().train()


def test_training_forward_and_backward_match_the_reference():
    """Tolerances: the fixture is fp32 on the CPU, this run fp32 on the GPU (MIOpen convolutions, the HIP global match and its
    backward, torch's grid_sample on the device), chained through two train-mode BatchNorms per refiner and up to seven refiner
    calls.  Outputs and BatchNorm buffers: 1e-4 (relative, at least absolute).  Gradients: 1e-3 of the tensor's largest entry --
    they sum over every later iteration and scale, and the biases in front of a BatchNorm have an analytical gradient of zero (the
    floor of test_train_cpu.compare_to_g12)."""
    g = load_golden("g12_train_grads")
    torch.manual_seed(0)
    model = g12_model(g)
    pyr0, pyr1 = g12_pyramids(g, "cuda")
    corresps = model.forward_pyramids(pyr0, pyr1, tuple(int(v) for v in g["image_hw"]))
    for s in SCALES:
        for d in corresps[s].values():
            assert d["flow"].grad_fn is not None and d["certainty"].grad_fn is not None, f"scale {s}: no autograd graph"
    loss = weighted_loss(g, corresps)
    loss.backward()
    torch.cuda.synchronize()
    assert abs(loss.item() - float(g["loss"])) <= 1e-4 * max(1.0, abs(float(g["loss"])))
    refiners = {s: model.conv_refiner[s] for s in SCALES}
    worst = compare_to_g12(g, corresps, pyr0, pyr1, refiners, 1e-4, 1e-3)
    print(f"G12 on the GPU: worst err / tol {worst}")


def test_scale16_pyramid_gradient_reaches_both_maps_through_the_global_match():
    """The global match alone (ops.corr_softargmax, model/network.py:251-252) gives both scale-16 maps a gradient."""
    from gfnet_amd import ops

    g = load_golden("g12_train_grads")
    f0 = torch.from_numpy(g["pyr0.16"]).cuda().requires_grad_()
    f1 = torch.from_numpy(g["pyr1.16"]).cuda().requires_grad_()
    flow = ops.corr_softargmax(f0, f1)
    (flow * torch.from_numpy(g["wflow.16.1"]).cuda()).sum().backward()
    assert f0.grad.abs().max() > 0 and f1.grad.abs().max() > 0


# ---- flow update ----------------------------------------------------------------------------------------------------------------
def restated_flow_update(flow, cert, d_flow, d_cert, prev, scale, W0, H0, zero_small):
    """model/network.py:262-268 (prev: the previous displacement, 1e-7 before the first iteration, :256)"""
    disp = scale * torch.stack((d_flow[:, 0] / (4 * W0), d_flow[:, 1] / (4 * H0)), dim=1)
    if zero_small:
        prev = torch.as_tensor(prev, dtype=disp.dtype, device=disp.device)
        disp = torch.where((disp - prev).abs() / prev.abs() < 1e-6, torch.zeros_like(disp), disp)
    return flow + disp, cert + d_cert, disp.detach()


def _inputs(B, G, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(shape, generator=g).cuda() for shape in ((B, 2, G, G), (B, 1, G, G), (B, 2, G, G), (B, 1, G, G))]


def _grads(outs, ins, w):
    return torch.autograd.grad(outs, ins, w)


@pytest.mark.parametrize("refiner_output_slices", [False, True])
def test_flow_update_backward_without_zeroing(refiner_output_slices):
    """training mode (zero_small off): d flow_out / d d_flow = scale / (4 W0), scale / (4 H0); flow and certainty pass through"""
    from gfnet_amd import ops

    B, G, scale, W0, H0 = 2, 9, 8, 96, 80
    flow, cert, d_flow, d_cert = _inputs(B, G, 1)
    w_flow, w_cert = _inputs(B, G, 2)[:2]
    if refiner_output_slices:                   # the refiner's (B,3,G,G) output, split into two channel views
        out = torch.cat((d_flow, d_cert), 1).requires_grad_()
        d_flow, d_cert = out[:, :2], out[:, 2:3]
        leaves = [flow.requires_grad_(), cert.requires_grad_(), out]
    else:
        leaves = [t.requires_grad_() for t in (flow, cert, d_flow, d_cert)]
    disp_prev = torch.empty_like(flow)
    fo, co = ops.flow_update(flow, cert, d_flow, d_cert, disp_prev, scale, W0, H0, zero_small=False, first_iteration=True)
    with torch.no_grad():
        pf, pc = ops.flow_update(flow, cert, d_flow, d_cert, torch.empty_like(flow), scale, W0, H0, zero_small=False)
    assert torch.equal(fo, pf) and torch.equal(co, pc)              # the autograd path launches the same kernel
    got = _grads((fo, co), leaves, (w_flow, w_cert))
    l64 = [t.detach().double().requires_grad_() for t in leaves]
    if refiner_output_slices:
        args = (l64[0], l64[1], l64[2][:, :2], l64[2][:, 2:3])
    else:
        args = tuple(l64)
    rf, rc, _ = restated_flow_update(*args, 1e-7, scale, W0, H0, False)
    want = _grads((rf, rc), l64, (w_flow.double(), w_cert.double()))
    for a, b in zip(got, want):
        torch.testing.assert_close(a.double(), b, rtol=1e-6, atol=1e-9)


def test_flow_update_backward_with_zeroing_masks_the_zeroed_cells():
    """eval with grad (zero_small on): the cells whose displacement the kernel zeroed (network.py:264-265) get no d_flow gradient.
    Second iteration, d_flow equal to the first iteration's on half the cells: the displacement repeats there, so the mask fires."""
    from gfnet_amd import ops

    B, G, scale, W0, H0 = 2, 8, 4, 64, 48
    flow, cert, d1, d_cert = _inputs(B, G, 3)
    d2 = d1.clone()
    d2[..., G // 2:] = torch.randn(B, 2, G, G - G // 2, generator=torch.Generator().manual_seed(4)).cuda()
    w_flow, w_cert = _inputs(B, G, 5)[:2]
    disp_prev = torch.empty_like(flow)
    ops.flow_update(flow, cert, d1, d_cert, disp_prev, scale, W0, H0, zero_small=True, first_iteration=True)
    leaves = [t.clone().requires_grad_() for t in (flow, cert, d2, d_cert)]
    fo, co = ops.flow_update(*leaves, disp_prev, scale, W0, H0, zero_small=True, first_iteration=False)
    got = _grads((fo, co), leaves, (w_flow, w_cert))

    _, _, prev = restated_flow_update(flow.double(), cert.double(), d1.double(), d_cert.double(), 1e-7, scale, W0, H0, True)
    l64 = [t.detach().double().requires_grad_() for t in leaves]
    rf, rc, disp = restated_flow_update(*l64, prev, scale, W0, H0, True)
    want = _grads((rf, rc), l64, (w_flow.double(), w_cert.double()))
    zeroed = (disp == 0)
    assert zeroed[..., : G // 2].all() and not zeroed[..., G // 2:].any()   # the mask fires exactly where d_flow repeats
    torch.testing.assert_close(fo.detach().double(), rf.detach(), rtol=1e-6, atol=1e-7)
    assert (got[2][..., : G // 2] == 0).all() and (got[2][..., G // 2:] != 0).all()
    for a, b in zip(got, want):
        torch.testing.assert_close(a.double(), b, rtol=1e-6, atol=1e-9)


def test_training_forward_keeps_no_reused_concat_tensor():
    """ConvRefiner.may_reuse_d: in training every refiner parameter asks for gradients, so no iteration overwrites the concat tensor
    an autograd graph has saved (GFNet.forward_pyramids passes the slot on scales with two iterations)"""
    g = load_golden("g12_train_grads")
    model = g12_model(g)
    pyr0, pyr1 = g12_pyramids(g, "cuda")
    ref = model.conv_refiner["16"]
    assert not ref.may_reuse_d(pyr0["16"], pyr1["16"], torch.zeros(2, 2, 6, 6, device="cuda"))
    seen = []
    orig = ref.assemble

    def spy(num_grid, x, y, flow, scale_factor=1, reuse=None):
        seen.append(reuse)
        return orig(num_grid, x, y, flow, scale_factor, reuse=reuse)

    ref.assemble = spy
    model.forward_pyramids(pyr0, pyr1, tuple(int(v) for v in g["image_hw"]))
    assert len(seen) == int(g["num_itr"][0]) and all(r is None for r in seen)
