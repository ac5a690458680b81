"""ops.resize_bilinear: interpolate_bilinear's forward with gfn_interp_bilinear_bwd, a gather without atomics, as its backward.

Gradient bound, derived as tests/test_flow_tail_gpu.py derives its fp32 class: 4 * E32 + 2^-22 * max|ref|, where ref is float64
F.interpolate autograd on the CPU and E32 is the error of fp32 CPU autograd against it on the same input -- the error a correct fp32
implementation of this adjoint has here -- plus four fp32 roundings of the largest entry for the cases whose fp32 weights are exact
(E32 = 0: the identity, the broadcast and the 2:1 mean)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# (BC planes as (B, C), input size, output size): 8 -> 14 is the backbone's resize at a 112-pixel image, 32 -> 56 at 448
SIZES = [((2, 5), (8, 8), (14, 14)), ((1, 7), (32, 32), (56, 56)), ((2, 3), (5, 7), (3, 11)), ((1, 4), (64, 64), (3, 3)),
         ((2, 2), (1, 1), (4, 4)), ((1, 3), (4, 4), (1, 1)), ((1, 2), (9, 6), (9, 6))]


def size_id(s):
    (B, C), (H, W), (Ho, Wo) = s
    return f"{B}x{C}_{H}x{W}_to_{Ho}x{Wo}"


def tensors(s, seed=0):
    (B, C), (H, W), (Ho, Wo) = s
    gen = torch.Generator().manual_seed(100 + seed + H * 7 + Wo)
    return torch.randn(B, C, H, W, generator=gen), torch.randn(B, C, Ho, Wo, generator=gen)


def cpu_grad(x, g, size, dtype):
    t = x.detach().clone().to(dtype).requires_grad_(True)
    F.interpolate(t, size=size, mode="bilinear", align_corners=False).backward(g.to(dtype))
    return t.grad


def hip_grad(x, g, size):
    from gfnet_amd import ops

    t = x.detach().cuda().requires_grad_(True)
    out = ops.resize_bilinear(t, size)
    out.backward(g.cuda())
    return out.detach(), t.grad


@pytest.mark.parametrize("s", SIZES, ids=size_id)
def test_gradient_matches_float64_autograd(s):
    x, g = tensors(s)
    ref = cpu_grad(x, g, s[2], torch.float64)
    e32 = float((cpu_grad(x, g, s[2], torch.float32).double() - ref).abs().max())
    _, got = hip_grad(x, g, s[2])
    assert got.dtype == torch.float32 and got.shape == x.shape
    err = float((got.double().cpu() - ref).abs().max())
    bound = 4 * e32 + 2.0 ** -22 * float(ref.abs().max())
    print(f"{size_id(s)}: err {err:.3e}, bound {bound:.3e} (E32 {e32:.3e}), ratio {err / bound:.3f}")
    assert err <= bound


@pytest.mark.parametrize("s", SIZES, ids=size_id)
def test_forward_is_interpolate_bilinears_launch_and_two_runs_are_equal(s):
    from gfnet_amd import ops

    x, g = tensors(s, seed=1)
    out, grad = hip_grad(x, g, s[2])
    assert torch.equal(out, ops.interpolate_bilinear(x.cuda(), s[2]))
    out2, grad2 = hip_grad(x, g, s[2])
    assert torch.equal(out, out2) and torch.equal(grad.view(torch.int32), grad2.view(torch.int32))
    with torch.no_grad():
        plain = ops.resize_bilinear(x.cuda().requires_grad_(True), s[2])
    assert plain.grad_fn is None and torch.equal(plain, out)


def test_interpolate_bilinear_stays_graph_free():
    """the scale loop relies on it as its .detach()"""
    from gfnet_amd import ops

    x = torch.randn(2, 3, 6, 6).cuda().requires_grad_(True)
    assert ops.interpolate_bilinear(x, 9).grad_fn is None
    a, b = ops.interpolate_bilinear_pair(x, x[:, :1], 9)
    assert a.grad_fn is None and b.grad_fn is None
    assert ops.resize_bilinear(x, 9).grad_fn is not None
    assert ops.resize_bilinear(x.detach(), 9).grad_fn is None


def test_half_input_gets_a_half_gradient_and_many_planes_take_every_block():
    """fp16 in: fp32 out as interpolate_bilinear gives it, the gradient cast back once; 200 planes are 67 plane groups, the last one ragged"""
    from gfnet_amd import ops

    x, g = torch.randn(4, 50, 8, 8), torch.randn(4, 50, 14, 14)
    ref = cpu_grad(x, g, (14, 14), torch.float64)
    _, got = hip_grad(x, g, (14, 14))
    e32 = float((cpu_grad(x, g, (14, 14), torch.float32).double() - ref).abs().max())
    assert float((got.double().cpu() - ref).abs().max()) <= 4 * e32 + 2.0 ** -22 * float(ref.abs().max())
    h = x.detach().half().cuda().requires_grad_(True)
    out = ops.resize_bilinear(h, (14, 14))
    assert out.dtype == torch.float32
    out.backward(g.cuda())
    assert h.grad.dtype == torch.float16
    want = cpu_grad(x.half().float(), g, (14, 14), torch.float64)
    # the fp32 gradient rounded to fp16 once: half an fp16 ulp, 2^-11 of the entry, and as much again for the fp32 error in front of it
    assert float((h.grad.double().cpu() - want).abs().max()) <= 2.0 ** -10 * float(want.abs().max())
