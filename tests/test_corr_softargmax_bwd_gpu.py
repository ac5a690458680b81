"""Backward of the fused global correlation + soft-argmax (csrc/corr_softargmax_bwd.hip) against torch float64 autograd of the
reference's unfused restatement (model/network.py:415-440: einsum -> softmax -> einsum), on the forward suite's shape cases and input
regimes and on the production shapes; its exactness properties; and that it never materialises the volume.

Tolerance, from the operands as test_corr_softargmax_gpu.py derives the forward's.  With T_i = max_j sum_c |f0_ci f1_cj| / sqrt(C):
every logit is off by at most (C + 4) U T_i, so P_ji and the normalisation move by at most 2 (C + 4) U T_i relative; the weight
G_i . gamma_j - D_i, |.| <= 2 |G_i|_1, and the sums over N positions add (sqrt(N) + 16) U in the mean.  Per A-position
rho_i = 2 (C + 4) U T_i + (sqrt(N) + 16) U, and
  tol_f0[c,i] = K_GRAD rho_i sum_j P_ji 2 |G_i|_1 |f1_cj| / sqrt(C),   tol_f1[c,j] = K_GRAD sum_i rho_i P_ji 2 |G_i|_1 |f0_ci| / sqrt(C)
plus FLOOR_REL of the largest magnitude sum: fp32 cannot resolve a gradient far below it (the peaked regime's exact gradients
are ~1e-80, the kernel's underflow to 0).  The worst err / tol per case is printed."""
import math

import pytest
import torch

from test_corr_softargmax_gpu import CASES, REGIMES, make_inputs

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
# K_GRAD: the worst-case sums above, scaled down as the forward's K_FLOW is (rounding errors add like a random walk and the softmax
# averages them); at 1.0 the worst case of the whole suite used 0.016 of the bound
K_GRAD = 0.1
FLOOR_REL = 1e-6
STATS = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if STATS:
        print("\ncorr_softargmax_bwd: worst err / tol")
        for name in sorted(STATS):
            print(f"  {name:48s} {STATS[name]:.3f}")


def _lib():
    from gfnet_amd import _lib

    return _lib


def call_bwd(f0, f1, flow, gflow, sym=False, need0=True, need1=True, fill=float("nan")):
    """gfn_corr_softargmax_bwd through the C ABI; outputs pre-filled with `fill` (they must be overwritten)"""
    lib = _lib()
    L = lib.lib()
    B, C, H0, W0 = f0.shape
    _, _, H1, W1 = f1.shape
    nb = 2 * B if sym else B
    dt = lib.GFN_F16 if f0.dtype == torch.float16 else lib.GFN_F32
    g0 = torch.full(f0.shape, fill, device="cuda") if need0 else None
    g1 = torch.full(f1.shape, fill, device="cuda") if need1 else None
    n = int(L.gfn_corr_softargmax_bwd_ws_bytes(nb, C, H0, W0, H1, W1))
    ws = torch.empty(n, device="cuda", dtype=torch.uint8)
    lib.check(L.gfn_corr_softargmax_bwd(lib.ptr(f0), lib.ptr(f1), dt, lib.ptr(flow), lib.ptr(gflow), lib.ptr(g0), lib.ptr(g1), nb, C, H0,
                                        W0, H1, W1, int(sym), lib.ptr(ws), n, lib.stream_ptr(f0.device)), "gfn_corr_softargmax_bwd")
    torch.cuda.synchronize()
    return g0, g1


def grid64(H1, W1, device):
    """B-grid cell centres (N1, 2) as the forward's fp32 linspace, widened"""
    xs = torch.linspace(-1 + 1 / W1, 1 - 1 / W1, W1, device=device)
    ys = torch.linspace(-1 + 1 / H1, 1 - 1 / H1, H1, device=device)
    gy, gx = torch.meshgrid(ys, xs, indexing="ij")
    return torch.stack((gx, gy), -1).reshape(-1, 2).double()


def restated(f0, f1, sym=False):
    """float64 pos_embed(corr_volume(.)) with the symmetric batch concatenated: (flow, P (B,N1,N0), A-maps, B-maps)"""
    a, b = (torch.cat((f0, f1)), torch.cat((f1, f0))) if sym else (f0, f1)
    B, C, H0, W0 = a.shape
    H1, W1 = b.shape[-2:]
    s = torch.einsum("bci,bcj->bji", a.reshape(B, C, -1), b.reshape(B, C, -1)) / math.sqrt(C)
    P = s.softmax(dim=1)
    flow = torch.einsum("bji,jd->bdi", P, grid64(H1, W1, f0.device)).reshape(B, 2, H0, W0)
    return flow, P


def ref_grads(f0, f1, gflow, sym=False):
    a = f0.detach().double().requires_grad_()
    b = f1.detach().double().requires_grad_()
    flow, P = restated(a, b, sym)
    g0, g1 = torch.autograd.grad(flow, (a, b), gflow.double())
    return g0, g1, P.detach()


def grad_tol(f0, f1, gflow, P, sym=False):
    """(tol_f0, tol_f1) of the module docstring, float64"""
    a, b = (torch.cat((f0, f1)), torch.cat((f1, f0))) if sym else (f0, f1)
    a, b = a.double(), b.double()
    B, C = a.shape[:2]
    N0, N1 = a[0, 0].numel(), b[0, 0].numel()
    aa, bb = a.abs().reshape(B, C, -1), b.abs().reshape(B, C, -1)
    T = (torch.einsum("bci,bcj->bji", aa, bb) / math.sqrt(C)).amax(dim=1)            # (B, N0)
    rho = 2 * (C + 4) * U * T + (math.sqrt(max(N0, N1)) + 16) * U
    g1n = 2 * gflow.double().abs().reshape(B, 2, -1).sum(1)                           # 2 |G_i|_1
    Pg = P * g1n[:, None, :]                                                          # (B, N1, N0)
    mag0 = torch.einsum("bji,bcj->bci", Pg, bb) / math.sqrt(C)
    mag1 = torch.einsum("bji,bci->bcj", Pg, aa) / math.sqrt(C)
    t0 = K_GRAD * rho[:, None, :] * mag0
    t1 = K_GRAD * torch.einsum("bji,bci->bcj", Pg * rho[:, None, :], aa) / math.sqrt(C)
    floor = FLOOR_REL * max(mag0.max().item(), mag1.max().item())
    t0, t1 = t0 + floor, t1 + floor
    if sym:
        h = B // 2
        t0, t1 = t0[:h] + t1[h:], t1[:h] + t0[h:]
    return t0.reshape(f0.shape), t1.reshape(f1.shape)


def check(name, got, ref, tol):
    got, ref = got.double(), ref.double()
    assert torch.isfinite(got).all(), f"{name}: non-finite gradient"
    tol = tol.clamp_min(1e-300)    # (an all-zero gradient, f0 = 0: tolerance 0, error 0)
    ratio = ((got - ref).abs() / tol).max().item()
    STATS[name] = max(STATS.get(name, 0.0), ratio)
    assert ratio <= 1.0, f"{name}: err / tol {ratio:.3f}, max err {(got - ref).abs().max().item():.3e}"


def forward_flow(f0, f1, sym=False):
    from gfnet_amd import ops

    with torch.no_grad():
        return ops.corr_softargmax(f0, f1, symmetric=sym)


def grad_flow(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g).cuda()


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("C,H0,W0,H1,W1", CASES, ids=[f"C{c[0]}-A{c[1]}x{c[2]}-B{c[3]}x{c[4]}" for c in CASES])
def test_backward_against_float64(C, H0, W0, H1, W1, regime):
    a, b, _ = make_inputs(regime, 2, C, H0, W0, H1, W1, seed=C + 7 * H1 + W1)
    f0, f1 = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    flow = forward_flow(f0, f1)
    gf = grad_flow(flow.shape, C * 100 + W1)
    g0, g1 = call_bwd(f0, f1, flow, gf)
    r0, r1, P = ref_grads(f0, f1, gf)
    t0, t1 = grad_tol(f0, f1, gf, P)
    check(f"KS{8 if C <= 16 else 16 if C <= 32 else 32 if C <= 64 else 64} {regime} dF0", g0, r0, t0)
    check(f"KS{8 if C <= 16 else 16 if C <= 32 else 32 if C <= 64 else 64} {regime} dF1", g1, r1, t1)


PRODUCTION = [(32, 64, 32, 32, False), (16, 64, 48, 48, False), (8, 64, 32, 32, True)]


@pytest.mark.parametrize("B,C,H,W,sym", PRODUCTION, ids=[f"B{p[0]}-C{p[1]}-{p[2]}x{p[3]}{'-sym' if p[4] else ''}" for p in PRODUCTION])
@pytest.mark.parametrize("regime", ["mag1", "mag0.05", "mag8"])
def test_production_shapes_against_float64(B, C, H, W, sym, regime):
    a, b, _ = make_inputs(regime, B, C, H, W, H, W, seed=B + H)
    f0, f1 = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    flow = forward_flow(f0, f1, sym)
    gf = grad_flow(flow.shape, B * H)
    g0, g1 = call_bwd(f0, f1, flow, gf, sym=sym)
    r0, r1, P = ref_grads(f0, f1, gf, sym)
    t0, t1 = grad_tol(f0, f1, gf, P, sym)
    check(f"production {regime} dF0", g0, r0, t0)
    check(f"production {regime} dF1", g1, r1, t1)
    if regime == "mag1":
        # a fixed bar at unit scale as well: 1e-4 of the gradient's largest entry
        for got, ref in ((g0, r0), (g1, r1)):
            err = (got.double() - ref).abs().max().item() / ref.abs().max().item()
            print(f"B{B} {H}x{W} sym={sym}: max err / max |grad| = {err:.2e}")
            assert err <= 1e-4


def _rand(B, C, H, W, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (scale * torch.randn(B, C, H, W, generator=g)).cuda()


EXACT_CASES = [(64, 32, 32, 32, 32), (33, 7, 9, 48, 48), (7, 5, 7, 16, 28), (128, 9, 5, 40, 35)]


@pytest.mark.parametrize("C,H0,W0,H1,W1", EXACT_CASES, ids=[f"C{c[0]}-A{c[1]}x{c[2]}-B{c[3]}x{c[4]}" for c in EXACT_CASES])
def test_two_calls_are_bit_identical_and_null_outputs_skip_only_their_share(C, H0, W0, H1, W1):
    f0, f1 = _rand(3, C, H0, W0, 1), _rand(3, C, H1, W1, 2)
    flow = forward_flow(f0, f1)
    gf = grad_flow(flow.shape, 3)
    g0, g1 = call_bwd(f0, f1, flow, gf)
    h0, h1 = call_bwd(f0, f1, flow, gf, fill=0.0)
    assert torch.equal(g0, h0) and torch.equal(g1, h1)
    only0, none1 = call_bwd(f0, f1, flow, gf, need1=False)
    none0, only1 = call_bwd(f0, f1, flow, gf, need0=False)
    assert none1 is None and none0 is None
    assert torch.equal(only0, g0) and torch.equal(only1, g1)


@pytest.mark.parametrize("C,H0,W0,H1,W1", EXACT_CASES, ids=[f"C{c[0]}-A{c[1]}x{c[2]}-B{c[3]}x{c[4]}" for c in EXACT_CASES])
def test_fp16_maps_give_the_gradient_of_their_fp32_copy(C, H0, W0, H1, W1):
    h0, h1 = _rand(2, C, H0, W0, 4).half(), _rand(2, C, H1, W1, 5).half()
    flow = forward_flow(h0, h1)
    gf = grad_flow(flow.shape, 6)
    a0, a1 = call_bwd(h0, h1, flow, gf)
    b0, b1 = call_bwd(h0.float(), h1.float(), flow, gf)
    assert torch.equal(a0, b0) and torch.equal(a1, b1)


@pytest.mark.parametrize("C,H,W", [(64, 32, 32), (17, 7, 9), (96, 5, 48)])
def test_symmetric_call_is_the_sum_of_the_two_plain_calls(C, H, W):
    f0, f1 = _rand(2, C, H, W, 7), _rand(2, C, H, W, 8)
    flow = forward_flow(f0, f1, sym=True)
    gf = grad_flow(flow.shape, 9)
    s0, s1 = call_bwd(f0, f1, flow, gf, sym=True)
    p0, p1 = call_bwd(f0, f1, flow[:2].contiguous(), gf[:2].contiguous())      # direction A -> B
    q1, q0 = call_bwd(f1, f0, flow[2:].contiguous(), gf[2:].contiguous())      # direction B -> A: its "f0" is f1
    assert torch.equal(s0, p0 + q0) and torch.equal(s1, p1 + q1)
    # a NULL output in a symmetric call leaves the other one as it is
    only0, _ = call_bwd(f0, f1, flow, gf, sym=True, need1=False)
    _, only1 = call_bwd(f0, f1, flow, gf, sym=True, need0=False)
    assert torch.equal(only0, s0) and torch.equal(only1, s1)


@pytest.mark.parametrize("sym", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_autograd_flow_is_the_no_grad_flow_and_backward_is_the_kernel(sym, dtype):
    from gfnet_amd import ops

    f0, f1 = _rand(2, 64, 32, 32, 10).to(dtype), _rand(2, 64, 32, 32, 11).to(dtype)
    plain = forward_flow(f0, f1, sym)
    a, b = f0.clone().requires_grad_(), f1.clone().requires_grad_()
    flow = ops.corr_softargmax(a, b, symmetric=sym)
    assert flow.grad_fn is not None
    assert torch.equal(flow, plain)
    gf = grad_flow(flow.shape, 12)
    flow.backward(gf)
    k0, k1 = call_bwd(f0, f1, plain, gf, sym=sym)
    assert a.grad.dtype == dtype and b.grad.dtype == dtype
    assert torch.equal(a.grad, k0.to(dtype)) and torch.equal(b.grad, k1.to(dtype))


def test_inference_calls_take_the_plain_path():
    from gfnet_amd import ops

    f0, f1 = _rand(2, 16, 8, 8, 13).requires_grad_(), _rand(2, 16, 8, 8, 14).requires_grad_()
    with torch.inference_mode():
        assert ops.corr_softargmax(f0, f1).grad_fn is None
    with torch.no_grad():
        assert ops.corr_softargmax(f0, f1).grad_fn is None


def test_backward_never_materialises_the_volume():
    """B = 8, C = 64, 48^2 maps: one correlation volume is 8 * 2304^2 * 4 B = 170 MB; forward + backward stay under a quarter"""
    from gfnet_amd import ops

    B, C, H = 8, 64, 48
    a, b = _rand(B, C, H, H, 15).requires_grad_(), _rand(B, C, H, H, 16).requires_grad_()
    gf = grad_flow((B, 2, H, H), 17)
    volume = B * (H * H) ** 2 * 4
    ops.corr_softargmax(a.detach(), b.detach())          # warm the library and the allocator's small pools
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    flow = ops.corr_softargmax(a, b)
    flow.backward(gf)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print(f"forward + backward peak rise {rise / 1e6:.1f} MB, volume {volume / 1e6:.1f} MB")
    assert rise < volume / 4
