"""GPU: the sampling modes (nearest / bilinear / bicubic x zeros / border / reflection) of local_correlation, grid_sample and the
refiner input (utils/local_correlation.py:55-58, 66-68; model/network.py:464, 537, 547, 553-554) against the reference-generated
G10 / G11, against F.grid_sample on the same GPU, and against autograd of the restated reference formula.
Tolerance: |d| <= 1e-4 * max(1, |ref|), as the rest of the suite."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import synth
from conftest import assert_close, load_golden
from test_sampling_modes_cpu import PADDING_MODES, SAMPLE_MODES, _g10_scale4_inputs, restated_local_correlation

pytestmark = pytest.mark.gpu

TOL = 1e-4
ALL_MODES = [(sm, pm) for sm in SAMPLE_MODES for pm in PADDING_MODES]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def uniform(shape, seed, scale):
    """Uniform in [-scale, scale): plain random floats, generic coordinates for the 1e-4 comparisons of this module.  The decision
    points (the k/4096 lattice of synth.lattice_uniform would put nearest-mode samples on exact .5 ties) are not left open: a tie
    rounds half to even, in the kernels as in ATen, and test_sampling_exact_gpu.py pins the ties, mirrors and clamps by equality."""
    return (torch.rand(shape, generator=torch.Generator().manual_seed(seed)) * (2 * scale) - scale).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.detach().float().cpu().numpy()


def lc(f0, f1, r, G, **kw):
    from gfnet_amd.utils.local_correlation import local_correlation

    return local_correlation(tuple(f1.shape), f0, f1, r, G, **kw)


def restated(f0, f1, r, G, chunk=8, **kw):
    """restated_local_correlation on the GPU, a few batch elements at a time (the sampled tensor of the bench shape is 1.4 GB)."""
    flow = kw.pop("flow", None)
    outs = [restated_local_correlation(f0[b:b + chunk], f1[b:b + chunk].float(), r, G, flow=None if flow is None else flow[b:b + chunk], **kw)
            for b in range(0, f1.shape[0], chunk)]
    return torch.cat(outs)


# ---- G10 / G11: the reference itself ------------------------------------------------------------------------------------------
def test_g10_golden_every_mode_and_option():
    g = load_golden("g10_local_corr_modes")
    r, G = int(g["a_r"]), int(g["a_G"])
    for sm, pm in ALL_MODES:
        out = lc(dev(g["a_f0"]), dev(g["a_f1"]), r, G, flow=dev(g["a_flow"]), sample_mode=sm, padding_mode=pm)
        assert_close(host(out), g[f"a_out_{sm}_{pm}"], TOL, f"{sm}/{pm}")
    r, G = int(g["b_r"]), int(g["b_G"])
    f0, f1, flow = dev(g["b_f0"]), dev(g["b_f1"]), dev(g["b_flow"])
    for sm, pm in (("nearest", "reflection"), ("bicubic", "border")):
        kw = dict(sample_mode=sm, padding_mode=pm)
        assert_close(host(lc(f0, f1, r, G, flow=flow, grid_based_correlation=True, **kw)), g[f"b_grid_based_{sm}_{pm}"], TOL, "grid_based")
        assert_close(host(lc(f0, f1, r, G, flow=flow, num_level=2, **kw)), g[f"b_num_level2_{sm}_{pm}"], TOL, "num_level=2")
        assert_close(host(lc(f0, f1, r, G, flow=None, **kw)), g[f"b_flow_none_{sm}_{pm}"], TOL, "flow=None")
    f0, f1, flow, G, r = _g10_scale4_inputs(g)
    idx = g["c_probe_idx"]
    for sm, pm in (("nearest", "reflection"), ("bicubic", "border"), ("bicubic", "zeros")):
        out = host(lc(dev(f0), dev(f1), r, G, flow=dev(flow), sample_mode=sm, padding_mode=pm))
        assert_close(out[idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]], g[f"c_probe_val_{sm}_{pm}"], TOL, f"probes {sm}/{pm}")
        np.testing.assert_allclose(out.astype(np.float64).sum(axis=(0, 2, 3)), g[f"c_sum_per_k_{sm}_{pm}"], rtol=0, atol=5e-2)


def _toy_refiner(sample_mode, sd=None, c=8, disp=6, r=2, hidden_blocks=1):
    from gfnet_amd.model.network import ConvRefiner

    dim = 2 * c + disp + (2 * r + 1) ** 2
    ref = ConvRefiner(dim, dim, 3, kernel_size=5, dw=True, hidden_blocks=hidden_blocks, displacement_emb="linear", displacement_emb_dim=disp,
                      local_corr_num=r, corr_in_other=True, amp=False, bn_momentum=0.01, sample_mode=sample_mode)
    if sd is not None:
        ref.load_state_dict(sd, strict=True)
    return ref.cuda().eval()


@pytest.mark.parametrize("sample_mode", ["nearest", "bicubic"])
def test_g11_refiner_forward_matches_reference(sample_mode):
    g = load_golden("g11_refiner_modes")
    pre = f"{sample_mode}.sd."
    sd = {k[len(pre):]: torch.from_numpy(g[k]) for k in g.files if k.startswith(pre)}
    ref = _toy_refiner(sample_mode, sd, r=int(g["r"]), hidden_blocks=int(g["hidden_blocks"]))
    G, sf = int(g["G"]), float(g["scale_factor"])
    x, y, flow = dev(g["x"]), dev(g["y"]), dev(g["flow"])
    with torch.no_grad():
        d, _ = ref.assemble(G, x, y, flow, sf)
        dflow, dcert, lcorr = ref(G, x, y, flow, scale_factor=sf)
    assert_close(host(d), g[f"{sample_mode}.d"], TOL, "d")
    assert_close(host(lcorr), g[f"{sample_mode}.local_corr"], TOL, "local_corr")
    assert_close(host(dflow), g[f"{sample_mode}.delta_flow"], TOL, "delta_flow")
    assert_close(host(dcert), g[f"{sample_mode}.delta_cert"], TOL, "delta_cert")


# ---- grid_sample against F.grid_sample ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_grid_sample_every_mode_matches_torch(dtype):
    from gfnet_amd import ops

    x = dev(synth.lattice_normalish((2, 5, 13, 17), 1201)).to(dtype)
    grid = uniform((2, 9, 11, 2), 1202, 3.0)  # out to +-3: far outside the image on every side
    for sm, pm in ALL_MODES:
        out = ops.grid_sample(x, grid, mode=sm, padding_mode=pm)
        want = F.grid_sample(x.float(), grid, mode=sm, padding_mode=pm, align_corners=False)
        assert out.dtype == torch.float32 and out.shape == want.shape
        assert_close(host(out), host(want), TOL, f"{sm}/{pm} {dtype}")


# ---- local_correlation against the restated reference on the same GPU ----------------------------------------------------------
SHAPES = {  # B, c, h, w, G, r
    "scale4_448b32": (32, 32, 112, 112, 64, 4),
    "r7_c64": (2, 64, 56, 56, 32, 7),
    "rect": (2, 16, 36, 52, 20, 2),
}


@pytest.mark.parametrize("shape,sm,pm", [("scale4_448b32", "nearest", "reflection"), ("scale4_448b32", "bicubic", "zeros"),
                                         ("scale4_448b32", "bilinear", "border"), ("r7_c64", "bicubic", "reflection"),
                                         ("r7_c64", "nearest", "border")] + [("rect", sm, pm) for sm, pm in ALL_MODES])
def test_local_correlation_matches_restated_reference(shape, sm, pm):
    B, c, h, w, G, r = SHAPES[shape]
    f0 = dev(synth.lattice_normalish((B, c, G, G), 1301))
    f1 = dev(synth.lattice_normalish((B, c, h, w), 1302))
    flow = synth.homography_flow(B, G, 1303)
    flow[B // 2:] *= np.float32(1.15)  # half the batch partly outside the image
    flow = dev(flow)
    out = lc(f0, f1, r, G, flow=flow, sample_mode=sm, padding_mode=pm)
    assert_close(host(out), host(restated(f0, f1, r, G, flow=flow, sample_mode=sm, padding_mode=pm)), TOL, f"{shape} {sm}/{pm}")


@pytest.mark.parametrize("sm,pm", [("nearest", "zeros"), ("bicubic", "border"), ("bicubic", "reflection"), ("nearest", "reflection")])
def test_local_correlation_options_fp16_and_out_slices(sm, pm):
    B, c, h, w, G, r = 2, 32, 30, 44, 24, 3
    f0 = dev(synth.lattice_normalish((B, c, G, G), 1401))
    f1 = dev(synth.lattice_normalish((B, c, h, w), 1402))
    flow = uniform((B, 2, G, G), 1403, 1.2)
    kw = dict(sample_mode=sm, padding_mode=pm)
    # fp16 feature maps are read as stored (the result is the same as from their fp32 widening)
    assert_close(host(lc(f0, f1.half(), r, G, flow=flow, **kw)), host(restated(f0, f1.half(), r, G, flow=flow, **kw)), TOL, "fp16 f1")
    assert_close(host(lc(f0, f1, r, G, flow=flow, grid_based_correlation=True, **kw)),
                 host(restated(f0, f1, r, G, flow=flow, grid_based=True, **kw)), TOL, "grid_based")
    assert_close(host(lc(f0, f1, r, G, flow=flow, num_level=2, **kw)), host(restated(f0, f1, r, G, flow=flow, num_level=2, **kw)), TOL,
                 "num_level=2")
    sq = f1[:, :, :G, :G].contiguous()
    assert_close(host(lc(f0, sq, r, G, flow=None, **kw)), host(restated(f0, sq, r, G, flow=None, **kw)), TOL, "flow=None")
    # out= into the channel slice of a concat buffer, f0 read from a slice of it too
    K = (2 * r + 1) ** 2
    buf = torch.full((B, c + 3 + K, G, G), 7.0, device="cuda")
    buf[:, :c] = f0
    lc(buf[:, :c], f1, r, G, flow=flow, out=buf[:, c + 3:], **kw)
    assert_close(host(buf[:, c + 3:]), host(restated(f0, f1, r, G, flow=flow, **kw)), TOL, "out slice")
    assert bool((buf[:, c:c + 3] == 7.0).all())


def test_bilinear_zeros_through_the_mode_kernel_is_bit_identical_to_the_general_kernel():
    from gfnet_amd import _lib

    L, st = _lib.lib(), _lib.stream_ptr(torch.device("cuda"))
    cases = [  # B, c, h, w, G, r, f1 dtype, symmetric, grid_based, flow
        (2, 8, 20, 28, 6, 2, torch.float32, False, 0, True),
        (4, 32, 40, 40, 16, 3, torch.float16, True, 0, True),
        (2, 16, 36, 52, 20, 7, torch.float32, True, 1, True),
        (1, 12, 12, 12, 12, 1, torch.float32, False, 0, False),
    ]
    for B, c, h, w, G, r, dt, symmetric, grid_based, has_flow in cases:
        K = (2 * r + 1) ** 2
        f0 = dev(synth.lattice_normalish((B, c, G, G), 1501))
        nmaps = B // 2 if symmetric else B
        f1 = dev(synth.lattice_normalish((nmaps, c, h, w), 1502)).to(dt)
        f1s = dev(synth.lattice_normalish((nmaps, c, h, w), 1503)).to(dt) if symmetric else None
        flow = uniform((B, 2, G, G), 1504, 1.3) if has_flow else None
        code = _lib.GFN_F16 if dt == torch.float16 else _lib.GFN_F32
        a = torch.full((B, K, G, G), float("nan"), device="cuda")
        b = torch.full((B, K, G, G), float("nan"), device="cuda")
        _lib.check(L.gfn_local_corr_fwd_dt(_lib.ptr(f0), c * G * G, _lib.ptr(f1), _lib.ptr(f1s), code, _lib.ptr(flow), _lib.ptr(a), K * G * G,
                                           B, c, G, h, w, r, grid_based, h, w, 0, None, 0, st), "general")
        _lib.check(L.gfn_local_corr_mode_fwd(_lib.ptr(f0), c * G * G, _lib.ptr(f1), _lib.ptr(f1s), code, _lib.ptr(flow), _lib.ptr(b), K * G * G,
                                             B, c, G, h, w, r, grid_based, h, w, 0, 0, st), "mode")
        torch.cuda.synchronize()
        assert torch.isfinite(a).all()
        assert torch.equal(a, b), (B, c, h, w, G, r, dt, symmetric, grid_based)


def test_bwd_f0_is_bit_identical_to_the_mode_gradient_with_bilinear_zeros():
    from gfnet_amd import _lib

    L, st = _lib.lib(), _lib.stream_ptr(torch.device("cuda"))
    cases = [  # B, c, h, w, G, r, symmetric, grid_based, flow
        (2, 13, 20, 28, 6, 2, False, 0, True),  # C not a multiple of 8
        (4, 32, 40, 40, 16, 3, True, 0, True),  # symmetric: f1_second
        (2, 16, 36, 52, 20, 7, True, 1, True),  # grid_based
        (1, 12, 12, 12, 12, 1, False, 0, False),  # flow == NULL
    ]
    for B, c, h, w, G, r, symmetric, grid_based, has_flow in cases:
        K = (2 * r + 1) ** 2
        gout = dev(synth.lattice_normalish((B, K, G, G), 1511))
        nmaps = B // 2 if symmetric else B
        f1 = dev(synth.lattice_normalish((nmaps, c, h, w), 1512))
        f1s = dev(synth.lattice_normalish((nmaps, c, h, w), 1513)) if symmetric else None
        flow = uniform((B, 2, G, G), 1514, 1.3) if has_flow else None
        a = torch.full((B, c, G, G), float("nan"), device="cuda")
        b = torch.full((B, c, G, G), float("nan"), device="cuda")
        _lib.check(L.gfn_local_corr_bwd_f0(_lib.ptr(gout), K * G * G, _lib.ptr(f1), _lib.ptr(f1s), _lib.ptr(flow), _lib.ptr(a), c * G * G,
                                           B, c, G, h, w, r, grid_based, h, w, st), "bwd_f0")
        _lib.check(L.gfn_local_corr_mode_bwd_f0(_lib.ptr(gout), K * G * G, _lib.ptr(f1), _lib.ptr(f1s), _lib.ptr(flow), _lib.ptr(b), c * G * G,
                                                B, c, G, h, w, r, grid_based, h, w, 0, 0, st), "mode bwd_f0")
        torch.cuda.synchronize()
        assert torch.isfinite(a).all()
        assert torch.equal(a, b), (B, c, h, w, G, r, symmetric, grid_based)


def test_grid_sample_fwd_is_bit_identical_to_the_mode_entry_point_with_bilinear_zeros():
    from gfnet_amd import _lib

    L, st = _lib.lib(), _lib.stream_ptr(torch.device("cuda"))
    for B, C, H, W, Ho, Wo in [(2, 5, 13, 17, 9, 11), (3, 16, 24, 24, 32, 32), (1, 3, 7, 1, 4, 6)]:
        x = dev(synth.lattice_normalish((B, C, H, W), 1521))  # fp32 input
        grid = uniform((B, Ho, Wo, 2), 1522, 3.0)  # out to +-3: far outside the image on every side
        a = torch.full((B, C, Ho, Wo), float("nan"), device="cuda")
        b = torch.full((B, C, Ho, Wo), float("nan"), device="cuda")
        _lib.check(L.gfn_grid_sample_fwd(_lib.ptr(x), _lib.ptr(grid), _lib.ptr(a), C * Ho * Wo, B, C, H, W, Ho, Wo, st), "grid_sample")
        _lib.check(L.gfn_grid_sample_mode_fwd(_lib.ptr(x), _lib.GFN_F32, _lib.ptr(grid), _lib.ptr(b), C * Ho * Wo, B, C, H, W, Ho, Wo, 0, 0, st),
                   "grid_sample_mode")
        torch.cuda.synchronize()
        assert torch.isfinite(a).all()
        assert torch.equal(a, b), (B, C, H, W, Ho, Wo)


def test_non_finite_and_far_flows_read_zeros_in_every_mode():
    B, c, h, w, G, r = 1, 8, 16, 16, 8, 1
    f0 = dev(synth.lattice_normalish((B, c, G, G), 1601))
    f1 = dev(synth.lattice_normalish((B, c, h, w), 1602))
    flow = (synth.lattice_uniform((B, 2, G, G), 1603) * 0.5).astype(np.float32)
    bad = [(0, 0, float("nan")), (0, 1, float("inf")), (0, 2, -float("inf")), (0, 3, 3e9), (1, 4, -7e8)]
    for comp, cell, v in bad:
        flow[0, comp].flat[cell] = v
    flow = dev(flow)
    for sm, pm in ALL_MODES:
        out = host(lc(f0, f1, r, G, flow=flow, sample_mode=sm, padding_mode=pm))
        assert np.isfinite(out).all(), (sm, pm)
        for _, cell, _ in bad:
            assert (out[0, :].reshape(-1, G * G)[:, cell] == 0).all(), (sm, pm, cell)


# ---- gradient with respect to feature0 ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("sm,pm", ALL_MODES)
def test_feature0_gradient_matches_autograd_of_the_restatement(sm, pm):
    B, c, h, w, G, r = 2, 12, 18, 26, 8, 2
    num_level = 2 if (sm, pm) in (("bicubic", "reflection"), ("nearest", "border")) else 1
    f0 = synth.lattice_normalish((B, c, G, G), 1701)
    f1 = dev(synth.lattice_normalish((B, c, h, w), 1702))
    flow = uniform((B, 2, G, G), 1703, 1.2)
    g = dev(synth.lattice_normalish((B, (2 * r + 1) ** 2 * num_level, G, G), 1704))
    t0 = dev(f0).requires_grad_(True)
    out = lc(t0, f1, r, G, flow=flow, sample_mode=sm, padding_mode=pm, num_level=num_level)
    (out * g).sum().backward()
    u0 = dev(f0).requires_grad_(True)
    (restated_local_correlation(u0, f1, r, G, flow=flow, sample_mode=sm, padding_mode=pm, num_level=num_level) * g).sum().backward()
    assert_close(host(t0.grad), host(u0.grad), TOL, f"grad f0 {sm}/{pm}")


# ---- ConvRefiner(sample_mode=...) in eval mode ---------------------------------------------------------------------------------
def _refiner_inputs(Bi, c=8, hs=14, ws=18, G=8, flows=1, seed=1800):
    x = dev(synth.lattice_normalish((Bi, c, hs, ws), seed))
    y = dev(synth.lattice_normalish((Bi, c, hs, ws), seed + 1))
    fl = [uniform((Bi * 2, 2, G, G), seed + 2 + k, 1.1) for k in range(flows)]
    return x, y, fl


@pytest.mark.parametrize("sample_mode", ["nearest", "bicubic"])
def test_refiner_symmetric_batch_equals_two_plain_calls(sample_mode):
    ref = _toy_refiner(sample_mode)
    x, y, (flow,) = _refiner_inputs(2)
    G = flow.shape[-1]
    with torch.no_grad():
        d, lcorr = ref.assemble(G, x, y, flow, 1.5)
        da, _ = ref.assemble(G, x, y, flow[:2], 1.5)
        db, _ = ref.assemble(G, y, x, flow[2:], 1.5)
        out = ref(G, x, y, flow, scale_factor=1.5)
        oa = ref(G, x, y, flow[:2], scale_factor=1.5)
        ob = ref(G, y, x, flow[2:], scale_factor=1.5)
    torch.cuda.synchronize()
    assert torch.equal(d, torch.cat((da, db)))
    assert torch.equal(lcorr, d[:, 2 * 8 + 6:])
    for k in range(3):
        assert_close(host(out[k]), host(torch.cat((oa[k], ob[k]))), 1e-6, f"output {k}")


@pytest.mark.parametrize("sample_mode", ["nearest", "bicubic"])
@pytest.mark.parametrize("symmetric", [False, True])
def test_refiner_second_iteration_with_reuse_d_equals_a_fresh_call(sample_mode, symmetric):
    ref = _toy_refiner(sample_mode)
    x, y, (f1, f2) = _refiner_inputs(2, flows=2)
    if not symmetric:
        f1, f2 = f1[:2], f2[:2]
    G = f1.shape[-1]
    slot = [None]
    with torch.no_grad():
        ref(G, x, y, f1, reuse_d=slot)
        first = slot[0]
        second = ref(G, x, y, f2, reuse_d=slot)
        assert slot[0] is first  # the same buffer, rewritten in place except for its grid_feature planes
        fresh_d, _ = ref.assemble(G, x, y, f2)
        fresh = ref(G, x, y, f2)
    torch.cuda.synchronize()
    assert torch.equal(slot[0], fresh_d)
    for k in range(3):
        assert torch.equal(second[k], fresh[k])


@pytest.mark.parametrize("sample_mode", ["nearest", "bicubic"])
def test_training_assembly_gives_the_eval_concat_tensor(sample_mode):
    ref = _toy_refiner(sample_mode)
    x, y, (flow,) = _refiner_inputs(2)
    flow = flow[:2]
    G = flow.shape[-1]
    with torch.no_grad():
        d_eval, _ = ref.assemble(G, x, y, flow, 1.25)
    xg = x.clone().requires_grad_(True)
    d_train, lc_train = ref.assemble(G, xg, y, flow, 1.25)  # x asks for gradients: the differentiable torch assembly
    assert d_train.requires_grad
    assert_close(host(d_train), host(d_eval), 1e-5, "d")
    d_train.sum().backward()  # reaches x through grid_feature and the local correlation's feature0 gradient
    assert xg.grad is not None and bool(torch.isfinite(xg.grad).all())
