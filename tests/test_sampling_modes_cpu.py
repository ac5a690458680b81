"""CPU side of the sampling modes (nearest / bilinear / bicubic x zeros / border / reflection, utils/local_correlation.py:55-58,
model/network.py:464, 537, 547, 553-554): the constructor and call arguments the reference accepts are accepted, the new C entry
points reject bad codes and null pointers before touching a device, and a torch-CPU restatement of the reference's formula
reproduces the G10 fixture (which pins it)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import synth
from conftest import assert_close, load_golden

SAMPLE_MODES = ("nearest", "bilinear", "bicubic")
PADDING_MODES = ("zeros", "border", "reflection")


def restated_local_correlation(f0, f1, r, G, flow=None, sample_mode="bilinear", padding_mode="zeros", grid_based=False, num_level=1):
    """out[b, ky*(2r+1)+kx, i, j] = sum_c f0[b,c,i,j] / sqrt(c) * grid_sample(f1[b,c], p(b,i,j) + (wx[kx], wy[ky])) with p the flow (or
    the identity grid), wx / wy = linspace(-2r/s, 2r/s, 2r+1), s = the map's width / height (num_grid when grid_based), and f1
    2x average-pooled between levels: the reference's formula (utils/local_correlation.py:17-72) as one grid_sample per level."""
    B, c, h, w = f1.shape
    D = 2 * r + 1
    kw = dict(device=f1.device, dtype=torch.float32)
    if flow is None:
        py, px = torch.meshgrid(torch.linspace(-1 + 1 / h, 1 - 1 / h, h, **kw), torch.linspace(-1 + 1 / w, 1 - 1 / w, w, **kw), indexing="ij")
        p = torch.stack((px, py), -1)[None].expand(B, G, G, 2)
    else:
        p = flow.permute(0, 2, 3, 1)
    sy, sx = (G, G) if grid_based else (h, w)
    oy, ox = torch.meshgrid(torch.linspace(-2 * r / sy, 2 * r / sy, D, **kw), torch.linspace(-2 * r / sx, 2 * r / sx, D, **kw), indexing="ij")
    off = torch.stack((ox, oy), -1).reshape(D * D, 2)
    grid = (p[:, None] + off[None, :, None, None]).reshape(B, D * D * G, G, 2)
    levels = []
    for _ in range(num_level):
        s = F.grid_sample(f1, grid, mode=sample_mode, padding_mode=padding_mode, align_corners=False).reshape(B, c, D * D, G, G)
        levels.append((f0[:, :, None] / c ** 0.5 * s).sum(1))
        f1 = F.avg_pool2d(f1, 2, 2)
    return torch.cat(levels, 1)


def restated_case(c, sm, pm, dtype=torch.float32, f0=None):
    """restated_local_correlation of a case of tests/golden/sampling_cases.py (f0, f1, flow, r, G, grid_based, num_level, shape).
    The restatement pools once more than it needs, which a map one pixel high cannot: there the same formula runs over the case
    oracle's own tap coordinates (which the other cases pin)."""
    import sampling_cases as sc

    B, C, H, W = c["shape"]
    f0 = torch.from_numpy(c["f0"]).to(dtype) if f0 is None else f0
    f1 = torch.from_numpy(c["f1"]).to(dtype)
    flow = None if c["flow"] is None else torch.from_numpy(c["flow"]).to(dtype)
    if flow is None and dtype != torch.float32:  # the restatement's identity grid is fp32: hand it over widened
        lin = torch.linspace(-1 + 1 / W, 1 - 1 / W, W)
        flow = torch.stack(torch.meshgrid(lin, lin, indexing="xy"))[None].expand(B, 2, W, W).to(dtype)
    if min(H, W) > 1:
        return restated_local_correlation(f0, f1, c["r"], c["G"], flow=flow, sample_mode=sm, padding_mode=pm, grid_based=c["grid_based"],
                                          num_level=c["num_level"])
    assert c["num_level"] == 1
    G, K = c["G"], (2 * c["r"] + 1) ** 2
    gx, gy = sc.tap_coords(c["flow"], B, G, H, W, c["r"], c["grid_based"])
    grid = torch.from_numpy(np.stack((gx, gy), -1)).to(dtype).reshape(B, K * G, G, 2)
    s = F.grid_sample(f1, grid, mode=sm, padding_mode=pm, align_corners=False).reshape(B, C, K, G, G)
    return (f0[:, :, None] / C ** 0.5 * s).sum(1)


def _refiner(sample_mode):
    from gfnet_amd.model.network import ConvRefiner

    dim = 2 * 8 + 6 + 25
    return ConvRefiner(dim, dim, 3, kernel_size=5, dw=True, hidden_blocks=1, displacement_emb="linear", displacement_emb_dim=6,
                       local_corr_num=2, corr_in_other=True, amp=True, bn_momentum=0.01, sample_mode=sample_mode)


@pytest.mark.parametrize("sample_mode", ["nearest", "bicubic", "bilinear"])
def test_refiner_accepts_the_reference_sample_modes(sample_mode):
    ref = _refiner(sample_mode)
    assert ref.sample_mode == sample_mode


@pytest.mark.parametrize("sample_mode", ["area", "BILINEAR", None])
def test_refiner_still_refuses_other_sample_modes(sample_mode):
    with pytest.raises(ValueError, match="bicubic"):
        _refiner(sample_mode)


def test_mode_entry_points_reject_bad_codes_and_null_pointers_without_a_gpu():
    from gfnet_amd import _lib

    L = _lib.lib()
    fake = _lib.c_vp(256)  # never dereferenced: every call below must return before a launch
    # gfn_local_corr_mode_fwd(f0, f0_bs, f1, f1_second, dtype, flow, out, out_bs, B, C, G, H, W, r, grid_based, win_h, win_w, sm, pm, s)
    lc = lambda f0, out, sm, pm: L.gfn_local_corr_mode_fwd(f0, 16 * 64, fake, None, 0, fake, out, 25 * 64, 1, 16, 8, 8, 8, 2, 0, 8, 8,
                                                           sm, pm, None)
    for sm, pm in ((3, 0), (-1, 0), (0, 3), (1, -1)):
        assert lc(fake, fake, sm, pm) == -1
        assert b"sample_mode" in L.gfn_last_error()
    assert lc(None, fake, 1, 2) == -1 and b"null" in L.gfn_last_error()
    assert lc(fake, None, 2, 1) == -1 and b"null" in L.gfn_last_error()
    assert L.gfn_local_corr_mode_fwd(fake, 16 * 64, fake, None, 2, fake, fake, 25 * 64, 1, 16, 8, 8, 8, 2, 0, 8, 8, 1, 0, None) == -1  # dtype
    assert L.gfn_local_corr_mode_fwd(fake, 16 * 64, fake, fake, 0, fake, fake, 25 * 64, 3, 16, 8, 8, 8, 2, 0, 8, 8, 1, 0, None) == -1  # odd symmetric
    # gfn_local_corr_mode_bwd_f0(gout, gout_bs, f1, f1_second, flow, gf0, gf0_bs, B, C, G, H, W, r, grid_based, win_h, win_w, sm, pm, s)
    bwd = lambda g, gf0, sm, pm: L.gfn_local_corr_mode_bwd_f0(g, 25 * 64, fake, None, fake, gf0, 16 * 64, 1, 16, 8, 8, 8, 2, 0, 8, 8, sm,
                                                              pm, None)
    assert bwd(fake, fake, 7, 0) == -1 and b"sample_mode" in L.gfn_last_error()
    assert bwd(None, fake, 2, 2) == -1 and b"null" in L.gfn_last_error()
    assert bwd(fake, None, 1, 1) == -1 and b"null" in L.gfn_last_error()
    # gfn_grid_sample_mode_fwd(in, dtype, grid, out, out_bs, B, C, H, W, Ho, Wo, sm, pm, s)
    gs = lambda x, sm, pm: L.gfn_grid_sample_mode_fwd(x, 0, fake, fake, 4 * 6 * 6, 1, 4, 8, 8, 6, 6, sm, pm, None)
    assert gs(fake, 1, 5) == -1 and b"padding_mode" in L.gfn_last_error()
    assert gs(fake, 4, 0) == -1 and b"sample_mode" in L.gfn_last_error()
    assert gs(None, 2, 2) == -1
    # gfn_refiner_input_mode_fwd_dt(f0, f1, dtype, flow, dw, db, d, d_bs, B, C, Hs, Ws, G, disp_dim, disp_scale, symmetric, sm, s)
    ri = lambda f0, sm: L.gfn_refiner_input_mode_fwd_dt(f0, fake, 0, fake, fake, fake, fake, 47 * 64, 2, 8, 14, 18, 8, 6, 1.25, 0, sm, None)
    assert ri(fake, 3) == -1 and b"sample_mode" in L.gfn_last_error()
    assert ri(fake, -1) == -1
    assert ri(None, 2) == -1 and b"null" in L.gfn_last_error()
    assert L.gfn_refiner_input_mode_fwd_dt(fake, fake, 0, fake, fake, fake, fake, 47 * 64, 3, 8, 14, 18, 8, 6, 1.25, 1, 1, None) == -1
    # B == 0 with valid arguments: nothing to do, nothing launched
    assert L.gfn_local_corr_mode_fwd(fake, 16 * 64, fake, None, 0, fake, fake, 25 * 64, 0, 16, 8, 8, 8, 2, 0, 8, 8, 2, 2, None) == 0


def test_local_correlation_modes_need_a_gpu_not_a_different_mode():
    from gfnet_amd._lib import GfnError
    from gfnet_amd.utils.local_correlation import local_correlation

    B, c, h, w, G, r = 1, 4, 8, 8, 4, 1
    f0, f1, flow = torch.zeros(B, c, G, G), torch.zeros(B, c, h, w), torch.zeros(B, 2, G, G)
    for sm in SAMPLE_MODES:
        for pm in PADDING_MODES:
            with pytest.raises(GfnError, match="no CPU path"):
                local_correlation((B, c, h, w), f0, f1, r, G, flow=flow, sample_mode=sm, padding_mode=pm)
    with pytest.raises(GfnError):  # the autograd route checks the same way
        local_correlation((B, c, h, w), f0.clone().requires_grad_(True), f1, r, G, flow=flow, sample_mode="bicubic")
    with pytest.raises(ValueError, match="nearest"):
        local_correlation((B, c, h, w), f0, f1, r, G, flow=flow, sample_mode="area")
    with pytest.raises(ValueError, match="reflection"):
        local_correlation((B, c, h, w), f0, f1, r, G, flow=flow, padding_mode="circular")


def test_grid_sample_and_refiner_input_modes_need_a_gpu():
    from gfnet_amd import ops
    from gfnet_amd._lib import GfnError

    x, grid = torch.zeros(1, 4, 8, 8), torch.zeros(1, 6, 6, 2)
    with pytest.raises(GfnError):
        ops.grid_sample(x, grid, mode="bicubic", padding_mode="reflection")
    with pytest.raises(ValueError, match="bicubic"):
        ops.grid_sample(x, grid, mode="area")
    with pytest.raises(GfnError):
        ops.refiner_input(4, x, x, torch.zeros(1, 2, 4, 4), torch.zeros(6, 2, 1, 1), torch.zeros(6), 1, sample_mode="nearest")
    with pytest.raises(ValueError, match="bicubic"):
        ops.refiner_input(4, x, x, torch.zeros(1, 2, 4, 4), torch.zeros(6, 2, 1, 1), torch.zeros(6), 1, sample_mode="area")


def _g10_scale4_inputs(g):
    B, c, h, w, G, r = [int(v) for v in g["c_shape"]]
    s0, s1, s2 = [int(v) for v in g["c_seeds"]]
    f0 = synth.lattice_normalish((B, c, G, G), s0)
    f1 = synth.lattice_normalish((B, c, h, w), s1)
    flow = synth.homography_flow(B, G, s2)
    flow[1] *= np.float32(1.1)
    return f0, f1, flow, G, r


def test_restated_reference_formula_reproduces_g10():
    g = load_golden("g10_local_corr_modes")
    t = lambda k: torch.from_numpy(g[k])
    r, G = int(g["a_r"]), int(g["a_G"])
    for sm in SAMPLE_MODES:
        for pm in PADDING_MODES:
            out = restated_local_correlation(t("a_f0"), t("a_f1"), r, G, flow=t("a_flow"), sample_mode=sm, padding_mode=pm)
            assert_close(out.numpy(), g[f"a_out_{sm}_{pm}"], 1e-4, f"{sm}/{pm}")
    # the padding modes must matter on this fixture (flows reach outside the image)
    assert not np.allclose(g["a_out_bicubic_zeros"], g["a_out_bicubic_reflection"])
    assert not np.allclose(g["a_out_nearest_border"], g["a_out_nearest_zeros"])
    r, G = int(g["b_r"]), int(g["b_G"])
    for sm, pm in (("nearest", "reflection"), ("bicubic", "border")):
        kw = dict(sample_mode=sm, padding_mode=pm)
        assert_close(restated_local_correlation(t("b_f0"), t("b_f1"), r, G, flow=t("b_flow"), grid_based=True, **kw).numpy(),
                     g[f"b_grid_based_{sm}_{pm}"], 1e-4, "grid_based")
        assert_close(restated_local_correlation(t("b_f0"), t("b_f1"), r, G, flow=t("b_flow"), num_level=2, **kw).numpy(),
                     g[f"b_num_level2_{sm}_{pm}"], 1e-4, "num_level=2")
        assert_close(restated_local_correlation(t("b_f0"), t("b_f1"), r, G, flow=None, **kw).numpy(), g[f"b_flow_none_{sm}_{pm}"], 1e-4,
                     "flow=None")
    f0, f1, flow, G, r = _g10_scale4_inputs(g)
    idx = g["c_probe_idx"]
    for sm, pm in (("nearest", "reflection"), ("bicubic", "border"), ("bicubic", "zeros")):
        out = restated_local_correlation(torch.from_numpy(f0), torch.from_numpy(f1), r, G, flow=torch.from_numpy(flow), sample_mode=sm,
                                         padding_mode=pm).numpy()
        assert_close(out[idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]], g[f"c_probe_val_{sm}_{pm}"], 1e-4, f"probes {sm}/{pm}")
        np.testing.assert_allclose(out.astype(np.float64).sum(axis=(0, 2, 3)), g[f"c_sum_per_k_{sm}_{pm}"], rtol=0, atol=5e-2)
