"""Pins the float64 oracle of tests/golden/sampling_cases.py (the definition tests/test_sampling_exact_gpu.py holds the kernels to)
without a GPU.

  exact family   the oracle equals F.grid_sample on the CPU in float64 and in float32, bit for bit, in all nine mode pairs: exact
                 pixel centres, nearest ties (half to even), the mirrors at -0.5 and size - 0.5 and their multiples, the border
                 clamp at size - 1, one-pixel-wide maps, floors at +-(10^6 - 1).  At the guard (floor <= -10^6 or >= 10^6,
                 non-finite) the oracle reads zeros by definition and torch does not: the documented deviation, asserted.
  generic kept   |oracle - torch float64| <= S, the coordinate allowance of the GPU module (torch un-normalises in double there, so
                 this shows S covers a coordinate rounding); |oracle - torch fp32| <= S + n * 2^-24 * A per output, A the oracle's
                 sum of |weight * value| and n the fp32 roundings of a sample's value after the coordinates (nearest 0; bilinear 8:
                 two subtractions and a product per weight, a product and an addition per corner, rounded up; bicubic 32: six per
                 coefficient polynomial value, two per tap and row).
  local corr.    the oracle equals restated_local_correlation (test_sampling_modes_cpu.py) on the exact family bit for bit, its
                 gradient equals autograd's, and it reproduces the reference-generated G10 fixture within that fixture's 1e-4 rule.
The builders assert their exactness budgets and kept shares when they build a case; test_budgets_and_kept_shares states them."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sampling_cases as sc
from conftest import assert_close, load_golden
from test_sampling_modes_cpu import restated_case, restated_local_correlation

ALL_MODES = sc.ALL_MODES
VALUE_ROUNDINGS = {"nearest": 0, "bilinear": 8, "bicubic": 32}


def torch_grid_sample(x, grid, sm, pm, dtype):
    return F.grid_sample(torch.from_numpy(np.asarray(x, np.float32)).to(dtype), torch.from_numpy(grid).to(dtype), mode=sm, padding_mode=pm,
                         align_corners=False).numpy()


@pytest.mark.parametrize("sm,pm", ALL_MODES)
def test_oracle_equals_torch_bit_for_bit_on_the_exact_family(sm, pm):
    differs_at_guard = False
    for H, W in sc.EXACT_MAPS:
        c = sc.exact_grid_case(H, W, 3)
        want = sc.exact_grid_oracle(H, W, 3, sm, pm)
        ok = ~c["guard"]
        assert (want[..., c["guard"]] == 0).all()
        for dtype in (torch.float64, torch.float32):
            got = torch_grid_sample(c["x"], c["grid"], sm, pm, dtype)
            assert np.array_equal(got[..., ok], want[..., ok].astype(got.dtype)), (H, W, dtype)
            with np.errstate(invalid="ignore"):
                differs_at_guard |= bool((got[..., c["guard"]] != 0).any())
    if pm != "zeros" and sm != "bicubic":  # the documented deviation: torch clamps or mirrors a far coordinate into the image
        assert differs_at_guard


def test_lattice_covers_the_decisions():
    gx, gy, guard, n = sc.exact_points(8, 16)
    assert n == 25425 and int(guard.sum()) >= 30 and int((~guard[n:]).sum()) >= 12
    px = sc.unnorm(gx[:n], 16)
    for v in (-0.5, 15.5, 15.0, 0.0, 0.5, 2.5, -16.5, 31.5, -48.0, 64.0):  # mirrors and their images, centres, ties, the ends
        assert (px == v).any(), v
    fl = np.floor(sc.unnorm(gx[n:], 16)[~guard[n:]])
    assert (fl == 999999).any() and (fl == -999999).any()


@pytest.mark.parametrize("H,W,C", sc.GENERIC_MAPS)
def test_generic_kept_points_against_torch(H, W, C):
    c = sc.generic_grid_case(H, W, C, False)
    for sm, pm in ALL_MODES:
        want, S, A = sc.generic_grid_oracle(H, W, C, False, sm, pm)
        t64 = sc.grid_kept(torch_grid_sample(c["x"], c["grid"], sm, pm, torch.float64), c["keep"])
        t32 = sc.grid_kept(torch_grid_sample(c["x"], c["grid"], sm, pm, torch.float32), c["keep"]).astype(np.float64)
        e64, e32 = float(np.abs(t64 - want).max()), np.abs(t32 - want)
        unit = S + VALUE_ROUNDINGS[sm] * 2.0 ** -24 * A
        print(f"{H}x{W} {sm}/{pm}: S {S:.2e}, |f64 - oracle| {e64:.2e}, fp32 err / unit {float((e32 / np.maximum(unit, 1e-300)).max()):.3f}")
        if sm == "nearest":
            assert S == 0 and e64 == 0 and float(e32.max()) == 0
        else:
            assert e64 <= S + 1e-13 * float(np.abs(want).max())
            assert (e32 <= unit).all()


@pytest.mark.parametrize("name", sorted(sc.EXACT_LC))
def test_local_correlation_oracle_equals_the_restatement_on_the_exact_family(name):
    c = sc.exact_lc_case(name)
    ok = np.broadcast_to(~c["extreme"][:, None], sc.exact_lc_oracle(name, "nearest", "zeros").shape)
    for sm, pm in ALL_MODES:
        want = sc.exact_lc_oracle(name, sm, pm)
        got = restated_case(c, sm, pm).numpy()
        assert np.isfinite(want).all()
        assert np.array_equal(got[ok], want[ok].astype(np.float32)), (name, sm, pm)
        # the gradient: autograd of the restatement in float64 (it divides each product by sqrt(C), the oracle the sum: the last bit)
        f0 = torch.from_numpy(c["f0"]).double().requires_grad_(True)
        out = restated_case(c, sm, pm, torch.float64, f0)
        keep = torch.from_numpy(np.ascontiguousarray(ok))
        (torch.where(keep, out, torch.zeros_like(out)) * torch.from_numpy(c["grad_out"]).double()).sum().backward()
        gwant = sc.exact_lc_grad_oracle(name, sm, pm)
        gok = np.broadcast_to(~c["extreme"][:, None], gwant.shape)
        np.testing.assert_allclose(f0.grad.numpy()[gok], gwant[gok], rtol=1e-14, atol=0)


def test_local_correlation_oracle_reproduces_g10():
    g = load_golden("g10_local_corr_modes")
    r, G = int(g["a_r"]), int(g["a_G"])
    for sm, pm in ALL_MODES:
        assert_close(sc.local_correlation(g["a_f0"], g["a_f1"], g["a_flow"], r, G, sm, pm), g[f"a_out_{sm}_{pm}"], 1e-4, f"{sm}/{pm}")
    r, G = int(g["b_r"]), int(g["b_G"])
    for sm, pm in (("nearest", "reflection"), ("bicubic", "border")):
        lc = lambda flow, **kw: sc.local_correlation(g["b_f0"], g["b_f1"], flow, r, G, sm, pm, **kw)
        assert_close(lc(g["b_flow"], grid_based=True), g[f"b_grid_based_{sm}_{pm}"], 1e-4, "grid_based")
        assert_close(lc(g["b_flow"], num_level=2), g[f"b_num_level2_{sm}_{pm}"], 1e-4, "num_level=2")
        assert_close(lc(None), g[f"b_flow_none_{sm}_{pm}"], 1e-4, "flow=None")


def test_refiner_input_oracle_is_the_three_parts_and_the_correlation():
    c = sc.exact_ri_case("c9_8x16_g4", True)
    C, Dd, G, flow = c["C"], c["Dd"], c["G"], c["flows"][0]
    d = sc.exact_ri_oracle("c9_8x16_g4", True, "bilinear", 0)
    q, s = np.concatenate((c["x"], c["y"])), np.concatenate((c["y"], c["x"]))  # directions (x vs y), then (y vs x)
    lin = torch.linspace(-1 + 1 / G, 1 - 1 / G, G)
    cy, cx = torch.meshgrid(lin, lin, indexing="ij")
    centres = torch.stack((cx, cy), -1)[None].expand(4, G, G, 2)
    gs = lambda a, grid: F.grid_sample(torch.from_numpy(a), grid, mode="bilinear", padding_mode="zeros", align_corners=False)
    fl = torch.from_numpy(flow).permute(0, 2, 3, 1)
    emb = F.conv2d(1.25 * (fl - centres).permute(0, 3, 1, 2), torch.from_numpy(c["dw"]), torch.from_numpy(c["db"]))
    gf = gs(q, centres)
    lcorr = restated_local_correlation(gf, torch.from_numpy(s), 1, G, flow=torch.from_numpy(flow))
    want = torch.cat((gf, gs(s, fl), emb, lcorr), 1).numpy()
    assert d.shape == (4, 2 * C + Dd + 9, G, G)
    assert np.array_equal(d.astype(np.float32), want)


def test_budgets_and_kept_shares():
    for H, W in sc.EXACT_MAPS:
        for C in (3, 9):
            sc.exact_grid_case(H, W, C)  # asserts sum |term| * denominator < 2^24 for the nine pairs
    for name in sc.EXACT_LC:
        sc.exact_lc_case(name)  # ... of the correlation and of the gradient's accumulator, and that every tap is on the lattice
    for r in (1, 4):
        sc.exact_route_case(r)
    for name in sc.EXACT_RI:
        for symmetric in (False, True):
            sc.exact_ri_case(name, symmetric)
    for H, W, C in sc.GENERIC_MAPS:
        for f16 in (False, True):
            c = sc.generic_grid_case(H, W, C, f16)
            assert c["dropped"] <= sc.MAX_DROPPED and max(c["deltas"]) < 2.0 ** -12
            print(f"generic grid {H}x{W} f16={f16}: {c['dropped']:.2%} of the points left out")
    for name in sorted(sc.GENERIC_LC):
        c = sc.generic_lc_case(name)
        assert c["dropped"] <= sc.MAX_DROPPED and c["cells"] >= sc.MIN_CELLS_KEPT and max(c["deltas"]) < 2.0 ** -12
        print(f"generic lc {name}: {c['dropped']:.2%} of the taps left out, {c['cells']:.1%} of the cells kept")
    # 200 000 uniform draws on a 13 x 17 map: the share within 2^-10 px of an integer or half-integer on either axis
    g = np.random.RandomState(1).uniform(-3, 3, size=(200000, 2)).astype(np.float32)
    out = 1.0 - float((sc.kept(g[:, 0], 17) & sc.kept(g[:, 1], 13)).mean())
    assert 0.006 < out < 0.009, out
