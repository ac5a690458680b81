"""GPU: the sampling modes (csrc/sample_modes.h: nearest / bilinear / bicubic x zeros / border / reflection) through every per-tap
kernel, against the float64 oracle of tests/golden/sampling_cases.py, which tests/test_sampling_exact_cpu.py pins to F.grid_sample.

Exact family: torch.equal.  Power-of-two maps, half-pixel coordinates and small integers leave every weight, product and partial sum
an fp32 number (the builders assert the budget), so a kernel EQUALS the oracle rounded to fp32 or is wrong: exact pixel centres with
the second corner outside, nearest ties, the mirrors and their multiples, the border clamp at size - 1, one-pixel-wide maps, the
channel tail of a group (C = 9), floors at +-(10^6 - 1) (sampled) and at +-10^6, NaN, +-inf (zeros, by the documented guard).

Generic family (odd maps, lattice_normalish values, uniform coordinates), kept points only -- those >= 2^-10 px from every integer and
half-integer pixel coordinate, where no decision can flip.  grid_sample in nearest mode: equality (the value is one map element).
Bilinear and bicubic, and the local correlation in every mode (a sum over the channels; S = 0 for nearest):

    |out - oracle| <= 4 * E32 + S        per output

  E32  the error of the same definition evaluated in fp32 on the CPU (F.grid_sample / restated_local_correlation in float32) against
       the oracle, over the case, floored at 2^-24 * max|oracle|; 4 as in test_fpn_gpu.py and test_cross_attn_gpu.py.
  S    the coordinate allowance: the kernel may fuse the multiply-adds of unnorm and linspace_at where the oracle rounds each
       operation.  S is the largest change of the oracle over the case when every point moves by +-delta on either axis, delta =
       (fp32 roundings in the coordinate chain) * ulp(largest intermediate magnitude of the case, (max|g| + 1) * size), in pixels.
       grid_sample: 3 roundings -- g + 1, * size, - 1 (the halving is exact).  Local correlation: 7 -- the step's division
       (end - start) / (D - 1), step * i, start + (or end -) that, flow + offset, then unnorm's 3.  A rounding made in normalised
       units is half an ulp of a number <= max|g| + 1 and reaches the pixel coordinate times size / 2, so one ulp of
       (max|g| + 1) * size bounds each.  delta < 2^-12 px is asserted, so a kept point cannot cross a decision.
       While the library is built with -ffp-contract=off nothing fuses and S has no source: then |out - oracle| <= 4 * E32 is
       asserted as well.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sampling_cases as sc
from test_sampling_modes_cpu import restated_case

pytestmark = pytest.mark.gpu

ALL_MODES = sc.ALL_MODES

MEASURED = """
error / bound on an MI355X, worst case per family (from the figures the generic tests print before they assert):
grid_sample        bilinear 0.010 (5x1 C=12 fp16, zeros: err 2.2e-07, E32 7.8e-07, S 2.0e-05, bound 2.3e-05)
grid_sample        bicubic  0.095 (5x1 C=12 fp16, border: err 4.3e-06, E32 4.3e-06, S 2.8e-05, bound 4.5e-05)
grid_sample        nearest  equal, every case
local_correlation  nearest  0.250 (every case: err = E32, the kernel sums the channels in the restatement's order; S = 0)
local_correlation  bilinear 0.003 (c5_1x7 reflection: err 4.5e-07, E32 4.5e-07, S 1.6e-04, bound 1.6e-04)
local_correlation  bicubic  0.027 (c5_1x7 border: err 4.3e-06, E32 3.8e-06, S 1.4e-04, bound 1.6e-04)
S dominates every bound and is unused slack on this build: -ffp-contract=off (gfnet_amd/build.py) leaves the kernels' coordinate
chain as unfused as the oracle's.  While that flag stands, _check also asserts err <= 4 * E32 alone: worst err / (4 * E32) 0.27
for grid_sample (13x17 C=5 bicubic border), 0.30 for the local correlation (c5_1x7 bilinear zeros).
Exact family: every comparison equal.
"""


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.detach().float().cpu().numpy()


def lc(c, f1=None, **kw):
    from gfnet_amd.utils.local_correlation import local_correlation

    f0 = kw.pop("f0", None)
    return local_correlation(c["shape"], dev(c["f0"]) if f0 is None else f0, dev(c["f1"]) if f1 is None else f1, c["r"], c["G"],
                             flow=None if c["flow"] is None else dev(c["flow"]), grid_based_correlation=c.get("grid_based", False),
                             num_level=c.get("num_level", 1), **kw)


def assert_equal(got, want, what):
    """torch.equal of the kernel's output and the float64 oracle rounded to fp32, with the first differing element in the message."""
    got, want = host(got), np.asarray(want, np.float64).astype(np.float32)
    assert got.shape == want.shape, f"{what}: shape {got.shape} vs {want.shape}"
    if not torch.equal(torch.from_numpy(got), torch.from_numpy(want)):
        bad = np.argwhere(~(got == want))
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {got.size} differ, first at {i}: got {got[i]!r}, oracle {want[i]!r}")


# ---- exact family ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [3, 9])
@pytest.mark.parametrize("H,W", sc.EXACT_MAPS)
def test_grid_sample_equals_the_oracle(H, W, C):
    from gfnet_amd import ops

    c = sc.exact_grid_case(H, W, C)
    grid = dev(c["grid"])
    for dtype in (torch.float32, torch.float16):
        x = dev(c["x"]).to(dtype)
        assert torch.equal(x.float().cpu(), torch.from_numpy(c["x"]))  # the fp16 copy is exact
        for sm, pm in ALL_MODES:
            out = ops.grid_sample(x, grid, mode=sm, padding_mode=pm)
            assert_equal(out, sc.exact_grid_oracle(H, W, C, sm, pm), f"grid_sample {H}x{W} C={C} {sm}/{pm} {dtype}")


@pytest.mark.parametrize("sm,pm", ALL_MODES)
def test_grid_sample_guard_points_read_zeros_and_their_neighbours_do_not(sm, pm):
    from gfnet_amd import ops

    for H, W in sc.EXACT_MAPS:
        c = sc.exact_grid_case(H, W, 3)
        n = c["guard"].size - len(sc.extreme_points(H, W)[0])
        out = host(ops.grid_sample(dev(c["x"]), dev(c["grid"]), mode=sm, padding_mode=pm))
        want = sc.exact_grid_oracle(H, W, 3, sm, pm)
        assert np.isfinite(out).all()
        assert (out[..., c["guard"]] == 0).all()
        assert np.array_equal(out[..., n:], want[..., n:].astype(np.float32))  # floors +-(10^6 - 1): the oracle's per-mode value
        if pm != "zeros":
            assert (want[..., n:][..., ~c["guard"][n:]] != 0).any()


@pytest.mark.parametrize("name", sorted(sc.EXACT_LC))
def test_local_correlation_equals_the_oracle(name):
    c = sc.exact_lc_case(name)
    B, C, H, W = c["shape"]
    G, K = c["G"], (2 * c["r"] + 1) ** 2 * c["num_level"]
    gx, gy = sc.tap_coords(c["flow"], B, G, H, W, c["r"], c["grid_based"])
    insane = ~sc.sane(sc.unnorm(gx, W), sc.unnorm(gy, H))  # level 1 of two: every tap of a guard cell
    for sm, pm in ALL_MODES:
        want = sc.exact_lc_oracle(name, sm, pm)
        kw = dict(sample_mode=sm, padding_mode=pm)
        out = lc(c, **kw)
        assert_equal(out, want, f"{name} {sm}/{pm}")
        assert np.isfinite(host(out)).all() and (host(out)[:, :K // c["num_level"]][insane] == 0).all()
        assert_equal(lc(c, f1=dev(c["f1"]).half(), **kw), want, f"{name} {sm}/{pm} fp16 feature1")
        buf = torch.full((B, C + 3 + K, G, G), 7.0, device="cuda")  # out= into the channel slice of a concat buffer, f0 from it too
        buf[:, :C] = dev(c["f0"])
        lc(c, f0=buf[:, :C], out=buf[:, C + 3:], **kw)
        assert_equal(buf[:, C + 3:], want, f"{name} {sm}/{pm} out slice")
        assert bool((buf[:, C:C + 3] == 7.0).all())
    if c["extreme"].any():
        assert insane.all(1)[c["extreme"]].sum() >= 5  # the far and non-finite flows: whole cells of zeros


@pytest.mark.parametrize("variant", [0, 1, 2, 4])
@pytest.mark.parametrize("r", [1, 4])
def test_bilinear_zeros_routes_equal_the_oracle(r, variant):
    """The lean (0, 4), general (1) and round-1 (2) routes of gfn_local_corr_fwd_dt, with integer fractions at the last row and column
    and far, guard and NaN cells for tap_general."""
    c = sc.exact_route_case(r)
    for f1 in (dev(c["f1"]), dev(c["f1"]).half()):
        assert_equal(lc(c, f1=f1, _variant=variant), c["want"], f"route r={r} variant {variant} {f1.dtype}")


@pytest.mark.parametrize("name", sorted(sc.EXACT_LC))
def test_feature0_gradient_equals_the_oracle(name):
    from gfnet_amd import _lib

    c = sc.exact_lc_case(name)
    B, C, H, W = c["shape"]
    G, r = c["G"], c["r"]
    K = (2 * r + 1) ** 2
    L, st = _lib.lib(), _lib.stream_ptr(torch.device("cuda"))
    gout, f1 = dev(c["grad_out"]), dev(c["f1"])
    flow = None if c["flow"] is None else dev(c["flow"])
    for sm, pm in ALL_MODES:
        want = sc.exact_lc_grad_oracle(name, sm, pm)
        f0 = dev(c["f0"]).requires_grad_(True)
        (lc(c, f0=f0, sample_mode=sm, padding_mode=pm) * gout).sum().backward()
        assert_equal(f0.grad, want, f"{name} autograd {sm}/{pm}")
        if c["num_level"] == 1:
            code_s, code_p = _lib.mode_codes(sm, pm, "test")
            g = torch.full((B, C, G, G), float("nan"), device="cuda")
            _lib.check(L.gfn_local_corr_mode_bwd_f0(_lib.ptr(gout), K * G * G, _lib.ptr(f1), None, _lib.ptr(flow), _lib.ptr(g), C * G * G, B, C, G, H, W,
                                                    r, 1 if c["grid_based"] else 0, H, W, code_s, code_p, st), "mode bwd_f0")
            assert_equal(g, want, f"{name} gfn_local_corr_mode_bwd_f0 {sm}/{pm}")


def _refiner_input(c, k, sm, name, dtype, reuse=None):
    from gfnet_amd import ops

    rr = sc.ri_radius(name, sm)
    with torch.no_grad():
        return ops.refiner_input(c["G"], dev(c["x"]).to(dtype), dev(c["y"]).to(dtype), dev(c["flows"][k]), dev(c["dw"]), dev(c["db"]),
                                 rr if rr is not None else 1, scale_factor=1.0, corr_in_other=rr is not None, reuse=reuse, sample_mode=sm)


@pytest.mark.parametrize("sm", sc.SAMPLE_MODES)
@pytest.mark.parametrize("symmetric", [False, True])
@pytest.mark.parametrize("name", sorted(sc.EXACT_RI))
def test_refiner_input_equals_the_oracle(name, symmetric, sm):
    """The whole d tensor -- grid_feature, x_hat, the displacement planes (disp_scale 1.25) and the local correlation -- on the first call
    and on the `reuse` call (the KEEP instantiation: grid_feature stays, the rest is rewritten for the new flow)."""
    c = sc.exact_ri_case(name, symmetric)
    for dtype in (torch.float32, torch.float16):
        d = _refiner_input(c, 0, sm, name, dtype)
        assert_equal(d, sc.exact_ri_oracle(name, symmetric, sm, 0), f"refiner_input {name} {sm} {dtype} symmetric={symmetric}")
        d2 = _refiner_input(c, 1, sm, name, dtype, reuse=d)
        assert d2.data_ptr() == d.data_ptr()
        assert_equal(d2, sc.exact_ri_oracle(name, symmetric, sm, 1), f"refiner_input reuse {name} {sm} {dtype} symmetric={symmetric}")


@pytest.mark.parametrize("sm", sc.SAMPLE_MODES)
def test_refiner_input_guard_points_read_zeros(sm):
    name = "c16_8x8_g8"
    c = sc.exact_ri_case(name, True, True)
    C, Dd, G = c["C"], c["Dd"], c["G"]
    d = host(_refiner_input(c, 0, sm, name, torch.float32))
    want = sc.exact_ri_oracle(name, True, sm, 0, True).astype(np.float32)
    sampled = np.r_[0:2 * C, 2 * C + Dd:d.shape[1]]
    assert np.isfinite(d[:, sampled]).all()
    assert np.array_equal(d[:, sampled], want[:, sampled])
    flow = c["flows"][0]
    gone = ~sc.sane(sc.unnorm(flow[:, 0], 8), sc.unnorm(flow[:, 1], 8))
    assert gone.sum() >= 5 and (np.moveaxis(d[:, C:2 * C], 1, -1)[gone] == 0).all()  # x_hat of a guard cell
    ok = ~c["extreme"][0]
    assert np.array_equal(np.moveaxis(d[:, 2 * C:2 * C + Dd], 1, -1)[ok], np.moveaxis(want[:, 2 * C:2 * C + Dd], 1, -1)[ok])


# ---- generic family -------------------------------------------------------------------------------------------------------------
def _check(err, e32, omax, S, what):
    from gfnet_amd import build

    unit = 4 * max(e32, 2.0 ** -24 * omax)
    bound = unit + S
    print(f"{what}: err {err:.3e}, E32 {e32:.3e}, S {S:.3e}, bound {bound:.3e}, err / bound {err / bound:.3f}, err / 4 E32 {err / unit:.3f}")
    assert err <= bound, what
    if "-ffp-contract=off" in build.FLAGS:  # nothing is fused: the kernel rounds the coordinate chain as the oracle does, S is slack
        assert err <= unit, f"{what}: within the allowance S, but S has no source while the build keeps contraction off"


@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("H,W,C", sc.GENERIC_MAPS)
def test_grid_sample_generic_kept_points(H, W, C, f16):
    from gfnet_amd import ops

    c = sc.generic_grid_case(H, W, C, f16)
    x32 = torch.from_numpy(np.asarray(c["x"], np.float32))
    x, grid = dev(c["x"]), dev(c["grid"])
    assert x.dtype == (torch.float16 if f16 else torch.float32)
    for sm, pm in ALL_MODES:
        want, S, _ = sc.generic_grid_oracle(H, W, C, f16, sm, pm)
        got = sc.grid_kept(host(ops.grid_sample(x, grid, mode=sm, padding_mode=pm)), c["keep"])
        what = f"grid_sample {H}x{W} C={C} f16={f16} {sm}/{pm}"
        if sm == "nearest":
            assert np.array_equal(got, want.astype(np.float32)), what
            continue
        cpu = F.grid_sample(x32, torch.from_numpy(c["grid"]), mode=sm, padding_mode=pm, align_corners=False).numpy()
        e32 = float(np.abs(sc.grid_kept(cpu, c["keep"]) - want).max())
        _check(float(np.abs(got - want).max()), e32, float(np.abs(want).max()), S, what)


@pytest.mark.parametrize("name", sorted(sc.GENERIC_LC))
def test_local_correlation_generic_kept_cells(name):
    c = sc.generic_lc_case(name)
    c32 = dict(c, f1=np.asarray(c["f1"], np.float32))
    for sm, pm in ALL_MODES:
        want, S = sc.generic_lc_oracle(name, sm, pm)
        got = sc.lc_kept(host(lc(c, sample_mode=sm, padding_mode=pm)), c["keep"])
        e32 = float(np.abs(sc.lc_kept(restated_case(c32, sm, pm).numpy(), c["keep"]) - want).max())
        _check(float(np.abs(got - want).max()), e32, float(np.abs(want).max()), S, f"local_correlation {name} {sm}/{pm}")


# ---- determinism ----------------------------------------------------------------------------------------------------------------
def test_every_entry_point_gives_the_same_bits_twice():
    from gfnet_amd import ops

    g = sc.generic_grid_case(13, 17, 12, False)
    a, b = (ops.grid_sample(dev(g["x"]), dev(g["grid"]), mode="bicubic", padding_mode="reflection") for _ in range(2))
    assert torch.equal(a, b)
    c = sc.generic_lc_case("c5_13x17_levels2")
    a, b = (lc(c, sample_mode="bicubic", padding_mode="border") for _ in range(2))
    assert torch.equal(a, b)
    a, b = (lc(c) for _ in range(2))  # bilinear + zeros: gfn_local_corr_fwd_dt
    assert torch.equal(a, b)
    grads = []
    for _ in range(2):
        f0 = dev(c["f0"]).requires_grad_(True)
        (lc(c, f0=f0, sample_mode="bilinear", padding_mode="reflection") * dev(c["grad_out"])).sum().backward()
        grads.append(f0.grad)
    assert torch.equal(*grads)
    r = sc.exact_ri_case("c16_16x16_g16", True)
    for sm in ("bilinear", "bicubic"):
        a, b = (_refiner_input(r, 0, sm, "c16_16x16_g16", torch.float16) for _ in range(2))
        assert torch.equal(a, b)
