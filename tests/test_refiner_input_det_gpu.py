"""The bit-reproducible dy of the refiner-input backward (gfn_refiner_input_bwd_det, ops.refiner_input_bwd(deterministic=True)):
the fp32 atomic scatter of the plain call as an order-independent sum in 64-bit fixed point.

Accuracy is tests/test_refiner_input_bwd_gpu.py's: its cases, its float64 autograd reference and its bound, 1e-4 * max(1, max|ref|).
Reproducibility is exact everywhere: equal bits between two runs, under a permutation of the grid cells (which changes the order
every add arrives in), with and without batch peers, for fp16 and fp32 maps, and through autograd under
torch.use_deterministic_algorithms(True).  The other four gradients are the plain call's bits."""
import numpy as np
import pytest
import torch

from test_refiner_input_bwd_gpu import CASES, NAMES, SF, SHAPES, cached_reference, case_id, inputs_of, library_grads, ratio, reference_grads

pytestmark = pytest.mark.gpu

# every cell of a sample flows to one interior point with fraction (0.3, 0.6): G * G = 1089 terms in each of four elements per channel
COLLAPSE = (2, 3, 12, 10, 33, 1, 0, "f32")


def det_grads(case, inp, grad_d, need=(True,) * 5):
    """library_grads with deterministic=True"""
    from gfnet_amd import ops

    r = case[6]
    c = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    out = ops.refiner_input_bwd(c(grad_d), c(inp["y"]), c(inp["flow"]), c(inp["w"]), r, SF, r > 0, need=need, deterministic=True)
    grads = dict(zip(NAMES, out))
    if grads["w"] is not None:
        grads["w"] = grads["w"].reshape(-1, 2, 1, 1)
    return grads


def bits_equal(a, b):
    """equal bit patterns (NaNs compare by their bits, -0 differs from +0)"""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def collapse_inputs():
    B, C, Hs, Ws, G, Dd, r, _ = COLLAPSE
    rng = np.random.default_rng(77)
    px, py = np.array([4.3, 6.3]), np.array([5.6, 2.6])  # per sample; corners (4,5),(5,5),(4,6),(5,6) and (6,2),(7,2),(6,3),(7,3)
    flow = np.empty((B, 2, G, G), np.float32)
    flow[:, 0] = ((2 * px + 1) / Ws - 1)[:, None, None]
    flow[:, 1] = ((2 * py + 1) / Hs - 1)[:, None, None]
    return dict(x=rng.normal(0, 1, (B, C, Hs, Ws)).astype(np.float32), y=rng.normal(0, 1, (B, C, Hs, Ws)).astype(np.float32), flow=flow,
                w=rng.uniform(-1, 1, (Dd, 2, 1, 1)).astype(np.float32), b=rng.uniform(-1, 1, (Dd,)).astype(np.float32),
                grad_d=rng.normal(0, 1, (B, 2 * C + Dd, G, G)).astype(np.float32))


def permuted(case, inp, seed):
    """the G * G cells of flow and of grad_d[:, C:2C] under one random permutation per sample: the same multiset of dy terms"""
    B, C, G = case[0], case[1], case[4]
    rng = np.random.default_rng(seed)
    flow, g = inp["flow"].copy().reshape(B, 2, G * G), inp["grad_d"].copy().reshape(B, -1, G * G)
    for b in range(B):
        perm = rng.permutation(G * G)
        assert not np.array_equal(perm, np.arange(G * G))
        flow[b] = flow[b][:, perm]
        g[b, C:2 * C] = g[b, C:2 * C][:, perm]
    out = dict(inp)
    out["flow"], out["grad_d"] = flow.reshape(inp["flow"].shape), g.reshape(inp["grad_d"].shape)
    return out


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_dy_matches_float64_and_the_other_gradients_are_the_plain_calls_bits(case):
    inp = inputs_of(case)
    ref = cached_reference(case)
    det = det_grads(case, inp, inp["grad_d"])
    plain = library_grads(case, inp, inp["grad_d"])
    worst = ratio(det["y"], ref["y"])
    print(f"{case_id(case)}: deterministic dy err / bound {worst:.3f} (plain {ratio(plain['y'], ref['y']):.3f})")
    assert det["y"].dtype == torch.float32 and torch.isfinite(det["y"]).all()
    assert worst <= 1.0
    for k in ("x", "flow", "w", "b"):
        assert bits_equal(det[k], plain[k]), k


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_two_runs_give_equal_bits_for_all_five_gradients(case):
    inp = inputs_of(case)
    first = det_grads(case, inp, inp["grad_d"])
    again = det_grads(case, inp, inp["grad_d"])
    for k in NAMES:
        assert bits_equal(first[k], again[k]), k
    alone = det_grads(case, inp, inp["grad_d"], need=(False, True, False, False, False))  # NULL for the other outputs
    assert all(alone[k] is None for k in NAMES if k != "y") and bits_equal(alone["y"], first["y"])


@pytest.mark.parametrize("which", ["small_outside", "planned_homography", "collapse"])
def test_dy_does_not_depend_on_the_order_of_the_cells(which):
    """the cells permuted, per sample: every atomic add arrives from another thread, wave and workgroup, and the sum keeps its bits"""
    if which == "collapse":
        case, inp = COLLAPSE + ("collapse",), collapse_inputs()
    else:
        case = (SHAPES[0] + ("outside",)) if which == "small_outside" else (SHAPES[2] + ("homography",))
        inp = inputs_of(case)
    base = det_grads(case, inp, inp["grad_d"])["y"]
    assert float(base.abs().max()) > 0
    for seed in (1, 2):
        moved = permuted(case, inp, seed)
        assert bits_equal(det_grads(case, moved, moved["grad_d"])["y"], base), seed
    if which == "collapse":
        B, C, Hs, Ws, G = case[:5]
        assert int((base != 0).sum()) == B * C * 4  # G * G terms in each of four elements per channel
        ref = reference_grads(case, inp, inp["grad_d"])["y"]
        worst = ratio(base, ref)
        print(f"collapse: {G * G} terms per element, err / bound {worst:.3f}, max |ref| {float(ref.abs().max()):.3f}")
        assert worst <= 1.0


def test_a_samples_dy_is_the_dy_of_the_sample_run_alone():
    case = SHAPES[2] + ("homography",)  # B = 3
    inp = dict(inputs_of(case))
    scale = np.array([1.0, 1e-3, 300.0], np.float32)[:, None, None, None]  # the samples' scales M_b far apart
    inp["grad_d"] = inp["grad_d"] * scale
    batch = det_grads(case, inp, inp["grad_d"])["y"]
    for b in range(case[0]):
        one = {k: (v[b:b + 1] if k in ("x", "y", "flow", "grad_d") else v) for k, v in inp.items()}
        alone = det_grads(case, one, np.ascontiguousarray(one["grad_d"]))["y"]
        assert bits_equal(alone[0], batch[b]), b


def corner_mask(inp, b, c, i, j):
    """the dy elements of channel c that cell (i, j) of sample b adds to: its corners inside the map (float64 on the fp32 flow; the
    inputs keep every sample >= 1e-3 pixels from an integer position)"""
    B, C, Hs, Ws = inp["y"].shape
    ix = ((float(inp["flow"][b, 0, i, j]) + 1) * Ws - 1) / 2
    iy = ((float(inp["flow"][b, 1, i, j]) + 1) * Hs - 1) / 2
    mask = torch.zeros(B, C, Hs, Ws, dtype=torch.bool)
    for y in (int(np.floor(iy)), int(np.floor(iy)) + 1):
        for x in (int(np.floor(ix)), int(np.floor(ix)) + 1):
            if 0 <= y < Hs and 0 <= x < Ws:
                mask[b, c, y, x] = True
    return mask


def test_non_finite_gradients_poison_exactly_their_corner_elements():
    case = SHAPES[0] + ("noise",)  # B = 2, C = 9, 8 x 8, G = 6
    inp = inputs_of(case)
    C = case[1]
    g = inp["grad_d"].copy()
    g[0, C + 2, 3, 2] = np.inf
    g[1, C + 5, 2, 4] = np.nan
    zeroed = g.copy()
    zeroed[0, C + 2, 3, 2] = zeroed[1, C + 5, 2, 4] = 0
    mask = corner_mask(inp, 0, 2, 3, 2) | corner_mask(inp, 1, 5, 2, 4)
    assert int(mask.sum()) == 8  # both cells lie inside the map
    dy = det_grads(case, inp, g)["y"].cpu()
    clean = det_grads(case, inp, zeroed)["y"].cpu()
    assert torch.equal(torch.isnan(dy), mask) and not torch.isinf(dy).any()
    assert bits_equal(dy[~mask], clean[~mask]) and torch.isfinite(clean).all()
    plain = library_grads(case, inp, g)["y"].cpu()
    assert torch.equal(~torch.isfinite(plain), mask)  # exactly the elements the plain call makes non-finite
    # a sample whose x_hat gradients are all non-finite or zero has no scale: its finite terms are zeros
    g2 = inp["grad_d"].copy()
    g2[0, C:2 * C] = 0
    g2[0, C + 2, 3, 2] = -np.inf
    dy2 = det_grads(case, inp, g2)["y"].cpu()
    m2 = corner_mask(inp, 0, 2, 3, 2)
    assert torch.equal(torch.isnan(dy2), m2) and float(dy2[0][~m2[0]].abs().max()) == 0
    assert bits_equal(dy2[1], det_grads(case, inp, inp["grad_d"])["y"].cpu()[1])


def test_an_all_zero_gradient_gives_an_all_zero_dy():
    case = SHAPES[1] + ("homography",)
    inp = inputs_of(case)
    dy = det_grads(case, inp, np.zeros_like(inp["grad_d"]))["y"]
    assert bits_equal(dy, torch.zeros_like(dy))


def test_tiny_and_huge_gradients_keep_their_accuracy():
    """the scale follows the sample: gradients of 1e-18 or 1e27 lose nothing against the same run at unit scale (powers of two that
    keep every fp32 term normal, so the terms scale exactly)"""
    case = SHAPES[0] + ("homography",)
    inp = inputs_of(case)
    base = det_grads(case, inp, inp["grad_d"])["y"]
    for e in (-60, 90):
        g = inp["grad_d"] * np.float32(2.0 ** e)
        assert bits_equal(det_grads(case, inp, g)["y"], base * 2.0 ** e), e


def test_fp16_and_fp32_maps_give_the_same_dy():
    case = SHAPES[3] + ("noise",)  # fp16 maps
    inp = dict(inputs_of(case))
    assert inp["y"].dtype == np.float16
    half = det_grads(case, inp, inp["grad_d"])["y"]
    inp["y"] = inp["y"].astype(np.float32)
    assert bits_equal(det_grads(case, inp, inp["grad_d"])["y"], half)


# ---- autograd -------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def deterministic_flag():
    was, warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True)
    yield
    torch.use_deterministic_algorithms(was, warn_only=warn)


def autograd_dy(case, inp, **kw):
    from gfnet_amd import ops

    r, G = case[6], case[4]
    t = {k: torch.from_numpy(inp[k]).cuda().requires_grad_(True) for k in NAMES}
    d = ops.refiner_input(G, t["x"], t["y"], t["flow"], t["w"], t["b"], r, scale_factor=SF, corr_in_other=r > 0, **kw)
    d.backward(torch.from_numpy(inp["grad_d"]).cuda())
    return t["y"].grad, t["x"].grad


AUTOGRAD_CASES = [SHAPES[0] + ("noise",), SHAPES[2] + ("homography",)]


@pytest.mark.parametrize("case", AUTOGRAD_CASES, ids=case_id)
def test_backward_under_the_torch_flag_is_the_deterministic_dy(case, deterministic_flag):
    inp = inputs_of(case)
    want = det_grads(case, inp, inp["grad_d"])
    dy, dx = autograd_dy(case, inp)
    assert bits_equal(dy, want["y"]) and bits_equal(dx, want["x"])
    dy, _ = autograd_dy(case, inp, deterministic=False)  # the plain scatter on request, flag or not
    assert ratio(dy, cached_reference(case)["y"]) <= 1.0


@pytest.mark.parametrize("case", AUTOGRAD_CASES, ids=case_id)
def test_the_keyword_alone_gives_the_same_without_the_flag(case):
    assert not torch.are_deterministic_algorithms_enabled()
    inp = inputs_of(case)
    want = det_grads(case, inp, inp["grad_d"])["y"]
    dy, _ = autograd_dy(case, inp, deterministic=True)
    assert bits_equal(dy, want)
    dy, _ = autograd_dy(case, inp)  # None without the flag: the plain scatter
    assert ratio(dy, cached_reference(case)["y"]) <= 1.0


def test_the_flag_is_read_when_the_forward_runs(deterministic_flag):
    from gfnet_amd import ops

    case = AUTOGRAD_CASES[0]
    inp = inputs_of(case)
    r, G = case[6], case[4]
    t = {k: torch.from_numpy(inp[k]).cuda().requires_grad_(True) for k in NAMES}
    d = ops.refiner_input(G, t["x"], t["y"], t["flow"], t["w"], t["b"], r, scale_factor=SF, corr_in_other=r > 0)
    torch.use_deterministic_algorithms(False)
    d.backward(torch.from_numpy(inp["grad_d"]).cuda())
    assert bits_equal(t["y"].grad, det_grads(case, inp, inp["grad_d"])["y"])
