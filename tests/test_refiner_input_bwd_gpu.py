"""ops.refiner_input's backward (gfn_refiner_input_bwd, csrc/refiner_input_bwd.hip) against float64 torch autograd of the
reference's refiner-input prefix (model/network.py:537-555: two grid_samples, the displacement embedding, the local correlation with
its window sampled under no_grad, utils/local_correlation.py:54-60), on CPU tensors built from the same seeded inputs.

Bound: 1e-4 * max(1, max|ref|) per gradient tensor, the project's tolerance for correlation and flow tensors.
fp16 maps: the bound holds for what leaves the library (fp32, ops.refiner_input_bwd); autograd then rounds dx / dy to the map's
dtype, which is checked as that rounding.

dflow is discontinuous where a sample sits on a pixel boundary, so the flows are constructed in pixel units with every fractional
position in [0.01, 0.99] and normalised afterwards; the test asserts the property (>= 1e-3 from an integer, in float64, on the fp32
flow the kernels read) and excludes no cell from any comparison."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import oracle
from test_sampling_modes_cpu import restated_local_correlation

pytestmark = pytest.mark.gpu
TOL = 1e-4
SF = 1.25  # scale_factor

# (B, C, Hs, Ws, G, Dd, r, map dtype): G below / equal to / above the map, G = 33 (crosses the forward's 2 x 32 wave shape), ragged
# grids, non-square maps, C in {1, 2, 3, 9, 16, 17}, Dd in {1, 3, 8, 16, 64}, r in {0, 1, 2}, B in {1, 2, 3}; (3, 16, 64, 64, 64, 16, 2)
# is planned inside the refiner-input launch (the lean local-correlation route); two shapes with fp16 maps
SHAPES = [(2, 9, 8, 8, 6, 8, 2, "f32"), (1, 3, 12, 10, 20, 1, 1, "f32"), (3, 16, 64, 64, 64, 16, 2, "f32"),
          (2, 2, 24, 24, 33, 64, 0, "f16"), (2, 17, 7, 9, 5, 3, 0, "f32"), (1, 1, 16, 16, 16, 8, 1, "f16")]
KINDS = ["noise", "homography", "outside"]
CASES = [s + (k,) for s in SHAPES for k in KINDS]
NAMES = ("x", "y", "flow", "w", "b")


def case_id(case):
    B, C, Hs, Ws, G, Dd, r, dt, kind = case
    return f"B{B}C{C}_{Hs}x{Ws}_G{G}_D{Dd}_r{r}_{dt}_{kind}"


def snap(p):
    """pixel positions with the fractional part moved into [0.01, 0.99]"""
    fl = np.floor(p)
    return fl + np.clip(p - fl, 0.01, 0.99)


def make_flow(kind, B, G, Hs, Ws, seed):
    """(flow (B,2,G,G) fp32, insane (B,G,G) bool, far (B,G,G) bool).  Built in pixel units (x = column, y = row), then normalised
    as grid_sample(align_corners=False) un-normalises: g = (2 p + 1) / size - 1."""
    rng = np.random.default_rng(seed)
    cx = ((np.arange(G) + 0.5) * Ws / G - 0.5)[None, None, :]
    cy = ((np.arange(G) + 0.5) * Hs / G - 0.5)[None, :, None]
    insane = np.zeros((B, G, G), bool)
    far = np.zeros((B, G, G), bool)
    if kind == "homography":
        lin = (np.arange(G) + 0.5) * 2 / G - 1
        gy, gx = np.meshgrid(lin, lin, indexing="ij")
        px, py = np.empty((B, G, G)), np.empty((B, G, G))
        for b in range(B):
            H = np.eye(3) + rng.uniform(-0.12, 0.12, (3, 3)) * np.array([[1, 1, 1], [1, 1, 1], [0.5, 0.5, 0]])
            den = H[2, 0] * gx + H[2, 1] * gy + 1
            u, v = (H[0, 0] * gx + H[0, 1] * gy + H[0, 2]) / den, (H[1, 0] * gx + H[1, 1] * gy + H[1, 2]) / den
            px[b], py[b] = (u + 1) * Ws / 2 - 0.5, (v + 1) * Hs / 2 - 0.5
    else:  # identity plus small noise
        px = cx + rng.normal(0, 0.6, (B, G, G))
        py = cy + rng.normal(0, 0.6, (B, G, G))
    sign = None
    if kind == "outside":  # a quarter of the cells pushed outside [-1, 1]
        n = B * G * G
        idx = rng.permutation(n)[:max(n // 4, 6)]
        groups = np.array_split(idx[4:], 4)
        fx, fy = px.reshape(-1), py.reshape(-1)
        fx[groups[0]] = rng.uniform(-0.9, -0.1, len(groups[0]))            # just over the left border: two corners in, two out
        fy[groups[1]] = Hs - 1 + rng.uniform(0.1, 0.9, len(groups[1]))     # just over the bottom border
        s2 = rng.choice([-1.0, 1.0], len(groups[2]))
        fx[groups[2]] = ((s2 * 3 + 1) * Ws - 1) / 2                        # +-3 in normalised units
        s3 = rng.choice([-1.0, 1.0], len(groups[3]))
        fy[groups[3]] = ((s3 * 3 + 1) * Hs - 1) / 2
        far.reshape(-1)[np.concatenate((groups[2], groups[3]))] = True
        insane.reshape(-1)[idx[:4]] = True                                 # a few cells at +-1e9
        sign = rng.choice([-1.0, 1.0], (4, 2))
    px, py = snap(px), snap(py)
    flow = np.stack(((2 * px + 1) / Ws - 1, (2 * py + 1) / Hs - 1), 1).astype(np.float32)
    if sign is not None:
        fl = flow.transpose(0, 2, 3, 1).reshape(-1, 2)
        fl[idx[:4]] = (sign * 1e9).astype(np.float32)
        flow = np.ascontiguousarray(fl.reshape(B, G, G, 2).transpose(0, 3, 1, 2))
    return flow, insane, far


def assert_off_pixel_boundaries(flow, Hs, Ws):
    """every sample that can touch the image sits >= 1e-3 pixels from an integer position, in float64, on the fp32 flow"""
    ix = ((flow[:, 0].astype(np.float64) + 1) * Ws - 1) / 2
    iy = ((flow[:, 1].astype(np.float64) + 1) * Hs - 1) / 2
    near = (ix > -1) & (ix < Ws) & (iy > -1) & (iy < Hs)
    assert near.any()
    for p in (ix[near], iy[near]):
        assert np.abs(p - np.round(p)).min() >= 1e-3


@functools.lru_cache(maxsize=None)
def inputs_of(case):
    B, C, Hs, Ws, G, Dd, r, dt, kind = case
    seed = 100 * SHAPES.index(case[:8]) + KINDS.index(kind)
    rng = np.random.default_rng(seed)
    ft = np.float16 if dt == "f16" else np.float32
    K = (2 * r + 1) ** 2 if r > 0 else 0
    flow, insane, far = make_flow(kind, B, G, Hs, Ws, seed + 50)
    assert_off_pixel_boundaries(flow, Hs, Ws)
    return dict(x=rng.normal(0, 1, (B, C, Hs, Ws)).astype(ft), y=rng.normal(0, 1, (B, C, Hs, Ws)).astype(ft), flow=flow,
                w=rng.uniform(-1, 1, (Dd, 2, 1, 1)).astype(np.float32), b=rng.uniform(-1, 1, (Dd,)).astype(np.float32),
                grad_d=rng.normal(0, 1, (B, 2 * C + Dd + K, G, G)).astype(np.float32), insane=insane, far=far)


def reference_grads(case, inp, grad_d):
    """float64 autograd of the restated prefix on the CPU: {name: float64 tensor}"""
    B, C, Hs, Ws, G, Dd, r = case[:7]
    t = {k: torch.from_numpy(inp[k].astype(np.float64)).requires_grad_(True) for k in NAMES}
    lin = torch.from_numpy(oracle.cell_centres(G)).double()  # the reference's fp32 linspace values
    gy, gx = torch.meshgrid(lin, lin, indexing="ij")
    coords = torch.stack((gx, gy))[None].expand(B, 2, G, G)
    x_hat = F.grid_sample(t["y"], t["flow"].permute(0, 2, 3, 1), mode="bilinear", padding_mode="zeros", align_corners=False)
    gf = F.grid_sample(t["x"], coords.permute(0, 2, 3, 1), mode="bilinear", padding_mode="zeros", align_corners=False)
    emb = (t["w"].reshape(Dd, 2) @ (40 / 32 * SF * (t["flow"] - coords)).reshape(B, 2, G * G)).reshape(B, Dd, G, G) + \
        t["b"][None, :, None, None]
    parts = [gf, x_hat, emb]
    if r > 0:  # window_feature under no_grad: feature1 and the flow detached
        parts.append(restated_local_correlation(gf, t["y"].detach(), r, G, flow=t["flow"].detach()))
    torch.cat(parts, 1).backward(torch.from_numpy(grad_d.astype(np.float64)))
    return {k: t[k].grad for k in NAMES}


@functools.lru_cache(maxsize=None)
def cached_reference(case):
    inp = inputs_of(case)
    return reference_grads(case, inp, inp["grad_d"])


def run_op(case, inp, grad_d, need=NAMES, no_grad=False):
    """d and {name: gradient} of ops.refiner_input with the inputs in `need` requiring grad"""
    from gfnet_amd import ops

    r, G = case[6], case[4]
    t = {k: torch.from_numpy(inp[k]).cuda().requires_grad_(k in need) for k in NAMES}
    with torch.set_grad_enabled(not no_grad):
        d = ops.refiner_input(G, t["x"], t["y"], t["flow"], t["w"], t["b"], r, scale_factor=SF, corr_in_other=r > 0)
    if no_grad:
        return d, {}
    d.backward(torch.from_numpy(grad_d).cuda())
    return d, {k: t[k].grad for k in need}


def library_grads(case, inp, grad_d, need=(True,) * 5):
    """the five fp32 gradients as they leave the library"""
    from gfnet_amd import ops

    r = case[6]
    c = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    out = ops.refiner_input_bwd(c(grad_d), c(inp["y"]), c(inp["flow"]), c(inp["w"]), r, SF, r > 0, need=need)
    grads = dict(zip(NAMES, out))
    if grads["w"] is not None:
        grads["w"] = grads["w"].reshape(-1, 2, 1, 1)  # disp_emb.weight's layout
    return grads


def ratio(got, ref):
    """max |got - ref| / (TOL * max(1, max|ref|)): within the bound when <= 1"""
    ref = ref.double()
    return float((got.double().cpu() - ref).abs().max() / (TOL * max(1.0, float(ref.abs().max()))))


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_forward_is_the_inference_launch_and_carries_a_graph(case):
    inp = inputs_of(case)
    d, _ = run_op(case, inp, inp["grad_d"])
    d0, _ = run_op(case, inp, inp["grad_d"], no_grad=True)
    assert d.grad_fn is not None and d0.grad_fn is None
    assert torch.equal(d.detach(), d0)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_all_five_gradients_match_float64_autograd(case):
    inp = inputs_of(case)
    ref = cached_reference(case)
    _, got = run_op(case, inp, inp["grad_d"])
    lib = library_grads(case, inp, inp["grad_d"])
    worst = {}
    for k in NAMES:
        assert got[k].dtype == torch.from_numpy(inp[k]).dtype and got[k].shape == ref[k].shape
        worst[k] = ratio(lib[k], ref[k])
    print(f"{case_id(case)}: worst err / bound " + ", ".join(f"d{k} {v:.3f}" for k, v in worst.items()))
    for k in NAMES:
        assert torch.isfinite(lib[k]).all()
        assert worst[k] <= 1.0, (k, worst[k])
        if got[k].dtype == torch.float32:  # autograd hands the library's tensor on
            assert ratio(got[k], ref[k]) <= 1.0, k
        else:  # fp16 maps: the library's fp32 gradient rounded once to the map's dtype
            scale = max(1.0, float(ref[k].abs().max()))
            err = (got[k].double().cpu() - ref[k]).abs()
            assert bool((err <= TOL * scale + 2.0 ** -11 * ref[k].abs()).all()), k
    assert torch.equal(got["x"], lib["x"].to(got["x"].dtype))  # dx is reproducible, so autograd's is the library's, cast


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_each_gradient_alone_equals_the_joint_run_and_runs_repeat(case):
    """one input requiring grad at a time (the C ABI then gets NULL for the other outputs): same values; a second joint run gives the
    same bits except for dy, whose atomic adds may arrive in another order (compared to the reference only)"""
    inp = inputs_of(case)
    ref = cached_reference(case)
    joint = library_grads(case, inp, inp["grad_d"])
    again = library_grads(case, inp, inp["grad_d"])
    for k in ("x", "flow", "w", "b"):
        assert torch.equal(joint[k], again[k]), k
    assert ratio(again["y"], ref["y"]) <= 1.0
    for n, k in enumerate(NAMES):
        alone = library_grads(case, inp, inp["grad_d"], need=tuple(m == n for m in range(5)))
        assert all(alone[o] is None for o in NAMES if o != k)
        _, auto = run_op(case, inp, inp["grad_d"], need=(k,))
        if k == "y":
            assert ratio(alone[k], ref[k]) <= 1.0
        else:
            assert torch.equal(alone[k], joint[k]), k
            assert torch.equal(auto[k], joint[k].to(auto[k].dtype)), k


def test_a_sample_does_not_depend_on_the_others():
    case = SHAPES[2] + ("homography",)  # B = 3
    inp = dict(inputs_of(case))
    base = library_grads(case, inp, inp["grad_d"])
    other = dict(inp)
    rng = np.random.default_rng(5)
    for k in ("x", "y", "flow", "grad_d"):
        a = inp[k].copy()
        a[1] = (a[1] + rng.normal(0, 0.01 if k == "flow" else 1, a[1].shape)).astype(a.dtype)
        other[k] = a
    moved = library_grads(case, other, other["grad_d"])
    for b in (0, 2):
        assert torch.equal(base["x"][b], moved["x"][b]) and torch.equal(base["flow"][b], moved["flow"][b])
        # dy: only the arrival order of this sample's own adds can differ -- a few fp32 roundings of sums of a handful of terms
        assert float((base["y"][b] - moved["y"][b]).abs().max()) <= 1e-5 * float(base["y"][b].abs().max())
    assert not torch.equal(base["x"][1], moved["x"][1])


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[3]], ids=lambda s: case_id(s + ("outside",)))
def test_insane_and_far_outside_cells(shape):
    """cells at +-1e9 (insane) and at +-3: nothing reaches dy from them, and their dflow is the embedding term exactly"""
    case = shape + ("outside",)
    inp = inputs_of(case)
    B, C, Hs, Ws, G, Dd = case[:6]
    off = torch.from_numpy(inp["insane"] | inp["far"])
    assert inp["insane"].sum() == 4 and inp["far"].sum() > 0
    g = torch.from_numpy(inp["grad_d"])
    only_off = torch.zeros_like(g)
    only_off[:, C:2 * C] = g[:, C:2 * C] * off[:, None]  # x_hat's gradient, on those cells alone
    dy = library_grads(case, inp, only_off.numpy())["y"]
    assert torch.equal(dy, torch.zeros_like(dy))
    no_xhat = g.clone()
    no_xhat[:, C:2 * C] = 0
    full = library_grads(case, inp, inp["grad_d"])["flow"].cpu()
    emb_only = library_grads(case, inp, no_xhat.numpy())["flow"].cpu()
    sel = off[:, None].expand(B, 2, G, G)
    assert torch.equal(full[sel], emb_only[sel])
    assert not torch.equal(full[~sel], emb_only[~sel])
    assert float(emb_only[sel].abs().max()) > 0


@pytest.mark.parametrize("case", [SHAPES[0] + ("noise",), SHAPES[2] + ("homography",), SHAPES[5] + ("outside",)], ids=case_id)
def test_dx_includes_the_local_correlations_feature0_gradient(case):
    """grad_d non-zero on the correlation slice only: dx is then the correlation's feature0 gradient carried through the
    grid_feature gather -- dropping gf0 would leave an exact zero"""
    inp = inputs_of(case)
    C, Dd = case[1], case[5]
    g = np.zeros_like(inp["grad_d"])
    g[:, 2 * C + Dd:] = inp["grad_d"][:, 2 * C + Dd:]
    ref = reference_grads(case, inp, g)
    assert float(ref["x"].abs().max()) > 1e-2
    got = library_grads(case, inp, g)
    assert ratio(got["x"], ref["x"]) <= 1.0
    for k in ("y", "flow", "w", "b"):  # the window is sampled under no_grad
        assert float(ref[k].abs().max()) == 0 and float(got[k].abs().max()) == 0, k


def test_flow_only_gradient_through_a_frozen_refiner():
    """frozen refiner parameters, pyramids without grad, a flow that requires grad: ConvRefiner.assemble in train() keeps the flow's
    gradient (through x_hat and the displacement embedding)"""
    from gfnet_amd.model.network import ConvRefiner

    C, Dd, r, G, hs = 8, 6, 2, 12, 16
    dim = 2 * C + Dd + (2 * r + 1) ** 2
    ref = ConvRefiner(dim, dim, 3, kernel_size=5, dw=True, hidden_blocks=1, displacement_emb="linear", displacement_emb_dim=Dd,
                      local_corr_num=r, corr_in_other=True, amp=True, bn_momentum=0.01).cuda().train()
    for p in ref.parameters():
        p.requires_grad_(False)
    gen = torch.Generator().manual_seed(3)
    x, y = torch.randn(2, C, hs, hs, generator=gen).cuda(), torch.randn(2, C, hs, hs, generator=gen).cuda()
    flow = torch.from_numpy(make_flow("noise", 2, G, hs, hs, 9)[0]).cuda().requires_grad_(True)
    d, lc = ref.assemble(G, x, y, flow, scale_factor=SF)
    assert d.grad_fn is not None and lc.shape == (2, (2 * r + 1) ** 2, G, G)
    d.square().sum().backward()
    assert flow.grad is not None and float(flow.grad.abs().max()) > 0
    out = ref(G, x, y, flow.detach().requires_grad_(True), scale_factor=SF)  # and through the whole refiner
    assert out[0].grad_fn is not None
