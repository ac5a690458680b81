"""The training loss on the GPU: gfnet_amd.losses.RobustLosses / get_gt_warp_homography and the ops under them (csrc/robust_loss.hip)
against the fixture G13 and against the float64 restatement of test_robust_loss_cpu.py, on shapes chosen to break a kernel: grids
narrower than a vector load, tails on both axes, exact multiples, many blocks; 1 to 8 iterations; non-integer grid ratios."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from test_robust_loss_cpu import (ALL_OUTSIDE, CASE_PARAMS, GPU_CASES, IDENTITY, LOCAL_DIST, NEAR_ID, OPS_CASES, PARAMS, SHIFTED, check_ratios,
                                  compare_to_g13, g13_corresps, grad_ratio, make_case, make_ops_case, nearest_exact, restated_gt_warp,
                                  restated_robust_loss, restated_scale, value_ratio)

pytestmark = pytest.mark.gpu


def to_gpu(corresps, requires_grad=True):
    return {s: {k: {n: t.detach().cuda().requires_grad_(requires_grad) for n, t in d.items()} for k, d in per.items()} for s, per in corresps.items()}


def leaves(corresps):
    return [t for per in corresps.values() for d in per.values() for t in (d["flow"], d["certainty"])]


def batch_of(H, S, T):
    return {"H_s2t": H.cuda(), "im_A": torch.zeros(H.shape[0], 3, S, S + 8, device="cuda"), "im_B": torch.zeros(H.shape[0], 3, T, T + 4, device="cuda")}


def run_module(corresps, H, S, T, params, scale=None):
    from gfnet_amd.losses import RobustLosses

    crit = RobustLosses(**params)
    loss = crit(corresps, batch_of(H, S, T))
    (loss if scale is None else loss * scale).backward()
    return loss.detach(), crit.last_losses


def compare_to_restatement(what, corresps_cpu, H, S, T, params):
    """RobustLosses on the GPU against the float64 restatement on the same inputs: loss, logged values and every gradient"""
    ref_c = {s: {k: {n: t.detach().double().requires_grad_() for n, t in d.items()} for k, d in per.items()} for s, per in corresps_cpu.items()}
    ref_loss, ref_logged, _ = restated_robust_loss(ref_c, H, S, T, **params)
    ref_loss.backward()
    got_c = to_gpu(corresps_cpu)
    loss, logged = run_module(got_c, H, S, T, params)
    assert set(logged) == set(ref_logged)
    ratios = {"loss": value_ratio(loss.cpu().numpy(), ref_loss.detach().numpy())}
    for k, v in ref_logged.items():
        assert logged[k].is_cuda and logged[k].dim() == 0
        ratios[k] = value_ratio(logged[k].cpu().numpy(), v.detach().numpy())
    for s, per in got_c.items():
        for k, d in per.items():
            for n in ("flow", "certainty"):
                ratios[f"g{n}.{s}.{k}"] = grad_ratio(d[n].grad.cpu().numpy(), ref_c[s][k][n].grad.numpy(), f"{what} {n} {s}.{k}")
    return check_ratios(ratios, what)


@pytest.mark.parametrize("name", sorted(PARAMS))
def test_g13_on_the_gpu(name):
    g = load_golden("g13_robust_loss")
    S = int(g["image_hw"][0])
    corresps = g13_corresps(g, device="cuda")
    loss, logged = run_module(corresps, torch.from_numpy(g["H_s2t"]), S, S, PARAMS[name])
    compare_to_g13(g, name, loss.cpu(), {k: v.cpu() for k, v in logged.items()}, corresps)


@pytest.mark.parametrize("name", sorted(GPU_CASES))
def test_hostile_shapes_through_the_module(name):
    corresps, H, S, T = make_case(**GPU_CASES[name])
    compare_to_restatement(f"case {name}", corresps, H, S, T, CASE_PARAMS)


@pytest.mark.parametrize("args", OPS_CASES, ids=lambda a: "%dx%dx%d_n%d" % (a[1], a[2][0], a[2][1], a[3]))
@pytest.mark.parametrize("want_epe", [False, True])
def test_hostile_shapes_through_ops(args, want_epe):
    """One scale through ops.robust_loss_scale_fwd / _bwd with im_A_coords and a prev_epe tensor, and ops.gt_warp_homography on the
    same cells, against the float64 restatement."""
    from gfnet_amd import _lib, ops

    cse = make_ops_case(*args)
    (h, w), n = args[2], args[3]
    a, cew, base, scale = 0.5, 0.02, 0.7, cse["scale"]
    flows64 = [f.double().requires_grad_() for f in cse["flows"]]
    certs64 = [c.double().requires_grad_() for c in cse["certs"]]
    x1_n, x2, x2_n, prob = restated_gt_warp(cse["H"].double(), h, w, cse["S"], cse["T"], cse["coords"].double())
    mask = prob * (nearest_exact(cse["prev"].double(), h, w) < cse["thr"]) if cse["prev"] is not None else prob
    ref_loss, ref_ce, ref_reg, ref_pck, ref_epe = restated_scale(flows64, certs64, x2_n, mask, scale, cew, a, 1e-3, base)
    (ref_loss * 3.0).backward()

    flows, certs = [f.cuda() for f in cse["flows"]], [c.cuda() for c in cse["certs"]]
    H, coords = cse["H"].cuda(), cse["coords"].cuda()
    prev = cse["prev"].cuda() if cse["prev"] is not None else None
    common = dict(prev_epe=prev, prev_thresh=cse["thr"], im_A_coords=coords)
    stats, epe = ops.robust_loss_scale_fwd(flows, certs, H, cse["S"] - 1, cse["T"] - 1, a, cse["cs"], cew, base, scale / 448, want_epe=want_epe, **common)
    gf, gc = ops.robust_loss_scale_bwd(torch.tensor(3.0, device="cuda"), stats, flows, certs, H, cse["S"] - 1, cse["T"] - 1, a, cse["cs"], cew, base,
                                       **common)
    st = stats.cpu().numpy()
    ratios = {"loss": value_ratio(st[_lib.RL_STAT_LOSS], ref_loss.item()), "ce": value_ratio(st[_lib.RL_STAT_CE], ref_ce.item()),
              "reg": value_ratio(st[_lib.RL_STAT_REG], ref_reg.item()), "pck": value_ratio(st[_lib.RL_STAT_PCK], ref_pck.item())}
    assert st[_lib.RL_STAT_COUNT] == float(mask.sum()) and 0 < st[_lib.RL_STAT_COUNT] < mask.numel()
    assert (epe is not None) == want_epe
    if want_epe:
        ratios["epe_last"] = value_ratio(epe.cpu().numpy(), ref_epe.numpy())
    for k in range(n):
        ratios[f"gflow.{k + 1}"] = grad_ratio(gf[k].cpu().numpy(), flows64[k].grad.numpy(), f"flow {k + 1}")
        ratios[f"gcert.{k + 1}"] = grad_ratio(gc[k].cpu().numpy(), certs64[k].grad.numpy(), f"certainty {k + 1}")
    # the public warp function on the same cells, normalised with x1_n and in pixels
    g_x2n, g_prob, g_x1n = ops.gt_warp_homography(H, h, w, cse["S"] - 1, cse["T"] - 1, im_A_coords=coords, return_x1_n=True)
    g_x2, g_prob2, none = ops.gt_warp_homography(H.double(), h, w, cse["S"] - 1, cse["T"] - 1, im_A_coords=coords, normalized=False)
    assert none is None and torch.equal(g_prob, g_prob2) and torch.equal(g_prob.cpu().double(), prob)
    assert torch.equal(g_x1n.cpu(), cse["coords"].permute(0, 2, 3, 1))
    ratios["x2_n"], ratios["x2"] = value_ratio(g_x2n.cpu().numpy(), x2_n.numpy()), value_ratio(g_x2.cpu().numpy(), x2.numpy())
    check_ratios(ratios, f"ops {args} epe_last={want_epe}")


def test_public_warp_function_returns_the_reference_tuples():
    from gfnet_amd.losses import get_gt_warp_homography

    H = torch.tensor([NEAR_ID, SHIFTED], dtype=torch.float64)
    src, tgt = torch.zeros(2, 3, 96, 120, device="cuda"), torch.zeros(2, 3, 80, 60, device="cuda")
    x1_ref, x2_ref, x2n_ref, prob_ref = restated_gt_warp(H, 5, 7, 96, 80)
    x2_n, prob = get_gt_warp_homography(H.cuda(), src, tgt, 5, 7)
    x1_n, x2_n_b, prob_b = get_gt_warp_homography(H.float().cuda(), src, tgt, 5, 7, return_x1_n=True)
    x2, prob_c = get_gt_warp_homography(H.float().cuda(), src, tgt, 5, 7, normalized=False, return_x1_n=True)
    assert x2_n.shape == (2, 5, 7, 2) and prob.shape == (2, 5, 7) and x2_n.dtype == torch.float32
    assert torch.equal(x2_n, x2_n_b) and torch.equal(prob, prob_b) and torch.equal(prob, prob_c) and torch.equal(prob.cpu().double(), prob_ref)
    check_ratios({"x1_n": value_ratio(x1_n.cpu().numpy(), x1_ref.numpy()), "x2_n": value_ratio(x2_n.cpu().numpy(), x2n_ref.numpy()),
                  "x2": value_ratio(x2.cpu().numpy(), x2_ref.numpy())}, "get_gt_warp_homography")


def test_empty_mask():
    """H_s2t maps every cell outside: count == 0.  The loss is finite and ce_weight * ce, flow gradients are exactly 0, nothing is NaN."""
    corresps_cpu, H, S, T = make_case(5, 2, [("16", (5, 7), 2), ("8", (10, 14), 1)], [ALL_OUTSIDE, ALL_OUTSIDE])
    corresps = to_gpu(corresps_cpu)
    loss, logged = run_module(corresps, H, S, T, CASE_PARAMS)
    vals = {k: float(v) for k, v in logged.items()}
    assert all(np.isfinite(v) for v in vals.values()) and np.isfinite(float(loss))
    for s in (16, 8):
        assert vals[f"delta_regression_loss_{s}"] == 0.0 and vals[f"train_pck_05_scale_{s}"] == 0.0 and vals[f"delta_certainty_loss_{s}"] > 0
    want = np.float32(0.01) * (np.float32(vals["delta_certainty_loss_16"]) + np.float32(vals["delta_certainty_loss_8"]))
    assert abs(float(loss) - float(want)) <= 1e-6 * abs(float(want))
    for per in corresps.values():
        for d in per.values():
            assert torch.equal(d["flow"].grad, torch.zeros_like(d["flow"]))
            assert torch.isfinite(d["certainty"].grad).all() and d["certainty"].grad.abs().max() > 0
    compare_to_restatement("empty mask", corresps_cpu, H, S, T, CASE_PARAMS)


def test_full_mask_and_zero_error():
    """Identity homography: every cell inside, and x2_n is the cell centre.  Where the flow equals x2_n bit for bit (epe == 0) the
    gradient is exactly 0 -- nothing divides by epe."""
    from gfnet_amd.losses import get_gt_warp_homography

    B, h, w = 2, 8, 12
    H = torch.tensor([IDENTITY, IDENTITY])
    batch = batch_of(H, 96, 96)
    x2_n, prob = get_gt_warp_homography(batch["H_s2t"], batch["im_A"], batch["im_B"], h, w)
    assert bool((prob == 1).all())
    gen = torch.Generator().manual_seed(7)
    exact = torch.rand(B, 1, h, w, generator=gen) < 0.3
    exact[0, 0, 0, 0], exact[0, 0, 0, 1] = True, False
    noise = (torch.rand(B, 2, h, w, generator=gen) - 0.5) * 0.05 + 0.002
    flow = (x2_n.permute(0, 3, 1, 2).cpu() + torch.where(exact, torch.zeros(()), noise)).contiguous()
    corresps_cpu = {"16": {1: {"flow": flow, "certainty": torch.randn(B, 1, h, w, generator=gen)}}}
    corresps = to_gpu(corresps_cpu)
    loss, logged = run_module(corresps, H, 96, 96, CASE_PARAMS)
    g = corresps["16"][1]["flow"].grad.cpu()
    sel = exact.expand(B, 2, h, w)
    assert torch.equal(g[sel], torch.zeros_like(g[sel])) and bool((g[~sel] != 0).all()) and torch.isfinite(g).all()
    compare_to_restatement("full mask", corresps_cpu, H, 96, 96, CASE_PARAMS)


def _fresh_run(case, params, scale=None, frozen=()):
    corresps_cpu, H, S, T = make_case(**GPU_CASES[case])
    corresps = to_gpu(corresps_cpu)
    for i, t in enumerate(leaves(corresps)):
        if i in frozen:
            t.requires_grad_(False)
    loss, _ = run_module(corresps, H, S, T, params, scale)
    return loss, leaves(corresps)


def test_identical_calls_give_identical_bits():
    (l1, t1), (l2, t2) = _fresh_run("many_blocks", CASE_PARAMS), _fresh_run("many_blocks", CASE_PARAMS)
    assert torch.equal(l1, l2)
    for a, b in zip(t1, t2):
        assert torch.equal(a.grad, b.grad)


def test_upstream_gradient_scales_every_gradient():
    """(loss * 1024).backward(): the backward kernel reads grad_output on the device; a power of two scales every gradient exactly."""
    (l1, t1), (l2, t2) = _fresh_run("ragged", CASE_PARAMS), _fresh_run("ragged", CASE_PARAMS, scale=1024.0)
    assert torch.equal(l1, l2)
    for a, b in zip(t1, t2):
        assert a.grad.abs().max() > 0 and torch.equal(a.grad * 1024.0, b.grad)


def test_need_subsets_leave_the_other_gradients_alone():
    """Only some flows and certainties require grad: the others get no .grad, the rest are unchanged bit for bit."""
    _, full = _fresh_run("ragged", CASE_PARAMS)
    frozen = {0, 3, 4, 5, 9, 20, len(full) - 1}      # a flow and a certainty of scale 16, several of scale 8's 8 iterations, the last map
    _, part = _fresh_run("ragged", CASE_PARAMS, frozen=frozen)
    for i, (a, b) in enumerate(zip(full, part)):
        if i in frozen:
            assert b.grad is None
        else:
            assert torch.equal(a.grad, b.grad)
    # nothing requires grad: a plain forward
    corresps_cpu, H, S, T = make_case(**GPU_CASES["tiny"])
    from gfnet_amd.losses import RobustLosses

    out = RobustLosses(**CASE_PARAMS)(to_gpu(corresps_cpu, requires_grad=False), batch_of(H, S, T))
    assert not out.requires_grad and torch.isfinite(out)


def test_forward_and_backward_replay_from_a_captured_graph():
    from gfnet_amd.losses import RobustLosses

    corresps_cpu, H, S, T = make_case(**GPU_CASES["ragged"])
    eager_loss, eager = _fresh_run("ragged", CASE_PARAMS)
    corresps = to_gpu(corresps_cpu)
    batch, crit = batch_of(H, S, T), RobustLosses(**CASE_PARAMS)
    inputs = leaves(corresps)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        loss = crit(corresps, batch)                 # a warm-up on the capture stream: scratch is allocated outside the capture
        torch.autograd.grad(loss, inputs)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        loss = crit(corresps, batch)
        grads = torch.autograd.grad(loss, inputs)
    loss.zero_()
    for gr in grads:
        gr.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(loss, eager_loss)
    for gr, t in zip(grads, eager):
        assert torch.equal(gr, t.grad)
    del graph
    from gfnet_amd import _lib

    _lib.release_retired()


def test_end_to_end_training_step_on_the_g12_model():
    """G12's model -> forward_pyramids -> RobustLosses -> backward: the loss is finite and equals the float64 restatement on the same
    corresps; every refiner parameter and both scale-16 pyramids receive a finite, non-zero gradient."""
    from gfnet_amd.losses import RobustLosses
    from test_train_cpu import g12_pyramids
    from test_train_gpu import g12_model

    g = load_golden("g12_train_grads")
    torch.manual_seed(0)
    model = g12_model(g)
    pyr0, pyr1 = g12_pyramids(g, "cuda")
    hw = tuple(int(v) for v in g["image_hw"])
    corresps = model.forward_pyramids(pyr0, pyr1, hw)
    H = torch.tensor([NEAR_ID, SHIFTED])
    batch = {"H_s2t": H.cuda(), "im_A": torch.zeros(2, 3, *hw, device="cuda"), "im_B": torch.zeros(2, 3, *hw, device="cuda")}
    params = dict(ce_weight=0.01, local_dist=LOCAL_DIST, local_largest_scale=8, alpha=0.5, c=1e-4, iteration_base=1)
    crit = RobustLosses(**params)
    loss = crit(corresps, batch)
    loss.backward()
    assert torch.isfinite(loss)
    for name, p in model.conv_refiner.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0, name
    for pyr in (pyr0, pyr1):
        assert pyr["16"].grad is not None and torch.isfinite(pyr["16"].grad).all() and pyr["16"].grad.abs().max() > 0
    cpu = {s: {k: {n: t.detach().cpu() for n, t in d.items()} for k, d in per.items()} for s, per in corresps.items()}
    ref_loss, ref_logged, aux = restated_robust_loss(cpu, H, hw[0], hw[0], **params)
    ratios = {"loss": value_ratio(loss.detach().cpu().numpy(), ref_loss.numpy())}
    for k, v in ref_logged.items():
        ratios[k] = value_ratio(crit.last_losses[k].cpu().numpy(), v.numpy())
    # (the model's own flows decide how close an upsampled error comes to its threshold; a cell within float32 rounding of it could
    # flip the mask -- report the margin with the figures)
    margin = min(float(((up - thr).abs() / thr).min()) for _, up, thr in aux.values() if up is not None)
    print(f"end to end: smallest relative distance of an upsampled prev_epe to its threshold {margin:.2e}")
    check_ratios(ratios, "end to end")
