"""The training loss (gfnet_amd.losses, csrc/robust_loss.hip) without a GPU: a plain-torch float64 restatement of the reference's
losses/robust_loss.py against the fixture G13 (tests/golden/make_golden_loss.py), the conditions the test inputs are chosen to
satisfy, the host-side refusals of the three entry points and the public interface's argument checks.  The GPU tests
(test_robust_loss_gpu.py) take the restatement and the input cases from here."""
import ctypes
import inspect
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, assert_close, load_golden

SCALES = ("16", "8", "4", "2", "1")
LOCAL_DIST = {1: 4, 2: 4, 4: 8, 8: 8}
# the two parameter sets of G13: the one train.py:98-106 constructs, and the constructor defaults with alpha per scale
PARAMS = {
    "train": dict(ce_weight=0.01, local_dist=LOCAL_DIST, local_largest_scale=8, alpha=0.5, c=1e-4, iteration_base=1),
    "default": dict(ce_weight=0.01, local_dist=LOCAL_DIST, local_largest_scale=8, alpha={16: 0.5, 8: 0.65, 4: 0.8, 2: 1.0, 1: 1.5}, c=1e-3,
                    iteration_base=0.85),
}
VALUE_TOL, GRAD_TOL = 1e-4, 1e-3   # values: 1e-4 * max(1, |ref|); gradients: 1e-3 of the tensor's largest entry
# A float32 x2_n on a 96-pixel image is up to about 5e-7 off (pixel coordinates near 100 have an ulp of 7.6e-6, carried through the
# matrix product, the division and the normalisation).  A flow closer to the ground truth than cs passes that offset into its
# gradient at full weight while, with alpha < 1, the tensor's largest gradient entry is about 0.6 * cs; at larger errors d the ratio
# falls like offset / (2 d).  With no flow closer than NOISE_FLOOR a float32 run stays near 0.2 of the gradient tolerance whatever cs
# is; the fixture generator (golden/make_golden_loss.py) keeps the same floor for the same reason.
NOISE_FLOOR = 1.2e-3


# ---- the reference's loss restated in plain torch -----------------------------------------------------------------------------------
def restated_gt_warp(H, h, w, S, T, coords=None):
    """robust_loss.py:9-42 in H's dtype: returns (x1_n, x2, x2_n, prob), (B,h,w,2) each and prob (B,h,w).  The image heights S and T
    scale both axes."""
    B, dt = H.shape[0], H.dtype
    if coords is None:
        cx = torch.linspace(-1 + 1 / w, 1 - 1 / w, w, dtype=dt, device=H.device)[None, None, :].expand(B, h, w)
        cy = torch.linspace(-1 + 1 / h, 1 - 1 / h, h, dtype=dt, device=H.device)[None, :, None].expand(B, h, w)
    else:
        cx, cy = coords[:, 0].to(dt), coords[:, 1].to(dt)
    ax, ay = (cx + 1) * (S - 1) * 0.5, (cy + 1) * (S - 1) * 0.5
    m = H[:, :, :, None, None]
    X, Y, Z = (m[:, r, 0] * ax + m[:, r, 1] * ay + m[:, r, 2] for r in range(3))
    zd = torch.where(Z.abs() > 1e-8, Z, torch.ones_like(Z))
    x2 = torch.stack((X / zd, Y / zd), dim=-1)
    x2_n = x2 / (T - 1) * 2 - 1
    prob = ((x2_n < 1) & (x2_n > -1)).all(dim=-1).to(dt)
    return torch.stack((cx, cy), dim=-1), x2, x2_n, prob


def nearest_exact(prev, h, w):
    """F.interpolate(prev[:, None], (h, w), mode="nearest-exact")[:, 0]: source index min(floor((i + 0.5) * in / out), in - 1)"""
    ph, pw = prev.shape[-2:]
    iy = torch.clamp((2 * torch.arange(h, device=prev.device) + 1) * ph // (2 * h), max=ph - 1)
    ix = torch.clamp((2 * torch.arange(w, device=prev.device) + 1) * pw // (2 * w), max=pw - 1)
    return prev[:, iy][:, :, ix]


def restated_scale(flows, certs, x2_n, prob, scale, ce_weight, a, c, iteration_base):
    """regression_loss, :65-90, for one scale: returns (loss, ce, reg, pck_05, last epe).  No boolean indexing: the empty mask is
    the explicit branch of :83-84, written as a torch.where on the count."""
    n, cs = len(flows), c * scale
    ce = reg_sum = 0.0
    count = prob.sum()
    for k, (flow, cert) in enumerate(zip(flows, certs), start=1):
        wk = iteration_base ** (n - k)
        epe = (flow.permute(0, 2, 3, 1) - x2_n).norm(dim=-1)
        z = cert[:, 0]
        ce = ce + wk * (z.clamp(min=0) - z * prob + torch.log1p(torch.exp(-z.abs()))).mean()
        reg_sum = reg_sum + wk * (prob * (cs ** a * ((epe / cs) ** 2 + 1) ** (a / 2))).sum()
    zero = torch.zeros_like(count)
    some = count > 0
    reg = torch.where(some, reg_sum / count.clamp(min=1), zero)
    pck = torch.where(some, (prob * (epe < scale / 448)).sum() / count.clamp(min=1), zero)
    return ce_weight * ce + reg, ce, reg, pck, epe.detach()


def restated_robust_loss(corresps, H_s2t, S, T, ce_weight=0.01, local_dist=None, local_largest_scale=8, alpha=1., c=1e-3, iteration_base=0.85,
                         dtype=torch.float64):
    """RobustLosses.forward, :92-128, in `dtype`.  Returns (loss, logged, aux): logged has the reference's wandb keys, aux per scale
    key the x2_n, the upsampled previous end-point error and its threshold (None where the scale is not narrowed)."""
    H = H_s2t.to(dtype)
    total, logged, aux, prev = 0.0, {}, {}, None
    for key, per_itr in corresps.items():
        scale, mode = (16, "gm") if key == "gm" else (int(key), "delta")
        flows = [per_itr[k]["flow"].to(dtype) for k in sorted(per_itr)]
        certs = [per_itr[k]["certainty"].to(dtype) for k in sorted(per_itr)]
        h, w = flows[0].shape[-2:]
        _, _, x2_n, prob = restated_gt_warp(H, h, w, S, T)
        up = thr = None
        if key != "gm" and local_largest_scale >= scale:
            up, thr = nearest_exact(prev, h, w), (2 / 448) * (local_dist[scale] * scale)
            prob = prob * (up < thr)
        a = alpha[scale] if isinstance(alpha, dict) else alpha
        loss, ce, reg, pck, prev = restated_scale(flows, certs, x2_n, prob, scale, ce_weight, a, c, iteration_base)
        total = total + loss
        logged[f"{mode}_certainty_loss_{scale}"], logged[f"{mode}_regression_loss_{scale}"], logged[f"train_pck_05_scale_{scale}"] = ce, reg, pck
        aux[key] = (x2_n.detach(), up, thr)
    return total, logged, aux


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
MILD_H = [[1.111, 0.07, 15.01], [-0.06, 1.087, -11.49], [7e-4, -4e-4, 1.0]]
NEAR_ID = [[1.001, 0.006, -0.19], [-0.004, 0.997, 0.29], [2e-5, 3e-5, 1.0]]
SHIFTED = [[0.967, -0.02, 4.19], [0.03, 1.019, -2.88], [-1e-4, 2e-4, 1.0]]
ALL_OUTSIDE = [[1.0, 0.0, 400.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]   # every cell lands right of the target image
IDENTITY = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]


def g13_corresps(g, device="cpu", requires_grad=True):
    grids, nitr = [int(v) for v in g["grids"]], [int(v) for v in g["num_itr"]]
    assert len(grids) == len(SCALES)
    out = {}
    for s, n in zip(SCALES, nitr):
        out[s] = {k: {"flow": torch.from_numpy(g[f"flow.{s}.{k}"]).to(device).requires_grad_(requires_grad),
                      "certainty": torch.from_numpy(g[f"cert.{s}.{k}"]).to(device).requires_grad_(requires_grad)} for k in range(1, n + 1)}
    return out


def make_case(seed, B, layout, Hs, S=96, T=96, c=1e-3, h64=False):
    """Random inputs like G13's for the GPU tests, built on the CPU in float32: layout is a list of (scale key, (h, w), iterations) in
    order, Hs a list of B 3x3 matrices.  A flow is the float64 ground-truth warp plus noise of log-uniform magnitude from 0.1 * cs (at
    least NOISE_FLOOR) to the larger of 100 * cs and three times the next scale's threshold.  Returns (corresps, H_s2t, S, T)."""
    gen = torch.Generator().manual_seed(seed)
    H = torch.tensor(Hs, dtype=torch.float64)
    assert H.shape == (B, 3, 3)
    corresps = {}
    for i, (key, (h, w), n) in enumerate(layout):
        scale = int(key)
        _, _, x2_n, _ = restated_gt_warp(H, h, w, S, T)
        nxt = int(layout[i + 1][0]) if i + 1 < len(layout) else None
        lo, hi = max(0.1 * c * scale, NOISE_FLOOR), max(100 * c * scale, 3 * (2 / 448) * LOCAL_DIST[nxt] * nxt if nxt else 0.0)
        corresps[key] = {}
        for k in range(1, n + 1):
            mag = torch.exp(torch.rand(B, h, w, generator=gen, dtype=torch.float64) * math.log(hi / lo) + math.log(lo))
            ang = torch.rand(B, h, w, generator=gen, dtype=torch.float64) * (2 * math.pi)
            flow = x2_n.permute(0, 3, 1, 2) + torch.stack((mag * torch.cos(ang), mag * torch.sin(ang)), dim=1)
            corresps[key][k] = {"flow": flow.float().contiguous(), "certainty": 2 * torch.randn(B, 1, h, w, generator=gen)}
    return corresps, (H if h64 else H.float()), S, T


# name -> make_case arguments.  Grids: 1x1, 5x7 (odd, narrower than any vector load), 37x41 (tails on both axes), 64x64 (exact
# multiples), 2 x 96 x 96 cells (many partials for the second stage), 10x14 (8-byte vectors); B in {1, 3} and the 2 of the 96x96 case;
# 1, 2, 3 and 8 iterations; previous grid to grid 6 -> 10, 8 -> 16, equal and others; one H_s2t in float64.
GPU_CASES = {
    "tiny": dict(seed=1, B=1, layout=[("16", (1, 1), 1), ("8", (5, 7), 2), ("4", (5, 7), 3)], Hs=[NEAR_ID]),
    "ragged": dict(seed=2, B=3, layout=[("16", (6, 6), 2), ("8", (10, 10), 8), ("4", (37, 41), 1), ("2", (64, 64), 2), ("1", (10, 14), 1)],
                   Hs=[MILD_H, NEAR_ID, SHIFTED]),
    "doubling": dict(seed=3, B=1, layout=[("16", (8, 8), 1), ("8", (16, 16), 3), ("4", (64, 64), 2)], Hs=[MILD_H], h64=True),
    "many_blocks": dict(seed=4, B=2, layout=[("16", (96, 96), 2), ("8", (96, 96), 1)], Hs=[MILD_H, SHIFTED]),
}
CASE_PARAMS = dict(ce_weight=0.01, local_dist=LOCAL_DIST, local_largest_scale=8, alpha={16: 0.5, 8: 0.65, 4: 0.8, 2: 1.0, 1: 1.5}, c=1e-3,
                   iteration_base=0.85)
# the cases that call ops on one scale directly: (seed, B, (h, w), iterations, previous grid or None)
OPS_CASES = [(11, 1, (5, 7), 2, None), (62, 3, (37, 41), 3, (6, 6)), (203, 1, (64, 64), 8, (64, 64)), (14, 3, (10, 14), 1, (10, 6))]


def make_ops_case(seed, B, hw, n, prev_hw, S=96, T=80, c=1e-3, scale=4):
    """One scale with im_A_coords (the regular centres, jittered) and a previous end-point error given as a tensor."""
    gen = torch.Generator().manual_seed(seed)
    h, w = hw
    H = torch.tensor(([MILD_H, NEAR_ID, SHIFTED] * B)[:B], dtype=torch.float64)
    x1_n = restated_gt_warp(H, h, w, S, T)[0]
    coords = (x1_n.permute(0, 3, 1, 2) + (torch.rand(B, 2, h, w, generator=gen, dtype=torch.float64) - 0.5) * (0.5 / max(h, w))).float().contiguous()
    x2_n = restated_gt_warp(H, h, w, S, T, coords.double())[2]
    cs, thr = c * scale, (2 / 448) * (LOCAL_DIST[scale] * scale)
    flows, certs = [], []
    for _ in range(n):
        mag = torch.exp(torch.rand(B, h, w, generator=gen, dtype=torch.float64) * math.log(1000) + math.log(0.1 * cs))
        ang = torch.rand(B, h, w, generator=gen, dtype=torch.float64) * (2 * math.pi)
        flows.append((x2_n.permute(0, 3, 1, 2) + torch.stack((mag * torch.cos(ang), mag * torch.sin(ang)), dim=1)).float().contiguous())
        certs.append(2 * torch.randn(B, 1, h, w, generator=gen))
    prev = None
    if prev_hw is not None:
        prev = torch.exp(torch.rand(B, *prev_hw, generator=gen) * math.log(100) + math.log(0.1 * thr))
    return dict(flows=flows, certs=certs, H=H.float(), coords=coords, prev=prev, thr=thr, S=S, T=T, scale=scale, cs=cs)


def check_input_conditions(x2_n, up, thr, what):
    """No cell within 1e-4 of the border of (-1, 1) on either axis, no upsampled prev_epe within 1e-4 relative of its threshold: a
    float32 run then draws the same mask as the float64 restatement.  The inputs are chosen so; nothing is ever excluded."""
    assert x2_n.dtype == torch.float64
    edge = float((x2_n.abs() - 1).abs().min())
    assert edge > 1e-4, f"{what}: a cell's x2_n lies {edge:.2e} from the border"
    if up is not None:
        rel = float(((up.double() - thr).abs() / thr).min())
        assert rel > 1e-4, f"{what}: an upsampled prev_epe lies {rel:.2e} (relative) from its threshold"


def test_inputs_keep_clear_of_the_mask_borders():
    g = load_golden("g13_robust_loss")
    S = int(g["image_hw"][0])
    for name, kw in PARAMS.items():
        _, _, aux = restated_robust_loss(g13_corresps(g, requires_grad=False), torch.from_numpy(g["H_s2t"]), S, S, **kw)
        for key, (x2_n, up, thr) in aux.items():
            check_input_conditions(x2_n, up, thr, f"G13 {name} scale {key}")
    # the mild warp sends roughly a third of the cells outside, the near-identity none
    assert 0.2 < float(g["outside_fraction"][0]) < 0.45 and float(g["outside_fraction"][1]) == 0.0
    for name, kw in GPU_CASES.items():
        corresps, H, S, T = make_case(**kw)
        _, _, aux = restated_robust_loss(corresps, H, S, T, **CASE_PARAMS)
        for key, (x2_n, up, thr) in aux.items():
            check_input_conditions(x2_n, up, thr, f"case {name} scale {key}")
    for args in OPS_CASES:
        cse = make_ops_case(*args)
        x2_n = restated_gt_warp(cse["H"].double(), *args[2], cse["S"], cse["T"], cse["coords"].double())[2]
        up = nearest_exact(cse["prev"], *args[2]) if cse["prev"] is not None else None
        check_input_conditions(x2_n, up, cse["thr"], f"ops case {args}")
    # the public function's test: a 5 x 7 grid, 96 -> 80 pixels
    check_input_conditions(restated_gt_warp(torch.tensor([NEAR_ID, SHIFTED], dtype=torch.float64), 5, 7, 96, 80)[2], None, None, "public warp")
    # the end-to-end test's homographies on the G12 grids
    for g_side in (6, 10, 14, 20):
        check_input_conditions(restated_gt_warp(torch.tensor([NEAR_ID, SHIFTED], dtype=torch.float64), g_side, g_side, 80, 80)[2], None, None,
                               f"end to end, grid {g_side}")


# ---- the restatement against the fixture ----------------------------------------------------------------------------------------------
def grad_ratio(got, ref, what):
    """max |got - ref| as a fraction of the tolerance, GRAD_TOL of the reference tensor's largest entry"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, what
    assert np.isfinite(got).all(), f"{what}: non-finite gradient"
    tol = GRAD_TOL * np.abs(ref).max()
    err = np.abs(got - ref).max()
    return (err / tol) if tol > 0 else (0.0 if err == 0 else float("inf"))


def value_ratio(got, ref):
    """|got - ref| as a fraction of the tolerance, VALUE_TOL * max(1, |ref|) (conftest.assert_close's measure)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all()
    return float((np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max() / VALUE_TOL) if got.size else 0.0


def check_ratios(ratios, what, limit=1.0):
    """Print the worst figures, then hold every one of them to `limit` times its tolerance."""
    worst = sorted(ratios.items(), key=lambda kv: -kv[1])[:4]
    print(f"{what}: worst err / tol " + ", ".join(f"{k} {v:.3f}" for k, v in worst))
    bad = {k: round(v, 3) for k, v in ratios.items() if not v <= limit}
    assert not bad, f"{what}: err / tol above {limit}: {bad}"
    return worst[0][1]


def compare_to_g13(g, name, loss, logged, corresps, limit=1.0):
    """loss, every logged component and every gradient against the fixture's parameter set `name`, each within `limit` times its
    tolerance; returns the worst err / tol."""
    ratios = {"loss": value_ratio(float(loss), g[f"{name}.loss"])}
    assert_close(float(loss), g[f"{name}.loss"], VALUE_TOL, f"{name} loss")
    keys = [k for k in g.files if k.startswith(f"{name}.log.")]
    assert len(keys) == 3 * len(SCALES) and {k.split(".")[-1] for k in keys} == set(logged)
    for k in keys:
        ratios[k.split(".")[-1]] = value_ratio(float(logged[k.split(".")[-1]].detach()), g[k])
    for s, per_itr in corresps.items():
        for k, d in per_itr.items():
            for kind, t in (("gflow", d["flow"]), ("gcert", d["certainty"])):
                ref = g[f"{name}.{kind}.{s}.{k}"]
                assert np.abs(ref).max() > 0
                ratios[f"{kind}.{s}.{k}"] = grad_ratio(t.grad.cpu().numpy(), ref, f"{name}.{kind}.{s}.{k}")
    return check_ratios(ratios, f"G13 {name}", limit)


@pytest.mark.parametrize("name", sorted(PARAMS))
def test_float64_restatement_matches_the_reference(name):
    """The reference ran in float32; the restatement here runs in float64 on the same inputs.  The fixture's inputs are chosen so that
    the two agree within HALF of the standing tolerances, which leaves the other half to a float32 device run."""
    g = load_golden("g13_robust_loss")
    S = int(g["image_hw"][0])
    corresps = g13_corresps(g)
    loss, logged, _ = restated_robust_loss(corresps, torch.from_numpy(g["H_s2t"]), S, S, **PARAMS[name])
    loss.backward()
    compare_to_g13(g, name, loss.detach(), logged, corresps, limit=0.5)


def test_fixture_is_small():
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "g13_robust_loss.npz")) < 100 * 1024


def test_restatement_handles_an_empty_mask():
    """count == 0: the regression term and pck_05 are exactly 0, the loss is ce_weight * ce and no flow receives a gradient"""
    corresps, H, S, T = make_case(5, 2, [("16", (5, 7), 2)], [ALL_OUTSIDE, ALL_OUTSIDE])
    for d in corresps["16"].values():
        d["flow"].requires_grad_(), d["certainty"].requires_grad_()
    loss, logged, _ = restated_robust_loss(corresps, H, S, T, **CASE_PARAMS)
    loss.backward()
    assert float(logged["delta_regression_loss_16"]) == 0.0 and float(logged["train_pck_05_scale_16"]) == 0.0
    assert float(loss) == pytest.approx(0.01 * float(logged["delta_certainty_loss_16"]), rel=1e-12) and math.isfinite(float(loss))
    for d in corresps["16"].values():
        assert torch.equal(d["flow"].grad, torch.zeros_like(d["flow"])) and d["certainty"].grad.abs().max() > 0


# ---- host-side refusals ---------------------------------------------------------------------------------------------------------------
def test_loss_entry_points_refuse_bad_arguments_without_a_gpu():
    """Every call below has exactly one bad argument and must be refused by the host checks, before a launch (every pointer is a
    host buffer that no kernel may ever see; the workspace it claims is large enough, so only the argument under test can refuse)."""
    from gfnet_amd import _lib

    L = _lib.lib()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) // 16 * 16)
    BIG = 1 << 40

    def ptrs(n=8, hole=None):
        arr = (ctypes.c_void_p * 8)()
        for k in range(n):
            arr[k] = None if k == hole else p.value
        return arr

    def fwd(flows=None, certs=None, n=2, H=p, coords=None, prev=None, ph=0, pw=0, thr=0.1, epe=p, stats=p, B=2, h=4, w=6, ea=95.0, eb=95.0,
            a=0.5, cs=1e-3, cew=0.01, base=0.85, pck=0.01, ws=p, nws=BIG):
        flows = ptrs() if flows is None else flows
        certs = ptrs() if certs is None else certs
        return L.gfn_robust_loss_fwd(flows, certs, n, H, coords, prev, ph, pw, thr, epe, stats, B, h, w, ea, eb, a, cs, cew, base, pck, ws, nws, None)

    def bwd(flows=None, certs=None, n=2, H=p, coords=None, prev=None, ph=0, pw=0, thr=0.1, stats=p, go=p, gf=None, gc=None, need=0x303, B=2,
            h=4, w=6, ea=95.0, eb=95.0, a=0.5, cs=1e-3, cew=0.01, base=0.85):
        flows = ptrs() if flows is None else flows
        certs = ptrs() if certs is None else certs
        gf = ptrs() if gf is None else gf
        gc = ptrs() if gc is None else gc
        return L.gfn_robust_loss_bwd(flows, certs, n, H, coords, prev, ph, pw, thr, stats, go, gf, gc, need, B, h, w, ea, eb, a, cs, cew, base, None)

    def warp(H=p, coords=None, out=p, prob=p, x1n=None, B=2, h=4, w=6, ea=95.0, eb=95.0, normalized=1):
        return L.gfn_gt_warp_homography_fwd(H, coords, out, prob, x1n, B, h, w, ea, eb, normalized, None)

    def refused(code, what):
        assert code == -1, what
        assert L.gfn_last_error(), what

    shared = {"null flows": dict(flows=ctypes.c_void_p(0)), "null certs": dict(certs=ctypes.c_void_p(0)), "null H": dict(H=None),
              "null stats": dict(stats=None), "null flow of iteration 2": dict(flows=ptrs(hole=1)),
              "null certainty of iteration 1": dict(certs=ptrs(hole=0)), "n_itr = 0": dict(n=0), "n_itr = 9": dict(n=9), "n_itr < 0": dict(n=-1),
              "B < 0": dict(B=-1), "h = 0": dict(h=0), "w = 0": dict(w=0), "w < 0": dict(w=-3), "a side above 32768": dict(w=32769, B=1, h=1),
              "more than 2^30 cells": dict(B=5, h=16384, w=16384), "cs = 0": dict(cs=0.0), "cs < 0": dict(cs=-1e-3), "cs NaN": dict(cs=float("nan")),
              "target extent 0": dict(eb=0.0), "source extent < 0": dict(ea=-1.0),
              "prev_epe on a 0 x 4 grid": dict(prev=p, ph=0, pw=4), "prev_epe on a 4 x 0 grid": dict(prev=p, ph=4, pw=0)}
    for what, kw in shared.items():
        refused(fwd(**kw), "fwd: " + what)
        refused(bwd(**kw), "bwd: " + what)
    for what, kw in {"null workspace": dict(ws=None), "misaligned workspace": dict(ws=ctypes.c_void_p(p.value + 4)),
                     "workspace one byte short": dict(nws=15)}.items():
        refused(fwd(**kw), "fwd: " + what)
    for what, kw in {"null grad_out": dict(go=None), "need names iteration 3 of 2": dict(need=0x4), "need names certainty 3 of 2": dict(need=0x400),
                     "need < 0": dict(need=-1), "need past 16 bits": dict(need=1 << 16), "needed flow gradient null": dict(gf=ptrs(hole=1)),
                     "needed certainty gradient null": dict(gc=ptrs(hole=0)), "null gradient array": dict(gf=ctypes.c_void_p(0))}.items():
        refused(bwd(**kw), "bwd: " + what)
    for what, kw in {"null H": dict(H=None), "null out": dict(out=None), "null prob": dict(prob=None), "B < 0": dict(B=-1), "h = 0": dict(h=0),
                     "w = 0": dict(w=0), "a side above 32768": dict(h=32769, B=1, w=1), "more than 2^30 cells": dict(B=5, h=16384, w=16384),
                     "target extent 0": dict(eb=0.0)}.items():
        refused(warp(**kw), "warp: " + what)
    # nothing to compute: an empty batch, or no gradient asked for -- valid, and no launch (not even a look at the workspace)
    assert fwd(B=0) == 0 and fwd(B=0, ws=None, nws=0) == 0 and bwd(B=0) == 0 and warp(B=0) == 0
    assert bwd(need=0) == 0 and bwd(need=0, gf=ctypes.c_void_p(0), gc=ctypes.c_void_p(0)) == 0
    # a gradient that is not asked for may be a null entry
    assert bwd(need=0, gf=ptrs(hole=0)) == 0
    # the workspace: four partial sums per block of 256 cells, rounded up to 16 bytes
    assert L.gfn_robust_loss_ws_bytes(2, 4, 6, 2) == 16
    assert L.gfn_robust_loss_ws_bytes(8, 448, 448, 1) == (8 * 448 * 448 // 256) * 16
    assert L.gfn_robust_loss_ws_bytes(3, 37, 41, 8) == ((3 * 37 * 41 + 255) // 256) * 16
    assert L.gfn_robust_loss_ws_bytes(0, 4, 6, 2) == 0


def test_loss_kernels_have_no_spills_and_no_scratch():
    obj = os.path.join(ROOT, "gfnet_amd", "csrc", "robust_loss.o")
    if not os.path.exists(obj):
        from gfnet_amd import build

        build.build()
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), obj], capture_output=True, text=True, check=True).stdout
    rows = [ln for ln in out.splitlines() if "rl_" in ln or "gt_warp_kernel" in ln]
    assert len(rows) == 8, out   # forward and backward at three vector widths, the second stage, the warp kernel
    for ln in rows:
        f = ln.split()
        vals = {f[k]: f[k + 1] for k in range(len(f) - 1) if f[k] in ("spill", "sspill", "scratch")}
        assert vals == {"spill": "0", "sspill": "0", "scratch": "0"}, ln
        assert int(f[f.index("vgpr") + 1]) <= 64, ln   # eight waves per SIMD


# ---- the public interface ---------------------------------------------------------------------------------------------------------------
def test_constructor_defaults_equal_the_reference():
    from gfnet_amd.losses import RobustLosses, get_gt_warp_homography

    sig = inspect.signature(RobustLosses.__init__)
    got = {k: v.default for k, v in sig.parameters.items() if k != "self"}
    assert got == dict(ce_weight=0.01, local_dist=None, local_largest_scale=8, depth_interpolation_mode="bilinear", alpha=1., c=1e-3,
                       iteration_base=0.85)
    assert list(got) == ["ce_weight", "local_dist", "local_largest_scale", "depth_interpolation_mode", "alpha", "c", "iteration_base"]
    m = RobustLosses()
    assert isinstance(m, torch.nn.Module) and m.last_losses == {} and not list(m.parameters())
    assert (m.ce_weight, m.local_dist, m.local_largest_scale, m.alpha, m.c, m.iteration_base) == (0.01, None, 8, 1., 1e-3, 0.85)
    wsig = inspect.signature(get_gt_warp_homography)
    assert list(wsig.parameters) == ["H_s2t", "img_src", "img_tgt", "H", "W", "im_A_coords", "normalized", "return_x1_n"]
    assert [wsig.parameters[k].default for k in ("im_A_coords", "normalized", "return_x1_n")] == [None, True, False]


def _cpu_corresps(layout, B=2):
    return {key: {k: {"flow": torch.zeros(B, 2, *hw), "certainty": torch.zeros(B, 1, *hw)} for k in range(1, n + 1)} for key, hw, n in layout}


def test_interface_refuses_what_it_cannot_compute():
    from gfnet_amd._lib import GfnError
    from gfnet_amd.losses import RobustLosses, get_gt_warp_homography

    im = torch.zeros(2, 3, 96, 96)
    batch = {"H_s2t": torch.eye(3).expand(2, 3, 3).contiguous(), "im_A": im, "im_B": im}
    two = [("16", (6, 6), 1), ("8", (6, 6), 1)]
    with pytest.raises(ValueError, match="local_dist"):                     # scale 8 is narrowed, local_dist is None
        RobustLosses()(_cpu_corresps(two), batch)
    with pytest.raises(ValueError, match="local_dist"):                     # ... or lacks the scale
        RobustLosses(local_dist={4: 8})(_cpu_corresps(two), batch)
    with pytest.raises(ValueError, match="first"):                          # a narrowed first key has no prev_epe
        RobustLosses(local_dist=LOCAL_DIST)(_cpu_corresps([("8", (6, 6), 1)]), batch)
    with pytest.raises(ValueError, match="iterations"):
        RobustLosses(local_dist=LOCAL_DIST)(_cpu_corresps([("16", (6, 6), 9)]), batch)
    bad = _cpu_corresps(two)
    bad["8"][1]["certainty"] = torch.zeros(2, 1, 6, 5)
    with pytest.raises(ValueError, match="grid"):
        RobustLosses(local_dist=LOCAL_DIST)(bad, batch)
    bad = _cpu_corresps([("16", (6, 6), 2)])
    bad["16"][2]["flow"] = torch.zeros(2, 2, 8, 8)
    with pytest.raises(ValueError, match="grid"):
        RobustLosses(local_dist=LOCAL_DIST)(bad, batch)
    # no CPU path
    with pytest.raises(GfnError):
        RobustLosses(local_dist=LOCAL_DIST)(_cpu_corresps(two), batch)
    with pytest.raises(GfnError):
        RobustLosses(local_largest_scale=0)(_cpu_corresps([("gm", (6, 6), 1), ("16", (6, 6), 1)]), batch)
    with pytest.raises(GfnError):
        get_gt_warp_homography(batch["H_s2t"], im, im, 6, 6)
    with pytest.raises(GfnError):
        get_gt_warp_homography(batch["H_s2t"].double(), im, im, 6, 6, normalized=False)
