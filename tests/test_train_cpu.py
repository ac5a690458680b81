"""Training mode without a GPU: the host checks of the global correlation's backward (csrc/corr_softargmax_bwd.hip), its register
budget, and a plain-torch CPU restatement of the reference's training forward (model/network.py:203-283, 415-440, 533-564)
against the reference-generated fixture G12 -- what tests/test_train_gpu.py holds the GPU path to."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT, load_golden
from test_sampling_modes_cpu import restated_local_correlation

SCALES = ("16", "8", "4", "2", "1")
GRAD_FLOOR = 1.0


def test_bwd_entry_points_refuse_bad_arguments_without_a_gpu():
    """Every call below has exactly one bad argument and must be refused by the host checks, before a launch (every pointer is a
    host buffer that no kernel may ever see; the workspace it claims is large enough, so only the argument under test can refuse)."""
    from gfnet_amd import _lib

    L = _lib.lib()
    buf = ctypes.create_string_buffer(256)
    base = ctypes.addressof(buf)
    p = ctypes.c_void_p((base + 15) // 16 * 16)
    F32, F16 = _lib.GFN_F32, _lib.GFN_F16
    BIG = 1 << 40

    def bwd(f0=p, f1=p, dt=F32, flow=p, gflow=p, g0=p, g1=p, B=2, C=16, H0=4, W0=4, H1=4, W1=4, sym=0, ws=p, nws=BIG):
        return L.gfn_corr_softargmax_bwd(f0, f1, dt, flow, gflow, g0, g1, B, C, H0, W0, H1, W1, sym, ws, nws, None)

    def refused(code, what):
        assert code == -1, what
        assert L.gfn_last_error(), what

    bad = {"C = 0": dict(C=0), "C = 129": dict(C=129), "B < 0": dict(B=-1), "null f0": dict(f0=None), "null f1": dict(f1=None),
           "null flow": dict(flow=None), "null grad_flow": dict(gflow=None), "H0 = 0": dict(H0=0), "W1 = 0": dict(W1=0),
           "A map of 2^24 positions": dict(H0=4096, W0=4096), "B map of 2^24 positions": dict(H1=1, W1=1 << 24),
           "symmetric, odd batch": dict(B=3, sym=1), "symmetric, unequal widths": dict(W1=5, sym=1),
           "symmetric, unequal heights": dict(H0=5, sym=1), "unknown dtype": dict(dt=7), "null workspace": dict(ws=None),
           "misaligned workspace": dict(ws=ctypes.c_void_p(p.value + 4)), "workspace too small": dict(nws=2 * 16 * 20 - 1)}
    for what, kw in bad.items():
        for dt in (F32, F16):
            refused(bwd(**{"dt": dt, **kw}), what)
    # nothing to compute: an empty batch, or neither gradient asked for -- valid, and no launch
    assert bwd(B=0) == 0 and bwd(g0=None, g1=None) == 0
    # the workspace size: 20 bytes per A-position and direction (the softmax statistics)
    assert L.gfn_corr_softargmax_bwd_ws_bytes(2, 16, 4, 4, 4, 4) == 2 * 16 * 20
    assert L.gfn_corr_softargmax_bwd_ws_bytes(0, 16, 4, 4, 4, 4) == 0


def test_bwd_kernels_have_no_spills_and_no_scratch():
    obj = os.path.join(ROOT, "gfnet_amd", "csrc", "corr_softargmax_bwd.o")
    if not os.path.exists(obj):
        from gfnet_amd import build

        build.build()
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), obj, "bwd_"], capture_output=True, text=True,
                         check=True).stdout
    rows = [ln for ln in out.splitlines() if "bwd_f" in ln]
    assert len(rows) == 16, out   # {f0, f1} kernels x KS {8, 16, 32, 64} x {fp32, fp16} maps
    for ln in rows:
        f = ln.split()
        vals = {f[k]: f[k + 1] for k in range(len(f) - 1) if f[k] in ("spill", "sspill", "scratch")}
        assert vals == {"spill": "0", "sspill": "0", "scratch": "0"}, ln


# ---- the reference's training forward restated in plain torch ---------------------------------------------------------------------
def restated_global_match(f0, f1):
    """pos_embed(corr_volume(f0, f1)), model/network.py:415-440"""
    B, C, H0, W0 = f0.shape
    H1, W1 = f1.shape[-2:]
    s = torch.einsum("bci,bcj->bji", f0.reshape(B, C, -1), f1.reshape(B, C, -1)) / math.sqrt(C)
    gx, gy = torch.meshgrid(torch.linspace(-1 + 1 / W1, 1 - 1 / W1, W1, device=f0.device),
                            torch.linspace(-1 + 1 / H1, 1 - 1 / H1, H1, device=f0.device), indexing="xy")
    grid = torch.stack((gx, gy), -1).reshape(H1 * W1, 2).to(s)
    return torch.einsum("bji,jd->bdi", s.softmax(dim=1), grid).reshape(B, 2, H0, W0)


def restated_refiner(ref, G, x, y, flow):
    """ConvRefiner.forward, model/network.py:533-564 (bilinear, amp off); the window of the local correlation is sampled without
    gradient, as utils/local_correlation.py:54-60 does"""
    b = x.shape[0]
    x_hat = F.grid_sample(y, flow.permute(0, 2, 3, 1), align_corners=False)
    lin = torch.linspace(-1 + 1 / G, 1 - 1 / G, G, device=x.device)
    gy, gx = torch.meshgrid(lin, lin, indexing="ij")
    coords = torch.stack((gx, gy))[None].expand(b, 2, G, G)
    grid_feature = F.grid_sample(x, coords.permute(0, 2, 3, 1), align_corners=False)
    parts = [grid_feature, x_hat, ref.disp_emb(40 / 32 * (flow - coords))]
    if ref.corr_in_other:
        parts.append(restated_local_correlation(grid_feature, y.detach(), ref.local_corr_radius, G, flow=flow.detach()))
    out = ref.out_conv(ref.hidden_blocks(ref.block1(torch.cat(parts, dim=1))).float())
    return out[:, :2], out[:, 2:3]


def restated_train_forward(pyr0, pyr1, refiners, num_grid, num_itr, image_hw):
    """GFNet.forward's loop in training mode, model/network.py:230-283: no small-displacement zeroing, the resize detached"""
    H0, W0 = image_hw
    corresps = {}
    for idx, s in enumerate(SCALES):
        f0, f1 = pyr0[s], pyr1[s]
        if idx == 0:
            flow = restated_global_match(f0, f1)
            cert = torch.zeros_like(flow)[:, :1]
        corresps[s] = {}
        for itr in range(num_itr[idx]):
            dflow, dcert = restated_refiner(refiners[s], num_grid[idx], f0, f1, flow)
            flow = flow + int(s) * torch.stack((dflow[:, 0].float() / (4 * W0), dflow[:, 1].float() / (4 * H0)), dim=1)
            cert = cert + dcert
            corresps[s][itr + 1] = {"flow": flow, "certainty": cert}
        if s != "1":
            flow = F.interpolate(flow, size=num_grid[idx + 1], mode="bilinear").detach()
            cert = F.interpolate(cert, size=num_grid[idx + 1], mode="bilinear").detach()
    return corresps


def g12_refiners(g, device="cpu"):
    """This package's ConvRefiners with the fixture's weights, in train()"""
    from gfnet_amd.model.network import ConvRefiner

    refiners = {}
    for i, s in enumerate(SCALES):
        c, disp, r = int(g["feat_ch"][i]), int(g["disp"][i]), int(g["radius"][i])
        dim = 2 * c + disp + ((2 * r + 1) ** 2 if r > 0 else 0)
        ref = ConvRefiner(dim, dim, 3, kernel_size=5, dw=True, hidden_blocks=int(g["hidden_blocks"]), displacement_emb="linear",
                          displacement_emb_dim=disp, local_corr_num=r, corr_in_other=r > 0, amp=False, bn_momentum=0.01)
        ref.load_state_dict({k[len(f"sd.{s}."):]: torch.from_numpy(g[k]) for k in g.files if k.startswith(f"sd.{s}.")}, strict=True)
        refiners[s] = ref.to(device).train()
    return refiners


def g12_pyramids(g, device="cpu"):
    return tuple({s: torch.from_numpy(g[f"{p}.{s}"]).to(device).requires_grad_() for s in SCALES} for p in ("pyr0", "pyr1"))


def weighted_loss(g, corresps):
    """the fixture's fixed random weighting of every (scale, iteration) flow and certainty"""
    dev = corresps["16"][1]["flow"].device
    loss = torch.zeros((), device=dev)
    for s in SCALES:
        for itr, d in corresps[s].items():
            loss = loss + (torch.from_numpy(g[f"wflow.{s}.{itr}"]).to(dev) * d["flow"]).sum() + \
                (torch.from_numpy(g[f"wcert.{s}.{itr}"]).to(dev) * d["certainty"]).sum()
    return loss


def compare_to_g12(g, corresps, pyr0, pyr1, refiners, out_tol, grad_tol):
    """every recorded tensor: |got - want| <= out_tol * max(1, |want|) for outputs and buffers, <= grad_tol * max|want| for gradients;
    returns the worst ratio per kind"""
    worst = {"outputs": 0.0, "gradients": 0.0}

    def close(name, got, want, tol, rel_to_max):
        got = got.detach().double().cpu().numpy()
        want = np.asarray(want, np.float64)
        assert got.shape == want.shape, (name, got.shape, want.shape)
        assert np.isfinite(got).all(), f"{name}: non-finite"
        # (gradients: of the tensor's largest entry, but not below GRAD_FLOOR -- the bias of a conv that feeds a train-mode BatchNorm
        # has an analytically zero gradient, and what either side records there is rounding noise)
        scale = max(np.abs(want).max(), GRAD_FLOOR) if rel_to_max else np.maximum(1.0, np.abs(want))
        r = float((np.abs(got - want) / (tol * scale)).max())
        kind = "gradients" if rel_to_max else "outputs"
        worst[kind] = max(worst[kind], r)
        assert r <= 1.0, f"{name}: err {np.abs(got - want).max():.3e}, {r:.2f} x the tolerance"

    for s in SCALES:
        for itr, d in corresps[s].items():
            close(f"flow.{s}.{itr}", d["flow"], g[f"flow.{s}.{itr}"], out_tol, False)
            close(f"cert.{s}.{itr}", d["certainty"], g[f"cert.{s}.{itr}"], out_tol, False)
        assert pyr0[s].grad is not None and pyr1[s].grad is not None, f"no gradient reached the scale-{s} pyramids"
        close(f"grad0.{s}", pyr0[s].grad, g[f"grad0.{s}"], grad_tol, True)
        close(f"grad1.{s}", pyr1[s].grad, g[f"grad1.{s}"], grad_tol, True)
        for k, prm in refiners[s].named_parameters():
            assert prm.grad is not None, f"no gradient for refiner {s} {k}"
            close(f"pgrad.{s}.{k}", prm.grad, g[f"pgrad.{s}.{k}"], grad_tol, True)
        for k, buf in refiners[s].named_buffers():
            close(f"buf_after.{s}.{k}", buf, g[f"buf_after.{s}.{k}"], out_tol, False)
    return worst


def test_cpu_restatement_reproduces_g12():
    """Same device class as the fixture (fp32 on the CPU); the restatement sums in other orders (the local correlation in one
    grid_sample, not per image), so a few fp32 roundings through the BatchNorm chain: 1e-5 for outputs.  Gradients: 1e-4 of the
    tensor's largest entry, floored at GRAD_FLOOR -- the biases in front of a train-mode BatchNorm have an analytical gradient of
    zero and record the cancellation noise of every term behind them (~1e-5 here)."""
    g = load_golden("g12_train_grads")
    torch.manual_seed(0)
    refiners = g12_refiners(g)
    pyr0, pyr1 = g12_pyramids(g)
    corresps = restated_train_forward(pyr0, pyr1, refiners, [int(v) for v in g["num_grid"]], [int(v) for v in g["num_itr"]],
                                      tuple(int(v) for v in g["image_hw"]))
    loss = weighted_loss(g, corresps)
    loss.backward()
    assert abs(loss.item() - float(g["loss"])) <= 1e-5 * max(1.0, abs(float(g["loss"])))
    worst = compare_to_g12(g, corresps, pyr0, pyr1, refiners, 1e-5, 1e-4)
    print(f"G12 CPU restatement: worst err / tol {worst}")


def test_g12_covers_what_the_fixture_promises():
    g = load_golden("g12_train_grads")
    assert (int(g["num_grid"][0]) ** 2) % 32 and int(g["feat_ch"][0]) % 2         # ragged A-tile, odd channel count
    assert max(int(v) for v in g["num_itr"]) >= 2
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "g12_train_grads.npz")) <= 400 * 1024
    assert str(g["torch_version"])
