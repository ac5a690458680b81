#!/usr/bin/env python3
"""Generate the sampling-mode fixtures G10 / G11 by running the REFERENCE itself (like make_golden.py, whose import stubs it uses):

    python tests/golden/make_golden_modes.py

G10 (g10_local_corr_modes.npz): utils/local_correlation.py:4-72 with every sample_mode x padding_mode the reference hands to
F.grid_sample (:55-58, :66-68).  G11 (g11_refiner_modes.npz): the reference's ConvRefiner (model/network.py:444-564) built with
sample_mode="nearest" and "bicubic" (:464, 502, used at :537, 547, 553-554).  Each .npz records the torch version it was made
with (meta.json describes the G1..G9 run and is left alone).
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import synth  # noqa: E402
from make_golden import OUT, REF, install_stubs, save, t2n  # noqa: E402

SAMPLE_MODES = ("nearest", "bilinear", "bicubic")
PADDING_MODES = ("zeros", "border", "reflection")
# the combinations the option and probe sets cover
OPTION_MODES = (("nearest", "reflection"), ("bicubic", "border"))
PROBE_MODES = (("nearest", "reflection"), ("bicubic", "border"), ("bicubic", "zeros"))


def g10_local_corr_modes(local_correlation):
    """utils/local_correlation.py:4-72, all nine sampling combinations."""
    g = torch.Generator().manual_seed(1010)
    arrays = {"torch_version": np.array(torch.__version__)}
    # (a) non-square map, flows partly outside the image (the padding modes differ there), every combination
    B, c, h, w, G, r = 2, 8, 20, 28, 6, 2
    f0 = torch.randn(B, c, G, G, generator=g)
    f1 = torch.randn(B, c, h, w, generator=g)
    flow = torch.rand(B, 2, G, G, generator=g) * 2.6 - 1.3
    arrays.update(a_f0=t2n(f0), a_f1=t2n(f1), a_flow=t2n(flow), a_r=np.int64(r), a_G=np.int64(G))
    for sm in SAMPLE_MODES:
        for pm in PADDING_MODES:
            out = local_correlation((B, c, h, w), f0, f1, local_radius=r, num_grid=G, flow=flow, padding_mode=pm, sample_mode=sm)
            arrays[f"a_out_{sm}_{pm}"] = t2n(out)

    # (b) options: grid_based_correlation=True, num_level=2, flow=None (G == h == w)
    B, c, h, w, G, r = 1, 4, 12, 12, 12, 1
    f0 = torch.randn(B, c, G, G, generator=g)
    f1 = torch.randn(B, c, h, w, generator=g)
    flow = torch.rand(B, 2, G, G, generator=g) * 2.4 - 1.2
    arrays.update(b_f0=t2n(f0), b_f1=t2n(f1), b_flow=t2n(flow), b_r=np.int64(r), b_G=np.int64(G))
    for sm, pm in OPTION_MODES:
        kw = dict(local_radius=r, num_grid=G, padding_mode=pm, sample_mode=sm)
        arrays[f"b_grid_based_{sm}_{pm}"] = t2n(local_correlation((B, c, h, w), f0, f1, flow=flow, grid_based_correlation=True, **kw))
        arrays[f"b_num_level2_{sm}_{pm}"] = t2n(local_correlation((B, c, h, w), f0, f1, flow=flow, num_level=2, **kw))
        arrays[f"b_flow_none_{sm}_{pm}"] = t2n(local_correlation((B, c, h, w), f0, f1, flow=None, **kw))

    # (c) the scale-4 shape (c32, 112^2, G64, r4) in the style of G1b: inputs regenerated from tests/golden/synth.py, batch 1's
    #     flow stretched partly outside the image; 512 probe entries + per-tap sums per combination
    B, c, h, w, G, r = 2, 32, 112, 112, 64, 4
    K = (2 * r + 1) ** 2
    f0 = torch.from_numpy(synth.lattice_normalish((B, c, G, G), 21))
    f1 = torch.from_numpy(synth.lattice_normalish((B, c, h, w), 22))
    flow_np = synth.homography_flow(B, G, 23)
    flow_np[1] *= np.float32(1.1)
    flow = torch.from_numpy(flow_np)
    idx = torch.stack((torch.randint(0, B, (512,), generator=g), torch.randint(0, K, (512,), generator=g),
                       torch.randint(0, G, (512,), generator=g), torch.randint(0, G, (512,), generator=g)), 1)
    arrays.update(c_seeds=np.array([21, 22, 23]), c_shape=np.array([B, c, h, w, G, r]), c_probe_idx=t2n(idx))
    for sm, pm in PROBE_MODES:
        out = local_correlation((B, c, h, w), f0, f1, local_radius=r, num_grid=G, flow=flow, padding_mode=pm, sample_mode=sm)
        arrays[f"c_probe_val_{sm}_{pm}"] = t2n(out[idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]])
        arrays[f"c_sum_per_k_{sm}_{pm}"] = t2n(out.double().sum(dim=(0, 2, 3)))
    save("g10_local_corr_modes", **arrays)


def g11_refiner_modes(network):
    """model/network.py:533-564 with ConvRefiner(sample_mode="nearest" | "bicubic"), toy widths as G4 (smaller maps, one hidden block)."""
    c, disp, r, G, hs, ws, B = 8, 6, 2, 8, 14, 18, 2
    K = (2 * r + 1) ** 2
    dim = 2 * c + disp + K
    arrays = {"torch_version": np.array(torch.__version__), "G": np.int64(G), "r": np.int64(r), "scale_factor": np.float64(1.25),
              "hidden_blocks": np.int64(1)}
    torch.manual_seed(1111)
    x = torch.randn(B, c, hs, ws)
    y = torch.randn(B, c, hs, ws)
    flow = torch.rand(B, 2, G, G) * 2.2 - 1.1
    arrays.update(x=t2n(x), y=t2n(y), flow=t2n(flow))
    for sm in ("nearest", "bicubic"):
        ref = network.ConvRefiner(dim, dim, 3, kernel_size=5, dw=True, hidden_blocks=1, displacement_emb="linear",
                                  displacement_emb_dim=disp, local_corr_num=r, corr_in_other=True, amp=True,
                                  disable_local_corr_grad=True, bn_momentum=0.01, sample_mode=sm).eval()
        for m in ref.modules():  # non-trivial BN statistics
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.3)
                m.running_var.uniform_(0.5, 1.5)
        captured = {}
        ref.block1.register_forward_pre_hook(lambda mod, inp: captured.__setitem__("d", inp[0].detach().clone()))
        with torch.no_grad():
            dflow, dcert, lc = ref(G, x, y, flow, scale_factor=1.25)
        arrays.update({f"{sm}.d": t2n(captured["d"]), f"{sm}.local_corr": t2n(lc), f"{sm}.delta_flow": t2n(dflow),
                       f"{sm}.delta_cert": t2n(dcert)})
        for k, v in ref.state_dict().items():
            arrays[f"{sm}.sd.{k}"] = t2n(v)
    save("g11_refiner_modes", **arrays)


def main():
    torch.set_num_threads(4)
    install_stubs()
    sys.path.insert(0, REF)
    from utils.local_correlation import local_correlation
    import model.network as network

    g10_local_corr_modes(local_correlation)
    g11_refiner_modes(network)
    total = sum(os.path.getsize(os.path.join(OUT, f + ".npz")) for f in ("g10_local_corr_modes", "g11_refiner_modes"))
    print(f"G10 + G11: {total/1024:.1f} KiB")


if __name__ == "__main__":
    main()
