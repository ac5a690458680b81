"""The judge of the refiner-input tests, judged: oracle.refiner_input (ConvRefiner.forward up to the concat, model/network.py:533-558)
against a float64 torch restatement of the same prefix -- F.grid_sample (align_corners=False) for grid_feature at the cell centres and
for x_hat along the flow, an einsum for the displacement embedding, and restated_local_correlation on the float64 grid_feature.
The hard flows of the GPU suite (windows that leave the image, magnification, scattered and noisy flows, rotations) in plain and
concatenated-symmetric batches: if the oracle misread grid_sample's zeros padding or the window offsets off the image, the GPU tests
that trust it would pass anyway.  No GPU needed."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import oracle
import synth
from conftest import assert_close
from test_local_corr_gpu import _flows_of_kind
from test_sampling_modes_cpu import restated_local_correlation

TOL = 1e-4
# every finite flow kind of _flows_of_kind, and the mild magnifications that only fit the lean stage without its pitch padding
FLOW_KINDS = ["homography", "zoom", "random", "noisy", "border", "rot", "zoom1.2", "zoom1.35"]


def hard_flows(kind, B, G, seed):
    """(B, 2, G, G) fp32 flows of one kind (B >= 4: `border` shifts directions 0..3 off the image, one side each)."""
    if kind.startswith("zoom") and kind != "zoom":
        return synth.homography_flow(B, G, seed + 7, scale=float(kind[4:])).astype(np.float32)
    return np.ascontiguousarray(_flows_of_kind(kind, B, G, seed), dtype=np.float32)


def restated_refiner_input(G, x, y, flow, w, bias, r, scale_factor, corr_in_other=True):
    """cat(grid_sample(x, centres), grid_sample(y, flow), disp_emb(40/32 * scale_factor * (flow - centres)), local_correlation) in
    float64 (the coordinates stay the reference's fp32 values: cell centres from oracle.cell_centres, the flow as given)."""
    X, Y, FL = (torch.from_numpy(np.ascontiguousarray(a)).double() for a in (x, y, flow))
    B = X.shape[0]
    lin = torch.from_numpy(oracle.cell_centres(G)).double()
    gy, gx = torch.meshgrid(lin, lin, indexing="ij")
    coords = torch.stack((gx, gy))[None].expand(B, 2, G, G)
    grid_feature = F.grid_sample(X, coords.permute(0, 2, 3, 1), mode="bilinear", padding_mode="zeros", align_corners=False)
    x_hat = F.grid_sample(Y, FL.permute(0, 2, 3, 1), mode="bilinear", padding_mode="zeros", align_corners=False)
    Wd = torch.from_numpy(np.asarray(w, np.float64)).reshape(-1, 2)
    emb = torch.einsum("od,bdij->boij", Wd, 40 / 32 * scale_factor * (FL - coords)) + \
        torch.from_numpy(np.asarray(bias, np.float64))[None, :, None, None]
    parts = [grid_feature, x_hat, emb]
    if corr_in_other:
        parts.append(restated_local_correlation(grid_feature, Y, r, G, flow=FL))
    return torch.cat(parts, 1).numpy()


# (c, h, w, G, r): r = 1, 2, 4, 6; ragged grids (47, 22); one rectangular map; r = 0 without the correlation
SHAPES = [(16, 40, 40, 24, 1), (16, 40, 40, 24, 2), (16, 56, 56, 47, 2), (32, 36, 36, 22, 4), (16, 30, 44, 20, 6), (16, 40, 40, 24, 0)]


@pytest.mark.parametrize("c,h,w,G,r", SHAPES)
@pytest.mark.parametrize("kind", FLOW_KINDS)
def test_oracle_refiner_input_matches_float64_restatement(c, h, w, G, r, kind):
    Bh, Dd, sf = 2, 8, 1.25
    seed = 1000 + 10 * r + G
    a = synth.lattice_normalish((Bh, c, h, w), seed)
    b = synth.lattice_normalish((Bh, c, h, w), seed + 1)
    flow = hard_flows(kind, 2 * Bh, G, seed + 2)
    wt = synth.lattice_uniform((Dd, 2, 1, 1), seed + 3)
    bias = synth.lattice_uniform((Dd,), seed + 4)
    corr = r > 0
    plain = (synth.lattice_normalish((2 * Bh, c, h, w), seed + 5), synth.lattice_normalish((2 * Bh, c, h, w), seed + 6))
    symmetric = (np.concatenate((a, b)), np.concatenate((b, a)))  # the reference's concatenated batch (network.py:213-222)
    for form, (x, y) in (("plain", plain), ("symmetric", symmetric)):
        got = oracle.refiner_input(G, x, y, flow, wt, bias, r, scale_factor=sf, corr_in_other=corr)
        want = restated_refiner_input(G, x, y, flow, wt, bias, r, sf, corr_in_other=corr)
        assert got.shape == (2 * Bh, 2 * c + Dd + ((2 * r + 1) ** 2 if corr else 0), G, G)
        assert_close(got, want, TOL, f"{form} c{c} {h}x{w} G{G} r{r} {kind}")


def test_restatement_sees_the_flows_leave_the_image():
    """The cases above are hard only if their flows do leave the image: under `border` and `zoom` some x_hat samples and some windows
    fall wholly or partly outside it (exact zeros or partial zeros padding), and `random` scatters neighbouring cells."""
    G, r = 24, 2
    for kind in ("border", "zoom"):
        flow = hard_flows(kind, 4, G, 77)
        assert (np.abs(flow) > 1).any(axis=1).mean() > 0.01, kind  # cells whose x_hat sample centre is off the image
        assert (np.abs(flow) < 1 - 4.0 * r / 40).all(axis=1).mean() > 0.1, kind  # and cells whose whole window is on it
    rnd = hard_flows("random", 4, G, 77)
    assert np.abs(np.diff(rnd, axis=3)).mean() > 0.3
