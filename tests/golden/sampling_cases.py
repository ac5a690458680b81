"""The float64 oracle of a sample (csrc/sample_modes.h, ATen's grid_sampler_2d with align_corners=False) and the seeded cases of
tests/test_sampling_exact_cpu.py / test_sampling_exact_gpu.py.  numpy only.

Definition.  The COORDINATES follow the fp32 sequence of ATen and of sample_modes.h, one rounding per operation (numpy never
fuses): unnorm, clip_coord, reflect_coord (fmod, floor(in / span)), rint for nearest, floor of the un-padded coordinate for bicubic
with each of the 4 x 4 taps padded on its own and read as 0 outside the image.  WEIGHTS and SUMS are float64.  The documented guard
is part of the definition: a non-finite coordinate, or one whose un-padded floor is <= -10^6 or >= 10^6, reads zeros in every mode
(F.grid_sample differs there in border and reflection padding).

Two families of cases.
  exact    power-of-two map sides, pixel coordinates on the half-pixel lattice (g = (2p + 1) / size - 1 reproduces p in fp32, fused
           or not), small integer values: every weight, product and partial sum is a dyadic rational that fp32 holds, so a kernel
           has no rounding to hide behind and must EQUAL the oracle.  Each builder asserts that budget (exact_budget).
  generic  odd sides, lattice_normalish values, uniform coordinates; a point is KEPT when both pixel coordinates are >= 2^-10 px
           from every integer and half-integer (the floors, the nearest ties, the mirrors and their images), so that a coordinate
           rounding (delta below, < 2^-12 px) cannot flip a decision."""
import functools

import numpy as np

import synth

F32 = np.float32
SAMPLE_MODES = ("nearest", "bilinear", "bicubic")
PADDING_MODES = ("zeros", "border", "reflection")
ALL_MODES = [(sm, pm) for sm in SAMPLE_MODES for pm in PADDING_MODES]
KEEP_DIST = 2.0 ** -10  # px: kept points stay this far from every decision
MAX_DROPPED = 0.02      # share of a generic case's points that may fall inside KEEP_DIST
MIN_CELLS_KEPT = 0.80   # share of a generic local-correlation case's cells whose taps are all kept


# ---- coordinates: fp32 (or, for the perturbed evaluations of `allowance`, whatever dtype they arrive in) ------------------------
def unnorm(g, size):
    g = np.asarray(g, F32)
    return ((g + F32(1)) * F32(size) - F32(1)) / F32(2)


def clip_coord(x, size):
    t = x.dtype.type
    return np.minimum(t(size - 1), np.maximum(x, t(0)))


def reflect_coord(x, size):
    t = x.dtype.type
    mn, span = t(-0.5), t(size)
    a = np.abs(x - mn)
    extra = np.fmod(a, span)
    flips = np.floor(a / span)
    return np.where(np.fmod(flips, t(2)) == 0, extra + mn, span - extra + mn)


def pad_coord(x, size, pad):
    if pad == "border":
        return clip_coord(x, size)
    if pad == "reflection":
        return clip_coord(reflect_coord(x, size), size)
    assert pad == "zeros", pad
    return x


def linspace_at(start, end, steps, i):
    """torch.linspace(start, end, steps)[i] in fp32, filled from both ends (gfn::linspace_at)."""
    start, end, i = F32(start), F32(end), np.asarray(i)
    if steps == 1:
        return np.full(i.shape, start, F32)
    step = (end - start) / F32(steps - 1)
    return np.where(i < steps // 2, start + step * i.astype(F32), end - step * (steps - i - 1).astype(F32)).astype(F32)


def sane(ix, iy):
    with np.errstate(invalid="ignore"):
        fx, fy = np.floor(ix), np.floor(iy)
        return np.isfinite(ix) & np.isfinite(iy) & (fx > -1e6) & (fx < 1e6) & (fy > -1e6) & (fy < 1e6)


def _cubic(t):
    """get_cubic_upsample_coefficients, A = -0.75, in float64: (..., 4)."""
    A = -0.75
    c1 = lambda x: ((A + 2) * x - (A + 3)) * x * x + 1
    c2 = lambda x: ((A * x - 5 * A) * x + 8 * A) * x - 4 * A
    return np.stack((c2(t + 1), c1(t), c1(1 - t), c2(2 - t)), -1)


def _gather(img, y, x, ok):
    H, W = img.shape[-2:]
    v = img[:, np.where(ok, y, 0), np.where(ok, x, 0)]
    return np.where(ok, v, 0.0)


def sample_px(img, ix, iy, mode, pad, absolute=False):
    """img (C, H, W), pixel coordinates ix, iy (N,) -> (C, N) float64.  absolute: the sum of |weight * value| instead."""
    img = np.asarray(img, np.float64)
    if absolute:
        img = np.abs(img)
    H, W = img.shape[-2:]
    ok0 = sane(ix, iy)
    ix, iy = np.where(ok0, ix, ix.dtype.type(0)), np.where(ok0, iy, iy.dtype.type(0))
    inside = lambda x, y: ok0 & (x >= 0) & (x < W) & (y >= 0) & (y < H)
    if mode == "nearest":
        x = np.rint(pad_coord(ix, W, pad)).astype(np.int64)  # half to even
        y = np.rint(pad_coord(iy, H, pad)).astype(np.int64)
        return _gather(img, y, x, inside(x, y))
    if mode == "bilinear":
        px, py = pad_coord(ix, W, pad), pad_coord(iy, H, pad)
        fx, fy = np.floor(px), np.floor(py)
        tx, ty = px.astype(np.float64) - fx, py.astype(np.float64) - fy
        x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
        out = 0.0
        for dy, wy in ((0, 1 - ty), (1, ty)):
            for dx, wx in ((0, 1 - tx), (1, tx)):
                w = wx * wy
                out = out + (np.abs(w) if absolute else w) * _gather(img, y0 + dy, x0 + dx, inside(x0 + dx, y0 + dy))
        return out
    assert mode == "bicubic", mode
    fx, fy = np.floor(ix), np.floor(iy)
    cx, cy = _cubic(ix.astype(np.float64) - fx), _cubic(iy.astype(np.float64) - fy)
    if absolute:
        cx, cy = np.abs(cx), np.abs(cy)
    one = ix.dtype.type(1)
    out = 0.0
    for r in range(4):
        y = pad_coord(fy - one + ix.dtype.type(r), H, pad).astype(np.int64)
        for c in range(4):
            x = pad_coord(fx - one + ix.dtype.type(c), W, pad).astype(np.int64)
            out = out + cy[:, r] * cx[:, c] * _gather(img, y, x, inside(x, y))
    return out


def sample(img, gx, gy, mode, pad, shift=(0.0, 0.0), absolute=False):
    """grid_sample of one image: img (C, H, W), normalised fp32 coordinates gx, gy (N,) -> (C, N) float64.
    shift: move every point by that many pixels (float64) after un-normalising -- for `allowance` only."""
    H, W = np.shape(img)[-2:]
    ix, iy = unnorm(gx, W), unnorm(gy, H)
    if shift != (0.0, 0.0):
        ix, iy = ix.astype(np.float64) + shift[0], iy.astype(np.float64) + shift[1]
    return sample_px(img, ix, iy, mode, pad, absolute)


def grid_sample(x, grid, mode, pad, **kw):
    """x (B, C, H, W), grid (B, Ho, Wo, 2) -> (B, C, Ho, Wo) float64."""
    B, C = x.shape[:2]
    Ho, Wo = grid.shape[1:3]
    return np.stack([sample(x[b], grid[b, ..., 0].ravel(), grid[b, ..., 1].ravel(), mode, pad, **kw).reshape(C, Ho, Wo) for b in range(B)])


# ---- local correlation ----------------------------------------------------------------------------------------------------------
def tap_coords(flow, B, G, h, w, r, grid_based):
    """Normalised fp32 tap coordinates (B, K, G, G) x 2, formed as local_corr_mode_kernel, window_ends and cell_coords form them."""
    D = 2 * r + 1
    sy, sx = (G, G) if grid_based else (h, w)
    xlo, xhi, ylo, yhi = F32(-2.0 * r / sx), F32(2.0 * r / sx), F32(-2.0 * r / sy), F32(2.0 * r / sy)
    if flow is None:  # identity grid
        assert G == h == w
        nx = np.broadcast_to(linspace_at(F32(-1 + 1.0 / w), F32(1 - 1.0 / w), w, np.arange(G))[None, None, :], (B, G, G))
        ny = np.broadcast_to(linspace_at(F32(-1 + 1.0 / h), F32(1 - 1.0 / h), h, np.arange(G))[None, :, None], (B, G, G))
    else:
        flow = np.asarray(flow, F32)
        nx, ny = flow[:, 0], flow[:, 1]
    k = np.arange(D * D)
    with np.errstate(invalid="ignore"):
        gx = nx[:, None] + linspace_at(xlo, xhi, D, k % D)[None, :, None, None]
        gy = ny[:, None] + linspace_at(ylo, yhi, D, k // D)[None, :, None, None]
    return gx.astype(F32), gy.astype(F32)


def pooled_levels(f1, num_level):
    f1 = np.asarray(f1, np.float64)
    out = [f1]
    for _ in range(1, num_level):
        B, C, h, w = f1.shape
        f1 = f1[:, :, :h // 2 * 2, :w // 2 * 2].reshape(B, C, h // 2, 2, w // 2, 2).mean((3, 5))
        out.append(f1)
    return out


def sampled_taps(f1, flow, r, G, mode, pad, grid_based=False, num_level=1, **kw):
    """S[b, c, level * K + k, i, j]: the sample of (the pooled level of) f1[b, c] at tap k of cell (i, j), float64."""
    B, C, h, w = f1.shape
    K = (2 * r + 1) ** 2
    gx, gy = tap_coords(flow, B, G, h, w, r, grid_based)
    return np.concatenate([np.stack([sample(fl[b], gx[b].ravel(), gy[b].ravel(), mode, pad, **kw).reshape(C, K, G, G) for b in range(B)])
                           for fl in pooled_levels(f1, num_level)], 2)


def local_correlation(f0, f1, flow, r, G, mode, pad, grid_based=False, num_level=1, **kw):
    """out[b, level * K + ky * D + kx, i, j] = sum_c f0[b, c, i, j] / sqrt(C) * S[b, c, ., i, j]  (utils/local_correlation.py)."""
    S = sampled_taps(f1, flow, r, G, mode, pad, grid_based, num_level, **kw)
    q = np.asarray(f0, np.float64) / np.sqrt(float(f1.shape[1]))
    if kw.get("absolute"):
        q = np.abs(q)
    return (q[:, :, None] * S).sum(1)


def local_correlation_grad_f0(grad_out, f1, flow, r, G, mode, pad, grid_based=False, num_level=1, **kw):
    """d sum(out * grad_out) / d f0: (sum_k grad_out[b, k] * S[b, c, k]) / sqrt(C), summed over the levels."""
    S = sampled_taps(f1, flow, r, G, mode, pad, grid_based, num_level, **kw)
    g = np.asarray(grad_out, np.float64)
    if kw.get("absolute"):
        g = np.abs(g)
    return (g[:, None] * S).sum(2) / np.sqrt(float(f1.shape[1]))


# ---- refiner input --------------------------------------------------------------------------------------------------------------
def refiner_input(x, y, flow, disp_w, disp_b, G, scale_factor, mode, r=None, absolute=False):
    """d = cat(grid_feature, x_hat, disp_emb[, local correlation of radius r]) as refiner_input_mode_kernel lays it out; flow with
    twice the batch of x / y is the symmetric call: directions (x vs y), then (y vs x).  The cell centres and flow - centre are fp32,
    the rest float64; the local correlation reads grid_feature rounded to fp32, as the kernel reads it back from d."""
    flow = np.asarray(flow, F32)
    B, Bi = flow.shape[0], x.shape[0]
    q, s = (np.concatenate((x, y)), np.concatenate((y, x))) if B == 2 * Bi else (x, y)
    c = linspace_at(F32(-1 + 1.0 / G), F32(1 - 1.0 / G), G, np.arange(G))
    cx, cy = np.broadcast_to(c[None, :], (G, G)).ravel(), np.broadcast_to(c[:, None], (G, G)).ravel()
    C = x.shape[1]
    kw = dict(absolute=absolute)
    gf = np.stack([sample(q[b], cx, cy, mode, "zeros", **kw).reshape(C, G, G) for b in range(B)])
    xh = np.stack([sample(s[b], flow[b, 0].ravel(), flow[b, 1].ravel(), mode, "zeros", **kw).reshape(C, G, G) for b in range(B)])
    ds = F32(40 / 32 * scale_factor)
    with np.errstate(invalid="ignore"):
        dx = np.float64(ds) * (flow[:, 0] - cx.reshape(G, G)).astype(np.float64)
        dy = np.float64(ds) * (flow[:, 1] - cy.reshape(G, G)).astype(np.float64)
        w, bias = np.asarray(disp_w, np.float64).reshape(-1, 2), np.asarray(disp_b, np.float64).reshape(-1)
        if absolute:
            dx, dy, w, bias = np.abs(dx), np.abs(dy), np.abs(w), np.abs(bias)
        emb = w[None, :, 0, None, None] * dx[:, None] + w[None, :, 1, None, None] * dy[:, None] + bias[None, :, None, None]
    parts = [gf, xh, emb]
    if r is not None:
        parts.append(local_correlation(gf.astype(F32), s, flow, r, G, mode, "zeros", **kw))
    return np.concatenate(parts, 1)


# ---- the exactness budget -------------------------------------------------------------------------------------------------------
def weight_den(mode, q):
    """Common denominator of a sample's weights for pixel coordinates on the 1/q lattice: bilinear q per axis; the cubic
    convolution (A = -3/4) is a cubic in t = n/q, 4 q^3 per axis (q = 2: 19/32, -3/32)."""
    return {"nearest": 1, "bilinear": q * q, "bicubic": (4 * q ** 3) ** 2}[mode]


def exact_budget(value, absolute, den, what):
    """Over the common denominator `den` every output is an integer and its sum of |term| stays below 2^24: all partial sums are
    then fp32 numbers, in any order, fused or not."""
    v, a = np.asarray(value, np.float64) * den, np.asarray(absolute, np.float64) * den
    fin = np.isfinite(v)
    assert (v[fin] == np.rint(v[fin])).all(), f"{what}: not a multiple of 1/{den}"
    assert float(a[fin].max()) < 2.0 ** 24, f"{what}: sum of |term| * {den} = {float(a[fin].max()):.4g} >= 2^24"
    return float(a[fin].max()) / 2.0 ** 24


def ints(shape, seed, lim):
    """Seeded integers in [-lim, lim] as float32."""
    n = int(np.prod(shape))
    return ((synth.hash_u32(n, seed) % np.uint32(2 * lim + 1)).astype(np.int64) - lim).astype(F32).reshape(shape)


def norm_of(p, size):
    """The normalised fp32 coordinate of pixel coordinate p, checked to give p back in fp32."""
    p = np.asarray(p, np.float64)
    g = ((2 * p + 1) / size - 1).astype(F32)
    assert (unnorm(g, size).astype(np.float64) == p).all()
    return g


def half_pixels(size):
    """Every half-pixel coordinate from -3 size to +4 size."""
    return np.arange(-6 * size, 8 * size + 1) / 2.0


# floors exactly +-(10^6 - 1): sane, sampled per the definition; floors exactly +-10^6 and beyond, and non-finite: zeros
EXTREME_SANE = (999999.0, 999999.5, -999999.0, -999998.5)
EXTREME_GUARD = (1000000.0, 1000000.5, -1000000.0, -999999.5, -1000000.5, float("nan"), float("inf"), -float("inf"))


def _norm_any(p, size):
    p = np.asarray(p, np.float64)
    fin = np.isfinite(p)
    return np.where(fin, norm_of(np.where(fin, p, 0.0), size), p.astype(F32)).astype(F32)


def extreme_points(H, W):
    """(px, py, guard) of the points around the guard: each extreme value on either axis with an ordinary one on the other, and on
    both."""
    pts = []
    for v in EXTREME_SANE + EXTREME_GUARD:
        g = v in EXTREME_GUARD or v != v
        for o in (0.0, 0.5):
            pts += [(v, o, g), (o, v, g)]
        pts.append((v, v, g))
    pts += [(999999.0, -1000000.0, True), (float("nan"), 999999.5, True), (-999999.0, 999999.5, False)]
    px, py, guard = (np.array(c) for c in zip(*pts))
    return px, py, guard.astype(bool)


@functools.lru_cache(maxsize=None)
def exact_points(H, W):
    """The exact family's points on an H x W map: the half-pixel lattice from -3 size to +4 size on both axes, then the extreme
    points.  Returns normalised fp32 (gx, gy), the guard mask (points that read zeros by definition) and the lattice count."""
    ly, lx = np.meshgrid(half_pixels(H), half_pixels(W), indexing="ij")
    ex, ey, eg = extreme_points(H, W)
    px, py = np.concatenate((lx.ravel(), ex)), np.concatenate((ly.ravel(), ey))
    guard = np.concatenate((np.zeros(lx.size, bool), eg))
    gx, gy = _norm_any(px, W), _norm_any(py, H)
    assert (~sane(unnorm(gx, W), unnorm(gy, H)) == guard).all()
    return gx, gy, guard, lx.size


EXACT_MAPS = ((8, 16), (1, 4), (4, 1), (2, 2))


@functools.lru_cache(maxsize=None)
def exact_grid_case(H, W, C):
    """x (2, C, H, W) of integers in [-64, 64] (exact in fp16 too), grid (2, 1, N, 2), guard (N,), oracle budget asserted."""
    x = ints((2, C, H, W), 7001 + 100 * H + 10 * W + C, 64)
    gx, gy, guard, _ = exact_points(H, W)
    grid = np.ascontiguousarray(np.broadcast_to(np.stack((gx, gy), -1)[None, None], (2, 1, gx.size, 2)))
    for sm, pm in ALL_MODES:
        exact_budget(grid_sample(x, grid, sm, pm), grid_sample(x, grid, sm, pm, absolute=True), weight_den(sm, 2), f"grid {H}x{W} {sm}/{pm}")
    return dict(x=x, grid=grid, guard=guard)


@functools.lru_cache(maxsize=None)
def exact_grid_oracle(H, W, C, sm, pm):
    c = exact_grid_case(H, W, C)
    return grid_sample(c["x"], c["grid"], sm, pm)


# name: C, H, W, G, r, grid_based, num_level, flow, f1 step, f1 limit, f0 limit, grad limit.  f1 = step * integers in +-limit (the
# step of 4 keeps the pooled level integral), f0 = sqrt(C) * integers, so that f0 / sqrt_c is an integer.
EXACT_LC = {
    "c4_r1": (4, 8, 16, 4, 1, False, 1, True, 1, 64, 4, 3),
    "c9_r2": (9, 8, 16, 8, 2, False, 1, True, 1, 64, 4, 3),       # one-channel tail in the 8-wide and in the 4-wide group
    "c16_r1_tall": (16, 16, 8, 8, 1, False, 1, True, 1, 64, 4, 3),
    "c9_grid_based": (9, 8, 16, 4, 1, True, 1, True, 1, 64, 4, 3),
    "c4_levels2": (4, 8, 16, 4, 1, False, 2, True, 4, 2, 1, 1),  # level 2 is on the quarter-pixel lattice: (4 * 4^3)^2 = 2^16
    "c9_flow_none": (9, 8, 8, 8, 2, False, 1, False, 1, 64, 4, 3),
    "c16_thin": (16, 1, 4, 4, 1, False, 1, True, 1, 64, 4, 3),
}


# non-finite flows: every corner of the set-up is outside the image and its weights are NaN; the sample is zero all the same
NON_FINITE_FLOWS = [(float("nan"), 0.0), (1.0, float("inf")), (-float("inf"), 0.5)]
# around the guard: floors +-(10^6 - 1) next to it, exactly +-10^6 on it (a window's taps straddle it), and cells wholly beyond
GUARD_FLOWS = [(999999.0, 1.0), (1.0, -999999.0), (999998.5, 0.0), (1000000.0, 1.0), (-1000000.0, 1.0), (1.0, -1000000.0), (1000008.0, 0.0),
               (0.5, -1000008.0)]


def lattice_flow(B, G, H, W, seed, reach=3, extremes=True):
    """Flows (B, 2, G, G) on the half-pixel lattice from -reach to size + reach - 1 px (outside the map on every side), with the
    decision points written over the first cells of batch element 0 and -- if asked -- the guard's surroundings and the non-finite
    flows over the first cells of batch element 1.  Returns the flow and the mask (B, G, G) of cells with an extreme coordinate."""
    n = B * G * G
    px = (synth.hash_u32(n, seed) % np.uint32(2 * (W + 2 * reach) - 1)).astype(np.float64) / 2 - reach
    py = (synth.hash_u32(n, seed + 1) % np.uint32(2 * (H + 2 * reach) - 1)).astype(np.float64) / 2 - reach
    special = [(W - 1.0, H - 1.0), (0.0, 0.0), (-0.5, H - 0.5), (W - 0.5, -0.5), (W - 1.0, 0.5), (0.5, H - 1.0)]
    extreme = GUARD_FLOWS + NON_FINITE_FLOWS if extremes else []
    assert B >= 2 and max(len(special), len(extreme)) <= G * G
    mask = np.zeros(n, bool)
    for k, (sx, sy) in enumerate(special):
        px[k], py[k] = sx, sy
    for k, (sx, sy) in enumerate(extreme):
        px[G * G + k], py[G * G + k], mask[G * G + k] = sx, sy, True
    flow = np.stack((_norm_any(px, W).reshape(B, G, G), _norm_any(py, H).reshape(B, G, G)), 1)
    return flow, mask.reshape(B, G, G)


@functools.lru_cache(maxsize=None)
def exact_lc_case(name):
    C, H, W, G, r, grid_based, num_level, has_flow, step, vlim, flim, glim = EXACT_LC[name]
    B, K, seed = 2, (2 * r + 1) ** 2, 7100 + 10 * sorted(EXACT_LC).index(name)
    root = int(round(C ** 0.5))
    assert root * root == C
    f0 = ints((B, C, G, G), seed, flim) * F32(root)
    f1 = ints((B, C, H, W), seed + 1, vlim) * F32(step)
    gout = ints((B, K * num_level, G, G), seed + 2, glim)
    flow, extreme = lattice_flow(B, G, H, W, seed + 3) if has_flow else (None, np.zeros((B, G, G), bool))
    case = dict(f0=f0, f1=f1, flow=flow, grad_out=gout, extreme=extreme, r=r, G=G, grid_based=grid_based, num_level=num_level, shape=(B, C, H, W))
    q = 2 ** num_level  # the pixel lattice of the coarsest level
    gx, gy = tap_coords(flow, B, G, H, W, r, grid_based)
    with np.errstate(invalid="ignore"):
        for g, size in ((gx, W), (gy, H)):
            ix = unnorm(g, size >> (num_level - 1)).astype(np.float64) * q
            assert (ix[np.isfinite(ix)] == np.rint(ix[np.isfinite(ix)])).all(), f"{name}: taps off the 1/{q} pixel lattice"
    args = (f1, flow, r, G)
    kw = dict(grid_based=grid_based, num_level=num_level)
    for sm, pm in ALL_MODES:
        den = weight_den(sm, q)
        exact_budget(local_correlation(f0, *args, sm, pm, **kw), local_correlation(f0, *args, sm, pm, absolute=True, **kw), den, f"{name} {sm}/{pm}")
        # the gradient's accumulator, before the one division by sqrt_c that ends it
        exact_budget(local_correlation_grad_f0(gout, *args, sm, pm, **kw) * root, local_correlation_grad_f0(gout, *args, sm, pm, absolute=True, **kw) * root,
                     den, f"{name} grad {sm}/{pm}")
    return case


@functools.lru_cache(maxsize=None)
def exact_lc_oracle(name, sm, pm):
    c = exact_lc_case(name)
    return local_correlation(c["f0"], c["f1"], c["flow"], c["r"], c["G"], sm, pm, grid_based=c["grid_based"], num_level=c["num_level"])


@functools.lru_cache(maxsize=None)
def exact_lc_grad_oracle(name, sm, pm):
    c = exact_lc_case(name)
    return local_correlation_grad_f0(c["grad_out"], c["f1"], c["flow"], c["r"], c["G"], sm, pm, grid_based=c["grid_based"], num_level=c["num_level"])


@functools.lru_cache(maxsize=None)
def exact_route_case(r):
    """Bilinear + zeros on the tiled routes: C = 16, G = 16 on a 16 x 16 map, flows near the identity on the half-pixel lattice so
    that the tiles stage, with integer fractions at the last row and column."""
    B, C, H, W, G = 2, 16, 16, 16, 16
    seed = 7300 + r
    f0 = ints((B, C, G, G), seed, 4) * F32(4)
    f1 = ints((B, C, H, W), seed + 1, 64)
    jj, ii = np.meshgrid(np.arange(G, dtype=np.float64), np.arange(G, dtype=np.float64))
    px = jj[None] + (synth.hash_u32(B * G * G, seed + 2) % np.uint32(5)).astype(np.float64).reshape(B, G, G) / 2 - 1
    py = ii[None] + (synth.hash_u32(B * G * G, seed + 3) % np.uint32(5)).astype(np.float64).reshape(B, G, G) / 2 - 1
    px[0, :, -1], py[0, -1, :] = W - 1.0, H - 1.0  # fraction 0 with the second corner outside
    px[1, 3, 4:9], py[1, 3, 4:9] = (-9.5, 40.0, 999999.0, -1000000.0, float("nan")), (2.0, -30.5, 3.5, 4.0, 5.0)  # flagged cells
    flow = np.stack((_norm_any(px, W), _norm_any(py, H)), 1)
    want = local_correlation(f0, f1, flow, r, G, "bilinear", "zeros")
    exact_budget(want, local_correlation(f0, f1, flow, r, G, "bilinear", "zeros", absolute=True), 4, f"route r={r}")
    return dict(f0=f0, f1=f1, flow=flow, r=r, G=G, shape=(B, C, H, W), want=want)


# name: C, Hs, Ws, G, r (C = 16 with r = 1 is a shape the fused lean plan takes; C = 9 leaves the group tails; G = 4 on 8 x 16 puts the
# cell centres on the half-pixel lattice too)
EXACT_RI = {"c16_8x8_g8": (16, 8, 8, 8, 1), "c9_8x16_g4": (9, 8, 16, 4, 1), "c9_8x8_g8": (9, 8, 8, 8, 2), "c16_16x16_g16": (16, 16, 16, 16, 2)}


def ri_radius(name, sm):
    """The local-correlation radius of the case, None for no correlation planes (corr_in_other=False): bicubic with off-centre cells
    squares the 2^10 weight denominator in the correlation, which no integer data keeps under 2^24."""
    C, Hs, Ws, G, r = EXACT_RI[name]
    return None if (sm == "bicubic" and (G != Hs or G != Ws)) else r


@functools.lru_cache(maxsize=None)
def exact_ri_case(name, symmetric, extremes=False):
    """x, y = sqrt(C) * integers in [-4, 4], half-pixel flows, integer displacement weights; scale_factor 1 (disp_scale 1.25).
    extremes: the guard's surroundings among the flows (their displacement planes are huge or non-finite: `extreme` masks the cells)."""
    C, Hs, Ws, G, r = EXACT_RI[name]
    Bi, Dd, seed = 2, 6, 7200 + 10 * sorted(EXACT_RI).index(name) + (5 if symmetric else 0)
    root = int(round(C ** 0.5))
    x, y = ints((Bi, C, Hs, Ws), seed, 4) * F32(root), ints((Bi, C, Hs, Ws), seed + 1, 4) * F32(root)
    B = 2 * Bi if symmetric else Bi
    flows = [lattice_flow(B, G, Hs, Ws, seed + 2 + 2 * k, extremes=extremes) for k in range(2)]  # first call, then the `reuse` call
    dw, db = ints((Dd, 2, 1, 1), seed + 6, 2), ints((Dd,), seed + 7, 3)
    case = dict(x=x, y=y, flows=[f for f, _ in flows], extreme=[m for _, m in flows], dw=dw, db=db, G=G, C=C, Dd=Dd)
    if not extremes:
        for sm in SAMPLE_MODES:
            wd = weight_den(sm, 2)
            # grid_feature / sqrt_c carries the weights' denominator into the correlation when the centres are off the pixels; the
            # displacement is a multiple of 1.25 / size
            dens = ((0, 2 * C, wd), (2 * C, 2 * C + Dd, 8 * max(Hs, Ws)), (2 * C + Dd, None, wd * (1 if G == Hs == Ws else wd)))
            for f in case["flows"]:
                rr = ri_radius(name, sm)
                val, mag = refiner_input(x, y, f, dw, db, G, 1.0, sm, rr), refiner_input(x, y, f, dw, db, G, 1.0, sm, rr, absolute=True)
                for lo, hi, den in dens:
                    if val[:, lo:hi].size:
                        exact_budget(val[:, lo:hi], mag[:, lo:hi], den, f"refiner {name} {sm} planes {lo}:{hi}")
    return case


@functools.lru_cache(maxsize=None)
def exact_ri_oracle(name, symmetric, sm, k, extremes=False):
    c = exact_ri_case(name, symmetric, extremes)
    return refiner_input(c["x"], c["y"], c["flows"][k], c["dw"], c["db"], c["G"], 1.0, sm, ri_radius(name, sm))


# ---- the generic family ---------------------------------------------------------------------------------------------------------
def kept(g, size):
    """Both sides of every integer and half-integer by at least KEEP_DIST px."""
    t = 2.0 * unnorm(g, size).astype(np.float64)
    return np.abs(t - np.rint(t)) / 2.0 >= KEEP_DIST


def ulp(x):
    return float(np.spacing(F32(abs(x))))


def delta_px(roundings, gmax, size):
    """The coordinate allowance in pixels: `roundings` fp32 roundings of the chain, each at most one ulp of the largest intermediate
    magnitude of the case, (|g| + 1) * size."""
    return roundings * ulp((gmax + 1.0) * size)


def allowance(f, deltas):
    """S: the largest change of the oracle f(shift) when every point moves by +-delta on either axis."""
    base = f((0.0, 0.0))
    dx, dy = deltas
    return max(float(np.abs(f(s) - base).max()) for s in ((dx, 0.0), (-dx, 0.0), (0.0, dy), (0.0, -dy)))


GENERIC_MAPS = ((13, 17, 5), (13, 17, 12), (1, 7, 5), (5, 1, 12))  # H, W, C
UNNORM_ROUNDINGS = 3  # g + 1, * size, - 1 (the halving is exact)


def _uniform(shape, seed, lim):
    return np.random.RandomState(seed).uniform(-lim, lim, size=shape).astype(F32)


def _values(shape, seed, f16):
    v = synth.lattice_normalish(shape, seed)
    return v.astype(np.float16) if f16 else v


@functools.lru_cache(maxsize=None)
def generic_grid_case(H, W, C, f16):
    x = _values((2, C, H, W), 7501 + H * W + C, f16)
    grid = _uniform((2, 24, 40, 2), 7502 + H * W + C, 3.0)
    keep = kept(grid[..., 0], W) & kept(grid[..., 1], H)
    dropped = 1.0 - float(keep.mean())
    assert dropped <= MAX_DROPPED, f"generic grid {H}x{W}: {dropped:.2%} of the points within 2^-10 px of a decision"
    gmax = float(np.abs(grid).max())
    deltas = (delta_px(UNNORM_ROUNDINGS, gmax, W), delta_px(UNNORM_ROUNDINGS, gmax, H))
    assert max(deltas) < 2.0 ** -12
    return dict(x=x, grid=grid, keep=keep, dropped=dropped, deltas=deltas)


@functools.lru_cache(maxsize=None)
def generic_grid_oracle(H, W, C, f16, sm, pm):
    """(oracle, S, A) at the kept points: the float64 value (n,), the coordinate allowance, the sum of |weight * value| (n,)."""
    c = generic_grid_case(H, W, C, f16)
    x = np.asarray(c["x"], F32)
    f = lambda shift: grid_kept(grid_sample(x, c["grid"], sm, pm, shift=shift), c["keep"])
    return f((0.0, 0.0)), allowance(f, c["deltas"]), grid_kept(grid_sample(x, c["grid"], sm, pm, absolute=True), c["keep"])


def grid_kept(out, keep):
    """(B, C, Ho, Wo) -> the kept points' values (n, C)."""
    return np.moveaxis(np.asarray(out), 1, -1)[keep]


# name: C, H, W, G, r, grid_based, num_level, f16
GENERIC_LC = {
    "c5_13x17_r2": (5, 13, 17, 6, 2, False, 1, False),
    "c12_13x17_grid_based": (12, 13, 17, 9, 1, True, 1, True),
    "c5_13x17_levels2": (5, 13, 17, 7, 1, False, 2, False),
    "c5_1x7": (5, 1, 7, 5, 1, False, 1, True),
    "c12_5x1": (12, 5, 1, 6, 2, False, 1, False),
}
# 1 / (2r) division of the step, step * i, start + ., flow + ., then unnorm's three
TAP_ROUNDINGS = 4 + UNNORM_ROUNDINGS


@functools.lru_cache(maxsize=None)
def generic_lc_case(name):
    C, H, W, G, r, grid_based, num_level, f16 = GENERIC_LC[name]
    B, seed = 3, 7600 + 10 * sorted(GENERIC_LC).index(name)
    f0 = synth.lattice_normalish((B, C, G, G), seed)
    f1 = _values((B, C, H, W), seed + 1, f16)
    flow = _uniform((B, 2, G, G), seed + 2, 3.0)
    flow[B - 1] = _uniform((2, G, G), seed + 3, 1.2)  # one batch element mostly inside the map
    gout = synth.lattice_normalish((B, (2 * r + 1) ** 2 * num_level, G, G), seed + 4)
    gx, gy = tap_coords(flow, B, G, H, W, r, grid_based)
    keep = np.ones((B, G, G), bool)
    dropped = 0.0
    for lv in range(num_level):  # every tap of the cell, at each level's own map size
        k = kept(gx, W >> lv) & kept(gy, H >> lv)
        dropped = max(dropped, 1.0 - float(k.mean()))
        keep &= k.all(1)
    cells = float(keep.mean())
    assert dropped <= MAX_DROPPED, f"generic lc {name}: {dropped:.2%} of a level's taps within 2^-10 px of a decision"
    assert cells >= MIN_CELLS_KEPT, f"generic lc {name}: only {cells:.1%} of the cells keep all their taps"
    gmax = float(max(np.abs(gx).max(), np.abs(gy).max()))
    deltas = (delta_px(TAP_ROUNDINGS, gmax, W), delta_px(TAP_ROUNDINGS, gmax, H))
    assert max(deltas) < 2.0 ** -12
    return dict(f0=f0, f1=f1, flow=flow, grad_out=gout, keep=keep, cells=cells, dropped=dropped, deltas=deltas, r=r, G=G, grid_based=grid_based,
                num_level=num_level, shape=(B, C, H, W))


@functools.lru_cache(maxsize=None)
def generic_lc_oracle(name, sm, pm):
    """(oracle at the kept cells (n, K), S)."""
    c = generic_lc_case(name)
    kw = dict(grid_based=c["grid_based"], num_level=c["num_level"])
    f = lambda shift: lc_kept(local_correlation(c["f0"], np.asarray(c["f1"], F32), c["flow"], c["r"], c["G"], sm, pm, shift=shift, **kw), c["keep"])
    return f((0.0, 0.0)), allowance(f, c["deltas"])


def lc_kept(out, keep):
    """(B, K, G, G) -> the kept cells' rows (n, K)."""
    return np.moveaxis(np.asarray(out), 1, -1)[keep]
