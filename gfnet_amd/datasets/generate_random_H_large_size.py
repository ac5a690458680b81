"""datasets/generate_random_H_large_size.py of the reference (random_four_points :6-36, randomH :38-85) on csrc/pair_synth.hip.

The reference draws its random integers with `torch.randint(lo, hi, size=(1,))` in the middle of the image arithmetic, per sample
on host workers.  Here the draws are made first (`draw_random_h`: the same calls in the same order, so one sample under a seed
consumes the generator exactly as the reference does) and everything after them runs on the device for the whole batch
(`gfnet_amd.ops.random_h_batch`).  `reference_random_h` restates the reference's chain with torch on the CPU, in any dtype, from
explicit draws: the tests' oracle.  It restates kornia's published definitions (the 8 x 8 system of get_perspective_transform,
transform_points, the align_corners=True bilinear warp with zeros padding in pixel coordinates) and is NOT pinned against kornia
itself, which is not a dependency of this package.
"""
import torch
import torch.nn.functional as F

from .. import ops

IMAGENET_MEAN, IMAGENET_STD = ops.IMAGENET_MEAN, ops.IMAGENET_STD


def _randint(lo, hi, generator):
    return int(torch.randint(lo, hi, size=(1,), generator=generator))


def draw_random_h(n, w, h, crop_size, deform_area, generator=None):
    """The random integers of n calls of randomH on (pre-resized) images of width w and height h (ints, or one per sample):
    (n,18) int32 on the CPU, per sample crop_x, crop_y (:50-51), then random_four_points' draws for image 1 and for image 2 (:59-60),
    each tl x,y; tr x,y; br x,y; bl x,y (:7-22) on the crop_size x crop_size crop.  Image 2's eight are drawn for bi=False too, as the
    reference draws them."""
    ws = [int(w)] * n if isinstance(w, int) else [int(v) for v in w]
    hs = [int(h)] * n if isinstance(h, int) else [int(v) for v in h]
    if len(ws) != n or len(hs) != n:
        raise ValueError(f"draw_random_h: {n} samples, {len(ws)} widths, {len(hs)} heights")
    out = torch.empty((n, 18), dtype=torch.int32)
    c, d = int(crop_size), int(deform_area)
    for i in range(n):
        row = [_randint(0, ws[i] - c, generator), _randint(0, hs[i] - c, generator)]
        for _ in range(2):
            row += [_randint(0, d, generator), _randint(0, d, generator),              # topleft
                    _randint(c - d, c, generator), _randint(0, d, generator),          # topright
                    _randint(c - d, c, generator), _randint(c - d, c, generator),      # botright
                    _randint(0, d, generator), _randint(c - d, c, generator)]          # botleft
        out[i] = torch.tensor(row, dtype=torch.int32)
    return out


def pre_resize_size(h, w, crop_size):
    """:45-48 -- None when a (h, w) image holds the crop, else the size torchvision's Resize(crop_size + 10) gives it: the short side
    to crop_size + 10, the long side int(size * long / short)."""
    if w > crop_size and h > crop_size:
        return None
    size = crop_size + 10
    if w <= h:
        return int(size * h / w), size
    return size, int(size * w / h)


def pre_resize(img, crop_size):
    """:45-48 on the device: bicubic, no antialiasing (gfnet_amd.ops.resize_normalise with mean 0 / std 1), only where needed"""
    size = pre_resize_size(img.shape[1], img.shape[2], crop_size)
    if size is None:
        return img
    return ops.resize_normalise(img[None], size, "bicubic", (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))[0]


def randomH(img1, img2, crop_size, input_size, deformation_ratio=0.33, bi=True, generator=None):
    """The reference's randomH for one pair of (3,h,w) device images in [0,1]; input_size is the final (h, w) pair (the reference
    passes a torchvision Resize).  Returns, in the reference's order (:85), (img2, img1, H_s2t, warped_src): img1 warped by H_1t is
    the SECOND value -- the dataset assigns the tuple to `img0, img1` (homography_dataset_large_size.py:176) and hands them out as
    im_B, im_A, so H_s2t (3,3) float32 maps pixels of the second value to pixels of the first; warped_src is the second value warped
    by H_s2t.  Images are not normalised, as in the reference."""
    if img1.shape != img2.shape:
        raise ValueError(f"randomH: the images differ in shape: {tuple(img1.shape)} and {tuple(img2.shape)}")
    img1, img2 = pre_resize(img1, crop_size), pre_resize(img2, crop_size)
    deform_area = int(crop_size * deformation_ratio)
    draws = draw_random_h(1, img1.shape[2], img1.shape[1], crop_size, deform_area, generator)
    out = ops.random_h_batch([img1], [img2], draws, crop_size, input_size, deformation_ratio, bi, normalize=False, return_warped=True)
    return out["im_B"][0], out["im_A"][0], out["H_s2t"][0], out["warped_img1"][0]


# ---- the oracle: the same chain on the CPU ------------------------------------------------------------------------------------------
def _inv3(m):
    """adjugate / determinant, as the kernels invert: exact for the identity and for integer translations"""
    a = m.reshape(9)
    c = torch.stack([a[4] * a[8] - a[5] * a[7], a[2] * a[7] - a[1] * a[8], a[1] * a[5] - a[2] * a[4],
                     a[5] * a[6] - a[3] * a[8], a[0] * a[8] - a[2] * a[6], a[2] * a[3] - a[0] * a[5],
                     a[3] * a[7] - a[4] * a[6], a[1] * a[6] - a[0] * a[7], a[0] * a[4] - a[1] * a[3]])
    det = (a[0] * c[0] + a[1] * c[3]) + a[2] * c[6]
    return (c / det).reshape(3, 3)


def reference_perspective_transform(src, dst):
    """kornia's get_perspective_transform for one problem: src, dst (4,2) -> (3,3) in their dtype, torch.linalg.solve on the 8 x 8
    system with rows [x y 1 0 0 0 -xu -yu | u] and [0 0 0 x y 1 -xv -yv | v]"""
    one, zero = torch.ones_like(src[:, 0]), torch.zeros_like(src[:, 0])
    x, y, u, v = src[:, 0], src[:, 1], dst[:, 0], dst[:, 1]
    ax = torch.stack([x, y, one, zero, zero, zero, -x * u, -y * u], dim=1)
    ay = torch.stack([zero, zero, zero, x, y, one, -x * v, -y * v], dim=1)
    A = torch.stack([ax, ay], dim=1).reshape(8, 8)
    rhs = torch.stack([u, v], dim=1).reshape(8)
    sol = torch.linalg.solve(A, rhs)
    return torch.cat([sol, torch.ones(1, dtype=src.dtype)]).reshape(3, 3)


def reference_transform_points(H, pts):
    """kornia's transform_points: (n,2) points through H, the homogeneous divide as a multiplication by 1 / z (by 1 where
    |z| <= 1e-8)"""
    ph = torch.cat([pts, torch.ones_like(pts[:, :1])], dim=1) @ H.T
    z = ph[:, 2:]
    scale = torch.where(z.abs() > 1e-8, 1.0 / z, torch.ones_like(z))
    return ph[:, :2] * scale


def reference_sample(img, x, y):
    """Bilinear samples of img (C,H,W) at pixel coordinates x, y (any shape), a neighbour outside the image counting as 0; the blend
    in the kernels' order"""
    _, H, W = img.shape
    x0, y0 = torch.floor(x), torch.floor(y)
    fx, fy = x - x0, y - y0
    finite = torch.isfinite(x) & torch.isfinite(y)

    def tap(xi, yi):
        ok = finite & (xi >= 0) & (xi <= W - 1) & (yi >= 0) & (yi <= H - 1)
        xi, yi = torch.where(ok, xi, torch.zeros_like(xi)).long(), torch.where(ok, yi, torch.zeros_like(yi)).long()
        return torch.where(ok, img[:, yi, xi], torch.zeros((), dtype=img.dtype))

    fx, fy = torch.where(finite, fx, torch.zeros_like(fx)), torch.where(finite, fy, torch.zeros_like(fy))
    v00, v01, v10, v11 = tap(x0, y0), tap(x0 + 1, y0), tap(x0, y0 + 1), tap(x0 + 1, y0 + 1)
    return (1 - fy) * ((1 - fx) * v00 + fx * v01) + fy * ((1 - fx) * v10 + fx * v11)


def reference_warp_by_map(img, M, dsize):
    """out[:, v, u] = img sampled at M (u, v, 1) with a plain divide by the third coordinate: what gfn_warp_perspective_fwd
    computes, in the dtype of img"""
    Ho, Wo = dsize
    v, u = torch.meshgrid(torch.arange(Ho, dtype=img.dtype), torch.arange(Wo, dtype=img.dtype), indexing="ij")
    X = (M[0, 0] * u + M[0, 1] * v) + M[0, 2]
    Y = (M[1, 0] * u + M[1, 1] * v) + M[1, 2]
    Z = (M[2, 0] * u + M[2, 1] * v) + M[2, 2]
    return reference_sample(img, X / Z, Y / Z)


def reference_warp(img, H, dsize):
    """kornia's warp_perspective(img, H, dsize, align_corners=True) with bilinear sampling and zeros padding: the destination grid
    through H^-1 (transform_points), sampled in pixel coordinates"""
    Ho, Wo = dsize
    v, u = torch.meshgrid(torch.arange(Ho, dtype=img.dtype), torch.arange(Wo, dtype=img.dtype), indexing="ij")
    p = reference_transform_points(_inv3(H), torch.stack([u.reshape(-1), v.reshape(-1)], dim=1))
    return reference_sample(img, p[:, 0].reshape(Ho, Wo), p[:, 1].reshape(Ho, Wo))


def _resize_bicubic(img, size):
    return F.interpolate(img[None], size=tuple(size), mode="bicubic", align_corners=False)[0]


def reference_random_h(img1, img2, draws, crop_size, input_size, deformation_ratio=0.33, bi=True, dtype=torch.float64, normalize=False):
    """randomH (:38-85) followed by the dataset's Normalize (homography_dataset_large_size.py:184-185) restated with torch on the
    CPU in `dtype`, step by step as the reference takes them (pre-resize, crop, two warps at crop size, centre crops, H_1t2t, the
    corner flow, H_s2t, final resize and the rescale of :77-79, the third warp), from the 18 explicit draws of one sample.  bi=False
    takes H_2t as the identity (the solve of src == dst).  No GPU call.  Returns a dict: im_A (img1 under H_1t), im_B (img2 under
    H_2t), H_s2t, warped_img1 (the un-normalised im_A warped by H_s2t), and M_A, M_B: the output-pixel -> source-pixel maps
    translate(crop) H_it^-1 translate(deform_area // 2) that the device composes (before the final resize)."""
    img1, img2 = img1.detach().cpu().to(dtype), img2.detach().cpu().to(dtype)
    d = [int(v) for v in torch.as_tensor(draws).reshape(18).tolist()]
    size = pre_resize_size(img1.shape[1], img1.shape[2], crop_size)
    if size is not None:
        img1, img2 = _resize_bicubic(img1, size), _resize_bicubic(img2, size)
    cx, cy = d[0], d[1]
    img1, img2 = img1[:, cy:cy + crop_size, cx:cx + crop_size], img2[:, cy:cy + crop_size, cx:cx + crop_size]
    w = h = crop_size
    deform_area = int(w * deformation_ratio)
    d2 = deform_area // 2
    tgt = torch.tensor([[d2, d2], [w - d2 - 1, d2], [w - d2 - 1, h - d2 - 1], [d2, h - d2 - 1]], dtype=dtype)

    def four_points(img, corners, two_way):
        H = reference_perspective_transform(torch.tensor(corners, dtype=dtype).reshape(4, 2), tgt) if two_way else torch.eye(3, dtype=dtype)
        return H, reference_warp(img, H, (h, w))[:, d2:h - d2, d2:w - d2]

    H_1t, img1 = four_points(img1, d[2:10], True)
    H_2t, img2 = four_points(img2, d[10:18], bi)
    H_1t2t = H_2t @ _inv3(H_1t)
    flow = reference_transform_points(H_1t2t, tgt) - tgt
    _, hc, wc = img1.shape
    src = torch.tensor([[0, 0], [wc - 1, 0], [wc - 1, hc - 1], [0, hc - 1]], dtype=dtype)
    H_s2t = reference_perspective_transform(src, src + flow)
    T = lambda x, y: torch.tensor([[1, 0, x], [0, 1, y], [0, 0, 1]], dtype=dtype)  # noqa: E731
    M_A, M_B = T(cx, cy) @ _inv3(H_1t) @ T(d2, d2), T(cx, cy) @ _inv3(H_2t) @ T(d2, d2)
    h_in, w_in = int(input_size[0]), int(input_size[1])
    if h_in != hc or w_in != wc:
        img1, img2 = _resize_bicubic(img1, (h_in, w_in)), _resize_bicubic(img2, (h_in, w_in))
        left = torch.diag(torch.tensor([h_in / hc, h_in / hc, 1.0], dtype=dtype))
        right = torch.diag(torch.tensor([1.0, 1.0, 1.0], dtype=dtype) / torch.tensor([w_in / wc, w_in / wc, 1.0], dtype=dtype))
        H_s2t = left @ H_s2t @ right
    warped = reference_warp(img1, H_s2t, (h_in, w_in))
    if normalize:
        mean, std = torch.tensor(IMAGENET_MEAN, dtype=dtype)[:, None, None], torch.tensor(IMAGENET_STD, dtype=dtype)[:, None, None]
        img1, img2 = (img1 - mean) / std, (img2 - mean) / std
    return {"im_A": img1, "im_B": img2, "H_s2t": H_s2t, "warped_img1": warped, "M_A": M_A, "M_B": M_B}
