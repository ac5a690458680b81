"""Seeded point sets for the KDE tests (tests/test_kde_cpu.py, tests/test_kde_gpu.py): (N, 4) float32 rows
(A-image x, y, B-image x, y), the shapes on which a streaming / culled density kernel can go wrong."""
import numpy as np

IDENTICAL = np.array([0.05, -0.03, 0.02, 0.04], np.float32)  # near the origin: a padding point at 0 would be 0.4 std away


def curve_key16(pts):
    """Restatement of curve_key16 in csrc/kde.hip: 16-bit Hilbert position of the A-image coordinates, 8 bits per axis, fp32
    arithmetic, clamped (fmaxf / fminf drop a NaN: it lands in cell 0)."""
    pts = np.asarray(pts, np.float32)
    keys = np.empty(len(pts), np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        cell = (pts[:, :2] + np.float32(1)) * np.float32(128)
    for i, (cx, cy) in enumerate(cell):
        x = 0 if np.isnan(cx) else int(min(max(float(cx), 0.0), 255.0))
        y = 0 if np.isnan(cy) else int(min(max(float(cy), 0.0), 255.0))
        d, s = 0, 128
        while s > 0:
            rx, ry = int(bool(x & s)), int(bool(y & s))
            d += s * s * ((3 * rx) ^ ry)
            if not ry:
                if rx:
                    x, y = 255 - x, 255 - y
                x, y = y, x
            s >>= 1
        keys[i] = d
    return keys


def _match(rng, N, extent=1.0, outliers=0.0):
    a = rng.uniform(-extent, extent, size=(N, 2))
    b = np.stack([0.85 * a[:, 0] + 0.1 * a[:, 1] + 0.05 * extent, -0.08 * a[:, 0] + 0.9 * a[:, 1] - 0.03 * extent], -1)
    b += 0.01 * rng.standard_normal(b.shape)
    k = int(round(outliers * N))
    if k:
        b[rng.permutation(N)[:k]] = rng.uniform(-extent, extent, size=(k, 2))
    return np.concatenate((a, b), -1)


def satellite_distance(std, term):
    """distance at which one Gaussian term equals `term`"""
    return std * np.sqrt(2.0 * np.log(1.0 / term))


def make(geom, N, seed=0, std=0.1):
    """One point set.  geom:
    match / outliers  A uniform over the image, B a near-affine image of A + noise; 30 % of the B positions random
    identical         N copies of one point (density = M exactly in the difference form)
    kfold             every distinct point five times, shuffled
    clusters32        runs of 32 near-identical points inside Hilbert cells 9 std apart: after the sort every 32-point
                      tile is one cluster, and a tile that is tested with its neighbour's box loses its whole density
    line / lattice    exact distance ties (multiples of 1/64 and 1/8)
    one_cell          every A position in one Hilbert cell (all keys equal: the sort must keep the order, no compaction)
    outside           every A position outside [-1, 1] (keys clamp to the border cells, boxes overlap)
    extent<E>         match-like over [-E, E] (extent3, extent10, extent1.6, ...)
    satellite         N - 1 copies of one point and a last point on the far end of the curve whose N - 1 cross terms are
                      0.9 * 2^-26 each: they reach it through the symmetric kernel's fixed-point column sums only, in pieces
                      of 64 terms (6e-7), and add up to 2.7e-4 of its density at N = 20000
    """
    rng = np.random.default_rng(1000 + seed)
    if geom == "match":
        x = _match(rng, N)
    elif geom == "outliers":
        x = _match(rng, N, outliers=0.3)
    elif geom == "identical":
        x = np.tile(IDENTICAL, (N, 1))
    elif geom == "kfold":
        base = _match(rng, (N + 4) // 5)
        x = np.repeat(base, 5, axis=0)[:N][rng.permutation(N)]
    elif geom == "clusters32":
        nc = (N + 31) // 32
        ids = rng.permutation(225)[np.arange(nc) % 225]  # 9 A cells x 25 B positions, all >= 0.896 = 9 std apart
        grid_a = np.array([-0.9, 0.004, 0.9])            # each well inside one Hilbert cell (cells 12, 128, 243)
        grid_b = np.array([-1.8, -0.9, 0.0, 0.9, 1.8])
        centres = np.stack((grid_a[ids % 3], grid_a[(ids // 3) % 3], grid_b[(ids // 9) % 5], grid_b[ids // 45]), -1)
        # the rows of a cluster stay consecutive: the stable sort keeps them together, one cluster per 32-point tile
        x = np.repeat(centres, 32, axis=0)[:N] + 1e-3 * rng.uniform(-1, 1, size=(N, 4))
    elif geom == "line":
        t = (np.arange(N) % 128) / 64.0 - 1.0
        x = np.stack((t, 0.5 * t, -t, 0.25 + 0 * t), -1)
    elif geom == "lattice":
        i = np.arange(N)
        a = np.stack(((i % 16) / 8.0 - 1.0, ((i // 16) % 16) / 8.0 - 1.0), -1)
        x = np.concatenate((a, 0.5 * a), -1)
    elif geom == "one_cell":
        a = 0.25 + rng.uniform(0.0005, 0.007, size=(N, 2))  # cell [0.25, 0.2578)
        x = np.concatenate((a, rng.uniform(-1, 1, size=(N, 2))), -1)
    elif geom == "outside":
        a = rng.uniform(1.05, 1.6, size=(N, 2)) * rng.choice([-1.0, 1.0], size=(N, 2))
        x = np.concatenate((a, 0.6 * a + 0.01 * rng.standard_normal((N, 2))), -1)
    elif geom.startswith("extent"):
        x = _match(rng, N, extent=float(geom[6:]))
    elif geom == "satellite":
        d = satellite_distance(std, 0.9 * 2.0 ** -26)
        cloud = np.array([0.99 - d, -0.99, 0.3, 0.3])
        x = np.tile(cloud, (N, 1))
        x[N - 1] = [0.99, -0.99, 0.3, 0.3]  # Hilbert position 65535 side of the curve: sorts last
    else:
        raise ValueError(geom)
    return np.ascontiguousarray(x, dtype=np.float32)
