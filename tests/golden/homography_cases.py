"""Seeded correspondence sets for the homography-solve tests (tests/test_homography_cpu.py, tests/test_homography_gpu.py):
the shapes at which csrc/homography.hip takes another branch.  Every builder returns float32 (Bt, N, 4) pixel rows (x, y, u, v)
made with make_points / random_h of tests/test_homography_cpu.py; the CPU file asserts from the oracle's output that each set
still reaches the route it is named for, the GPU file runs the kernels on it.

Constants of homography.hip restated (a route is a function of these):"""
import numpy as np

HEAD = 16        # kHeadHyp: hypotheses the head kernel solves per thread and scores itself
SCORE_GROUP = 4  # kHypPerWave: hypotheses one wave of score_kernel scores
HYP_WAVE = 8     # hypotheses one wave of hyp_kernel solves (8 lanes each)
FIN_THREADS = 512  # kFinThreads
FIN_SCAN = 2048  # kFinScan: counts the finish kernel replays per chunk
CONF = 0.99999   # estimation.py:70
S = 448


def corner_dist(Ha, Hb, size=S):
    """Mean distance of the four image corners under Ha and Hb, both in float64.  oracle.corner_error rounds its first argument to
    float32 like the reference does with its ground truth, which alone is ~1e-5 px: too coarse a ruler for two fp64 results
    that should agree to rounding."""
    c = np.array([[0, 0, 1], [0, size - 1, 1], [size - 1, 0, 1], [size - 1, size - 1, 1]], np.float64)
    a, b = c @ np.asarray(Ha, np.float64).T, c @ np.asarray(Hb, np.float64).T
    return float(np.mean(np.linalg.norm(a[:, :2] / a[:, 2:] - b[:, :2] / b[:, 2:], axis=1)))


def points(seed, Bt, N, noise, outliers):
    """Bt pairs, each with a homography of its own; `outliers` one ratio or one per pair."""
    from test_homography_cpu import make_points, random_h

    rng = np.random.default_rng(seed)
    ratios = [outliers] * Bt if np.isscalar(outliers) else list(outliers)
    assert len(ratios) == Bt
    Hs = [random_h(rng) for _ in range(Bt)]
    return Hs, np.stack([make_points(rng, H, N, noise=noise, outliers=r) for H, r in zip(Hs, ratios)])


# ---- 1. replay beyond one scan chunk: iters = 6000, seed 4 ------------------------------------------------------------------
REPLAY = {"o75": (800, 0.75), "o78": (800, 0.78), "o88": (600, 0.88)}
REPLAY_ITERS, REPLAY_SEED = 6000, 4
ARGMAX_ITERS = 4 * FIN_THREADS + 1  # 2049: every thread of the arg-max takes four counts, thread 0 a fifth


def replay(name):
    N, outliers = REPLAY[name]
    return points(4, 4, N, 0.3, outliers)


# ---- 2. ragged score groups, hypothesis waves that straddle pairs ----------------------------------------------------------------
RAGGED_ALL = (517, 2003)          # confidence 0: T % 4 == 1, T % 8 != 0
RAGGED_ADAPTIVE = (17, 19, 21, 531)  # confidence rule: (T - 16) % 4 = 1, 3, 1, 3


def ragged():
    return points(52, 5, 300, 0.3, 0.3)


# ---- 3. one batch, different fates -------------------------------------------------------------------------------------------
FATES_OUTLIERS = (0.0, 0.5, 0.8, 0.3, 0.65)
FATES_ITERS = 2000


def fates():
    """Five solvable pairs and a sixth whose rows are all identical (every minimal subset is singular)."""
    Hs, pts = points(53, 5, 400, 0.3, FATES_OUTLIERS)
    dead = np.broadcast_to(np.array([100.0, 200.0, 120.0, 180.0], np.float32), (1, 400, 4))
    return Hs, np.concatenate((pts, dead))


# ---- 4. small N on real data ----------------------------------------------------------------------------------------------------
SMALL_N = (4, 5, 7, 8, 9, 15, 33, 63, 64, 65, 127, 511, 512, 513)
SMALL_ITERS = 40


def spread(seed, Bt, N, noise):
    """Like points(), but row k lies in quadrant k % 4 of image A, 40 px clear of the centre lines: even four or five rows span
    the image, so a tiny set is as well conditioned as a large one (tests/test_homography_cpu.py measures it) and a bound in
    pixels at the image corners means what it means at N = 5000."""
    from test_homography_cpu import make_points, random_h

    rng = np.random.default_rng(seed)
    Hs, out = [], []
    q = np.arange(N) % 4
    corner = np.stack(((q % 2) * (S / 2 + 39), (q // 2) * (S / 2 + 39)), -1)
    for _ in range(Bt):
        H = random_h(rng)
        a = rng.uniform(0, S / 2 - 40, size=(N, 2)) + corner
        Hs.append(H)
        out.append(make_points(rng, H, N, noise=noise, a=a))
    return Hs, np.stack(out)


def small(N):
    """Four pairs of N spread correspondences, 0.2 px noise; from N = 8 up the first N // 4 rows are pushed 40 px away."""
    Hs, pts = spread(1000 + N, 4, N, 0.2)
    if N >= 8:
        pts[:, : N // 4, 2:] += np.float32(40.0)
    return Hs, pts


def one_ulp_up(pts):
    """Every coordinate moved to the next float32: the input's own resolution, for the sensitivity of a solve."""
    return np.nextafter(pts, np.float32(np.inf), dtype=np.float32)


# ---- 6. confidence 0.5: bounds that shrink to different values within a batch ----------------------------------------------
def half_confidence():
    return ragged()


# ---- 7. weighted DLT ---------------------------------------------------------------------------------------------------------------
DLT_N = (4, 5, 64, 511, 512, 513, 1025)


def dlt(N):
    """Three noise-free pairs; spread rows, so that N = 4 determines H as well as float32 coordinates allow."""
    return spread(2000 + N, 3, N, 0.0)


# ---- 8. hostile rows among the outliers --------------------------------------------------------------------------------------
HOSTILE_ROWS = 15


def hostile():
    """N = 1000, 0.4 px noise, 30 % outliers (the first 300 rows); among them five rows with a NaN, five with +inf and five with
    1e30 in one coordinate, the coordinate cycling x, y, u, v.  Returns (Hs, clean, hostile)."""
    Hs, pts = points(58, 4, 1000, 0.4, 0.3)
    bad = pts.copy()
    for b in range(4):
        rows = 7 + 19 * np.arange(HOSTILE_ROWS) + b  # all below 300
        for i, (r, value) in enumerate(zip(rows, [np.nan] * 5 + [np.inf] * 5 + [1e30] * 5)):
            bad[b, r, (i + b) % 4] = value
    return Hs, pts, bad
