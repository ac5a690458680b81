"""Homography-solve oracle on known-H synthetic correspondences.

The reference's solver is cv2.findHomography (absent; parity with OpenCV unpinned -- see
oracle/homography_oracle.c).  These tests pin the restated pipeline by ground truth instead:
noise-free correspondences must give the true H to < 1e-3 px corner error, the weighted DLT must
agree with an independent numpy-SVD DLT, RANSAC must survive 40 % outliers."""
import numpy as np
import pytest

import homography_cases as cases
import oracle

S = 448


def random_h(rng, size=S, amp=0.15):
    """4-corner perturbation homography (same family as datasets/generate_random_H_large_size.py:6-36)."""
    src = np.array([[0, 0], [size - 1, 0], [size - 1, size - 1], [0, size - 1]], np.float64)
    dst = src + rng.uniform(-amp * size, amp * size, size=(4, 2))
    A = []
    for (x, y), (u, v) in zip(src, dst):
        A.append([x, y, 1, 0, 0, 0, -u * x, -u * y, -u])
        A.append([0, 0, 0, x, y, 1, -v * x, -v * y, -v])
    _, _, Vt = np.linalg.svd(np.array(A))
    H = Vt[-1].reshape(3, 3)
    return H / H[2, 2]


def make_points(rng, H, n, noise=0.0, outliers=0.0, size=S, a=None):
    """n correspondences under H; `a` (n, 2): given A-image positions instead of uniform ones."""
    if a is None:
        a = rng.uniform(0, size - 1, size=(n, 2))
    ah = np.c_[a, np.ones(n)] @ H.T
    b = ah[:, :2] / ah[:, 2:]
    b = b + noise * rng.standard_normal((n, 2))
    k = int(outliers * n)
    if k:
        b[:k] = rng.uniform(0, size - 1, size=(k, 2))
    return np.c_[a, b].astype(np.float32)


def ace(Ha, Hb):
    return oracle.corner_error(Ha, Hb, S, S, clamp=1e9)


def test_dlt_noise_free_recovers_h():
    rng = np.random.default_rng(1)
    Hs = [random_h(rng) for _ in range(4)]
    pts = np.stack([make_points(rng, H, 500) for H in Hs])
    Hest, ok = oracle.homography_dlt(pts)
    assert ok.all()
    for H, He in zip(Hs, Hest):
        # float32 input coordinates limit this to ~1e-4 px
        assert ace(H.astype(np.float32), He) < 1e-3


def test_dlt_matches_numpy_svd_on_noisy_weighted_points():
    rng = np.random.default_rng(2)
    H = random_h(rng)
    pts = make_points(rng, H, 800, noise=0.7)
    w = rng.uniform(0.1, 1.0, size=800)
    He, ok = oracle.homography_dlt(pts[None], w[None])
    assert ok[0]
    # the oracle follows OpenCV's per-axis mean-abs-deviation normalisation, the cross-check uses
    # Hartley's isotropic one: same algebraic minimiser up to the normalisation -> close, not equal
    assert ace(oracle.homography_dlt_svd(pts, w), He[0]) < 0.05
    # unweighted, noise-free: both are exact
    pts0 = make_points(rng, H, 300)
    He0, _ = oracle.homography_dlt(pts0[None])
    assert ace(oracle.homography_dlt_svd(pts0), He0[0]) < 1e-3


def test_ransac_with_outliers_and_noise():
    rng = np.random.default_rng(3)
    Hs = [random_h(rng) for _ in range(3)]
    pts = np.stack([make_points(rng, H, 2000, noise=0.5, outliers=0.4) for H in Hs])
    Hest, ninl, best, mask = oracle.homography_ransac(pts, thresh=3.0, iters=500, seed=7, return_mask=True)
    for b, H in enumerate(Hs):
        assert best[b] >= 0 and ninl[b] > 1100
        assert mask[b].sum() == ninl[b]
        assert ace(H, Hest[b]) < 0.25  # 0.5 px noise on 1200 inliers
    # stages: LM must not be worse than the inlier DLT in reprojection error
    Hd, _, _ = oracle.homography_ransac(pts, thresh=3.0, iters=500, seed=7, stage=2)

    def rms(H, p, m):
        ph = np.c_[p[:, :2], np.ones(len(p))] @ H.T
        return np.sqrt((((ph[:, :2] / ph[:, 2:]) - p[:, 2:]) ** 2).sum(1)[m.astype(bool)].mean())

    for b in range(3):
        assert rms(Hest[b], pts[b], mask[b]) <= rms(Hd[b], pts[b], mask[b]) + 1e-9


def test_ransac_is_deterministic_in_seed_and_noise_free_exact():
    rng = np.random.default_rng(4)
    H = random_h(rng)
    pts = make_points(rng, H, 1000)[None]
    H1, n1, b1 = oracle.homography_ransac(pts, iters=64, seed=11)
    H2, n2, b2 = oracle.homography_ransac(pts, iters=64, seed=11)
    np.testing.assert_array_equal(H1, H2)
    assert n1[0] == 1000 and b1[0] == b2[0] == 0  # every hypothesis is perfect: the first one wins ties
    assert ace(H.astype(np.float32), H1[0]) < 1e-3
    H3, _, b3 = oracle.homography_ransac(pts, iters=64, seed=12)
    assert b3[0] == 0


def test_failure_convention_diag001():
    # fewer than 4 points / all-degenerate input -> H = diag(0,0,1) (estimation.py:74-76)
    pts = np.zeros((1, 3, 4), np.float32)
    H, n, b = oracle.homography_ransac(pts, iters=16)
    np.testing.assert_array_equal(H[0], np.diag([0.0, 0.0, 1.0]))
    assert b[0] == -1
    pts = np.ones((1, 50, 4), np.float32)  # all points identical: every 4-point system is singular
    H, n, b = oracle.homography_ransac(pts, iters=16)
    np.testing.assert_array_equal(H[0], np.diag([0.0, 0.0, 1.0]))


def test_convert_matches_is_float32_numpy_formula():
    rng = np.random.default_rng(5)
    m = rng.uniform(-1, 1, size=(100, 4)).astype(np.float32)
    pts = oracle.convert_matches(m, 640, 480, 320, 200)
    pa, pb = oracle.convert_coordinates(m[:, :2], m[:, 2:], 640, 480, 320, 200)
    np.testing.assert_array_equal(pts[:, :2], pa.astype(np.float32))
    np.testing.assert_array_equal(pts[:, 2:], pb.astype(np.float32))


def test_iteration_bound_follows_opencv_rule():
    """cv::RANSACUpdateNumIters(confidence = 0.99999, modelPoints = 4): the loop stops at log(1e-5) / log(1 - w^4) once a
    hypothesis with inlier ratio w has been seen (estimation.py:66-72 passes that confidence)."""
    rng = np.random.default_rng(3)
    H = random_h(rng, 448)
    for outl, expect in ((0.0, 1), (0.3, 42), (0.6, 444)):
        pts = make_points(rng, H, 4000, noise=0.0, outliers=outl)[None]
        _, n, b, used = oracle.homography_ransac(pts, iters=2000, seed=9, return_iters=True)
        w = n[0] / 4000.0
        bound = np.log(1e-5) / np.log(1 - w ** 4) if w < 1 else 0
        assert abs(int(used[0]) - max(int(round(bound)), 0)) <= 1 or used[0] == 2000, (outl, used, bound)
        assert abs(used[0] - expect) <= 0.35 * expect + 2, (outl, used)
        assert 0 <= b[0] < max(used[0], 1)
    # confidence 0: every hypothesis is scored
    _, _, _, used = oracle.homography_ransac(pts, iters=300, seed=9, confidence=0, return_iters=True)
    assert used[0] == 300


# ---- the seeded sets of tests/golden/homography_cases.py: each must keep reaching the route of homography.hip it is named for ----
# (tests/test_homography_gpu.py runs the kernels on them; a generator change that silently leaves a route fails here, without a GPU)
def _used(pts, **kw):
    return oracle.homography_ransac(pts, return_iters=True, **kw)


@pytest.mark.parametrize("name", list(cases.REPLAY))
def test_cases_replay_reaches_later_scan_chunks(name):
    _, pts = cases.replay(name)
    _, n, b, used = _used(pts, iters=cases.REPLAY_ITERS, seed=cases.REPLAY_SEED, confidence=cases.CONF)
    assert cases.REPLAY_ITERS > 2 * cases.FIN_SCAN and (b >= 0).all()
    if name == "o88":  # 12 % inliers: the bound never shrinks, winners fall in the second and third chunk
        assert (used == cases.REPLAY_ITERS).all() and (b >= cases.FIN_SCAN).sum() >= 2, (used, b)
    else:  # 25 % / 22 %: the bound ends between 2048 and 6000, after the winner
        assert ((used > cases.FIN_SCAN) & (used < cases.REPLAY_ITERS)).all() and (b < cases.FIN_SCAN).all(), (used, b)


def test_cases_ragged_and_half_confidence():
    _, pts = cases.ragged()
    assert all(T % cases.SCORE_GROUP and T % cases.HYP_WAVE for T in cases.RAGGED_ALL)
    for T in cases.RAGGED_ADAPTIVE:
        assert (T - cases.HEAD) % cases.SCORE_GROUP in (1, 3) and (T - cases.HEAD) % cases.HYP_WAVE
        used = _used(pts, iters=T, seed=4, confidence=cases.CONF)[3]
        # short loops keep their bound (the ragged tail group runs); at 531 it ends behind the head, long before the pair's last wave
        assert (used == T).all() if T < 32 else ((used > cases.HEAD) & (used < T - cases.HYP_WAVE)).all(), (T, used)
    used = _used(cases.half_confidence()[1], iters=2000, seed=4, confidence=0.5)[3]
    assert (used < 2000).all() and len(set(used.tolist())) >= 3, used


def test_cases_fates_mix_every_bound_and_a_failure():
    _, pts = cases.fates()
    H, n, b, used = _used(pts, iters=cases.FATES_ITERS, seed=4, confidence=cases.CONF)
    assert (used < cases.HEAD).any() and ((used >= cases.HEAD) & (used < cases.FATES_ITERS)).any() and (used[:5] == cases.FATES_ITERS).any(), used
    assert b[5] == -1 and n[5] == 0 and used[5] == cases.FATES_ITERS and (b[:5] >= 0).all()
    np.testing.assert_array_equal(H[5], np.diag([0.0, 0.0, 1.0]))
    assert ((b[:5] >= cases.HEAD).sum() >= 2) and ((b[:5] < cases.HEAD).sum() >= 2)  # winners from the head and from behind it


@pytest.mark.parametrize("N", cases.SMALL_N)
def test_cases_small_sets_are_well_conditioned(N):
    """One float32 ulp on every coordinate moves the oracle's H by less than 1e-4 px at the corners: a tenth of the 1e-3 px the
    device is held to on these sets, so that bound measures the kernels and not the conditioning of a tiny set."""
    Hs, pts = cases.small(N)
    for confidence in (0.0, cases.CONF):
        kw = dict(iters=cases.SMALL_ITERS, seed=4, confidence=confidence)
        for stage in (2, 0):
            H, n, b, used = _used(pts, stage=stage, **kw)
            H1, n1, b1, _ = _used(cases.one_ulp_up(pts), stage=stage, **kw)
            np.testing.assert_array_equal(b, b1)
            np.testing.assert_array_equal(n, n1)
            assert max(ace(H[i], H1[i]) for i in range(4)) < 1e-4, (N, confidence, stage)
        assert (b >= 0).all()
        if N == 4:
            assert (n == 4).all()  # `cnt == 4`: the hypothesis is returned as it is
        elif N < 16:
            assert ((n >= 5) & (n <= 12)).all(), n  # DLT + LM on a handful of inliers
        if confidence > 0:
            assert (used == 0).all() if N < 8 else ((used > cases.HEAD) & (used < cases.SMALL_ITERS)).all(), used


def test_cases_hostile_rows_change_nothing_for_the_oracle():
    """Rows outside the inlier mask are skipped, and a row that is not finite is never inside it (an infinite x or y makes both
    sides of the inlier test +inf): NaN, inf and 1e30 among the outliers leave the mask and H of the clean set."""
    Hs, clean, bad = cases.hostile()
    for confidence in (0.0, cases.CONF):
        kw = dict(iters=2000, seed=4, confidence=confidence, return_mask=True)
        H, n, b, m = oracle.homography_ransac(bad, **kw)
        Hc, nc, bc, mc = oracle.homography_ransac(clean, **kw)
        np.testing.assert_array_equal(m, mc)
        np.testing.assert_array_equal(b, bc)
        assert not m[:, :300].any() and (n == 700).all()
        np.testing.assert_array_equal(H, Hc)
        assert max(ace(Hs[i], H[i]) for i in range(4)) < 0.5
    # the inlier test itself: rows with x = +inf beside 40 inliers.  Both sides of the test are +inf for the row whose signs of u
    # and v match those of the winner's h31 and h21 (the others give inf - inf = NaN), so all four sign pairs: none may count
    row = np.array([[np.inf, 10.0, su * 5.0, sv * 10.0] for su in (1, -1) for sv in (1, -1)] * 2, np.float32)
    pts = np.concatenate((bad[0, 300:340], row))[None]
    _, n, b, m = oracle.homography_ransac(pts, iters=50, seed=1, confidence=0.0, return_mask=True)
    assert b[0] >= 0 and not m[0, 40:].any()


def test_cases_dlt_sets():
    for N in cases.DLT_N:
        Hs, pts = cases.dlt(N)
        H, ok = oracle.homography_dlt(pts)
        assert ok.all() and max(ace(Hs[i].astype(np.float32), H[i]) for i in range(3)) < (1e-3 if N < 64 else 1e-4), N
    # zero weight == row dropped, for the oracle too
    Hs, pts = cases.dlt(513)
    w = np.random.default_rng(71).uniform(0.1, 1.0, size=(3, 513))
    w[:, ::3] = 0
    keep = np.arange(513) % 3 != 0
    Hz, _ = oracle.homography_dlt(pts, w)
    Hd, _ = oracle.homography_dlt(pts[:, keep], w[:, keep])
    assert max(cases.corner_dist(Hz[i], Hd[i]) for i in range(3)) < 1e-6
    H0, ok0 = oracle.homography_dlt(pts, np.zeros((3, 513)))
    assert not ok0.any()
    np.testing.assert_array_equal(H0[0], np.diag([0.0, 0.0, 1.0]))
