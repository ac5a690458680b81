"""Every launch route of csrc/homography.hip against the float64 oracle (oracle/homography_oracle.c, pinned by
tests/test_homography_cpu.py) and, where stated, the known H.  The inputs are the seeded sets of tests/golden/homography_cases.py;
each test asserts from the ORACLE's output that its set reaches the route it is there for.

Routes (constants of homography.hip restated in homography_cases):
  head        confidence > 0: ransac_head_kernel solves hypotheses 0..15 one per thread and sets bound[b]
  tail        hyp_kernel (8 lanes per hypothesis, ge_solve8.h) + score_kernel (4 hypotheses per wave) for 16 <= t < bound[b];
              for every t when confidence == 0
  replay      finish_kernel walks the counts in chunks of 2048 (confidence > 0) or takes the arg-max (confidence == 0)
  finish      mask, DLT on the inliers, LM; `cnt == 4` returns the hypothesis, `best < 0` returns diag(0,0,1)
  dlt         finish_kernel in weighted one-shot mode

"Equal to the oracle" (check()): chosen hypothesis, inlier count, mask and iteration bound are identical; the stage-1 H (the
4-point hypothesis) is identical bit for bit; the stage-2 H (inlier DLT: LU + inverse iteration here, Jacobi in the oracle) lies
within 1e-4 px corner error, the final H within 1e-3 px (448 x 448, the bounds of tests/test_ops_gpu.py A9).  Every comparison
prints its worst corner error as a `HOMOG_ERR` line (pytest -s).
"""
import numpy as np
import pytest
import torch

import homography_cases as cases
import oracle

pytestmark = pytest.mark.gpu
TOL = {2: 1e-4, 0: 1e-3}  # px, by stage (stage 1 is compared bit for bit)
FAIL_H = np.diag([0.0, 0.0, 1.0])


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def ace(Ha, Hb):
    return oracle.corner_error(Ha, Hb, cases.S, cases.S, clamp=1e9)


def solve(pts, **kw):
    """(H, ninl, best, mask, used) of the device as numpy arrays."""
    from gfnet_amd import ops

    return tuple(host(t) for t in ops.find_homography(dev(pts), return_mask=True, return_iters=True, **kw))


_REF = {}


def ref(key, pts, **kw):
    """The oracle's (H, ninl, best, mask, used) of a named case, computed once per argument set and shared."""
    k = (key, tuple(sorted(kw.items())))
    if k not in _REF:
        out = oracle.homography_ransac(pts, return_mask=True, return_iters=True, **kw)
        for a in out:
            a.setflags(write=False)
        _REF[k] = out
    return _REF[k]


def check(key, pts, stages=(1, 2, 0), item="", **kw):
    """Device == oracle on `pts` at every stage (see the module docstring); returns the oracle's output at the last stage."""
    for stage in stages:
        H, ninl, best, mask, used = solve(pts, stage=stage, **kw)
        Ho, no, bo, mo, uo = ref(key, pts, stage=stage, **kw)
        what = f"{item} {key} {kw} stage={stage}"
        np.testing.assert_array_equal(best, bo, what)
        np.testing.assert_array_equal(ninl, no, what)
        np.testing.assert_array_equal(mask, mo, what)
        np.testing.assert_array_equal(used, uo, what)
        assert np.isfinite(H).all(), what
        # a pair without refinement (failure, or exactly four inliers: the hypothesis is returned as it is) must give the oracle's
        # bits at every stage; ace() cannot judge it, because it rounds the oracle's H to float32 like the reference's ground
        # truth, and on the wild H of a four-inlier hypothesis that rounding alone moves the corners by 5e-3 px
        raw = (bo < 0) | (no <= 4)
        err = [0.0 if raw[b] else ace(Ho[b], H[b]) for b in range(len(H))]
        print(f"HOMOG_ERR {what} worst={max(err):.3e} fp64_ruler={max(cases.corner_dist(Ho[b], H[b]) for b in range(len(H))):.3e}")
        if stage == 1:
            np.testing.assert_array_equal(H, Ho, what)  # same operations in the same order, -ffp-contract=off on both sides
        else:
            np.testing.assert_array_equal(H[raw], Ho[raw], what)
            assert max(err) < TOL[stage], (what, err)
        for b in np.flatnonzero(bo < 0):
            np.testing.assert_array_equal(H[b], FAIL_H, what)
    return Ho, no, bo, mo, uo


# ---- 1. replay beyond one scan chunk ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.REPLAY))
def test_replay_runs_past_the_first_scan_chunk(name):
    """iters = 6000: the head's bound lets hyp / score run thousands of hypotheses, and finish_kernel's sequential replay has to
    carry best, bestc and the shrinking bound from one chunk of 2048 counts into the next."""
    _, pts = cases.replay(name)
    _, no, bo, _, uo = check(name, pts, item="1", iters=cases.REPLAY_ITERS, seed=cases.REPLAY_SEED, confidence=cases.CONF)
    if name == "o88":
        assert (uo == cases.REPLAY_ITERS).all() and (bo >= cases.FIN_SCAN).any(), (uo, bo)  # a winner in the 2nd / 3rd chunk
    else:
        assert ((uo > cases.FIN_SCAN) & (uo < cases.REPLAY_ITERS)).any(), uo  # the replay stops inside a later chunk
        assert (bo < uo).all()


@pytest.mark.parametrize("name", list(cases.REPLAY))
def test_argmax_over_more_than_four_counts_per_thread(name):
    """confidence 0, iters = 2049 = 4 * 512 + 1: the strided arg-max gives thread 0 a fifth count; ties keep the lowest t."""
    _, pts = cases.replay(name)
    _, _, bo, _, uo = check(name, pts, item="1", iters=cases.ARGMAX_ITERS, seed=cases.REPLAY_SEED, confidence=0.0)
    assert cases.ARGMAX_ITERS > 4 * cases.FIN_THREADS and (uo == cases.ARGMAX_ITERS).all() and (bo >= 0).all()


# ---- 2. ragged score groups, hypothesis waves that straddle pairs --------------------------------------------------------------
@pytest.mark.parametrize("iters", cases.RAGGED_ALL)
def test_ragged_last_score_group_all_hypotheses(iters):
    """confidence 0: every pair's last score group holds one hypothesis or three (T % 4 = 1, 3; the clamp min(t0 + h, T - 1) reads
    the last hypothesis again and its count must go nowhere), and T % 8 != 0 puts hypotheses of two pairs into one wave of
    hyp_kernel."""
    _, pts = cases.ragged()
    assert iters % cases.SCORE_GROUP != 0 and iters % cases.HYP_WAVE != 0 and len(pts) == 5
    _, _, _, _, uo = check("ragged", pts, item="2", iters=iters, seed=4, confidence=0.0)
    assert (uo == iters).all()  # every hypothesis, the ragged group included, was scored


@pytest.mark.parametrize("iters", cases.RAGGED_ADAPTIVE)
def test_ragged_score_group_behind_the_head(iters):
    """Confidence rule: hyp / score cover t = 16 .. bound[b] - 1.  T = 17, 19, 21: the tail is one or two groups, the last one
    ragged, and it runs (the bound stays at T).  T = 531: 515 tail hypotheses per pair, so the waves of hyp_kernel straddle pairs
    and hold live lanes (t < bound[b + 1]) next to lanes that left (t >= bound[b])."""
    _, pts = cases.ragged()
    tail = iters - cases.HEAD
    assert tail % cases.SCORE_GROUP in (1, 3) and tail % cases.HYP_WAVE != 0
    _, _, _, _, uo = check("ragged", pts, item="2", iters=iters, seed=4, confidence=cases.CONF)
    if iters < 32:
        assert (uo == iters).all(), uo  # bound == T: the ragged group at the end of the tail is scored
    else:
        assert ((uo > cases.HEAD) & (uo < iters - cases.HYP_WAVE)).all(), uo  # live heads, dead ends in the straddling waves


# ---- 3. one batch, different fates ----------------------------------------------------------------------------------------------
def test_mixed_bounds_and_a_failing_pair_in_one_batch():
    _, pts = cases.fates()
    kw = dict(iters=cases.FATES_ITERS, seed=4, confidence=cases.CONF)
    Ho, no, bo, mo, uo = check("fates", pts, item="3", **kw)
    T = cases.FATES_ITERS
    assert (uo < cases.HEAD).any() and ((uo >= cases.HEAD) & (uo < T)).any() and (uo[:5] == T).any(), uo  # nothing / part / all of the tail
    assert bo[5] == -1 and uo[5] == T and no[5] == 0 and (bo[:5] >= 0).all()
    np.testing.assert_array_equal(Ho[5], FAIL_H)
    full = solve(pts, **kw)
    np.testing.assert_array_equal(full[0][5], FAIL_H)
    assert full[2][5] == -1 and full[4][5] == T and not full[3][5].any()
    # the RNG is keyed on the batch index: without the failing pair the others, at the same indices, give the same bits
    for got, want in zip(solve(pts[:5], **kw), full):
        np.testing.assert_array_equal(got, want[:5])


# ---- 4. small N, real data ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("confidence", [0.0, cases.CONF])
@pytest.mark.parametrize("N", cases.SMALL_N)
def test_small_point_sets(N, confidence):
    """N below one finish workgroup (512), below one wave (64), and 4..15 where repeated draws and checkSubset re-draws dominate;
    `cnt == 4` returns the hypothesis, 5..9 inliers go through DLT + LM."""
    Hs, pts = cases.small(N)
    Ho, no, bo, _, uo = check(f"small{N}", pts, item="4", iters=cases.SMALL_ITERS, seed=4, confidence=confidence)
    assert (bo >= 0).all()
    if N == 4:
        assert (no == 4).all()  # the early exit: H is the 4-point hypothesis itself
        np.testing.assert_array_equal(Ho, ref(f"small{N}", pts, stage=1, iters=cases.SMALL_ITERS, seed=4, confidence=confidence)[0])
    elif N < 16:
        assert ((no >= 5) & (no <= 12)).all(), no
    if confidence > 0:
        assert (uo == 0).all() if N < 8 else ((uo > cases.HEAD) & (uo < cases.SMALL_ITERS)).all(), uo
    for b in range(4):
        assert ace(Hs[b], Ho[b]) < 1.0  # 0.2 px noise on at least four spread inliers


# ---- 5. bit identity of the hypothesis -----------------------------------------------------------------------------------------
def test_hypothesis_is_bit_identical_from_both_solvers():
    """The header of homography.hip promises the chosen hypothesis bit for bit.  Two codes solve it: ransac_head_kernel (one
    thread per system, t < 16 under the confidence rule) and hyp_kernel / ge_solve8 (8 lanes per system: t >= 16, and every t
    when confidence == 0).  Winners from both, per pair."""
    sets = [(name, cases.replay(name)[1], dict(iters=cases.REPLAY_ITERS, seed=cases.REPLAY_SEED)) for name in cases.REPLAY]
    sets += [("ragged", cases.ragged()[1], dict(iters=531, seed=4)), ("fates", cases.fates()[1], dict(iters=cases.FATES_ITERS, seed=4))]
    sets += [(f"small{N}", cases.small(N)[1], dict(iters=cases.SMALL_ITERS, seed=4)) for N in (4, 9, 64, 513)]
    routes = {"head": 0, "tail": 0, "all": 0}
    for key, pts, kw in sets:
        for confidence in (cases.CONF, 0.0):
            if confidence == 0.0:
                kw = dict(kw, iters=min(kw["iters"], cases.ARGMAX_ITERS))
            H = solve(pts, stage=1, confidence=confidence, **kw)[0]
            Ho, _, bo, _, _ = ref(key, pts, stage=1, confidence=confidence, **kw)
            for b in range(len(pts)):
                assert np.array_equal(H[b], Ho[b]), (key, confidence, b, int(bo[b]), H[b] - Ho[b])
                if bo[b] >= 0:
                    routes["all" if confidence == 0.0 else "head" if bo[b] < cases.HEAD else "tail"] += 1
    print("HOMOG_ROUTES", routes)
    assert min(routes.values()) >= 4, routes


# ---- 6. short loops, LM, other arguments ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iters", [1, 3, 15, 16])
def test_loops_that_end_inside_the_head(iters):
    """The head kernel always runs 16 threads; t >= T must neither be written nor counted, and no tail is launched."""
    _, pts = cases.ragged()
    _, _, bo, _, uo = check("ragged", pts, item="6", iters=iters, seed=4, confidence=cases.CONF)
    assert (uo <= iters).all() and (bo < iters).all()


def test_bound_shrinks_differently_per_pair_at_confidence_one_half():
    _, pts = cases.half_confidence()
    _, _, bo, _, uo = check("ragged", pts, item="6", iters=2000, seed=4, confidence=0.5)
    assert (uo < 2000).all() and len(set(uo.tolist())) >= 3, uo
    assert (bo > uo).any()  # (the last update may leave the bound below the winner)


@pytest.mark.parametrize("lm_iters", [0, 1, 3])
def test_lm_iteration_counts(lm_iters):
    _, pts = cases.ragged()
    kw = dict(iters=64, seed=4, confidence=cases.CONF)
    check("ragged", pts, stages=(0,), item="6", lm_iters=lm_iters, **kw)
    if lm_iters == 0:  # nothing but the kernel's h = H / H[8] separates the result from the inlier DLT
        H0, H2 = solve(pts, stage=0, lm_iters=0, **kw)[0], solve(pts, stage=2, **kw)[0]
        np.testing.assert_array_equal(H0, H2 / H2[:, 2:, 2:])


@pytest.mark.parametrize("thresh", [0.5, 10.0])
def test_other_thresholds(thresh):
    _, pts = cases.ragged()
    _, no, _, _, _ = check("ragged", pts, item="6", iters=200, seed=4, confidence=cases.CONF, thresh=thresh)
    assert (no < 210).all() if thresh == 0.5 else (no >= 210).all(), no  # 0.3 px noise: 0.5 px cuts into the 210 inliers, 10 px adds


def test_seed_above_32_bits_and_unbatched_input():
    _, pts = cases.ragged()
    seed = 2 ** 40 + 3
    _, _, bo, _, _ = check("ragged", pts, item="6", iters=64, seed=seed, confidence=0.0)
    assert (bo != ref("ragged", pts, stage=0, iters=64, seed=3, confidence=0.0)[2]).any()  # the high bits count
    single = solve(pts[0], iters=64, seed=seed, confidence=0.0)  # (N, 4): one pair, batch index 0
    for got, want in zip(single, solve(pts[:1], iters=64, seed=seed, confidence=0.0)):
        np.testing.assert_array_equal(got, want)
    assert single[0].shape == (1, 3, 3)


def test_plain_c_entry_equals_confidence_zero():
    from gfnet_amd import _lib

    _, pts = cases.ragged()
    Bt, N, _ = pts.shape
    iters = 67
    p = dev(pts)
    H = torch.empty((Bt, 3, 3), device="cuda", dtype=torch.float64)
    ninl, best = (torch.empty((Bt,), device="cuda", dtype=torch.int32) for _ in range(2))
    mask = torch.empty((Bt, N), device="cuda", dtype=torch.uint8)
    nb = int(_lib.lib().gfn_homography_scratch_bytes(Bt, iters))
    scratch = torch.empty((nb // 8 + 1,), device="cuda", dtype=torch.float64)
    code = _lib.lib().gfn_homography_ransac(_lib.ptr(p), Bt, N, 3.0, iters, 4, 10, 0, _lib.ptr(H), _lib.ptr(ninl), _lib.ptr(best), _lib.ptr(mask),
                                            _lib.ptr(scratch), nb, _lib.stream_ptr(torch.device("cuda")))
    assert code == 0
    want = solve(pts, iters=iters, seed=4, confidence=0.0)
    for got, w in zip((H, ninl, best, mask), want):
        np.testing.assert_array_equal(host(got), w)


def test_estimate_homographies_on_non_square_images():
    from gfnet_amd import estimation

    sizes = (640, 480, 320, 200)
    Hs, pts = cases.ragged()
    scale = (np.array(sizes, np.float32) - 1) / (cases.S - 1)
    m = (2 * pts / (cases.S - 1) - 1).astype(np.float32)  # normalised rows; pixels are m's image, whatever the rounding here
    px = np.stack([oracle.convert_matches(mb, *sizes) for mb in m])
    np.testing.assert_allclose(px, pts * scale, atol=1e-3)
    H = host(estimation.estimate_homographies(dev(m), sizes, seed=7))
    Ho, _, bo = oracle.homography_ransac(px, thresh=estimation.RANSAC_THRESHOLD, iters=estimation.RANSAC_ITERS, seed=7,
                                         confidence=estimation.RANSAC_CONFIDENCE)
    assert (bo >= 0).all()
    err = [oracle.corner_error(Ho[b], H[b], sizes[0], sizes[1], clamp=1e9) for b in range(len(H))]
    print(f"HOMOG_ERR 6 estimate_homographies worst={max(err):.3e}")
    assert max(err) < 1e-3, err
    single = host(estimation.estimate_homographies(dev(m[0]), sizes, seed=7))
    np.testing.assert_array_equal(single[0], H[0])


def test_argument_refusals():
    from gfnet_amd import _lib, ops

    L = _lib.lib()
    _, pts = cases.ragged()
    Bt, N, _ = pts.shape
    p = dev(pts)
    H = torch.empty((Bt, 3, 3), device="cuda", dtype=torch.float64)
    ninl, best = (torch.empty((Bt,), device="cuda", dtype=torch.int32) for _ in range(2))
    nb = int(L.gfn_homography_scratch_bytes(Bt, 64))
    scratch = torch.empty((nb // 8 + 1,), device="cuda", dtype=torch.float64)
    stream = _lib.stream_ptr(torch.device("cuda"))

    def call(thresh=3.0, iters=64, confidence=cases.CONF, scratch_bytes=nb, lm_iters=10, stage=0):
        return L.gfn_homography_ransac_ex(_lib.ptr(p), Bt, N, thresh, iters, confidence, 4, lm_iters, stage, _lib.ptr(H), _lib.ptr(ninl),
                                          _lib.ptr(best), None, None, _lib.ptr(scratch), scratch_bytes, stream)

    assert call() == 0
    for bad in (dict(iters=0), dict(iters=-5), dict(thresh=0.0), dict(thresh=-1.0), dict(thresh=float("nan")), dict(confidence=1.0),
                dict(confidence=1.5), dict(confidence=float("nan")), dict(lm_iters=-1), dict(stage=3)):
        assert call(**bad) == _lib.ERR_INVALID_ARG, bad
        assert b"homography_ransac" in L.gfn_last_error()
    assert call(scratch_bytes=nb - 1) == _lib.ERR_SCRATCH
    assert call(scratch_bytes=0) == _lib.ERR_SCRATCH
    assert L.gfn_homography_scratch_bytes(Bt, 65) > nb and call(iters=65) == _lib.ERR_SCRATCH  # sized for 64 hypotheses
    with pytest.raises(_lib.GfnError):
        ops.find_homography(p, iters=0)
    with pytest.raises(_lib.GfnError):
        ops.find_homography(p, confidence=1.0)
    torch.cuda.synchronize()


# ---- 7. weighted DLT -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", cases.DLT_N)
def test_dlt_noise_free_sizes(N):
    """One-shot DLT at one row per thread or fewer (N <= 512), one over (513) and two rounds plus one (1025); N = 4 is the exactly
    determined system (rank 8: the smallest eigenvalue is rounding)."""
    from gfnet_amd import ops

    Hs, pts = cases.dlt(N)
    H, ok = ops.homography_dlt(dev(pts), None)
    Ho, oko = oracle.homography_dlt(pts)
    assert host(ok).all() and oko.all()
    err = [ace(Ho[b], host(H)[b]) for b in range(3)]
    true = [ace(Hs[b].astype(np.float32), host(H)[b]) for b in range(3)]
    print(f"HOMOG_ERR 7 dlt N={N} worst={max(err):.3e} vs_true={max(true):.3e}")
    assert max(err) < 1e-4, err   # the stage-2 bound: same sums, another null-vector method
    assert max(true) < 1e-3, true  # float32 coordinates (tests/test_homography_cpu.py: test_dlt_noise_free_recovers_h)


def test_dlt_zero_weights():
    from gfnet_amd import ops

    N = 513
    Hs, pts = cases.dlt(N)
    H, ok = ops.homography_dlt(dev(pts), dev(np.zeros((3, N), np.float32)))
    assert not host(ok).any()
    for b in range(3):
        np.testing.assert_array_equal(host(H)[b], FAIL_H)
    # zero weight on every third row == those rows dropped: the same sums in another order
    w = np.random.default_rng(71).uniform(0.1, 1.0, size=(3, N)).astype(np.float32)
    w[:, ::3] = 0
    keep = np.arange(N) % 3 != 0
    Hz, okz = ops.homography_dlt(dev(pts), dev(w))
    Hd, okd = ops.homography_dlt(dev(pts[:, keep]), dev(w[:, keep]))
    assert host(okz).all() and host(okd).all()
    err = [cases.corner_dist(host(Hd)[b], host(Hz)[b]) for b in range(3)]  # (the float32 rounding inside ace() alone is 1e-5 px)
    print(f"HOMOG_ERR 7 dlt zero-weight vs dropped fp64_ruler={max(err):.3e}")
    assert max(err) < 1e-6, err
    Ho, _ = oracle.homography_dlt(pts, w.astype(np.float64))
    assert max(ace(Ho[b], host(Hz)[b]) for b in range(3)) < 1e-4


# ---- 8. hostile rows -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("confidence", [0.0, cases.CONF])
def test_non_finite_rows_among_the_outliers(confidence):
    """A rejected correspondence may be NaN, inf or 1e30 (a warp that went through fp16 maps): the oracle skips what is outside
    the inlier mask, so the kernel must leave such a row out by selection -- 0 * NaN is NaN -- in the centroid, the deviations,
    the DLT rows and the LM rows; and a row with an infinite x or y must not pass the inlier test as inf <= inf."""
    Hs, clean, pts = cases.hostile()
    hostile_rows = ~np.isfinite(pts).all(-1) | (np.abs(pts) > 1e20).any(-1)
    assert (hostile_rows.sum(1) == cases.HOSTILE_ROWS).all() and not hostile_rows[:, 300:].any()
    kw = dict(iters=2000, seed=4, confidence=confidence)
    Ho, no, bo, mo, _ = check("hostile", pts, item="8", **kw)
    assert (bo >= 0).all() and not mo[hostile_rows].any()
    np.testing.assert_array_equal(mo, ref("clean", clean, stage=0, **kw)[3])  # what the clean rows alone decide
    for stage in (2, 0):
        H = solve(pts, stage=stage, **kw)[0]
        true = [ace(Hs[b], H[b]) for b in range(4)]
        print(f"HOMOG_ERR 8 hostile confidence={confidence} stage={stage} vs_true={max(true):.3e}")
        assert max(true) < 0.5, true
