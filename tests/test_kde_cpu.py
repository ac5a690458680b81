"""oracle.kde against an independent float64 numpy restatement of utils/kde.py:4-13.

tests/test_kde_gpu.py measures every KDE route of csrc/kde.hip against oracle.kde(variant="f64") (oracle_kde in
oracle/gfnet_oracle.c), so the oracle has to be right first: on duplicates, exact distance ties, points far outside the
image, `down` with a ragged tail, `half=True` rounding, and on a NaN / an infinite coordinate (which the GPU module uses to
check that a poisoned row stays contained).  The restatement shares no code with the oracle: numpy broadcasting, float64
throughout, pairwise summation.
"""
import numpy as np
import pytest

import oracle

import kde_cases as cases


def np_kde(x, std, half, down):
    """density_n = sum_m exp(-|x_n - y_m|^2 / (2 std^2)), y = x[::down]; x rounded to fp16 first when half (kde.py:6)."""
    x = np.asarray(x)
    if half:
        x = x.astype(np.float16)
    xd = x.astype(np.float32).astype(np.float64)
    y = xd[::down] if down is not None else xd
    out = np.empty(len(xd))
    with np.errstate(invalid="ignore", over="ignore"):
        for n0 in range(0, len(xd), 256):  # chunked: (256, M, D) at a time
            d2 = ((xd[n0:n0 + 256, None, :] - y[None, :, :]) ** 2).sum(-1)
            out[n0:n0 + 256] = np.exp(-d2 / (2.0 * std * std)).sum(1)
    return out


GEOMETRIES = ["match", "outliers", "identical", "kfold", "clusters32", "line", "lattice", "one_cell", "outside", "extent3", "extent10",
              "satellite"]


@pytest.mark.parametrize("geom", GEOMETRIES)
@pytest.mark.parametrize("N", [1, 2, 33, 130, 257])
def test_oracle_kde_matches_numpy_float64(geom, N):
    """f64 variant: the same float64 arithmetic in another summation order -> 1e-12 relative (N <= 257 terms of rounding 1.1e-16).
    f32 variant: differences, squares and their sum are rounded to fp32, (D + 2) roundings of 6e-8 on an exponent e, i.e. a
    relative error of 4e-7 * e on a term; a term that is still a normal fp32 number has e < 87.4, so 4e-5 < 1e-4 relative covers
    every term, and 1e-37 absolute covers the ones that fall under the normal range."""
    x = cases.make(geom, N, seed=N)
    for std in (0.3, 0.1, 0.02):
        for half in (False, True):
            for down in (None, 1, 3, 8):
                want = np_kde(x, std, half, down)
                got64 = oracle.kde(x, std, half=half, down=down, variant="f64")
                assert got64.dtype == np.float64 and got64.shape == (N,)
                np.testing.assert_allclose(got64, want, rtol=1e-12, atol=1e-300, err_msg=f"f64 {geom} std={std} half={half} down={down}")
                got32 = oracle.kde(x, std, half=half, down=down, variant="f32")
                assert got32.dtype == np.float32
                np.testing.assert_allclose(got32, want, rtol=1e-4, atol=1e-37, err_msg=f"f32 {geom} std={std} half={half} down={down}")


def test_oracle_kde_exact_values():
    """Densities that are known without any arithmetic: identical points give M, k-fold duplicates of far-apart points give k,
    a ragged `down` keeps ceil(N / down) reference points, and half=True acts on the inputs (1 + 2^-12 rounds to 1 in fp16)."""
    x = cases.make("identical", 37, seed=0)
    for down, M in ((None, 37), (1, 37), (3, 13), (8, 5), (37, 1), (100, 1)):
        assert np.array_equal(oracle.kde(x, 0.1, half=False, down=down, variant="f64"), np.full(37, float(M)))
    far = np.array([[-9, 0, 0, 0], [9, 0, 0, 0], [0, 9, 0, 0], [0, 0, 9, 0], [0, 0, 0, 9]], np.float32)  # 90 std apart: terms underflow to 0
    x = np.repeat(far, 7, axis=0)
    assert np.array_equal(oracle.kde(x, 0.1, half=False, variant="f64"), np.full(35, 7.0))
    assert np.array_equal(oracle.kde(x, 0.1, half=False, variant="f32"), np.full(35, 7.0, np.float32))
    # x[::3] of the 35 rows: rows 0,3,..,33 -> 12 points, cluster c (rows 7c..7c+6) keeps those with (row % 3 == 0)
    want = np.array([sum(1 for r in range(7 * c, 7 * c + 7) if r % 3 == 0) for c in range(5)], np.float64)
    assert np.array_equal(oracle.kde(x, 0.1, half=False, down=3, variant="f64"), np.repeat(want, 7))
    a = np.array([[1.0, 0, 0, 0], [1.0 + 2.0 ** -12, 0, 0, 0]], np.float32)
    d = 2.0 ** -12
    assert np.array_equal(oracle.kde(a, 1e-4, half=True, variant="f64"), [2.0, 2.0])
    np.testing.assert_allclose(oracle.kde(a, 1e-4, half=False, variant="f64"), np.full(2, 1 + np.exp(-d * d / 2e-8)), rtol=1e-14)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_oracle_kde_on_a_poisoned_point(bad):
    """One NaN coordinate makes every density NaN (each query meets that point).  One infinite coordinate makes the point's own
    density NaN (inf - inf) and removes it from every other sum (exp(-inf) = 0).  The numpy restatement agrees element by element."""
    x = cases.make("match", 130, seed=3)
    clean = oracle.kde(np.delete(x, 17, axis=0), 0.1, half=False, variant="f64")
    x[17, 2] = bad
    for variant in ("f64", "f32"):
        got = oracle.kde(x, 0.1, half=False, variant=variant)
        want = np_kde(x, 0.1, False, None)
        assert np.array_equal(np.isnan(got), np.isnan(want))
        if np.isnan(bad):
            assert np.isnan(got).all()
        else:
            assert np.isnan(got[17]) and np.isfinite(np.delete(got, 17)).all()
            np.testing.assert_allclose(np.delete(got, 17), clean, rtol=1e-12 if variant == "f64" else 1e-4)
