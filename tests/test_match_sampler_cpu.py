"""The oracle of tests/test_match_sampler_gpu.py checked by itself, without a GPU: the restated generator against SplitMix64's
published output, the restated race (tests/golden/sampler_cases.py) against an exponential race drawn with numpy's own generator,
and the independence of its seeds and rows against the hypergeometric law.

Bounds: 6 standard errors on a mean and 6 sigma on a single value -- 2e-9 per comparison under the law, a few dozen comparisons.
Figures the tests print: class z-scores within +-1.4 (seed 2024 against default_rng(1)); overlap mean z -0.89 (seeds 77, 78)
and +0.65 (rows of seed 77), worst single overlap 3.24 sigma."""
import numpy as np

import sampler_cases as cases


def test_splitmix64_first_output():
    assert int(cases.splitmix64(0)[0]) == 0xE220A8397B1DCDAF  # the published first output from state 0
    z = np.array([[0, 1], [2 ** 63, 2 ** 64 - 1]], np.uint64)
    assert cases.splitmix64(z).shape == (2, 2) and int(cases.splitmix64(z)[0, 0]) == 0xE220A8397B1DCDAF


def test_uniforms_are_24_bit_and_in_range():
    u = cases.uniforms(cases.SEEDS[1], 3, 4100)
    assert u.shape == (3, 4100) and u.min() > 0 and u.max() <= 1
    assert np.array_equal(u * 2 ** 24, np.round(u * 2 ** 24))
    assert np.array_equal(u.astype(np.float32).astype(np.float64), u)
    assert not np.array_equal(u[0], u[1]) and not np.array_equal(u, cases.uniforms(cases.SEEDS[0], 3, 4100))
    assert np.array_equal(u[:, :100], cases.uniforms(cases.SEEDS[1], 3, 100))  # a function of (seed, row, index) alone


def test_keys64_and_select_edges():
    u = np.array([0.5, 0.5, 0.5, 1.0, 0.5, 0.5, 0.25])
    w = np.array([1.0, 0.0, -1.0, 1.0, np.nan, np.inf, 0.2], np.float32)
    k = cases.keys64(w, u)
    assert k[1] == 0 and k[2] == 0 and k[4] == 0
    assert k[0] == 1 / np.log(2) and k[3] == 1 / cases.E_MIN and k[5] == cases.KEY_MAX
    k2 = cases.keys64(w, u, one_above=0.2)  # exactly the threshold: stays
    assert k2[6] == float(np.float32(0.2)) / np.log(4) and k2[0] == k[0]
    assert cases.keys64(w, u, one_above=0.1)[6] == 1 / np.log(4)
    assert cases.select(np.array([3, 9, 3, 3, 1], np.uint32), 3).tolist() == [0, 1, 2]  # ties in index order
    assert cases.select(np.array([3.0, 9.0, 3.0, 3.0, 1.0]), 2).tolist() == [0, 1]
    assert cases.ks(50000) == [1, 2, 7142, 25000, 49999, 50000] and cases.ks(1) == [1] and cases.ks(7) == [1, 2, 3, 6, 7]


def test_restated_race_follows_the_law_of_an_independent_one():
    got = cases.class_counts(cases.restated_draws(2024, 64, cases.LAW_WEIGHTS, cases.LAW_K))
    ref = cases.independent_race_counts(512, 1)
    z = cases.class_z_scores(got, ref)
    print("class z-scores:", np.round(z, 2))
    assert got[:, 0].max() == 0 and ref[:, 0].max() == 0  # zero weights are never drawn while positives remain
    assert np.all(np.abs(z) <= 6), z


def test_restated_seeds_and_rows_are_independent():
    w = np.ones(cases.LAW_N, np.float32)
    a = cases.restated_draws(77, 64, w, cases.LAW_K)
    b = cases.restated_draws(78, 64, w, cases.LAW_K)
    for what, (zmean, worst) in (("seeds s, s+1", cases.overlap_z(a, b)), ("rows b, b+1", cases.overlap_z(a[:-1], a[1:]))):
        print(f"overlap, {what}: mean z {zmean:+.2f}, worst single {worst:.2f} sigma")
        assert abs(zmean) <= 6 and worst <= 6, (what, zmean, worst)
