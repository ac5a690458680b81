"""The match sampler (csrc/sample.hip: gfn_sample_without_replacement, gfn_gather_matches), gfn_balance_weights and
network.sample_batched on the GPU, against tests/golden/sampler_cases.py (itself checked by tests/test_match_sampler_cpu.py).

The keys are a deterministic function of (seed, row, index, weight) and the call leaves them, with the first-pass histogram, in the
caller's scratch (include/gfnet_hip.h).  So per case:
  a. keys       device keys against float64 keys on the exact uniforms.  Bound 2^-16 relative where -log u >= 2^-10 (set by the
                arithmetic class with room: a 1-ulp hardware log2, one multiply, one division suggest ~2^-21); for the largest keys
                (-log u < 2^-10, where the fast log loses relative accuracy and which win anyway) only key >= w * 2^9; a weight
                that is not positive gives key 0 exactly
  b. histogram  hist1[row] == bincount(keys[row] >> 21) exactly
  c. select     out == the K largest DEVICE keys, ties in index order, increasing: bit for bit
  d. select     against the float64 keys: every element of the symmetric difference lies within 2^-16 * T of the float64 cut T,
                on inputs where the float64 oracle alone has at most max(2, K / 1000) such elements
The law then follows from (a)-(d) and the CPU file; a statistical guard on the device's own draws stands beside it (6 standard
errors / 6 sigma, as there).  Measured on an MI355X: MEASURED below, from the figures every test prints before it asserts.
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import sampler_cases as cases

pytestmark = pytest.mark.gpu

# on an MI355X (ROCm 7.0, torch 2.10), from the printed figures:
MEASURED = """
worst key error where -log u >= 2^-10, over both seeds (bound 2^-16 = 1.526e-05):
  N 1: 0 (the one weight is zero)   N 7: 1.43e-07   N 255: 1.53e-07   N 256: 1.59e-07   N 257: 1.65e-07   N 1024: 1.78e-07
  N 1028: 1.82e-07   N 4096: 1.84e-07   N 4100: 1.90e-07   N 8192: 2.00e-07   N 8193: 1.84e-07   N 8196: 1.86e-07
  N 16384: 1.94e-07   N 16388: 2.10e-07 (= 2^-22.18, the worst)   N 16390: 1.91e-07   N 50000: 2.02e-07   N 49999: 2.01e-07
near-cut elements of the float64 oracle (allowed max(2, K / 1000)): at most 2 (N 8192, N 16390), 1 or 0 elsewhere; the device's
  selection differed from the float64 one in no case (largest symmetric difference 0)
natural ties (N 2^20, Bt 64, weights 1, 3.10 % of sorted neighbours equal): K = 2^18; seed 1: 4 of 64 rows have the cut inside a
  tie, seed 3: 3 rows  (seeds 2 and 4: 2 and 1 rows; K = 300000 with seed 1: none)
law on the device: class z-scores 0, 1.05, -0.78, -0.35, -0.31, 1.18, 0.68, -1.32; overlap mean z -0.89 (seeds 77, 78) and +0.65
  (rows), worst single overlap 3.24 sigma -- the figures of the CPU file: the device's draws equal the restated sampler's
balance_weights: worst relative error 3.1e-08 (round_fp16 off), 3.0e-08 (on); bound 2^-23 = 1.19e-07
sample_batched against sampler="torch": cluster share 0.0395 / 0.0399, z -0.29 (threshold_balanced); 0.2168 / 0.2109, z +1.98 (threshold)
"""

INF = float("inf")
# the natural-tie case (N = 2^20, Bt = 64, all weights 1): seeds and K found on an MI355X, see MEASURED
NATURAL_TIE_SEEDS = (1, 3)
NATURAL_TIE_K = 1 << 18


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def draw(w, K, seed, one_above=None, N=None, scratch=None, out=None):
    """gfn_sample_without_replacement through the raw ABI on w (Bt, row_stride) float32 on the device, the first N of every row.
    Returns (status, out (Bt, K) int64, keys (Bt, N) int32 bit patterns, hist1 (Bt, 2048) int32), all on the device."""
    from gfnet_amd import _lib

    Bt, rs = w.shape
    N = rs if N is None else N
    if out is None:
        out = torch.full((Bt, max(K, 1)), -7, device="cuda", dtype=torch.int64)
    if scratch is None:
        scratch = torch.full((Bt * (N + 2048),), -1, device="cuda", dtype=torch.int32)
    rc = _lib.lib().gfn_sample_without_replacement(_lib.ptr(w), rs, _lib.ptr(out), _lib.ptr(scratch), Bt, N, K, int(seed) & (2 ** 64 - 1),
                                                   INF if one_above is None else float(one_above), _lib.stream_ptr(w.device))
    keys = scratch[:Bt * N].view(Bt, N)
    hist = scratch[Bt * N:Bt * (N + 2048)].view(Bt, 2048)
    return rc, out[:, :K], keys, hist


def host_keys(keys):
    return keys.cpu().numpy().view(np.uint32)


def cut_state(keys_row, K):
    """(T, need, count): the K-th largest key of a row, how many of the elements equal to it are taken, how many there are."""
    T = np.sort(keys_row)[len(keys_row) - K]
    return T, K - int(np.count_nonzero(keys_row > T)), int(np.count_nonzero(keys_row == T))


def assert_exact_selection(out, keys, K):
    """(b) and (c) on host copies."""
    out, keys = out.cpu().numpy(), host_keys(keys)
    for b in range(len(keys)):
        np.testing.assert_array_equal(out[b], cases.select(keys[b], K), err_msg=f"row {b}, K {K}")
    return out, keys


def assert_histogram(hist, keys):
    hist = hist.cpu().numpy()
    for b in range(len(keys)):
        np.testing.assert_array_equal(hist[b], np.bincount(keys[b] >> 21, minlength=2048), err_msg=f"row {b}")


@pytest.mark.parametrize("N", cases.NS)
def test_keys_histogram_and_selection(N):
    Bt = cases.batch(N)
    w = cases.weights(Bt, N)
    wd = dev(w)
    worst, worst_near, worst_diff = 0.0, 0, 0
    for seed in cases.SEEDS:
        u = cases.uniforms(seed, Bt, N)
        e = -np.log(u)
        k64 = cases.keys64(w, u)
        o64 = [cases.order_desc(r) for r in k64]
        # (d)'s condition on the inputs, from the oracle alone, before the device is looked at
        cuts = {}
        for K in cases.ks(N):
            for b in range(Bt):
                T, near = cases.near_cut(k64[b], K)
                if T > 0:
                    assert near <= max(2, K / 1000), (N, K, seed, b, near)
                    cuts[K, b] = T
                    worst_near = max(worst_near, near)
        first = order = None
        for K in cases.ks(N):
            rc, out, keys, hist = draw(wd, K, seed)
            assert rc == 0
            out, keys = out.cpu().numpy(), host_keys(keys)
            assert_histogram(hist, keys)                                                         # (b)
            if first is None:
                first, order = keys, [cases.order_desc(r) for r in keys]
                kf = keys.view(np.float32).astype(np.float64)                                    # (a)
                pos = w > 0
                assert np.all(keys[~pos] == 0)
                body, top = pos & (e >= 2.0 ** -10), pos & (e < 2.0 ** -10)
                if body.any():
                    worst = max(worst, float((np.abs(kf[body] - k64[body]) / k64[body]).max()))
                assert np.all(kf[top] >= w[top].astype(np.float64) * 2.0 ** 9)
            else:
                np.testing.assert_array_equal(keys, first)                                       # the keys do not depend on K
            for b in range(Bt):
                np.testing.assert_array_equal(out[b], np.sort(order[b][:K]), err_msg=f"row {b}, K {K}, seed {seed}")   # (c)
                if (K, b) in cuts:                                                                                      # (d)
                    T = cuts[K, b]
                    diff = np.setxor1d(out[b], np.sort(o64[b][:K]))
                    worst_diff = max(worst_diff, len(diff))
                    assert np.all(np.abs(k64[b, diff] - T) <= cases.NEAR * T), (N, K, seed, b, diff)
    print(f"N {N}: worst key error {worst:.3e} = 2^{np.log2(max(worst, 1e-300)):.2f} (bound 2^-16), most near-cut elements {worst_near}, "
          f"largest symmetric difference {worst_diff}")
    assert worst <= cases.NEAR


def test_weights_that_are_not_positive_get_key_zero():
    N = 300
    w = cases.weights(1, N, seed=9)
    w[0, 1::5] = -w[0, 1::5]
    w[0, 2::11] = np.nan
    w[0, 3::13] = -0.0
    w[0, 4] = -np.inf
    pos = w[0] > 0
    K = int(pos.sum())
    rc, out, keys, hist = draw(dev(w), K, 5)
    assert rc == 0
    out, keys = assert_exact_selection(out, keys, K)
    assert np.all(keys[0][~pos] == 0) and np.all(keys[0][pos] > 0)
    np.testing.assert_array_equal(out[0], np.flatnonzero(pos))


@pytest.mark.parametrize("N,npos,K", [(1000, 10, 15), (4100, 100, 600)])
def test_cut_inside_the_zero_keys(N, npos, K):
    w = np.zeros((3, N), np.float32)
    rng = np.random.default_rng(N)
    for b in range(3):
        w[b, rng.permutation(N)[:npos]] = rng.uniform(0.1, 1.0, npos)
    for seed in cases.SEEDS:
        rc, out, keys, hist = draw(dev(w), K, seed)
        assert rc == 0
        out, keys = assert_exact_selection(out, keys, K)
        assert_histogram(hist, keys)
        for b in range(3):
            T, need, count = cut_state(keys[b], K)
            assert T == 0 and 0 < need < count, (T, need, count)
            zeros = np.flatnonzero(w[b] == 0)
            np.testing.assert_array_equal(out[b], np.sort(np.concatenate((np.flatnonzero(w[b] > 0), zeros[:need]))))


def test_cut_inside_and_beyond_the_clamped_keys():
    N = 4100
    w = np.full((3, N), 3e38, np.float32)
    w[2] = np.inf
    clamp = np.float32(3.0e38).view(np.uint32)
    for seed in cases.SEEDS:
        for K in (500, 3500):
            rc, out, keys, hist = draw(dev(w), K, seed)
            assert rc == 0
            out, keys = assert_exact_selection(out, keys, K)
            assert_histogram(hist, keys)
            assert keys.max() == clamp and np.all(keys[2] == clamp)
            for b in range(3):
                T, need, count = cut_state(keys[b], K)
                nclamp = int(np.count_nonzero(keys[b] == clamp))
                if b == 2 or K == 500:   # the cut lies in the group of clamped keys (63 % of a 3e38 row, all of the inf row)
                    assert T == clamp and 0 < need < count == nclamp, (b, K, T, need, count)
                    np.testing.assert_array_equal(out[b], np.flatnonzero(keys[b] == clamp)[:K])
                else:                    # beyond it
                    assert 2000 < nclamp < K and T < clamp
                    assert np.isin(np.flatnonzero(keys[b] == clamp), out[b]).all()


def test_cut_inside_a_natural_24_bit_collision():
    """All weights 1: two elements that drew the same 24-bit u have the same key (~3 % of 2^20).  On the fixed seeds at least one
    row's cut must fall between such a pair; the oracle is torch's stable sort of the device keys."""
    Bt, N, K = 64, 1 << 20, NATURAL_TIE_K
    w = torch.ones((Bt, N), device="cuda")
    out = torch.empty((Bt, K), device="cuda", dtype=torch.int64)
    scratch = torch.empty((Bt * (N + 2048),), device="cuda", dtype=torch.int32)
    tie_rows = 0
    for seed in NATURAL_TIE_SEEDS:
        rc, got, keys, hist = draw(w, K, seed, scratch=scratch, out=out)
        assert rc == 0
        vals, order = torch.sort(keys, dim=1, descending=True, stable=True)
        T = vals[:, K - 1:K]
        need, count = K - (keys > T).sum(1), (keys == T).sum(1)
        tie_rows += int((need < count).sum())
        assert torch.equal(got, order[:, :K].sort(dim=1).values)
        top = (keys >> 21) + 2048 * torch.arange(Bt, device="cuda", dtype=torch.int32)[:, None]
        assert torch.equal(hist.reshape(-1).long(), torch.bincount(top.reshape(-1), minlength=Bt * 2048))
        print(f"seed {seed}, K {K}: {int((need < count).sum())} of {Bt} rows have the cut inside a tie")
    assert tie_rows >= 1


def test_one_above_on_the_fly():
    N, thr = 4100, 0.05
    w = np.random.default_rng(2).uniform(0.0, 0.1, size=(3, N)).astype(np.float32)
    w[:, ::7] = 0.0
    w[:, 5::50] = np.float32(thr)  # exactly the threshold: stays as it is
    pre = np.where(w > np.float32(thr), np.float32(1), w)
    assert np.count_nonzero(pre == np.float32(thr)) == np.count_nonzero(w == np.float32(thr)) > 0 and (pre == 1).any()
    rc1, out1, keys1, _ = draw(dev(w), 1000, 31, one_above=thr)
    rc2, out2, keys2, _ = draw(dev(pre), 1000, 31)
    assert rc1 == 0 and rc2 == 0
    assert torch.equal(keys1, keys2) and torch.equal(out1, out2)
    kf = host_keys(keys1).view(np.float32).astype(np.float64)
    u = cases.uniforms(31, 3, N)
    k64 = cases.keys64(w, u, one_above=thr)  # the oracle thresholds alike
    body = (k64 > 0) & (-np.log(u) >= 2.0 ** -10)
    assert np.all(np.abs(kf - k64)[body] <= cases.NEAR * k64[body]) and np.all(kf[k64 == 0] == 0)


def test_strided_rows_and_unaligned_scratch():
    N = 4100
    w = cases.weights(3, N)
    padded = np.full((3, N + 5), 1e6, np.float32)  # a kernel that read the padding would draw other elements
    padded[:, :N] = w
    rc0, want, keys0, _ = draw(dev(w), 1000, 17)
    rc1, got, keys1, _ = draw(dev(padded), 1000, 17, N=N)
    assert rc0 == 0 and rc1 == 0 and torch.equal(keys0, keys1) and torch.equal(got, want)
    for N in (4096, 16384):  # vector-eligible rows; a scratch 4 bytes off a 16-byte boundary takes the scalar walks
        wd = dev(cases.weights(3, N))
        buf = torch.full((3 * (N + 2048) + 1,), -1, device="cuda", dtype=torch.int32)
        assert buf.data_ptr() % 16 == 0
        for K in (1, N // 7, N - 1):
            rc0, want, keys0, hist0 = draw(wd, K, 17)
            rc1, got, keys1, hist1 = draw(wd, K, 17, scratch=buf[1:])
            assert rc0 == 0 and rc1 == 0
            assert torch.equal(keys0, keys1) and torch.equal(hist0, hist1) and torch.equal(got, want)
            assert_exact_selection(got, keys1, K)


def test_smallest_normal_weights():
    # (subnormal weights, and keys that would be subnormal, are out of scope: the device may flush them)
    N = 4100
    w = np.zeros((3, N), np.float32)
    w[:, 3::9] = 2.0 ** -120  # keys 2^-120 / -log u >= 2^-120 / 16.7 > 2^-125: normal
    K = int((w[0] > 0).sum())
    rc, out, keys, _ = draw(dev(w), K, 3)
    assert rc == 0
    out, keys = assert_exact_selection(out, keys, K)
    for b in range(3):
        np.testing.assert_array_equal(out[b], np.flatnonzero(w[b] > 0))


def test_refusals_leave_out_untouched():
    from gfnet_amd import _lib

    N = 100
    wd = dev(cases.weights(2, N))
    for kw in (dict(K=N + 1), dict(K=0), dict(K=10, N=N + 1)):  # (N above the row stride)
        rc, out, _, _ = draw(wd, seed=1, **kw)
        assert rc == _lib.ERR_INVALID_ARG, kw
        assert (out == -7).all(), kw
    out = torch.full((2, 10), -7, device="cuda", dtype=torch.int64)
    rc = _lib.lib().gfn_sample_without_replacement(_lib.ptr(wd), N, _lib.ptr(out), None, 2, N, 10, 1, INF, _lib.stream_ptr(wd.device))
    assert rc == _lib.ERR_INVALID_ARG and (out == -7).all()
    assert draw(wd, 10, 1)[0] == 0


def test_law_on_the_device():
    from gfnet_amd import ops

    w = dev(np.broadcast_to(cases.LAW_WEIGHTS, (64, cases.LAW_N)))
    got = cases.class_counts(ops.sample_without_replacement(w, cases.LAW_K, seed=2024).cpu().numpy())
    ref = cases.independent_race_counts(512, 1)
    z = cases.class_z_scores(got, ref)
    print("class z-scores:", np.round(z, 2))
    assert got[:, 0].max() == 0 and np.all(np.abs(z) <= 6), z
    ones = torch.ones((64, cases.LAW_N), device="cuda")
    a = ops.sample_without_replacement(ones, cases.LAW_K, seed=77).cpu().numpy()
    b = ops.sample_without_replacement(ones, cases.LAW_K, seed=78).cpu().numpy()
    for what, (zmean, worst) in (("seeds s, s+1", cases.overlap_z(a, b)), ("rows b, b+1", cases.overlap_z(a[:-1], a[1:]))):
        print(f"overlap, {what}: mean z {zmean:+.2f}, worst single {worst:.2f} sigma")
        assert abs(zmean) <= 6 and worst <= 6, (what, zmean, worst)


def test_gather_matches_edges():
    from gfnet_amd import _lib, ops

    g = torch.Generator().manual_seed(5)
    for Bt, N in ((1, 50), (3, 257)):
        m = torch.randn(Bt, N, 4, generator=g).cuda()
        c = torch.rand(Bt, N, generator=g).cuda() * 0.1
        c[:, 7] = 0.05  # exactly the threshold
        idx = torch.stack([torch.tensor([0, N - 1, N - 1, 7, 0, N // 2, 1, N - 2]) for _ in range(Bt)]).cuda()
        K = idx.shape[1]
        for thr in (None, 0.05):
            om, oc = ops.gather_matches(m, c, idx, one_above=thr)
            cw = c if thr is None else torch.where(c > thr, torch.ones_like(c), c)
            assert torch.equal(om, torch.gather(m, 1, idx[..., None].expand(Bt, K, 4)))
            assert torch.equal(oc, torch.gather(cw, 1, idx))
            assert thr is None or (oc[:, 3] == 0.05).all()
        # K = 0 is accepted and writes nothing; a matches pointer off a 16-byte boundary is refused
        om, oc = torch.full((Bt, K, 4), -7.0, device="cuda"), torch.full((Bt, K), -7.0, device="cuda")
        call = lambda mp, omp, k: _lib.lib().gfn_gather_matches(mp, _lib.ptr(c), _lib.ptr(idx), omp, _lib.ptr(oc), Bt, N, k, INF,  # noqa: E731
                                                                _lib.stream_ptr(m.device))
        assert call(_lib.ptr(m), _lib.ptr(om), 0) == 0
        off = torch.zeros(Bt * N * 4 + 4, device="cuda")
        assert off.data_ptr() % 16 == 0
        assert call(_lib.ptr(off[1:]), _lib.ptr(om), K) == _lib.ERR_INVALID_ARG
        assert call(_lib.ptr(m), _lib.ptr(off[1:]), K) == _lib.ERR_INVALID_ARG
        assert (om == -7).all() and (oc == -7).all()
        assert call(_lib.ptr(m), _lib.ptr(om), K) == 0 and torch.equal(om, torch.gather(m, 1, idx[..., None].expand(Bt, K, 4)))


@pytest.mark.parametrize("round_fp16", [False, True])
def test_balance_weights_at_the_edges(round_fp16):
    from gfnet_amd import ops

    d = np.array([0, 9.99, 9.998, 10, 10.004, 65504, 7e4], np.float32)
    with np.errstate(over="ignore"):
        used = d.astype(np.float16).astype(np.float64) if round_fp16 else d.astype(np.float64)
    want = np.where(used < 10.0, float(np.float32(1e-7)), 1.0 / (used + 1.0))
    floored = (used < 10.0).tolist()
    assert floored == ([True, True, False, False, False, False, False] if round_fp16 else [True, True, True, False, False, False, False])
    assert not round_fp16 or (used[2] == 10.0 and np.isinf(used[6]) and want[6] == 0)
    got = ops.balance_weights(dev(d), round_fp16=round_fp16).cpu().numpy().astype(np.float64)
    print("round_fp16", round_fp16, "worst relative error", float(np.max(np.abs(got - want)[want > 0] / want[want > 0])))
    assert np.all(np.abs(got - want) <= 2.0 ** -23 * want), (got, want)


# ---- network.sample_batched ----------------------------------------------------------------------------------------------------
CLUSTER = (-0.2, -0.25, 0.9, -0.9)  # centre of the dense cluster; every other match has |B| <= 0.51


@functools.lru_cache(maxsize=None)
def synthetic_pairs():
    """(warp (4, 64, 128, 4), certainty (4, 64, 128)) on the device: A positions on the grid, B = A / 2 (a plane in 4-D, density
    around 25 at 2000 draws: both sides of balance_weights' floor of 10 occur), one dense cluster of matches (1600 cells within 0.05 of
    one 4-D position), certainties a sigmoid of noise (a third under the 0.05 threshold), a band of exact zeros."""
    g = torch.Generator().manual_seed(11)
    B, H, W = 4, 64, 128
    ys = torch.linspace(-1 + 1 / H, 1 - 1 / H, H)
    xs = torch.linspace(-1 + 1 / W, 1 - 1 / W, W)
    a = torch.stack(torch.meshgrid(xs, ys, indexing="xy"), -1)[None].expand(B, H, W, 2)
    warp = torch.cat((a, 0.5 * a + 0.002 * torch.randn(B, H, W, 2, generator=g)), -1).contiguous()
    warp[:, 8:40, 30:80] = torch.tensor(CLUSTER) + 0.05 * torch.randn(B, 32, 50, 4, generator=g)
    cert = torch.sigmoid(2.0 * torch.randn(B, H, W, generator=g) - 2.0)
    cert[:, 50:56] = 0.0
    return warp.cuda(), cert.cuda()


def cluster_share(matches):
    """(B,) share of the returned matches that lie in the dense cluster."""
    return (matches[..., 2] > 0.7).double().mean(1).cpu().numpy()


@pytest.mark.parametrize("mode", ["threshold_balanced", "threshold"])
def test_sample_batched_is_its_chain_of_ops(mode):
    from gfnet_amd import ops
    from gfnet_amd.model.network import sample_batched

    warp, cert = synthetic_pairs()
    model = SimpleNamespace(sample_mode=mode, sample_thresh=0.05)
    B, num, thr = warp.shape[0], 500, 0.05
    m, c = warp.reshape(B, -1, 4), cert.reshape(B, -1)
    n1 = 4 * num if "balanced" in mode else num
    for s in (0, 12345):
        torch.manual_seed(s)
        gm, gc = sample_batched(model, warp, cert, num, sampler="hip")
        torch.manual_seed(s)
        s1, s2 = (int(torch.randint(0, 2 ** 62, (1,)).item()) for _ in range(2))
        good = ops.sample_without_replacement(c, n1, seed=s1, one_above=thr)
        wm = torch.gather(m, 1, good[..., None].expand(B, n1, 4)).contiguous()
        wc = torch.gather(ops.threshold_certainty(c, thr), 1, good)
        if "balanced" in mode:
            p = ops.balance_weights(ops.kde_density(wm, std=0.1, round_fp16=True), round_fp16=True)
            assert (p > 2e-7).any() and (p < 2e-7).any()  # both sides of the density floor
            bal = ops.sample_without_replacement(p, num, seed=s2)
            wm, wc = torch.gather(wm, 1, bal[..., None].expand(B, num, 4)), torch.gather(wc, 1, bal)
        assert gm.shape == (B, num, 4) and gc.shape == (B, num)
        assert torch.equal(gm, wm) and torch.equal(gc, wc)
        assert (gc > 0).all() and ((gc == 1) | (gc <= thr)).all()
        for b in range(B):
            rows = {r.tobytes() for r in m[b].cpu().numpy()}
            assert all(r.tobytes() in rows for r in gm[b].cpu().numpy())
        torch.manual_seed(s)
        gm2, gc2 = sample_batched(model, warp, cert, num, sampler="hip")
        assert torch.equal(gm, gm2) and torch.equal(gc, gc2)


@pytest.mark.parametrize("mode", ["threshold_balanced", "threshold"])
def test_sample_batched_has_the_law_of_the_torch_sampler(mode):
    from gfnet_amd.model.network import sample_batched

    warp, cert = synthetic_pairs()
    model = SimpleNamespace(sample_mode=mode, sample_thresh=0.05)
    share = {}
    for sampler in ("hip", "torch"):
        rows = []
        for rep in range(16):
            torch.manual_seed(1000 + rep)
            rows.append(cluster_share(sample_batched(model, warp, cert, 500, sampler=sampler)[0]))
        share[sampler] = np.stack(rows)  # (16 repetitions, 4 pairs): per pair, 16 independent draws on each side
    h, t = share["hip"], share["torch"]
    diff = (h.mean(0) - t.mean(0)).mean()
    se = np.sqrt((h.var(0, ddof=1) / len(h) + t.var(0, ddof=1) / len(t)).sum()) / h.shape[1]
    print(f"{mode}: cluster share hip {h.mean():.4f}, torch {t.mean():.4f}, z {diff / se:+.2f}")
    assert 0 < t.mean() < 1 and se > 0
    assert abs(diff) <= 6 * se, (diff, se)
