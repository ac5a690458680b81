"""The match sampler (csrc/sample.hip) restated in numpy and float64 for tests/test_match_sampler_cpu.py and
tests/test_match_sampler_gpu.py: the counter-based uniforms (exact), the race keys (float64), the selection (stable sort), the
case table, and the statistics both files apply to a set of draws.  No GPU, no torch."""
import functools

import numpy as np

U64 = np.uint64


def splitmix64(z):
    """One SplitMix64 output from state z (uint64, any shape): gfn::splitmix64 of csrc/common.h."""
    z = np.atleast_1d(np.asarray(z, dtype=U64))
    z = z + U64(0x9E3779B97F4A7C15)  # (uint64 arrays wrap silently)
    z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
    return z ^ (z >> U64(31))


def uniforms(seed, Bt, N):
    """u (Bt, N) float64 in (0, 1], 24 bits, exactly the kernel's: h = splitmix64(seed ^ splitmix64((row << 32) | i)),
    u = ((h >> 40) + 1) * 2^-24 (both factors are exact in fp32 too)."""
    row = np.arange(Bt, dtype=U64)[:, None]
    i = np.arange(N, dtype=U64)[None, :]
    h = splitmix64(U64(int(seed) & (2 ** 64 - 1)) ^ splitmix64((row << U64(32)) | i))
    return ((h >> U64(40)).astype(np.float64) + 1.0) * 2.0 ** -24


KEY_MAX = float(np.float32(3.0e38))     # the kernel's clamp
E_MIN = float(np.float32(1e-30))        # its floor of -log u (reached only by u == 1)


def keys64(w, u, one_above=np.inf):
    """The race keys in float64: w > one_above counts as 1 (compared in fp32, as the kernel does), key = w / max(-log u, 1e-30)
    for w > 0, else 0 (zero, negative and NaN weights), clamped to float32(3.0e38)."""
    w32 = np.asarray(w, np.float32)
    with np.errstate(invalid="ignore"):
        w64 = np.where(w32 > np.float32(one_above), 1.0, w32.astype(np.float64))
        pos = w64 > 0
    e = np.maximum(-np.log(np.asarray(u, np.float64)), E_MIN)
    with np.errstate(over="ignore", invalid="ignore"):
        key = np.where(pos, np.where(pos, w64, 0.0) / e, 0.0)
    return np.minimum(key, KEY_MAX)


def order_desc(keys):
    """Indices of one row by decreasing key, ties in index order (stable)."""
    k = np.asarray(keys)
    if k.dtype.kind in "ui":
        k = k.astype(np.int64)
    return np.argsort(-k, kind="stable")


def select(keys, K):
    """Indices of the K largest keys of one row, ties in index order, returned increasing."""
    return np.sort(order_desc(keys)[:K])


# ---- the case table ----------------------------------------------------------------------------------------------------------
# N: the smallest row lengths that reach each path of race_keys_kernel / race_select_kernel
NS = (1, 7,                    # one lane, one wave
      255, 256, 257,           # one 256-step of wave 0; scalar and vector tails
      1024, 1028,              # one select-thread stride
      4096, 4100,              # every wave exactly one step; then wave 8 holds 4 elements and waves 9-15 none
      8192, 8193, 8196,        # one and two key blocks per row (first-pass histogram flushed by two workgroups)
      16384, 16388, 16390,     # second iteration of the unrolled histogram loops, vector and scalar
      50000, 49999)            # the sizes of tests/test_ops_gpu.py
SEEDS = (123, (1 << 63) | 0x2545F4914F6CDD1D)  # one small seed, one with bit 63 set


def batch(N):
    return 1 if N <= 7 else 3


def ks(N):
    return sorted({min(max(k, 1), N) for k in (1, 2, N // 7, N // 2, N - 1, N)})


def weights(Bt, N, seed=4):
    """uniform(0, 1) float32 with every 7th set to 0, as in tests/test_ops_gpu.py."""
    w = np.random.default_rng(seed).uniform(0.0, 1.0, size=(Bt, N)).astype(np.float32)
    w[:, ::7] = 0.0
    return w


NEAR = 2.0 ** -16  # the bound on a key's relative error, and with it the width of the band around the cut in which the sets may differ


def near_cut(k64_row, K):
    """(T, count): the K-th largest float64 key of a row and how many OTHER elements lie within NEAR * T of it."""
    T = float(np.sort(k64_row)[len(k64_row) - K])
    return T, int(np.count_nonzero(np.abs(k64_row - T) <= NEAR * T)) - 1


# ---- the law -----------------------------------------------------------------------------------------------------------------
LAW_N, LAW_K = 20000, 5000
LAW_CLASSES = np.array([0, .01, .05, .3, 1, 1, 1, 4], np.float32)
LAW_WEIGHTS = np.tile(LAW_CLASSES, LAW_N // 8)


def class_counts(idx):
    """(rows, 8): how many of each row's drawn indices fall in each weight class (index mod 8)."""
    idx = np.asarray(idx)
    return np.stack([np.bincount(r % 8, minlength=8) for r in idx]).astype(np.float64)


@functools.lru_cache(maxsize=None)
def independent_race_counts(rows=512, seed=1):
    """Class counts of an exponential race drawn with numpy's generator: independent of everything restated above."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(rows):
        with np.errstate(divide="ignore"):
            key = LAW_WEIGHTS.astype(np.float64) / rng.standard_exponential(LAW_N)
        out.append(np.argpartition(-key, LAW_K - 1)[:LAW_K])
    return class_counts(np.stack(out))


def class_z_scores(a, b):
    """Per class, (mean_a - mean_b) / standard error, the error from the two samples' own per-row variances.  A class neither
    sample ever varies in (the zero-weight one) scores 0 if the means agree and inf if not."""
    diff = a.mean(0) - b.mean(0)
    se = np.sqrt(a.var(0, ddof=1) / len(a) + b.var(0, ddof=1) / len(b))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(se > 0, diff / se, np.where(diff == 0, 0.0, np.inf))


OVERLAP_MEAN = LAW_K ** 2 / LAW_N                                                        # hypergeometric: |A n B| of two
OVERLAP_SIGMA = (LAW_K ** 2 * (LAW_N - LAW_K) ** 2 / (LAW_N ** 2 * (LAW_N - 1))) ** 0.5  # independent uniform K-subsets of N


def overlap_z(sel_a, sel_b):
    """(z of the mean overlap, worst single overlap in sigma) of paired rows of selections under the hypergeometric law."""
    ov = np.array([np.intersect1d(a, b, assume_unique=True).size for a, b in zip(sel_a, sel_b)], np.float64)
    return float((ov.mean() - OVERLAP_MEAN) / (OVERLAP_SIGMA / len(ov) ** 0.5)), float(np.abs(ov - OVERLAP_MEAN).max() / OVERLAP_SIGMA)


def restated_draws(seed, Bt, w_row, K):
    """(Bt, K) selections of the restated sampler (float64 keys) on Bt copies of one weight row."""
    k = keys64(np.broadcast_to(w_row, (Bt, len(w_row))), uniforms(seed, Bt, len(w_row)))
    return np.stack([select(r, K) for r in k])
