"""The symmetric KDE kernel's workgroup map and its column sums over 0 to 20 blocks (csrc/kde.hip: kde_wg).

kde4_mfma_kernel runs on a one-dimensional grid whose linear workgroup id is unpacked into (x, ms, bt) by kde_wg(); a wave sends the
column value of every surviving off-diagonal block to the fixed-point accumulators of that block's points.  The map changes no
wave's arithmetic: a wrong or non-bijective map shows as a row that depends on its place in the batch.  The second test walks the
number of column values a wave sends through every count from 0 to 20, i.e. across the edges (0, 7, 8, 9, 16, 17) of a scheme that
batches them eight at a time -- one was built and measured level, kde.hip sends them one by one -- on geometries where a column
value that is dropped, repeated or misplaced is a density that misses float64.

The bound is the one tests/test_kde_gpu.py holds the symmetric route to: |got - ref| <= 1e-4 * ref, element by element, against
the float64 oracle on the float32 points the kernel sees.
"""
import ctypes

import numpy as np
import pytest
import torch

import kde_cases as cases
import oracle

pytestmark = pytest.mark.gpu
RTOL = 1e-4
STD = 0.1
RING = 8  # the batch whose edges the block counts cross


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ref64(x):
    """float64 density of the float32 rows x (N,4) against themselves"""
    x = np.ascontiguousarray(x, np.float32)
    out = np.empty(len(x), np.float64)
    oracle.lib("f64").oracle_kde(x.ctypes.data_as(ctypes.c_void_p), ctypes.c_int(len(x)), x.ctypes.data_as(ctypes.c_void_p), ctypes.c_int(len(x)),
                                 ctypes.c_int(4), ctypes.c_double(STD), out.ctypes.data_as(ctypes.c_void_p))
    return out


def check(got, ref, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all(), what
    err = np.abs(got - ref)
    print(f"KDE_ERR {what} worst_rel={float(np.max(err / ref)):.3e}")
    bad = err > RTOL * ref
    assert not bad.any(), f"{what}: worst relative error {float(np.max(err / ref)):.3e} > {RTOL:.0e} at {int(np.argmax(err - RTOL * ref))}"


def culled_ms(Bt, N):
    """the split rule of gfn_kde_density_sorted, restated (tests/test_kde_gpu.py pins it against the library)"""
    nblk, blocks, ms = (((N + 1) & ~1) + 63) // 64, Bt * ((N + 255) // 256), 1
    while blocks * ms < 2048 and nblk // (ms * 2) >= 8 and ms < 32:
        ms *= 2
    return ms


# ---- batch position -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("round_fp16", [False, True])
def test_a_row_does_not_depend_on_its_batch_position(round_fp16):
    """Five different point sets of 777 points (13 blocks; 4 workgroups per row, the last one with 9 queries): every row of the
    batched call has the bits of the same set run alone (Bt = 1: the map is the identity in bt) and of the same set at another
    position of another batch.  A map that sends two ids to one (x, ms, bt), or a workgroup to another row's bt, breaks this."""
    from gfnet_amd import ops

    N = 777
    geoms = ["match", "outliers", "clusters32", "kfold", "one_cell"]
    x = dev(np.stack([cases.make(g, N, seed=40 + i) for i, g in enumerate(geoms)]))
    kw = dict(std=STD, cull=True, round_fp16=round_fp16)
    assert culled_ms(5, N) == 1 and culled_ms(1, N) == 1
    got = ops.kde_density(x, **kw)
    assert torch.equal(got, ops.kde_density(x, **kw))
    order = [3, 4, 0, 1, 2]  # no row keeps its place
    moved = ops.kde_density(x[order].contiguous(), **kw)
    for b, g in enumerate(geoms):
        alone = ops.kde_density(x[b:b + 1].contiguous(), **kw)
        assert torch.equal(got[b], alone[0]), f"{g}: row {b} of the batch differs from the set run alone"
        assert torch.equal(got[b], moved[order.index(b)]), f"{g}: row {b} differs at batch position {order.index(b)}"
    assert len({got[b].cpu().numpy().tobytes() for b in range(5)}) == 5  # five different rows did come back


# ---- block counts ---------------------------------------------------------------------------------------------------------------
N_RING = 1300  # 21 blocks of 64


def tight_cluster(seed):
    """every point within 0.1 std of one centre: no block is culled, every off-diagonal block a wave visits sends a column value"""
    rng = np.random.default_rng(7000 + seed)
    c = rng.uniform(-0.8, 0.8, size=4)
    return (c + 0.01 * rng.uniform(-1, 1, size=(N_RING, 4))).astype(np.float32)


def far_clusters(seed):
    """two clusters 10 std apart in the A image (the blocks of one are culled for the waves of the other; the block that straddles
    both is not), the second one small, and a satellite 4.4 std from the first that sorts last along the curve, like kde_cases'
    satellite: its cross terms (2^-14 each, 0.04 to 0.06 in all) reach it through the column sums alone, and are 400 to 600 times the
    1e-4 bound on its density, so the bound itself sees a column value that is lost or added twice (one is 64 terms: 0.004)"""
    rng = np.random.default_rng(7100 + seed)
    d = cases.satellite_distance(STD, 2.0 ** -14)
    a = np.array([0.99 - d, -0.99, 0.3, 0.3]) + 1e-3 * rng.uniform(-1, 1, size=(N_RING, 4))
    nb = 300 + 37 * seed
    a[:nb] = np.array([0.99 - d - 1.0, -0.99, 0.3, 0.3]) + 1e-3 * rng.uniform(-1, 1, size=(nb, 4))
    a = a[rng.permutation(N_RING)]
    a[N_RING - 1] = [0.99, -0.99, 0.3, 0.3]
    return a.astype(np.float32)


def column_counts(nblk, ms):
    """how many off-diagonal blocks the waves of a row visit when nothing is culled: split m of wave q walks the blocks p >= q of
    its range [m * per, m * per + per)"""
    per, out = (nblk + ms - 1) // ms, set()
    for q in range(nblk):
        for m in range(ms):
            lo, hi = max(m * per, q), min(nblk, m * per + per)
            out.add(max(0, hi - lo - (1 if lo == q else 0)))
    return out


_REF = {}


def rows_and_ref(geom):
    """eight distinct rows of a geometry and their float64 densities, computed once and shared (read-only)"""
    if geom not in _REF:
        rows = np.stack([(tight_cluster if geom == "tight" else far_clusters)(s) for s in range(8)])
        ref = np.stack([ref64(r) for r in rows])
        rows.setflags(write=False)
        ref.setflags(write=False)
        _REF[geom] = (rows, ref)
    return _REF[geom]


@pytest.mark.parametrize("geom", ["tight", "far"])
@pytest.mark.parametrize("Bt", [32, 344])
def test_column_sums_at_every_block_count(Bt, geom):
    """N = 1300 is 21 blocks.  The library splits the 32-row call in two (MS = 2, 11 blocks per split): its waves send 0 to 10
    column values, which covers a batch of eight that is empty, one short of full, full, and full plus one (0, 7, 8, 9).  With 344
    rows the call is not split and the wave of block q sends 20 - q: every count from 0 to 20, i.e. also the second full batch and
    one past it (16, 17).  The rows are eight distinct sets repeated; every row is held to float64."""
    from gfnet_amd import ops

    rows, ref = rows_and_ref(geom)
    ms = culled_ms(Bt, N_RING)
    assert ms == (2 if Bt == 32 else 1)
    counts = column_counts(21, ms)
    assert counts >= ({0, RING - 1, RING, RING + 1} | ({2 * RING, 2 * RING + 1} if ms == 1 else set())), sorted(counts)
    xd = dev(rows[np.arange(Bt) % 8])
    got = ops.kde_density(xd, std=STD, cull=True)
    assert torch.equal(got, ops.kde_density(xd, std=STD, cull=True))  # the order in which the column values arrive does not show
    got = got.cpu().numpy()
    for b in range(Bt):
        assert np.array_equal(got[b], got[b % 8]), f"row {b} differs from row {b % 8}, the same point set"
    for b in range(8):
        check(got[b], ref[b], f"route=sym ms={ms} geom={geom} N={N_RING} Bt={Bt} row={b} std={STD}")
        if geom == "far":  # the satellite's cross terms are far above the bound that check() has just applied to its density
            assert 0.03 < ref[b][-1] - 1 < 0.08
