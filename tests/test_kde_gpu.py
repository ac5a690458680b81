"""Every route of csrc/kde.hip against float64 (oracle_kde, oracle/gfnet_oracle.c, pinned by tests/test_kde_cpu.py).

Routes (a pure function of the arguments; the rules of kde.hip are restated below and asserted per case):
  dense   gfn_kde_density, D == 4 with scratch for the pre-scaled copies: kde4_kernel, MS = gfn_kde_msplit() splits over M
  generic gfn_kde_density, D != 4 or no (or misaligned) scratch: kde_generic_kernel, same split
  culled  gfn_kde_density_sorted, x != y or N != M: kde4_mfma_kernel<false> (+ kde_combine_kernel when MS > 1 or perm)
  sym     gfn_kde_density_sorted, x == y and N == M: kde4_mfma_kernel<true> + kde_combine_kernel
The reference sees exactly the float32 values the kernel sees.  Tolerance: 1e-4 relative on every route (README; the
difference-form kernels hold it with two orders of margin).  Where a density can be arbitrarily small (a query far from every
reference point) the culled routes get M * 2^-32 absolute on top, the truncation kde.hip promises for its 6.7-std cut-off.
Every comparison prints its worst error as a `KDE_ERR` line (pytest -s); DESIGN.md holds the table measured on an MI355X.
"""
import ctypes

import numpy as np
import pytest
import torch

import kde_cases as cases
import oracle

pytestmark = pytest.mark.gpu
RTOL = 1e-4
CUT = 2.0 ** -32  # a culled term is below this (kKdeCutoffLog2 = 32)
SIZES = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 4095, 4096, 4097]
STD_MIN_CULLED = 0.0625  # ops.KDE_CULL_MIN_STD: the smallest std the matrix-core routes accept (include/gfnet_hip.h)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def ref64(x, y, std):
    """float64 density of the float32 rows x (N,D) against y (M,D): differences, squares and sums in double."""
    x, y = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(y, np.float32)
    N, D = x.shape
    assert y.shape[1] == D and N * len(y) <= 20000 * 20000
    out = np.empty(N, np.float64)
    for n0 in range(0, N, 4096):  # chunked over the queries
        n1 = min(N, n0 + 4096)
        oracle.lib("f64").oracle_kde(x[n0:n1].ctypes.data_as(ctypes.c_void_p), ctypes.c_int(n1 - n0), y.ctypes.data_as(ctypes.c_void_p),
                                     ctypes.c_int(len(y)), ctypes.c_int(D), ctypes.c_double(std), out[n0:n1].ctypes.data_as(ctypes.c_void_p))
    return out


def check(got, ref, what, atol=0.0):
    """|got - ref| <= 1e-4 * ref + atol, element by element; prints the worst relative error first."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, what
    assert np.isfinite(got).all(), f"{what}: non-finite density"
    err = np.abs(got - ref)
    rel = float(np.max(err / np.maximum(ref, 1e-300))) if atol == 0.0 else float(np.max(np.maximum(err - atol, 0) / np.maximum(ref, 1e-300)))
    print(f"KDE_ERR {what} worst_rel={rel:.3e}")
    bad = err > RTOL * ref + atol
    assert not bad.any(), f"{what}: worst relative error {rel:.3e} > {RTOL:.0e} at {int(np.argmax(err - RTOL * ref - atol))}"
    return rel


# ---- the routing rules of kde.hip, restated ---------------------------------------------------------------------------------
def dense_ms(Bt, N, M):
    blocks, ms = Bt * ((N + 255) // 256), 1
    while blocks * ms < 2048 and M // (ms * 2) >= 512:
        ms *= 2
    return ms


def culled_ms(Bt, N, M):
    Mp = (M + 1) & ~1
    nblk, blocks, ms = (Mp + 63) // 64, Bt * ((N + 255) // 256), 1
    while blocks * ms < 2048 and nblk // (ms * 2) >= 8 and ms < 32:
        ms *= 2
    return ms


def L():
    from gfnet_amd import _lib

    return _lib.lib()


def test_restated_split_rules_match_the_library():
    for Bt, N, M in [(1, 777, 777), (1, 3000, 3000), (2, 2100, 2100), (32, 10000, 10000), (1, 1, 1), (3, 4097, 4097), (1, 5000, 1025)]:
        assert L().gfn_kde_msplit(Bt, N, M) == dense_ms(Bt, N, M)
    assert dense_ms(1, 777, 777) == 1 and dense_ms(1, 3000, 3000) == 4 and dense_ms(2, 2100, 2100) == 4
    assert culled_ms(1, 257, 257) == 1 and culled_ms(1, 4096, 4096) == 8 and culled_ms(3, 4097, 4097) == 8 and culled_ms(32, 10000, 10000) == 2


# ---- C ABI, called directly --------------------------------------------------------------------------------------------------
def abi_density(x, y, std, M=None, rs=None, bs=None, scratch="full", misalign=False):
    """gfn_kde_density on (Bt,N,D) / (Bt,My,D) device tensors; scratch: "full" | "pre" (pre-scaled copies only) | None."""
    from gfnet_amd import _lib

    Bt, N, D = x.shape
    M = y.shape[1] if M is None else M
    rs = D if rs is None else rs
    bs = y.shape[1] * D if bs is None else bs
    out = torch.full((Bt, N), -1.0, device="cuda")
    Mp = (M + 1) & ~1
    n = {"full": int(L().gfn_kde_scratch_floats(Bt, N, M, D)), "pre": Bt * N * 4 + Bt * Mp * 4, None: 0}[scratch]
    buf = torch.empty(n + 8, device="cuda")
    sp = buf[1:] if misalign else buf
    _lib.check(L().gfn_kde_density(_lib.ptr(x), _lib.ptr(y), _lib.ptr(out), Bt, N, M, D, rs, bs, float(std), _lib.ptr(sp) if scratch else None,
                                   n, _lib.stream_ptr(x.device)), "gfn_kde_density")
    return host(out)


def abi_sorted(x, y, std, perm=None, round_fp16=False, same=False):
    """gfn_kde_density_sorted on Morton-sorted (Bt,N,4) / (Bt,M,4) device tensors; same: y is x (the symmetric kernel)."""
    from gfnet_amd import _lib

    Bt, N, _ = x.shape
    M = N if same else y.shape[1]
    out = torch.full((Bt, N), -1.0, device="cuda")
    n = int(L().gfn_kde_sorted_scratch_floats(Bt, N, M))
    buf = torch.empty(n, device="cuda")
    _lib.check(L().gfn_kde_density_sorted(_lib.ptr(x), _lib.ptr(x if same else y), _lib.ptr(out), _lib.ptr(perm), Bt, N, M, float(std),
                                          1 if round_fp16 else 0, _lib.ptr(buf), n, _lib.stream_ptr(x.device)), "gfn_kde_density_sorted")
    return host(out)


def morton_sorted(x):
    from gfnet_amd import ops

    xs, perm = ops._morton_sorted(x, x.device, long_perm=False)
    return xs, perm


# ---- dense and generic routes ------------------------------------------------------------------------------------------------
GEOMS = ["match", "outliers", "identical", "kfold", "clusters32", "line", "lattice", "one_cell", "outside", "satellite"]


@pytest.mark.parametrize("geom", GEOMS + ["extent3", "extent10"])
@pytest.mark.parametrize("N", [1, 33, 777, 3000])
def test_dense_kde4_kernel_every_geometry(geom, N):
    from gfnet_amd import ops

    x = cases.make(geom, N, seed=N)
    ms = dense_ms(1, N, N)
    assert (ms > 1) == (N == 3000)  # kde4_kernel alone / kde4_kernel + kde_reduce_kernel
    got = host(ops.kde_density(dev(x), std=0.1, cull=False))
    check(got, ref64(x, x, 0.1), f"route=dense ms={ms} geom={geom} N={N} std=0.1")
    if geom == "identical":
        assert np.array_equal(got, np.full(N, float(N), np.float32))  # differences are exactly 0, the sum of N ones is exact


@pytest.mark.parametrize("std", [0.3, 0.2, 0.1, 0.05, 0.02, 0.01])
@pytest.mark.parametrize("N", [777, 3000])
def test_dense_kde4_kernel_every_std(std, N):
    from gfnet_amd import ops

    x = cases.make("outliers", N, seed=5)
    check(host(ops.kde_density(dev(x), std=std, cull=False)), ref64(x, x, std), f"route=dense ms={dense_ms(1, N, N)} geom=outliers N={N} std={std}")


@pytest.mark.parametrize("D", [1, 2, 3, 5, 8])
@pytest.mark.parametrize("N", [300, 2100])
def test_generic_kernel_point_dimensions(D, N):
    """D != 4 always takes kde_generic_kernel; two batch rows with different points (the batch stride of y is used)."""
    from gfnet_amd import ops

    rng = np.random.default_rng(D * 100 + N)
    x = rng.uniform(-1, 1, size=(2, N, D)).astype(np.float32)
    x[1] = 0.5 * x[1] + 0.2
    y = rng.uniform(-1, 1, size=(2, N // 2 + 1, D)).astype(np.float32)
    assert (dense_ms(2, N, N) > 1) == (N == 2100)
    std = 0.1 * np.sqrt(D / 4.0) + 0.05  # keeps the densities of sparse high-D sets away from underflow
    got, goty = host(ops.kde_density(dev(x), std=std)), host(ops.kde_density(dev(x), dev(y), std=std))
    for b in range(2):
        check(got[b], ref64(x[b], x[b], std), f"route=generic D={D} N={N} row={b} std={std:.3f}")
        check(goty[b], ref64(x[b], y[b], std), f"route=generic-y D={D} N={N} row={b} std={std:.3f}", atol=1e-30)


@pytest.mark.parametrize("D", [4, 5])
@pytest.mark.parametrize("down", [2, 3, 8])
def test_strided_reference_points(D, down):
    """y = x[::down] as a strided view (y_row_stride = down * D), N not a multiple of down: M = ceil(N / down)."""
    from gfnet_amd import ops

    N = 1001
    assert N % down
    rng = np.random.default_rng(down)
    x = rng.uniform(-1, 1, size=(2, N, D)).astype(np.float32)
    x[1] *= 0.5
    got = host(ops.kde_density(dev(x), dev(x), std=0.2, y_row_stride=down * D, cull=False))
    for b in range(2):
        y = x[b, ::down]
        assert len(y) == (N + down - 1) // down
        check(got[b], ref64(x[b], y, 0.2), f"route={'dense' if D == 4 else 'generic'}-strided D={D} down={down} row={b} std=0.2")
    # the same through the C ABI without scratch: kde_generic_kernel at D = 4 too
    got0 = abi_density(dev(x), dev(x), 0.2, M=(N + down - 1) // down, rs=down * D, bs=N * D, scratch=None)
    for b in range(2):
        check(got0[b], ref64(x[b], x[b, ::down], 0.2), f"route=generic-noscratch-strided D={D} down={down} row={b} std=0.2")


@pytest.mark.parametrize("geom", ["outliers", "kfold", "extent10"])
def test_scratch_fallbacks_of_gfn_kde_density(geom):
    """D = 4, N = M = 3000 (MS = 4 with full scratch).  Scratch for the pre-scaled copies only: kde4_kernel in one pass.  No scratch, or
    a misaligned one: kde_generic_kernel.  Every one of them is held to the same 1e-4 against float64."""
    N = 3000
    x = np.stack((cases.make(geom, N, seed=1), cases.make("match", N, seed=2)))
    xd = dev(x)
    assert dense_ms(2, N, N) == 4
    for scratch, mis, route in (("full", False, "dense ms=4"), ("pre", False, "dense one-pass"), (None, False, "generic-noscratch"),
                                ("full", True, "generic-misaligned")):
        got = abi_density(xd, xd, 0.1, scratch=scratch, misalign=mis)
        for b in range(2):
            check(got[b], ref64(x[b], x[b], 0.1), f"route={route} geom={geom} N={N} row={b} std=0.1")


# ---- culled routes: sizes ----------------------------------------------------------------------------------------------------
ROW_GEOMS = ["match", "clusters32", "outliers", "kfold", "identical", "lattice", "one_cell", "outside", "line", "satellite"]


def batch(Bt, N, seed):
    """Bt rows of one batch, every row another geometry"""
    return np.stack([cases.make(ROW_GEOMS[(b + seed) % len(ROW_GEOMS)], N, seed=seed + b) for b in range(Bt)])


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("Bt", [1, 3])
def test_symmetric_route_at_every_edge_size(N, Bt):
    """kde4_mfma_kernel<true> at the wave (64), tile (32), workgroup (256) and auto-cull (4096) edges: the ragged last block must not
    leak padding rows into the column sums.  Rows of different geometry, each against float64; bit-identical from run to run."""
    from gfnet_amd import ops

    x = batch(Bt, N, seed=N % 7)
    xd = dev(x)
    ms = culled_ms(Bt, N, N)
    assert (ms > 1) == (N >= 4095)
    got = host(ops.kde_density(xd, std=0.1, cull=True))
    assert np.array_equal(got, host(ops.kde_density(xd, std=0.1, cull=True)))
    for b in range(Bt):
        check(got[b], ref64(x[b], x[b], 0.1), f"route=sym ms={ms} geom={ROW_GEOMS[(b + N % 7) % len(ROW_GEOMS)]} N={N} Bt={Bt} row={b} std=0.1")


@pytest.mark.parametrize("N", [33, 257, 4097])
def test_symmetric_route_32_rows(N):
    from gfnet_amd import ops

    Bt = 32
    x = batch(Bt, N, seed=3)
    ms = culled_ms(Bt, N, N)
    assert ms == (1 if N < 4097 else 4)
    got = host(ops.kde_density(dev(x), std=0.1, cull=True))
    for b in range(Bt):
        check(got[b], ref64(x[b], x[b], 0.1), f"route=sym ms={ms} geom={ROW_GEOMS[(b + 3) % len(ROW_GEOMS)]} N={N} Bt=32 row={b} std=0.1")


def test_production_row_count_32_x_10000():
    """GFNet.sample's call: 32 rows of 10000 matches, std 0.1, round_fp16, symmetric kernel with MS = 2."""
    from gfnet_amd import ops

    Bt, N = 32, 10000
    x = np.stack([cases.make("outliers" if b % 2 else "match", N, seed=b) for b in range(Bt)])
    assert culled_ms(Bt, N, N) == 2
    got = host(ops.kde_density(dev(x), std=0.1, round_fp16=True))  # automatic rule: N, M >= 4096, std <= 0.2 -> culled
    assert np.array_equal(got, host(ops.kde_density(dev(x), std=0.1, round_fp16=True, cull=True)))
    x16 = x.astype(np.float16).astype(np.float32)
    for b in range(Bt):
        check(got[b], ref64(x16[b], x16[b], 0.1), f"route=sym ms=2 geom=production N={N} Bt=32 row={b} std=0.1 fp16")


NONSYM = [(4097, 1), (257, 63), (1000, 333), (4096, 4095), (33, 129), (1, 257), (64, 64), (5000, 4097), (2, 31), (4095, 2049)]


@pytest.mark.parametrize("N,M", NONSYM)
def test_nonsymmetric_route_sizes_with_and_without_perm(N, M):
    """kde4_mfma_kernel<false>: N != M, M odd, M < 64, M = 1, MS = 1 and MS > 1.  Through ops (perm: densities come back in the
    caller's order through kde_combine_kernel) and through gfn_kde_density_sorted with perm = NULL (sorted order; straight into
    `out` when MS == 1).  y is another draw of the same geometry: a query can be far from every point, hence the absolute term."""
    from gfnet_amd import ops

    Bt = 2
    x = np.stack((cases.make("match", N, seed=N), cases.make("clusters32", N, seed=N + 1)))
    y = np.stack((cases.make("outliers", M, seed=M), cases.make("clusters32", M, seed=N + 1)))
    ms = culled_ms(Bt, N, M)
    assert (ms > 1) == (M >= 2049)
    xd, yd = dev(x), dev(y)
    got = host(ops.kde_density(xd, yd, std=0.1, cull=True))
    assert np.array_equal(got, host(ops.kde_density(xd, yd, std=0.1, cull=True)))
    xs, perm = morton_sorted(xd)
    ys, _ = morton_sorted(yd)
    plain = abi_sorted(xs, ys, 0.1)
    withperm = abi_sorted(xs, ys, 0.1, perm=perm)
    assert np.array_equal(withperm, got)
    p = host(perm).astype(np.int64)
    assert np.array_equal(np.take_along_axis(got, p, axis=1), plain)  # the same sums, written in the other order
    for b in range(Bt):
        check(got[b], ref64(x[b], y[b], 0.1), f"route=culled ms={ms} N={N} M={M} row={b} std=0.1", atol=M * CUT)


# ---- culled routes: geometry, std, extent -----------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", GEOMS)
@pytest.mark.parametrize("N", [257, 4097])
def test_culled_routes_every_geometry(geom, N):
    from gfnet_amd import ops

    x = cases.make(geom, N, seed=N + 11)
    xd = dev(x[None])
    ref = ref64(x, x, 0.1)
    sym = host(ops.kde_density(xd, std=0.1, cull=True))[0]
    non = host(ops.kde_density(xd, xd.clone(), std=0.1, cull=True))[0]
    check(sym, ref, f"route=sym geom={geom} N={N} std=0.1")
    check(non, ref, f"route=culled geom={geom} N={N} std=0.1")
    np.testing.assert_allclose(non, sym, rtol=2e-5)
    if geom == "identical":
        np.testing.assert_allclose(sym, N, rtol=RTOL)


def test_satellite_point_gets_its_column_sums():
    """20000 points: 19999 copies of one point and one point 6 std away, last along the curve.  Its density is 1 + 19999 terms of
    1.34e-8, which reach it 64 at a time (8.6e-7) through the fixed-point column accumulator of the symmetric kernel: 2.7e-4 of the
    density in pieces that an accumulator coarser than 2^-21 would drop."""
    from gfnet_amd import ops

    N = 20000
    x = cases.make("satellite", N)
    keys = cases.curve_key16(x[[0, N - 1]])
    assert keys[1] > keys[0]
    ref = ref64(x, x, 0.1)
    assert 2.5e-4 < ref[N - 1] - 1 < 2.9e-4
    got = host(ops.kde_density(dev(x), std=0.1, cull=True))
    check(got, ref, "route=sym geom=satellite N=20000 std=0.1")
    assert abs((got[N - 1] - 1) - (ref[N - 1] - 1)) < 0.3 * (ref[N - 1] - 1)  # the cross terms themselves arrived


STD_EXTENT = [(s, e) for e in (1, 3, 10) for s in (0.3, 0.2, 0.1, 0.0625, 0.05, 0.02, 0.01)] + [(0.1, 1.6), (0.2, 3.2), (0.3, 4.8)]


@pytest.mark.parametrize("std,extent", STD_EXTENT)
def test_culled_routes_std_and_extent(std, extent):
    """The matrix-core routes form the exponent as |x|^2 + |y|^2 - 2 x.y in fp32 accumulators: its error grows with
    (extent / std)^2, not with the distance.  For coordinates within +-E the accumulators carry up to
    log2(e) / (2 std^2) * 8 E^2 = 5.8 (E / std)^2, which stays below 2048 (one fp32 ulp = 2^-13, i.e. 8.5e-5 relative on a term) up
    to E = 16 std: that is the supported domain of the routes (include/gfnet_hip.h), chosen from the number format, and the cases
    (0.0625, 1), (0.1, 1.6), (0.2, 3.2), (0.3, 4.8) sit on its edge.
      * inside the domain every route is held to 1e-4;
      * std < 1/16 (the edge for image coordinates): ops.kde_density's automatic rule takes the dense kernels and is held to
        1e-4 there, cull=True is refused, gfn_kde_density_sorted refuses at the ABI;
      * std >= 1/16 with points beyond 16 std: the extent is only known on the device and is not checked (documented domain, no
        per-row fallback).  The dense route is held to 1e-4; the culled routes are MEASURED, printed and not asserted -- on an
        MI355X: 1.8e-4 at (0.1, 3), 2.8e-3 at (0.1, 10), 5.2e-4 at (0.0625, 3), 2.8e-4 at (0.3, 10)."""
    from gfnet_amd import _lib, ops

    N = 4097
    x = cases.make("outliers" if extent == 1 else f"extent{extent}", N, seed=int(std * 1000))
    assert np.abs(x[:, :2]).max() > 0.95 * extent
    xd = dev(x[None])
    ref = ref64(x, x, std)
    tag = f"geom=match N={N} std={std} extent={extent}"
    dense = host(ops.kde_density(xd, std=std, cull=False))[0]
    check(dense, ref, f"route=dense {tag}")
    auto = host(ops.kde_density(xd, std=std))[0]
    if std < STD_MIN_CULLED:
        assert ops.KDE_CULL_MIN_STD == STD_MIN_CULLED
        assert np.array_equal(auto, dense)  # the automatic rule went to kde4_kernel
        with pytest.raises(ValueError):
            ops.kde_density(xd, std=std, cull=True)
        xs, _ = morton_sorted(xd)
        with pytest.raises(_lib.GfnError, match="std"):
            abi_sorted(xs, None, std, same=True)
        return
    sym = host(ops.kde_density(xd, std=std, cull=True))[0]
    non = host(ops.kde_density(xd, xd.clone(), std=std, cull=True))[0]
    assert np.array_equal(auto, sym if std <= 0.2 else dense)
    if extent <= 16 * std:
        check(sym, ref, f"route=sym {tag}")
        check(non, ref, f"route=culled {tag}")
    else:
        for route, got in (("sym", sym), ("culled", non)):
            assert np.isfinite(got).all()
            print(f"KDE_ERR route={route} {tag} OUTSIDE-DOMAIN worst_rel={float(np.max(np.abs(got - ref) / ref)):.3e}")


@pytest.mark.parametrize("log2_term", [8, 15, 17, 24, 31, 31.9, 32.1, 33, 40])
@pytest.mark.parametrize("N,M", [(257, 129), (4097, 4097)])
def test_cutoff_sweep_between_two_clusters(log2_term, N, M):
    """Queries in one tight cluster, reference points in another, the gap such that a term is 2^-log2_term: just inside, at and
    just outside the 6.7-std cut-off (2^-32).  The density IS the cross term, so the truncation claim is tested rather than quoted:
    |culled - float64| and |culled - dense| stay below M * 2^-32 absolute plus 1e-4 relative.  (Rounding of the sums: M fp32
    additions of positive terms are off by at most (M / 2) * 2^-24 of the density in the worst case, which at M = 4097 is already
    1.2e-4; the parity bar 1e-4 is the tighter of the two and is what is used.)  A cut-off at 2^-16 would lose M * 2^-17 here."""
    from gfnet_amd import ops

    std = 0.1
    gap = cases.satellite_distance(std, 2.0 ** -log2_term)
    rng = np.random.default_rng(int(log2_term * 10))
    x = (np.array([-0.5, 0.2, -0.4, 0.1]) + 1e-3 * rng.uniform(-1, 1, size=(N, 4))).astype(np.float32)
    y = (np.array([-0.5 + gap, 0.2, -0.4, 0.1]) + 1e-3 * rng.uniform(-1, 1, size=(M, 4))).astype(np.float32)
    ref = ref64(x, y, std)
    culled = host(ops.kde_density(dev(x), dev(y), std=std, cull=True))
    dense = host(ops.kde_density(dev(x), dev(y), std=std, cull=False))
    check(dense, ref, f"route=dense geom=gap{log2_term} N={N} M={M} std=0.1", atol=1e-30)
    check(culled, ref, f"route=culled geom=gap{log2_term} N={N} M={M} std=0.1", atol=M * CUT)
    assert np.all(np.abs(culled.astype(np.float64) - dense) <= M * CUT + RTOL * ref)
    # both clusters in one symmetric call: density = own cluster + cross terms
    z = np.concatenate((x, y))
    check(host(ops.kde_density(dev(z), std=std, cull=True)), ref64(z, z, std), f"route=sym geom=gap{log2_term} N={N + M} std=0.1")


@pytest.mark.parametrize("N", [257, 4097])
def test_isolated_point(N):
    """One point 30 std from everything: symmetric density exactly its self term; as a query against the others alone, 0 within
    the truncation bound."""
    from gfnet_amd import ops

    x = cases.make("match", N, seed=9)
    x[N // 2] = [0.3, -0.2, 4.0, 0.1]
    for route, cull in (("sym", True), ("dense", False)):
        got = host(ops.kde_density(dev(x), std=0.1, cull=cull))
        check(got, ref64(x, x, 0.1), f"route={route} geom=isolated N={N} std=0.1")
        assert abs(got[N // 2] - 1.0) <= RTOL
    others = np.delete(x, N // 2, axis=0)
    got = host(ops.kde_density(dev(x), dev(others), std=0.1, cull=True))
    check(got, ref64(x, others, 0.1), f"route=culled geom=isolated-query N={N} std=0.1", atol=(N - 1) * CUT)
    assert got[N // 2] <= (N - 1) * CUT


# ---- bitwise properties ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [257, 4097])
def test_rows_are_independent_and_poison_is_contained(N):
    """Rows of a batch are independent: the same row inside a larger batch, or next to a changed row, is bit-identical (the split MS is
    the same for Bt = 1 and 3 at these sizes).  A row with a NaN or an infinite coordinate in one point (no address in kde.hip depends
    on a coordinate value: curve_key16 clamps through fmaxf / fminf, which drop a NaN) leaves every other row exact.  What the
    poisoned row itself returns is pinned per route:
      dense            what float64 gives: NaN in a point -> every density of the row NaN; inf -> that point NaN, and it is gone from
                       every other sum
      culled           the poisoned point's own density is NaN; every other density of the row is NaN (its tile met the point's tile) or
                       within 1e-4 of the float64 density with or without that point (the tile was culled, or the term is 0)
      sym              the poisoned point's own density is NaN; every other density is NaN or at most the clean one: a column sum
                       that went NaN is dropped as a whole by the fixed-point conversion, so terms can be lost, never invented
                       The reference's cdist gives NaN for the whole row; the difference is documented in DESIGN.md.
    """
    from gfnet_amd import ops

    assert culled_ms(1, N, N) == culled_ms(3, N, N)
    x = batch(3, N, seed=0)
    xd = dev(x)
    for route, kw in (("sym", dict(cull=True)), ("culled", dict(cull=True, y=True)), ("dense", dict(cull=False))):
        def run(t):
            return host(ops.kde_density(t, t.clone() if kw.get("y") else None, std=0.1, cull=kw["cull"]))

        full = run(xd)
        for b in range(3):
            assert np.array_equal(run(xd[b:b + 1])[0], full[b]), f"{route}: row {b} alone != inside the batch"
        for bad in (np.nan, np.inf, -np.inf):
            xp = x.copy()
            k = N // 3
            xp[1, k, 2] = bad
            got = run(dev(xp))
            assert np.array_equal(got[0], full[0]) and np.array_equal(got[2], full[2]), f"{route}: {bad} leaked into another row"
            row = got[1]
            with_pt = ref64(x[1], x[1], 0.1)
            without = ref64(x[1], np.delete(x[1], k, axis=0), 0.1)
            print(f"KDE_POISON route={route} N={N} bad={bad} nan={int(np.isnan(row).sum())} inf={int(np.isinf(row).sum())} own={row[k]}")
            assert np.isnan(row[k]), f"{route}: the poisoned point's own density is {row[k]}"
            if route == "dense":
                want = np.full(N, np.nan) if np.isnan(bad) else without
                fin = ~np.isnan(want)
                fin[k] = False
                assert np.array_equal(np.isnan(row), ~fin)
                if fin.any():
                    check(row[fin], want[fin], f"route=dense geom=poison{bad} N={N} std=0.1")
            else:
                fin = ~np.isnan(row)
                assert not np.isinf(row).any()
                assert (row[fin] >= 0).all() and (row[fin] <= with_pt[fin] * (1 + RTOL)).all(), f"{route}: a density above the clean one"
                if route == "culled":
                    ok = (np.abs(row - with_pt) <= RTOL * with_pt) | (np.abs(row - without) <= RTOL * without)
                    assert ok[fin].all(), f"{route}: a finite density of the poisoned row is neither with nor without the point"


@pytest.mark.parametrize("N", [257, 4097])
def test_round_fp16_equals_rounding_in_torch(N):
    from gfnet_amd import ops

    x = batch(2, N, seed=4)
    xd = dev(x)
    x16 = x.astype(np.float16).astype(np.float32)
    assert torch.equal(ops.kde_density(xd, std=0.1, cull=False, round_fp16=True), ops.kde_density(xd.half().float(), std=0.1, cull=False))
    for y in (None, xd.clone()):
        r1 = host(ops.kde_density(xd, y, std=0.1, cull=True, round_fp16=True))
        r2 = host(ops.kde_density(xd.half().float(), None if y is None else y.half().float(), std=0.1, cull=True))
        np.testing.assert_allclose(r1, r2, rtol=2e-5)  # the curve keys see the unrounded points: the sums are taken in another order
        for b in range(2):
            check(r1[b], ref64(x16[b], x16[b], 0.1), f"route={'sym' if y is None else 'culled'} geom=fp16 N={N} row={b} std=0.1")
    d = host(ops.kde_density(xd, std=0.1, cull=False, round_fp16=True))
    for b in range(2):
        check(d[b], ref64(x16[b], x16[b], 0.1), f"route=dense geom=fp16 N={N} row={b} std=0.1")


@pytest.mark.parametrize("N", [257, 4097])
def test_permuting_the_rows_permutes_the_densities(N):
    from gfnet_amd import ops

    x = cases.make("outliers", N, seed=21)
    p = np.random.default_rng(N).permutation(N)
    for cull in (False, True):
        a = host(ops.kde_density(dev(x), std=0.1, cull=cull))
        b = host(ops.kde_density(dev(x[p]), std=0.1, cull=cull))
        np.testing.assert_allclose(b, a[p], rtol=2e-5)  # the same terms in another order of summation
    ref = ref64(x, x, 0.1)
    check(host(ops.kde_density(dev(x[p]), std=0.1, cull=True)), ref[p], f"route=sym geom=permuted N={N} std=0.1")


# ---- the public function -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("half", [True, False])
@pytest.mark.parametrize("down", [None, 1, 3])
@pytest.mark.parametrize("N", [1000, 5000])
def test_utils_kde(half, down, N):
    """utils.kde.kde: half=True rounds the inputs to fp16 and returns fp16: one more rounding of 2^-11 on the result, or of 2^-25
    absolute below fp16's normal range (with down = 3 a query that is not a reference point can have a density that small)."""
    from gfnet_amd.utils.kde import kde

    x = cases.make("outliers", N, seed=N)
    got = kde(dev(x), 0.1, half=half, down=down)
    assert got.dtype == (torch.float16 if half else torch.float32) and tuple(got.shape) == (N,)
    xr = x.astype(np.float16).astype(np.float32) if half else x
    ref = ref64(xr, xr[::down] if down else xr, 0.1)
    np.testing.assert_allclose(ref, oracle.kde(x, 0.1, half=half, down=down, variant="f64"), rtol=1e-12)
    got = host(got.float()).astype(np.float64)
    tol = RTOL + (2.0 ** -11 * (1 + RTOL) if half else 0.0)
    atol = 2.0 ** -25 if half else 0.0
    rel = float(np.max(np.maximum(np.abs(got - ref) - atol, 0) / ref))
    print(f"KDE_ERR route=kde() half={half} down={down} N={N} worst_rel={rel:.3e}")
    assert rel <= tol


# ---- the sort key ------------------------------------------------------------------------------------------------------------
def test_curve_key16_matches_its_restatement():
    """gfn_kde_morton_keys against cases.curve_key16 on a grid that holds the clamped outside, -1, +1, the cell edges k / 128 - 1 with
    their fp32 neighbours, +-inf and NaN."""
    from gfnet_amd import _lib

    edges = [-np.inf, -3.0, -1.0000001, -1.0, -0.99999994, 1.0, 0.99999994, 1.0000001, 3.0, np.inf, np.nan, 0.0, -0.0]
    for k in (1, 2, 63, 64, 127, 128, 129, 200, 254, 255):
        e = np.float32(k / 128.0 - 1.0)
        edges += [e, np.nextafter(e, np.float32(-2)), np.nextafter(e, np.float32(2))]
    edges += list(np.random.default_rng(0).uniform(-1.2, 1.2, 40))
    v = np.array(edges, np.float32)
    gx, gy = np.meshgrid(v, v, indexing="ij")
    pts = np.stack((gx.ravel(), gy.ravel(), np.zeros(gx.size, np.float32), np.ones(gx.size, np.float32)), -1).astype(np.float32)
    keys = torch.empty(len(pts), device="cuda", dtype=torch.int32)
    pd = dev(pts)
    _lib.check(L().gfn_kde_morton_keys(_lib.ptr(pd), _lib.ptr(keys), len(pts), _lib.stream_ptr(pd.device)), "gfn_kde_morton_keys")
    got = host(keys).astype(np.int64)
    want = cases.curve_key16(pts)
    assert got.min() >= 0 and got.max() <= 65535
    assert np.array_equal(got, want), f"first mismatch at {pts[np.argmax(got != want)]}"
    assert len(np.unique(want)) > 500  # the grid reaches many cells
