// conv_train_common.h -- the refiner's training-mode conv block, said once for its classes.  A class K tells what the maps hold in
// HBM: K::map_t is the type of u, y, gy and gz, and K::value(v) the float a value becomes once it is stored in a map or read as an
// operand -- F32Maps (conv_stack_train.hip): float, v itself; F16Maps (conv_stack_train_half.hip, the fp16 autocast class): _Float16, v
// rounded to fp16; BF16Maps (conv_stack_train_bf16.hip, the bf16 autocast class): __bf16, v rounded to bf16 -- the two 16-bit classes
// being one template over their element (conv_train_16bit.h).  Here, for all:
//   * BatchNorm as one multiply-add (bn_affine / bn_pre: forward and backward form their ReLU mask through it) and its per-row
//     constants in LDS (stage_bn_rows)
//   * the depthwise kernels ct_dw_fwd_kernel<K, XT> and ct_dw_bwd_kernel<K, XT> (XT: the type of x and gx) on the 32x32 tile with its
//     halo (decode_tile, stage_halo, dw_taps, dw_param_partials)
//   * what the 1x1 kernels of both classes do around their GEMM loops: the masked gz and BatchNorm's partial sums after the
//     input-gradient product (pw_bwd_finish) and the partial matrix of a weight-gradient split (store_wgrad_partial)
//   * the three small reductions, which only ever see fp32 partial sums: ct_stats_kernel, ct_bn_bwd_kernel, ct_dw_wgrad_kernel
//   * the host side: the tiling (TrainShape), the workspace (TrainPlan), the argument checks and the launch sequence of both directions
//     (train_fwd, train_bwd).  A class supplies its three GEMM kernels and its split sum behind K::pw_fwd / pw_bwd / pw_wgrad /
//     pw_wgrad_sum and what it refuses beyond the common checks (K::check_class)
// Fixed-order sums everywhere, no floating-point atomics.  Opens its own anonymous namespace.
#pragma once
#include "pw_gemm_tile.h"
#include "reduce.h"

namespace {

using gfn::block_sum;
using gfn::half_wave_sum;
using gfn::wave_sum;

constexpr int kTile = 32;         // depthwise tile side in cells: 256 threads x 4 cells of a row
constexpr int kHalo = kTile + 4;  // staged side (2 cells of halo all round)
constexpr int kDwCols = 26;       // depthwise parameter gradients per channel: 25 taps + the bias
constexpr int kWgCells = 32;      // cells per wave and K step of the 1x1 weight gradient

// BatchNorm as one multiply-add per value.  Forward and backward both come through here (and -ffp-contract=off keeps the
// multiply and the add apart), so the backward's ReLU mask is the forward's, bit for bit.
__device__ __forceinline__ void bn_affine(float gamma, float beta, float mean, float invstd, float &alpha, float &betap) {
    alpha = gamma * invstd;
    betap = beta - mean * alpha;
}
__device__ __forceinline__ float bn_pre(float u, float alpha, float betap) { return u * alpha + betap; }

// thread i < rows: alpha, beta' of channel c0 + i into Al[i], Be[i] -- and, where Mn and Is are given, its mean and invstd; all zero
// past C.  LDS; the caller synchronises before it reads them
__device__ __forceinline__ void stage_bn_rows(int rows, int c0, int C, const float *gamma, const float *beta, const float *mean,
                                              const float *invstd, float *Al, float *Be, float *Mn = nullptr, float *Is = nullptr) {
    const int tid = threadIdx.x;
    if (tid < rows) {
        const int c = c0 + tid;
        float al = 0.f, be = 0.f, mn = 0.f, is = 0.f;
        if (c < C) {
            mn = mean[c], is = invstd[c];
            bn_affine(gamma[c], beta[c], mn, is, al, be);
        }
        Al[tid] = al, Be[tid] = be;
        if (Mn) Mn[tid] = mn, Is[tid] = is;
    }
}

struct TileId {
    int b, c, tile, row0, col0;
    size_t plane;  // b * C + c
};
__device__ __forceinline__ TileId decode_tile(unsigned bid, int C, int tiles_x, int tiles) {
    TileId t;
    t.tile = (int)(bid % (unsigned)tiles);
    const unsigned pl = bid / (unsigned)tiles;
    t.c = (int)(pl % (unsigned)C);
    t.b = (int)(pl / (unsigned)C);
    t.plane = pl;
    t.row0 = (t.tile / tiles_x) * kTile;
    t.col0 = (t.tile % tiles_x) * kTile;
    return t;
}

// the tile with its halo: Ts[cell] = f(the cell lies inside the map, its offset in the plane -- 0 outside)
template <typename F>
__device__ __forceinline__ void stage_halo(float *Ts, const TileId &t, int G, F f) {
    for (int e = threadIdx.x; e < kHalo * kHalo; e += 256) {
        const int hy = e / kHalo, hx = e - hy * kHalo;
        const int gy = t.row0 - 2 + hy, gx = t.col0 - 2 + hx;
        const bool ok = (unsigned)gy < (unsigned)G && (unsigned)gx < (unsigned)G;
        Ts[e] = f(ok, ok ? gy * G + gx : 0);
    }
}

// acc[q] = sum_k w[k] Ts[cell (r, c4 + q) + off_k], k = 5 dy + dx ascending: 25 fmas per cell; FLIP: w[24 - k], the transposed conv
template <bool FLIP>
__device__ __forceinline__ void dw_taps(const float *Ts, const float *wc, int r, int c4, float (&acc)[4]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q] = 0.f;
#pragma unroll
    for (int dy = 0; dy < 5; ++dy) {
        const float4 a = *reinterpret_cast<const float4 *>(&Ts[(r + dy) * kHalo + c4]);
        const float4 e = *reinterpret_cast<const float4 *>(&Ts[(r + dy) * kHalo + c4 + 4]);
        const float v[8] = {a.x, a.y, a.z, a.w, e.x, e.y, e.z, e.w};
#pragma unroll
        for (int dx = 0; dx < 5; ++dx)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] = fmaf(wc[FLIP ? 24 - (dy * 5 + dx) : dy * 5 + dx], v[q + dx], acc[q]);
    }
}

// the depthwise parameter gradients of a tile: column k < 25 is sum_p gu[p] x[p + off_k], column 25 sum_p gu[p], over the tile's
// cells (thread: the 4 cells (r, c4 .. c4 + 3)); Gs, Xs: the staged gu and x tiles with their halo -- gu is zero outside the map, so
// cells of the tile past the map's edge add nothing.  Waves, then the workgroup, in a fixed order; dst: the tile's kDwCols partials
__device__ __forceinline__ void dw_param_partials(const float *Gs, const float *Xs, int r, int c4, float (*red)[kDwCols], float *dst) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float pw[kDwCols];
    float gc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) gc[q] = Gs[(r + 2) * kHalo + c4 + 2 + q];
    pw[25] = (gc[0] + gc[1]) + (gc[2] + gc[3]);
#pragma unroll
    for (int dy = 0; dy < 5; ++dy) {
        const float4 a = *reinterpret_cast<const float4 *>(&Xs[(r + dy) * kHalo + c4]);
        const float4 e = *reinterpret_cast<const float4 *>(&Xs[(r + dy) * kHalo + c4 + 4]);
        const float v[8] = {a.x, a.y, a.z, a.w, e.x, e.y, e.z, e.w};
#pragma unroll
        for (int dx = 0; dx < 5; ++dx) {
            float s = gc[0] * v[dx];
#pragma unroll
            for (int q = 1; q < 4; ++q) s = fmaf(gc[q], v[q + dx], s);
            pw[dy * 5 + dx] = s;
        }
    }
#pragma unroll
    for (int j = 0; j < kDwCols; ++j) {
        const float s = wave_sum(pw[j]);
        if (lane == 0) red[wave][j] = s;
    }
    __syncthreads();
    if (tid < kDwCols) dst[tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}

// ---- the two depthwise kernels ----------------------------------------------------------------------------------------------------
// u = value(dw5x5(value(x), value(taps)) + b_dw) and the tile's (mean, M2 = sum (u - mean)^2) of the u that was stored: shifted sums,
// safe against cancellation.  Products of two fp16 or two bf16 values are exact in fp32, so F16Maps and BF16Maps run the fp32 tap loop
// on rounded values
template <class K, typename XT>
__global__ __launch_bounds__(256) void ct_dw_fwd_kernel(const XT *__restrict__ x, const float *__restrict__ dw_w,
                                                        const float *__restrict__ dw_b, typename K::map_t *__restrict__ u,
                                                        float *__restrict__ part, int C, int G, int tiles_x, int tiles, int nparts) {
    using map_t = typename K::map_t;
    typedef map_t map_x4 __attribute__((ext_vector_type(4)));
    __shared__ __attribute__((aligned(16))) float Xs[kHalo * kHalo];
    __shared__ float red[4];
    const int tid = threadIdx.x;
    const TileId t = decode_tile(blockIdx.x, C, tiles_x, tiles);
    const XT *xp = x + t.plane * (size_t)G * G;
    stage_halo(Xs, t, G, [&](bool ok, int off) {
        const float v = K::value(xp[off]);
        return ok ? v : 0.f;
    });
    float w[25];
#pragma unroll
    for (int k = 0; k < 25; ++k) w[k] = K::value(dw_w[(size_t)t.c * 25 + k]);
    __syncthreads();
    const int r = tid >> 3, c4 = (tid & 7) * 4;
    float acc[4];
    dw_taps<false>(Xs, w, r, c4, acc);
    const float bias = dw_b ? dw_b[t.c] : 0.f;
    const int gy = t.row0 + r, gx0 = t.col0 + c4;
    map_t *up = u + t.plane * (size_t)G * G + (size_t)gy * G + gx0;
    float uq[4], s = 0.f;
    bool ok[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        uq[q] = K::value(acc[q] + bias);
        ok[q] = gy < G && gx0 + q < G;
        s += ok[q] ? uq[q] : 0.f;
    }
    if (sizeof(map_t) == 2 && (G & 3) == 0) {  // 16-bit planes, rows and the thread's four cells all start on 8 bytes
        if (ok[0]) *reinterpret_cast<map_x4 *>(up) = map_x4{(map_t)uq[0], (map_t)uq[1], (map_t)uq[2], (map_t)uq[3]};
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (ok[q]) up[q] = (map_t)uq[q];
    }
    // the tile's mean, then its sum of squares about that mean
    const int rows = min(kTile, G - t.row0), cols = min(kTile, G - t.col0);
    const float mt = block_sum(s, red) / (float)(rows * cols);
    float d = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) d += ok[q] ? (uq[q] - mt) * (uq[q] - mt) : 0.f;
    const float m2 = block_sum(d, red);
    if (tid == 0) {
        float *p = part + ((size_t)t.c * nparts + (size_t)t.b * tiles + t.tile) * 2;
        p[0] = mt;
        p[1] = m2;
    }
}

// gu = alpha*(gz - dbeta/N - u_hat*dgamma/N) in fp32 while the gz / u halo tile is staged; gx = dw5x5 of gu with value(taps), flipped
// (the forward's stage_halo and dw_taps), written in x's type unrounded; per-workgroup partials of dW_dw[c, k] = sum_p gu[p] x[p + off_k]
// and db_dw = sum gu against the value(x) the forward multiplied.  need bit 0: gx, bit 1: the partials.
template <class K, typename XT>
__global__ __launch_bounds__(256) void ct_dw_bwd_kernel(const typename K::map_t *__restrict__ gz, const typename K::map_t *__restrict__ u,
                                                        const XT *__restrict__ x, const float *__restrict__ dw_w,
                                                        const float *__restrict__ gamma, const float *__restrict__ mean,
                                                        const float *__restrict__ invstd, const float *__restrict__ dgdb,
                                                        XT *__restrict__ gx, float *__restrict__ part, int C, int G, int tiles_x, int tiles,
                                                        int nparts, float inv_n, int need) {
    __shared__ __attribute__((aligned(16))) float Gs[kHalo * kHalo];
    __shared__ __attribute__((aligned(16))) float Xs[kHalo * kHalo];
    __shared__ float red[4][kDwCols];
    const int tid = threadIdx.x;
    const TileId t = decode_tile(blockIdx.x, C, tiles_x, tiles);
    const size_t pbase = t.plane * (size_t)G * G;
    const float mn = mean[t.c], is = invstd[t.c];
    const float al = gamma[t.c] * is;  // bn_affine's alpha
    const float k1 = dgdb[C + t.c] * inv_n, k2 = dgdb[t.c] * inv_n;
    const bool want_x = need & 1, want_w = need & 2;
    stage_halo(Gs, t, G, [&](bool ok, int off) {
        const float g = (float)gz[pbase + off], uu = (float)u[pbase + off];
        return ok ? al * (g - k1 - ((uu - mn) * is) * k2) : 0.f;
    });
    if (want_w)
        stage_halo(Xs, t, G, [&](bool ok, int off) {
            const float xv = K::value(x[pbase + off]);
            return ok ? xv : 0.f;
        });
    __syncthreads();
    const int r = tid >> 3, c4 = (tid & 7) * 4;
    if (want_x) {  // gx[q] = sum_k w[k] gu[q - off_k]: the forward's taps, flipped
        float w[25];
#pragma unroll
        for (int k = 0; k < 25; ++k) w[k] = K::value(dw_w[(size_t)t.c * 25 + k]);
        float acc[4];
        dw_taps<true>(Gs, w, r, c4, acc);
        const int yy = t.row0 + r, xx0 = t.col0 + c4;
        XT *gp = gx + pbase + (size_t)yy * G + xx0;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (yy < G && xx0 + q < G) gp[q] = (XT)acc[q];
    }
    if (want_w) dw_param_partials(Gs, Xs, r, c4, red, part + ((size_t)t.c * nparts + (size_t)t.b * tiles + t.tile) * kDwCols);
}

struct Moments {
    double n, mean, m2;
};
// Chan, Golub, LeVeque: the moments of the union of two sets
__device__ __forceinline__ void merge(Moments &a, const Moments &b) {
    if (b.n == 0.0) return;
    if (a.n == 0.0) {
        a = b;
        return;
    }
    const double n = a.n + b.n, d = b.mean - a.mean;
    a.mean += d * (b.n / n);
    a.m2 += b.m2 + d * d * (a.n * b.n / n);
    a.n = n;
}

// ---- the three small reductions -----------------------------------------------------------------------------------------------------
// one wave per channel (blockIdx.x): the tiles' (mean, M2) -> mean, invstd = 1/sqrt(var + eps) with the biased variance, and the
// running buffers; Chan's merge in double, in a fixed order
__global__ __launch_bounds__(64) void ct_stats_kernel(const float *__restrict__ part, float *__restrict__ mean, float *__restrict__ invstd,
                                                      float *__restrict__ running_mean, float *__restrict__ running_var, int G, int tiles_x,
                                                      int tiles, int nparts, double momentum, double eps) {
    __shared__ double sn[64], sm[64], s2[64];
    const int c = blockIdx.x, lane = threadIdx.x;
    Moments a = {0.0, 0.0, 0.0};
    for (int i = lane; i < nparts; i += 64) {
        const int tile = i % tiles;
        const int rows = min(kTile, G - (tile / tiles_x) * kTile), cols = min(kTile, G - (tile % tiles_x) * kTile);
        const float *p = part + ((size_t)c * nparts + i) * 2;
        const Moments b = {(double)(rows * cols), (double)p[0], (double)p[1]};
        merge(a, b);
    }
    sn[lane] = a.n, sm[lane] = a.mean, s2[lane] = a.m2;
    __syncthreads();
    for (int s = 32; s >= 1; s >>= 1) {
        if (lane < s) {
            Moments p = {sn[lane], sm[lane], s2[lane]};
            const Moments q = {sn[lane + s], sm[lane + s], s2[lane + s]};
            merge(p, q);
            sn[lane] = p.n, sm[lane] = p.mean, s2[lane] = p.m2;
        }
        __syncthreads();
    }
    if (lane == 0) {
        const double n = sn[0], mu = sm[0], var = s2[0] / n;  // biased: what normalises
        mean[c] = (float)mu;
        invstd[c] = (float)(1.0 / sqrt(var + eps));
        // torch: running = (1 - momentum) * running + momentum * batch, the variance unbiased
        running_mean[c] = (float)((1.0 - momentum) * (double)running_mean[c] + momentum * mu);
        running_var[c] = (float)((1.0 - momentum) * (double)running_var[c] + momentum * (s2[0] / (n - 1.0)));
    }
}

// dgamma[c] = sum gz*u_hat, dbeta[c] = sum gz: one wave per channel, double, fixed order.  dgdb: (2, C) = dgamma, dbeta
__global__ __launch_bounds__(64) void ct_bn_bwd_kernel(const float *__restrict__ part, int nparts, int C, float *__restrict__ dgdb,
                                                       float *__restrict__ dgamma, float *__restrict__ dbeta) {
    __shared__ double s1[64], s2[64];
    const int c = blockIdx.x, lane = threadIdx.x;
    double a1 = 0.0, a2 = 0.0;
    for (int i = lane; i < nparts; i += 64) {
        const float *p = part + ((size_t)c * nparts + i) * 2;
        a1 += (double)p[0], a2 += (double)p[1];
    }
    s1[lane] = a1, s2[lane] = a2;
    __syncthreads();
    for (int s = 32; s >= 1; s >>= 1) {
        if (lane < s) s1[lane] += s1[lane + s], s2[lane] += s2[lane + s];
        __syncthreads();
    }
    if (lane == 0) {
        const float db = (float)s1[0], dg = (float)s2[0];
        dgdb[c] = dg, dgdb[C + c] = db;
        if (dgamma) dgamma[c] = dg;
        if (dbeta) dbeta[c] = db;
    }
}

// per channel: 8 groups of 32 lanes walk the partials, lane j < 26 owns column j; then the groups in a fixed order
__global__ __launch_bounds__(256) void ct_dw_wgrad_kernel(const float *__restrict__ part, int nparts, float *__restrict__ d_dw_w,
                                                          float *__restrict__ d_dw_b) {
    __shared__ double s[8][32];
    const int c = blockIdx.x, g = threadIdx.x >> 5, j = threadIdx.x & 31;
    double a = 0.0;
    if (j < kDwCols)
        for (int p = g; p < nparts; p += 8) a += (double)part[((size_t)c * nparts + p) * kDwCols + j];
    s[g][j] = a;
    __syncthreads();
    if (threadIdx.x < kDwCols) {
        double tot = 0.0;
        for (int q = 0; q < 8; ++q) tot += s[q][j];
        if (j < 25) d_dw_w[(size_t)c * 25 + j] = (float)tot;
        else if (d_dw_b) d_dw_b[c] = (float)tot;
    }
}

// ---- around the GEMM loops of the 1x1 kernels -----------------------------------------------------------------------------------------
// After gt = W^T . gy (acc: the rows c0 .. of image b, the 128 cells from n0): gz = value(gt) where u*alpha + beta' > 0 -- the
// forward's own expression, so both masks agree bit for bit -- written as a C map, and the workgroup's partial sums of that gz and
// of gz*u_hat.  part: (C, B * gridDim.x, 2).  LDS: Al, Be, Mn, Is -- stage_bn_rows' constants of the 32*MT rows -- and red, the waves'
// sums; wave, col, kh: the lane's place as the kernel's GEMM loop already holds it
template <class K, int MT>
__device__ __forceinline__ void pw_bwd_finish(const PwAcc<MT> &acc, const float *Al, const float *Be, const float *Mn, const float *Is,
                                              float (*red)[32 * MT][2], const typename K::map_t *u, typename K::map_t *gz, float *part,
                                              int b, int c0, int n0, int C, int N, int wave, int col, int kh) {
    using map_t = typename K::map_t;
    const int tid = threadIdx.x;
    const int n = n0 + wave * 32 + col;
    const bool nok = n < N;
    const size_t base = (size_t)b * C * N + (nok ? n : 0);
    acc.each(kh, [&](int row, float a) {
        const int c = c0 + row;
        const bool ok = nok && c < C;
        const size_t at = base + (size_t)(ok ? c : 0) * N;
        const float uu = (float)u[at];
        const float g = ok && bn_pre(uu, Al[row], Be[row]) > 0.f ? K::value(a) : 0.f;
        if (ok) gz[at] = (map_t)g;
        const float s1 = half_wave_sum(g);
        const float s2 = half_wave_sum(ok ? g * ((uu - Mn[row]) * Is[row]) : 0.f);
        if (col == 0) red[wave][row][0] = s1, red[wave][row][1] = s2;
    });
    __syncthreads();
    if (tid < 32 * MT && c0 + tid < C) {
        float *p = part + ((size_t)(c0 + tid) * ((size_t)gridDim.z * gridDim.x) + (size_t)b * gridDim.x + blockIdx.x) * 2;
        p[0] = (red[0][tid][0] + red[1][tid][0]) + (red[2][tid][0] + red[3][tid][0]);
        p[1] = (red[0][tid][1] + red[1][tid][1]) + (red[2][tid][1] + red[3][tid][1]);
    }
}

// the lane's column cidx (C: db_pw) of partial (M, C + 1) matrix `slot`, rows from m0: every (split, cell group) of the weight
// gradient leaves a matrix of its own
template <int MT>
__device__ __forceinline__ void store_wgrad_partial(const PwAcc<MT> &acc, float *part, size_t slot, int m0, int cidx, int kh, int M, int C) {
    if (cidx <= C) {
        float *pp = part + slot * M * (C + 1) + cidx;
        acc.each(kh, [&](int row, float v) {
            if (m0 + row < M) pp[(size_t)(m0 + row) * (C + 1)] = v;
        });
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
inline int64_t align4(int64_t floats) { return (floats + 3) / 4 * 4; }
inline bool misaligned(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) != 0; }

// how a block's maps are cut up
struct TrainShape {
    int tiles_x, tiles;     // depthwise tiles per map
    int ntn;                // 128-cell groups per map (1x1 GEMMs)
    int wg_mt, wg_cw, wg_ks, wg_tm, wg_tc, wg_s, wg_chunk, wg_parts;  // 1x1 weight gradient

    TrainShape(int B, int C, int M, int G) {
        const int64_t N = (int64_t)G * G;
        tiles_x = (G + kTile - 1) / kTile;
        tiles = tiles_x * tiles_x;
        ntn = (int)((N + kBN - 1) / kBN);
        wg_cw = C + 1 <= 32 ? 1 : C + 1 <= 64 ? 2 : 4;
        wg_ks = 4 / wg_cw;
        const int mtiles = (M + 31) / 32, mt_max = wg_cw == 1 ? 2 : 4;
        wg_mt = mtiles >= mt_max ? mt_max : (mtiles == 3 ? 4 : mtiles);
        if (wg_mt > mt_max) wg_mt = mt_max;
        wg_tm = (M + 32 * wg_mt - 1) / (32 * wg_mt);
        wg_tc = (C + 1 + 32 * wg_cw - 1) / (32 * wg_cw);
        // enough workgroups to fill the chip (256 CUs), at least four K steps each
        const int kts = kWgCells * wg_ks;
        const int64_t per_image = (int64_t)wg_tm * wg_tc * (B > 0 ? B : 1);
        int64_t s = (512 + per_image - 1) / per_image;
        const int64_t s_max = (N + 4 * kts - 1) / (4 * kts);
        if (s > s_max) s = s_max;
        if (s < 1) s = 1;
        wg_chunk = (int)(((N + s - 1) / s + kts - 1) / kts * kts);
        wg_s = (int)((N + wg_chunk - 1) / wg_chunk);
        wg_parts = B * wg_s * wg_ks;
    }
};

// what both directions of both classes refuse; 0 when the sizes are fine
inline int check_train_sizes(const char *what, int B, int C, int M, int G) {
    if (B < 0 || C <= 0 || M <= 0 || G <= 0) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: bad size (B=%d C=%d M=%d G=%d)", what, B, C, M, G);
    if ((long)C * G * G > 0x1fffffffL || (long)M * G * G > 0x1fffffffL)
        return gfn::fail(GFN_ERR_INVALID_ARG, "%s: a map (C*G*G values) must stay below 2^29 values", what);
    if (B > 65535) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: batch > 65535", what);
    if (B > 0) {
        const TrainShape p(B, C, M, G);
        if ((int64_t)B * C * p.tiles > 0x7fffffffL || (int64_t)B * p.wg_s > 65535 || (int64_t)M * (C + 1) > 0x7fffffffL)
            return gfn::fail(GFN_ERR_INVALID_ARG, "%s: too many tiles", what);
        if ((int64_t)B * G * G < 2) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: batch statistics need more than one value per channel", what);
    }
    return GFN_OK;
}

// TrainShape and where the partial sums and the gz map lie in the workspace, in floats; gz_bytes: the size of a gz value
struct TrainPlan : TrainShape {
    int64_t fwd_floats;
    int64_t off_gz, off_bn, off_dgdb, off_dw, off_pw, bwd_floats;

    TrainPlan(int B, int C, int M, int G, int gz_bytes) : TrainShape(B, C, M, G) {
        const int64_t N = (int64_t)G * G;
        fwd_floats = align4((int64_t)C * B * tiles * 2);
        off_gz = 0;
        off_bn = off_gz + align4(((int64_t)B * C * N * gz_bytes + 3) / 4);
        off_dgdb = off_bn + align4((int64_t)C * B * ntn * 2);
        off_dw = off_dgdb + align4(2 * (int64_t)C);
        off_pw = off_dw + align4((int64_t)C * B * tiles * kDwCols);
        bwd_floats = off_pw + align4((int64_t)wg_parts * M * (C + 1));
    }
};
// 0 when (ws, ws_bytes) holds `floats`
inline int check_workspace(const char *what, const void *ws, int64_t ws_bytes, int64_t floats) {
    if (ws && !misaligned(ws) && ws_bytes >= floats * (int64_t)sizeof(float)) return GFN_OK;
    return gfn::fail(GFN_ERR_SCRATCH, "%s: workspace missing, not 16-byte aligned or too small (%lld bytes needed)", what,
                     (long long)(floats * (int64_t)sizeof(float)));
}

template <int MT, int CW>
struct WgShape {
    static constexpr int mt = MT, cw = CW;
};
// f(WgShape<MT, CW>()) for the eight (wg_mt, wg_cw) TrainShape chooses; false: none of them
template <typename F>
bool with_wgrad_shape(const TrainShape &p, F &&f) {
    switch (p.wg_cw * 8 + p.wg_mt) {
        case 8 + 1: f(WgShape<1, 1>()); return true;
        case 8 + 2: f(WgShape<2, 1>()); return true;
        case 16 + 1: f(WgShape<1, 2>()); return true;
        case 16 + 2: f(WgShape<2, 2>()); return true;
        case 16 + 4: f(WgShape<4, 2>()); return true;
        case 32 + 1: f(WgShape<1, 4>()); return true;
        case 32 + 2: f(WgShape<2, 4>()); return true;
        case 32 + 4: f(WgShape<4, 4>()); return true;
    }
    return false;
}

// f(XT()) for the type of x and gx: fp32, or the class's own 16-bit map type (K::check_class has refused every other x_dtype);
// fp32 maps go with fp32 x only
template <class K, typename F>
void with_x_type(int x_dtype, F &&f) {
    if constexpr (sizeof(typename K::map_t) == 2)
        if (x_dtype != GFN_F32) return f(typename K::map_t());
    f(float());
}

template <class K>
int64_t train_ws_bytes(int B, int C, int M, int G, int backward) {
    if (B <= 0 || C <= 0 || M <= 0 || G <= 0) return 0;
    const TrainPlan p(B, C, M, G, sizeof(typename K::map_t));
    return (backward ? p.bwd_floats : p.fwd_floats) * (int64_t)sizeof(float);
}

// The forward of class K (3 launches): x (x_dtype) -> u, mean, invstd, the running buffers, y
template <class K>
int train_fwd(const char *what, const void *x, int x_dtype, const float *dw_w, const float *dw_b, const float *bn_w, const float *bn_b,
              float *running_mean, float *running_var, const float *pw_w, const float *pw_b, void *u, float *mean, float *invstd, void *y,
              int B, int C, int M, int G, double momentum, double eps, void *ws, int64_t ws_bytes, gfn_stream_t stream) {
    using map_t = typename K::map_t;
    if (!x || !dw_w || !bn_w || !bn_b || !running_mean || !running_var || !pw_w || !pw_b || !u || !mean || !invstd || !y)
        return gfn::fail(GFN_ERR_INVALID_ARG, "%s: null pointer", what);
    if (int rc = K::check_class(what, x_dtype, C, M)) return rc;
    if (int rc = check_train_sizes(what, B, C, M, G)) return rc;
    if (x == u || x == y || u == y) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: x, u and y must be three different maps", what);
    if (!(momentum >= 0.0 && momentum <= 1.0) || !(eps >= 0.0)) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: momentum must lie in [0, 1] and eps be >= 0", what);
    if (B == 0) return GFN_OK;
    const TrainPlan p(B, C, M, G, sizeof(map_t));
    if (int rc = check_workspace(what, ws, ws_bytes, p.fwd_floats)) return rc;
    hipStream_t s = (hipStream_t)stream;
    float *part = static_cast<float *>(ws);
    map_t *um = static_cast<map_t *>(u);
    const int nparts = B * p.tiles;
    with_x_type<K>(x_dtype, [&](auto xt) {
        using XT = decltype(xt);
        hipLaunchKernelGGL((ct_dw_fwd_kernel<K, XT>), dim3((unsigned)(B * C * p.tiles)), dim3(256), 0, s, static_cast<const XT *>(x), dw_w, dw_b,
                           um, part, C, G, p.tiles_x, p.tiles, nparts);
    });
    if (int rc = gfn::check_launch("ct_dw_fwd_kernel")) return rc;
    hipLaunchKernelGGL(ct_stats_kernel, dim3((unsigned)C), dim3(64), 0, s, (const float *)part, mean, invstd, running_mean, running_var, G,
                       p.tiles_x, p.tiles, nparts, momentum, eps);
    if (int rc = gfn::check_launch("ct_stats_kernel")) return rc;
    return K::pw_fwd(p, s, um, bn_w, bn_b, mean, invstd, pw_w, pw_b, static_cast<map_t *>(y), B, C, M, G * G);
}

// The backward of class K (up to 7 launches, each skipped when the `need` mask does not ask for what it makes): gy = dL/dy and what
// the forward saved -> gx (x's type) and the seven parameter gradients
template <class K>
int train_bwd(const char *what, const void *gy, const void *x, int x_dtype, const void *u, const float *mean, const float *invstd,
              const float *dw_w, const float *bn_w, const float *bn_b, const float *pw_w, void *gx, float *d_dw_w, float *d_dw_b,
              float *d_bn_w, float *d_bn_b, float *d_pw_w, float *d_pw_b, int B, int C, int M, int G, int need, void *ws, int64_t ws_bytes,
              gfn_stream_t stream) {
    using map_t = typename K::map_t;
    if (!gy || !x || !u || !mean || !invstd || !dw_w || !bn_w || !bn_b || !pw_w) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: null pointer", what);
    if (int rc = K::check_class(what, x_dtype, C, M)) return rc;
    if (int rc = check_train_sizes(what, B, C, M, G)) return rc;
    if (need < 0 || need > GFN_CBT_NEED_ALL) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: unknown need mask %d", what, need);
    if (((need & GFN_CBT_NEED_X) && !gx) || ((need & GFN_CBT_NEED_DW) && !d_dw_w) || ((need & GFN_CBT_NEED_BN) && (!d_bn_w || !d_bn_b)) ||
        ((need & GFN_CBT_NEED_PW) && (!d_pw_w || !d_pw_b)))
        return gfn::fail(GFN_ERR_INVALID_ARG, "%s: the need mask asks for a gradient whose pointer is null", what);
    if (B == 0 || need == 0) return GFN_OK;
    const TrainPlan p(B, C, M, G, sizeof(map_t));
    if (int rc = check_workspace(what, ws, ws_bytes, p.bwd_floats)) return rc;
    hipStream_t s = (hipStream_t)stream;
    float *w = static_cast<float *>(ws);
    map_t *gz = reinterpret_cast<map_t *>(w + p.off_gz);
    float *part_bn = w + p.off_bn, *dgdb = w + p.off_dgdb, *part_dw = w + p.off_dw, *part_pw = w + p.off_pw;
    const map_t *gym = static_cast<const map_t *>(gy), *um = static_cast<const map_t *>(u);
    const int N = G * G;
    if (need & (GFN_CBT_NEED_X | GFN_CBT_NEED_DW | GFN_CBT_NEED_BN)) {
        if (int rc = K::pw_bwd(p, s, gym, um, bn_w, bn_b, mean, invstd, pw_w, gz, part_bn, B, C, M, N)) return rc;
        const bool bn = need & GFN_CBT_NEED_BN;
        hipLaunchKernelGGL(ct_bn_bwd_kernel, dim3((unsigned)C), dim3(64), 0, s, (const float *)part_bn, B * p.ntn, C, dgdb, bn ? d_bn_w : nullptr,
                           bn ? d_bn_b : nullptr);
        if (int rc = gfn::check_launch("ct_bn_bwd_kernel")) return rc;
    }
    if (need & GFN_CBT_NEED_PW) {
        if (int rc = K::pw_wgrad(what, p, s, gym, um, bn_w, bn_b, mean, invstd, part_pw, B, C, M, N)) return rc;
        if (int rc = K::pw_wgrad_sum(s, part_pw, p.wg_parts, M, C, d_pw_w, d_pw_b)) return rc;
    }
    if (need & (GFN_CBT_NEED_X | GFN_CBT_NEED_DW)) {
        const int nparts = B * p.tiles;
        with_x_type<K>(x_dtype, [&](auto xt) {
            using XT = decltype(xt);
            hipLaunchKernelGGL((ct_dw_bwd_kernel<K, XT>), dim3((unsigned)(B * C * p.tiles)), dim3(256), 0, s, (const map_t *)gz, um,
                               static_cast<const XT *>(x), dw_w, bn_w, mean, invstd, (const float *)dgdb, static_cast<XT *>(gx), part_dw, C, G,
                               p.tiles_x, p.tiles, nparts, 1.0f / ((float)B * (float)N), need & (GFN_CBT_NEED_X | GFN_CBT_NEED_DW));
        });
        if (int rc = gfn::check_launch("ct_dw_bwd_kernel")) return rc;
        if (need & GFN_CBT_NEED_DW) {
            hipLaunchKernelGGL(ct_dw_wgrad_kernel, dim3((unsigned)C), dim3(256), 0, s, (const float *)part_dw, nparts, d_dw_w, d_dw_b);
            if (int rc = gfn::check_launch("ct_dw_wgrad_kernel")) return rc;
        }
    }
    return GFN_OK;
}

}  // namespace
