// conv_train_common.h -- what the two training-mode conv block files (conv_stack_train.hip: fp32 maps; conv_stack_train_half.hip:
// fp16 maps, the autocast class) say once: BatchNorm as one multiply-add (bn_affine / bn_pre -- forward and backward of both
// classes form their ReLU mask through it), the 32x32 depthwise tile with its halo (decode_tile, stage_halo, dw_taps), the
// fixed-order workgroup sums, Chan's merge of (n, mean, M2), the bodies of the three small reductions that only ever see fp32
// partial sums (per-channel statistics, BatchNorm's two gradients, the depthwise parameter gradients), and the host-side tiling of a block (TrainShape).  Opens its own anonymous namespace.
#pragma once
#include "pw_gemm_tile.h"

namespace {

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

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}
__device__ __forceinline__ float half_wave_sum(float v) {  // over the 32 lanes that share lane >> 5
#pragma unroll
    for (int m = 16; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}
// sum over the workgroup's 256 threads in a fixed order, returned to every thread; red: 4 floats of LDS
__device__ __forceinline__ float block_sum(float v, float *red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
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

// ---- the three small reductions: bodies of one-line kernels in either file ----------------------------------------------------------
// one wave per channel (blockIdx.x): the tiles' (mean, M2) -> mean, invstd and the running buffers
__device__ __forceinline__ void stats_channel(const float *__restrict__ part, float *__restrict__ mean, float *__restrict__ invstd,
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
__device__ __forceinline__ void bn_bwd_channel(const float *__restrict__ part, int nparts, int C, float *__restrict__ dgdb,
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
__device__ __forceinline__ void dw_wgrad_channel(const float *__restrict__ part, int nparts, float *__restrict__ d_dw_w,
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

// ---- host ------------------------------------------------------------------------------------------------------------------------
inline int64_t align4(int64_t floats) { return (floats + 3) / 4 * 4; }
inline bool misaligned(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) != 0; }

// how a block's maps are cut up: the same in both classes
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

}  // namespace
