// conv_stack_train_half.hip -- one refiner conv block in TRAINING mode in the reference's autocast class: fp16 maps in HBM.
//
// Reference: every ConvRefiner is built with amp=True (model/network.py:90-152) and trainer/train.py:29-43 drives the step with a
// GradScaler, so block1 + hidden_blocks (network.py:560-562) train under fp16 autocast.  The block is that of conv_stack_train.hip,
//   Conv2d(C, C, 5x5, padding 2, groups=C[, bias])  ->  BatchNorm2d (batch statistics)  ->  ReLU  ->  Conv2d(C, M, 1x1),
// and so are its launches, its `need` mask and its fixed-order reductions (conv_train_common.h).  What differs is the class:
//   * maps in HBM are plain contiguous (B, C, G, G) fp16: x (the previous block's y), u, y, the backward's gz and gx.  Any C, any
//     G: with odd G a plane starts on a 2-byte boundary, so maps are read and written half by half unless G % 4 == 0 (G % 8 == 0
//     for the 16-byte loads of the weight gradient) makes a wider access aligned.  A stack's first block reads the fp32 concat and
//     rounds it on load (XT = float); its gx is then written fp32, unrounded, for the refiner input's backward
//   * parameters, their gradients, mean, invstd and every sum are fp32; depthwise taps and 1x1 weights are rounded to fp16 where
//     they become operands.  fp16 x fp16 products are exact in fp32, so the depthwise forward is the fp32 tap loop on rounded values
//   * u is rounded once; statistics, normalisation and backward all read the rounded u, so the block is an exact function of what
//     it stored.  t = relu(u*alpha + beta') is rounded as the B operand; alpha, beta' come from bn_affine / bn_pre in both
//     directions, so both ReLU masks agree bit for bit
//   * the three 1x1 products (y = W.t, gt = W^T.gy, dW = gy.t^T with its column of ones) run on v_mfma_f32_32x32x16_f16 with fp32
//     accumulators (pw_gemm_tile_half.h)
//   * every rounding is to nearest even and overflows to inf (as_half_value): a loss scale that is too large shows as inf / nan
// No floating-point atomics: two identical calls give identical bits.
#include "conv_train_common.h"
#include "pw_gemm_tile_half.h"

namespace {

// ---- forward ---------------------------------------------------------------------------------------------------------------------
// u = fp16(dw5x5(fp16 x, fp16 taps) + b_dw) and the tile's (mean, M2) of that rounded u; the tiling of ct_dw_fwd_kernel
template <typename XT>
__global__ __launch_bounds__(256) void cta_dw_fwd_kernel(const XT *__restrict__ x, const float *__restrict__ dw_w,
                                                         const float *__restrict__ dw_b, _Float16 *__restrict__ u,
                                                         float *__restrict__ part, int C, int G, int tiles_x, int tiles, int nparts) {
    __shared__ __attribute__((aligned(16))) float Xs[kHalo * kHalo];
    __shared__ float red[4];
    const int tid = threadIdx.x;
    const TileId t = decode_tile(blockIdx.x, C, tiles_x, tiles);
    const XT *xp = x + t.plane * (size_t)G * G;
    stage_halo(Xs, t, G, [&](bool ok, int off) {
        const float v = as_half_value(xp[off]);
        return ok ? v : 0.f;
    });
    float w[25];
#pragma unroll
    for (int k = 0; k < 25; ++k) w[k] = as_half_value(dw_w[(size_t)t.c * 25 + k]);
    __syncthreads();
    const int r = tid >> 3, c4 = (tid & 7) * 4;
    float acc[4];
    dw_taps<false>(Xs, w, r, c4, acc);
    const float bias = dw_b ? dw_b[t.c] : 0.f;
    const int gy = t.row0 + r, gx0 = t.col0 + c4;
    _Float16 *up = u + t.plane * (size_t)G * G + (size_t)gy * G + gx0;
    float uq[4], s = 0.f;
    bool ok[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        uq[q] = as_half_value(acc[q] + bias);
        ok[q] = gy < G && gx0 + q < G;
        s += ok[q] ? uq[q] : 0.f;
    }
    if ((G & 3) == 0) {  // planes, rows and the thread's four cells all start on 8 bytes
        if (ok[0]) *reinterpret_cast<f16x4 *>(up) = f16x4{(_Float16)uq[0], (_Float16)uq[1], (_Float16)uq[2], (_Float16)uq[3]};
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (ok[q]) up[q] = (_Float16)uq[q];
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

__global__ __launch_bounds__(64) void cta_stats_kernel(const float *__restrict__ part, float *__restrict__ mean, float *__restrict__ invstd,
                                                       float *__restrict__ running_mean, float *__restrict__ running_var, int G, int tiles_x,
                                                       int tiles, int nparts, double momentum, double eps) {
    stats_channel(part, mean, invstd, running_mean, running_var, G, tiles_x, tiles, nparts, momentum, eps);
}

// the B operand tile of a (K, N) fp16 map: Bs[cell][k] = f(k, map[k0 + k][n0 + cell]); channels past K and cells past N are zero
template <typename F>
__device__ __forceinline__ void stage_map_cells(_Float16 *Bs, const _Float16 *map, int k0, int K, int n0, int N, int tid, F f) {
    stage_half_tile<kBN, kHKT, true>(Bs, tid, [&](int cell, int k8) {
        const int n = n0 + cell;
        f16x8 h;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int kk = k0 + k8 + j;
            const bool ok = n < N && kk < K;
            const _Float16 v = map[ok ? (size_t)kk * N + n : 0];
            h[j] = ok ? f(k8 + j, v) : (_Float16)0.f;
        }
        return h;
    });
}

// One row tile per workgroup in the forward and the input-gradient GEMM: 32 rows x 128 cells.  The fp32 class's slabs of up to 7 row
// tiles leave a coarse grid with 128 workgroups for 256 CUs (417 rows on 32 x 32 cells, batch 8), one per CU and nothing to hide its
// loads behind; measured on the stack's step at the five widths, 1 row tile was the fastest or within 4 % of it.
constexpr int kHBM = 32;

// y[b] = fp16(W . t + bias), t = fp16(relu(u[b]*alpha + beta')); W (M, K) row major
__global__ __launch_bounds__(256, 2) void cta_pw_fwd_kernel(const _Float16 *__restrict__ u, const float *__restrict__ gamma,
                                                            const float *__restrict__ beta, const float *__restrict__ mean,
                                                            const float *__restrict__ invstd, const float *__restrict__ pw_w,
                                                            const float *__restrict__ pw_b, _Float16 *__restrict__ y, int M, int K, int N) {
    constexpr int BM = kHBM, P = half_pitch(kHKT);
    __shared__ __attribute__((aligned(16))) _Float16 As[BM * P];
    __shared__ __attribute__((aligned(16))) _Float16 Bs[kBN * P];
    __shared__ float Al[2][kHKT], Be[2][kHKT];  // the K tile's alpha, beta': the next tile's are formed while this one is staged
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.z, m0 = blockIdx.y * BM, n0 = blockIdx.x * kBN;
    const _Float16 *ub = u + (size_t)b * K * N;
    const int col = lane & 31, kh = lane >> 5;
    auto affine = [&](int buf, int k0) {
        if (tid < kHKT) {
            const int kk = k0 + tid;
            float al = 0.f, be = 0.f;
            if (kk < K) bn_affine(gamma[kk], beta[kk], mean[kk], invstd[kk], al, be);
            Al[buf][tid] = al, Be[buf][tid] = be;
        }
    };
    affine(0, 0);
    __syncthreads();
    PwAcc<1> acc;
    acc.zero();
    for (int k0 = 0, buf = 0; k0 < K; k0 += kHKT, buf ^= 1) {
        stage_half_tile<BM, kHKT, false>(As, tid, [&](int row, int k8) {
            const int m = m0 + row;
            f16x8 h;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const bool ok = m < M && k0 + k8 + j < K;
                const float v = pw_w[ok ? (size_t)m * K + k0 + k8 + j : 0];
                h[j] = ok ? (_Float16)v : (_Float16)0.f;
            }
            return h;
        });
        stage_map_cells(Bs, ub, k0, K, n0, N, tid,
                        [&](int k, _Float16 v) { return (_Float16)fmaxf(bn_pre((float)v, Al[buf][k], Be[buf][k]), 0.f); });
        affine(buf ^ 1, k0 + kHKT);
        __syncthreads();
        half_products<1, kHKT / 16, P>(acc, &As[col * P + 8 * kh], &Bs[(wave * 32 + col) * P + 8 * kh]);
        __syncthreads();
    }
    const int n = n0 + wave * 32 + col;
    if (n < N) {
        _Float16 *yb = y + (size_t)b * M * N + n;
        acc.each(kh, [&](int row, float v) {
            const int m = m0 + row;
            if (m < M) yb[(size_t)m * N] = (_Float16)(v + pw_b[m]);
        });
    }
}

// ---- backward --------------------------------------------------------------------------------------------------------------------
// gt[b] = W^T . gy[b] (rows = the C channels, k = the M output channels); gz = fp16(gt) where u*alpha + beta' > 0, written as a C
// map, and the per-workgroup partial sums of that rounded gz and of gz*u_hat.  part: (C, B * gridDim.x, 2).
__global__ __launch_bounds__(256, 2) void cta_pw_bwd_kernel(const _Float16 *__restrict__ gy, const _Float16 *__restrict__ u,
                                                            const float *__restrict__ gamma, const float *__restrict__ beta,
                                                            const float *__restrict__ mean, const float *__restrict__ invstd,
                                                            const float *__restrict__ pw_w, _Float16 *__restrict__ gz,
                                                            float *__restrict__ part, int M, int C, int N) {
    constexpr int BM = kHBM, P = half_pitch(kHKT);
    __shared__ __attribute__((aligned(16))) _Float16 As[BM * P];
    __shared__ __attribute__((aligned(16))) _Float16 Bs[kBN * P];
    __shared__ float Al[BM], Be[BM], Mn[BM], Is[BM];
    __shared__ float red[4][BM][2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.z, c0 = blockIdx.y * BM, n0 = blockIdx.x * kBN;
    const _Float16 *gb = gy + (size_t)b * M * N;
    const int col = lane & 31, kh = lane >> 5;
    if (tid < BM) {
        const int c = c0 + tid;
        float al = 0.f, be = 0.f, mn = 0.f, is = 0.f;
        if (c < C) {
            mn = mean[c], is = invstd[c];
            bn_affine(gamma[c], beta[c], mn, is, al, be);
        }
        Al[tid] = al, Be[tid] = be, Mn[tid] = mn, Is[tid] = is;
    }
    PwAcc<1> acc;
    acc.zero();
    for (int k0 = 0; k0 < M; k0 += kHKT) {
        stage_half_tile<BM, kHKT, true>(As, tid, [&](int cc, int k8) {  // A[c][m] = W[m][c]: consecutive lanes, consecutive c
            f16x8 h;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const bool ok = k0 + k8 + j < M && c0 + cc < C;
                const float v = pw_w[ok ? (size_t)(k0 + k8 + j) * C + c0 + cc : 0];
                h[j] = ok ? (_Float16)v : (_Float16)0.f;
            }
            return h;
        });
        stage_map_cells(Bs, gb, k0, M, n0, N, tid, [](int, _Float16 v) { return v; });
        __syncthreads();
        half_products<1, kHKT / 16, P>(acc, &As[col * P + 8 * kh], &Bs[(wave * 32 + col) * P + 8 * kh]);
        __syncthreads();
    }
    const int n = n0 + wave * 32 + col;
    const bool nok = n < N;
    const size_t base = (size_t)b * C * N + (nok ? n : 0);
    acc.each(kh, [&](int row, float a) {
        const int c = c0 + row;
        const bool ok = nok && c < C;
        const size_t at = base + (size_t)(ok ? c : 0) * N;
        const float uu = (float)u[at];
        const float g = ok && bn_pre(uu, Al[row], Be[row]) > 0.f ? as_half_value(a) : 0.f;
        if (ok) gz[at] = (_Float16)g;
        const float s1 = half_wave_sum(g);
        const float s2 = half_wave_sum(ok ? g * ((uu - Mn[row]) * Is[row]) : 0.f);
        if (col == 0) red[wave][row][0] = s1, red[wave][row][1] = s2;
    });
    __syncthreads();
    if (tid < BM && c0 + tid < C) {
        float *p = part + ((size_t)(c0 + tid) * ((size_t)gridDim.z * gridDim.x) + (size_t)b * gridDim.x + blockIdx.x) * 2;
        p[0] = (red[0][tid][0] + red[1][tid][0]) + (red[2][tid][0] + red[3][tid][0]);
        p[1] = (red[0][tid][1] + red[1][tid][1]) + (red[2][tid][1] + red[3][tid][1]);
    }
}

__global__ __launch_bounds__(64) void cta_bn_bwd_kernel(const float *__restrict__ part, int nparts, int C, float *__restrict__ dgdb,
                                                        float *__restrict__ dgamma, float *__restrict__ dbeta) {
    bn_bwd_channel(part, nparts, C, dgdb, dgamma, dbeta);
}

// One split of dW[m, c] = sum_p gy[m, p] t[c, p], c = C being a row of ones (db_pw); the workgroup and wave shapes of
// ct_pw_wgrad_kernel.  Both operands have their k -- the cells -- contiguous in HBM: the tiles are plain copies of map rows
// (16 bytes at a time where vec says every piece is aligned), t recomputed from u on the way.
template <int MT, int CW>
__global__ __launch_bounds__(256) void cta_pw_wgrad_kernel(const _Float16 *__restrict__ gy, const _Float16 *__restrict__ u,
                                                           const float *__restrict__ gamma, const float *__restrict__ beta,
                                                           const float *__restrict__ mean, const float *__restrict__ invstd,
                                                           float *__restrict__ part, int M, int C, int N, int S, int chunk, int vec) {
    constexpr int KS = 4 / CW, KTS = kWgCells * KS, BM = 32 * MT, BC = 32 * CW, P = half_pitch(KTS);
    __shared__ __attribute__((aligned(16))) _Float16 As[BM * P];
    __shared__ __attribute__((aligned(16))) _Float16 Bs[BC * P];
    __shared__ float Al[BC], Be[BC];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cw = wave % CW, ks = wave / CW;
    const int col = lane & 31, kh = lane >> 5;
    const int c0 = blockIdx.x * BC, m0 = blockIdx.y * BM;
    const int b = blockIdx.z / S, sp = blockIdx.z - b * S;
    const int n_begin = sp * chunk, n_end = min(N, n_begin + chunk);
    const _Float16 *gb = gy + (size_t)b * M * N;
    const _Float16 *ub = u + (size_t)b * C * N;
    if (tid < BC) {
        float al = 0.f, be = 0.f;
        if (c0 + tid < C) bn_affine(gamma[c0 + tid], beta[c0 + tid], mean[c0 + tid], invstd[c0 + tid], al, be);
        Al[tid] = al, Be[tid] = be;
    }
    __syncthreads();
    PwAcc<MT> acc;
    acc.zero();
    for (int nb = n_begin; nb < n_end; nb += KTS) {
        stage_half_tile<BM, KTS, false>(As, tid, [&](int row, int k8) {
            const int valid = m0 + row < M ? n_end - (nb + k8) : 0;
            return load_half8(gb + (valid > 0 ? (size_t)(m0 + row) * N + nb + k8 : 0), valid, vec);
        });
        stage_half_tile<BC, KTS, false>(Bs, tid, [&](int row, int k8) {
            const int c = c0 + row, cells = n_end - (nb + k8);
            const int valid = c < C ? cells : 0;
            const f16x8 uu = load_half8(ub + (valid > 0 ? (size_t)c * N + nb + k8 : 0), valid, vec);
            f16x8 h;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const _Float16 t = (_Float16)fmaxf(bn_pre((float)uu[j], Al[row], Be[row]), 0.f);
                h[j] = j < valid ? t : (_Float16)(c == C && j < cells ? 1.f : 0.f);
            }
            return h;
        });
        __syncthreads();
        half_products<MT, kWgCells / 16, P>(acc, &As[col * P + ks * kWgCells + 8 * kh], &Bs[(cw * 32 + col) * P + ks * kWgCells + 8 * kh]);
        __syncthreads();
    }
    const int cidx = c0 + cw * 32 + col;
    if (cidx <= C) {
        float *pp = part + (size_t)(blockIdx.z * KS + ks) * M * (C + 1) + cidx;
        acc.each(kh, [&](int row, float v) {
            if (m0 + row < M) pp[(size_t)(m0 + row) * (C + 1)] = v;
        });
    }
}

// The partial (M, C+1) matrices summed in a fixed order; column C is db_pw.  A narrow block on a large grid leaves thousands of small
// partial matrices (C = 24 on 256 x 256 cells, batch 8: 2048 of 600 entries), so a workgroup takes 16 consecutive entries x 16 groups
// of parts: group g adds parts g, g + 16, ... in double, then the 16 groups are added in order.
__global__ __launch_bounds__(256) void cta_pw_wgrad_sum_kernel(const float *__restrict__ part, int nparts, int M, int C,
                                                               float *__restrict__ d_pw_w, float *__restrict__ d_pw_b) {
    __shared__ double s[16][16];
    const int total = M * (C + 1);
    const int j = threadIdx.x & 15, g = threadIdx.x >> 4;
    const int idx = blockIdx.x * 16 + j;
    double a = 0.0;
    if (idx < total)
        for (int p = g; p < nparts; p += 16) a += (double)part[(size_t)p * total + idx];
    s[g][j] = a;
    __syncthreads();
    if (threadIdx.x < 16 && idx < total) {
        double tot = 0.0;
        for (int q = 0; q < 16; ++q) tot += s[q][j];
        const int m = idx / (C + 1), c = idx - m * (C + 1);
        if (c < C) d_pw_w[(size_t)m * C + c] = (float)tot;
        else d_pw_b[m] = (float)tot;
    }
}

// gu = alpha*(gz - dbeta/N - u_hat*dgamma/N) in fp32 from the fp16 gz and u while their halo tile is staged; gx = dw5x5 of gu with
// the rounded taps, flipped, written in x's type (fp32 unrounded for a first block, fp16 otherwise); per-workgroup partials of the
// depthwise parameter gradients against the rounded x the forward multiplied.  need bit 0: gx, bit 1: the partials.
template <typename XT>
__global__ __launch_bounds__(256) void cta_dw_bwd_kernel(const _Float16 *__restrict__ gz, const _Float16 *__restrict__ u,
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
            const float xv = as_half_value(x[pbase + off]);
            return ok ? xv : 0.f;
        });
    __syncthreads();
    const int r = tid >> 3, c4 = (tid & 7) * 4;
    if (want_x) {  // gx[q] = sum_k w[k] gu[q - off_k]: the forward's taps, flipped
        float w[25];
#pragma unroll
        for (int k = 0; k < 25; ++k) w[k] = as_half_value(dw_w[(size_t)t.c * 25 + k]);
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

__global__ __launch_bounds__(256) void cta_dw_wgrad_kernel(const float *__restrict__ part, int nparts, float *__restrict__ d_dw_w,
                                                           float *__restrict__ d_dw_b) {
    dw_wgrad_channel(part, nparts, d_dw_w, d_dw_b);
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
// TrainShape's tiling and the workspace of this class, in floats: the gz map takes half a float per value
struct HalfPlan : TrainShape {
    int64_t fwd_floats;
    int64_t off_gz, off_bn, off_dgdb, off_dw, off_pw, bwd_floats;

    HalfPlan(int B, int C, int M, int G) : TrainShape(B, C, M, G) {
        const int64_t N = (int64_t)G * G;
        fwd_floats = align4((int64_t)C * B * tiles * 2);
        off_gz = 0;
        off_bn = off_gz + align4(((int64_t)B * C * N + 1) / 2);
        off_dgdb = off_bn + align4((int64_t)C * B * ntn * 2);
        off_dw = off_dgdb + align4(2 * (int64_t)C);
        off_pw = off_dw + align4((int64_t)C * B * tiles * kDwCols);
        bwd_floats = off_pw + align4((int64_t)wg_parts * M * (C + 1));
    }
};

// what this class refuses beyond check_train_sizes
int check_half_args(const char *what, int x_dtype, int C, int M) {
    if (x_dtype != GFN_F32 && x_dtype != GFN_F16) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: x_dtype must be GFN_F32 or GFN_F16", what);
    if (C > 65535 * kHBM || M > 65535 * kHBM) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: more than %d channels", what, 65535 * kHBM);
    return GFN_OK;
}

}  // namespace

GFN_EXPORT int64_t gfn_conv_block_train_half_ws_bytes(int B, int C, int M, int G, int backward) {
    if (B <= 0 || C <= 0 || M <= 0 || G <= 0) return 0;
    const HalfPlan p(B, C, M, G);
    return (backward ? p.bwd_floats : p.fwd_floats) * (int64_t)sizeof(float);
}

GFN_EXPORT int gfn_conv_block_train_half_fwd(const void *x, int x_dtype, const float *dw_w, const float *dw_b, const float *bn_w,
                                             const float *bn_b, float *running_mean, float *running_var, const float *pw_w,
                                             const float *pw_b, void *u, float *mean, float *invstd, void *y, int B, int C, int M, int G,
                                             double momentum, double eps, void *ws, int64_t ws_bytes, gfn_stream_t stream) {
    const char *what = "conv_block_train_half_fwd";
    if (!x || !dw_w || !bn_w || !bn_b || !running_mean || !running_var || !pw_w || !pw_b || !u || !mean || !invstd || !y)
        return gfn::fail(GFN_ERR_INVALID_ARG, "%s: null pointer", what);
    if (int rc = check_half_args(what, x_dtype, C, M)) return rc;
    if (int rc = check_train_sizes(what, B, C, M, G)) return rc;
    if (x == u || x == y || u == y) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: x, u and y must be three different maps", what);
    if (!(momentum >= 0.0 && momentum <= 1.0) || !(eps >= 0.0)) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: momentum must lie in [0, 1] and eps be >= 0", what);
    if (B == 0) return GFN_OK;
    const HalfPlan p(B, C, M, G);
    if (!ws || misaligned(ws) || ws_bytes < p.fwd_floats * (int64_t)sizeof(float))
        return gfn::fail(GFN_ERR_SCRATCH, "%s: workspace missing, not 16-byte aligned or too small (%lld bytes needed)", what,
                         (long long)(p.fwd_floats * (int64_t)sizeof(float)));
    hipStream_t s = (hipStream_t)stream;
    float *part = static_cast<float *>(ws);
    _Float16 *uh = static_cast<_Float16 *>(u), *yh = static_cast<_Float16 *>(y);
    const int nparts = B * p.tiles, N = G * G;
    const dim3 dw_grid((unsigned)(B * C * p.tiles));
    if (x_dtype == GFN_F32)
        hipLaunchKernelGGL(cta_dw_fwd_kernel<float>, dw_grid, dim3(256), 0, s, static_cast<const float *>(x), dw_w, dw_b, uh, part, C, G,
                           p.tiles_x, p.tiles, nparts);
    else
        hipLaunchKernelGGL(cta_dw_fwd_kernel<_Float16>, dw_grid, dim3(256), 0, s, static_cast<const _Float16 *>(x), dw_w, dw_b, uh, part, C, G,
                           p.tiles_x, p.tiles, nparts);
    if (int rc = gfn::check_launch("cta_dw_fwd_kernel")) return rc;
    hipLaunchKernelGGL(cta_stats_kernel, dim3((unsigned)C), dim3(64), 0, s, (const float *)part, mean, invstd, running_mean, running_var, G,
                       p.tiles_x, p.tiles, nparts, momentum, eps);
    if (int rc = gfn::check_launch("cta_stats_kernel")) return rc;
    const dim3 grid((unsigned)p.ntn, (unsigned)((M + kHBM - 1) / kHBM), (unsigned)B);
    hipLaunchKernelGGL(cta_pw_fwd_kernel, grid, dim3(256), 0, s, (const _Float16 *)uh, bn_w, bn_b, (const float *)mean,
                       (const float *)invstd, pw_w, pw_b, yh, M, C, N);
    return gfn::check_launch("cta_pw_fwd_kernel");
}

GFN_EXPORT int gfn_conv_block_train_half_bwd(const void *gy, const void *x, int x_dtype, const void *u, const float *mean,
                                             const float *invstd, const float *dw_w, const float *bn_w, const float *bn_b,
                                             const float *pw_w, void *gx, float *d_dw_w, float *d_dw_b, float *d_bn_w, float *d_bn_b,
                                             float *d_pw_w, float *d_pw_b, int B, int C, int M, int G, int need, void *ws, int64_t ws_bytes,
                                             gfn_stream_t stream) {
    const char *what = "conv_block_train_half_bwd";
    if (!gy || !x || !u || !mean || !invstd || !dw_w || !bn_w || !bn_b || !pw_w) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: null pointer", what);
    if (int rc = check_half_args(what, x_dtype, C, M)) return rc;
    if (int rc = check_train_sizes(what, B, C, M, G)) return rc;
    if (need < 0 || need > GFN_CBT_NEED_ALL) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: unknown need mask %d", what, need);
    if (((need & GFN_CBT_NEED_X) && !gx) || ((need & GFN_CBT_NEED_DW) && !d_dw_w) || ((need & GFN_CBT_NEED_BN) && (!d_bn_w || !d_bn_b)) ||
        ((need & GFN_CBT_NEED_PW) && (!d_pw_w || !d_pw_b)))
        return gfn::fail(GFN_ERR_INVALID_ARG, "%s: the need mask asks for a gradient whose pointer is null", what);
    if (B == 0 || need == 0) return GFN_OK;
    const HalfPlan p(B, C, M, G);
    if (!ws || misaligned(ws) || ws_bytes < p.bwd_floats * (int64_t)sizeof(float))
        return gfn::fail(GFN_ERR_SCRATCH, "%s: workspace missing, not 16-byte aligned or too small (%lld bytes needed)", what,
                         (long long)(p.bwd_floats * (int64_t)sizeof(float)));
    hipStream_t s = (hipStream_t)stream;
    float *w = static_cast<float *>(ws);
    _Float16 *gz = reinterpret_cast<_Float16 *>(w + p.off_gz);
    float *part_bn = w + p.off_bn, *dgdb = w + p.off_dgdb, *part_dw = w + p.off_dw, *part_pw = w + p.off_pw;
    const _Float16 *gyh = static_cast<const _Float16 *>(gy), *uh = static_cast<const _Float16 *>(u);
    const int N = G * G;
    if (need & (GFN_CBT_NEED_X | GFN_CBT_NEED_DW | GFN_CBT_NEED_BN)) {
        const dim3 grid((unsigned)p.ntn, (unsigned)((C + kHBM - 1) / kHBM), (unsigned)B);
        hipLaunchKernelGGL(cta_pw_bwd_kernel, grid, dim3(256), 0, s, gyh, uh, bn_w, bn_b, mean, invstd, pw_w, gz, part_bn, M, C, N);
        if (int rc = gfn::check_launch("cta_pw_bwd_kernel")) return rc;
        const bool bn = need & GFN_CBT_NEED_BN;
        hipLaunchKernelGGL(cta_bn_bwd_kernel, dim3((unsigned)C), dim3(64), 0, s, (const float *)part_bn, B * p.ntn, C, dgdb,
                           bn ? d_bn_w : nullptr, bn ? d_bn_b : nullptr);
        if (int rc = gfn::check_launch("cta_bn_bwd_kernel")) return rc;
    }
    if (need & GFN_CBT_NEED_PW) {
        const dim3 grid((unsigned)p.wg_tc, (unsigned)p.wg_tm, (unsigned)(B * p.wg_s));
        // every 8-cell piece of a map row starts on 16 bytes: rows do when N % 8 == 0, pieces inside them always (chunks are
        // multiples of 32 cells)
        const int vec = N % 8 == 0 && !misaligned(gy) && !misaligned(u);
#define GFN_CTA(MT, CW)                                                                                                                  \
    hipLaunchKernelGGL((cta_pw_wgrad_kernel<MT, CW>), grid, dim3(256), 0, s, gyh, uh, bn_w, bn_b, mean, invstd, part_pw, M, C, N, p.wg_s, \
                       p.wg_chunk, vec)
        switch (p.wg_cw * 8 + p.wg_mt) {
            case 8 + 1: GFN_CTA(1, 1); break;
            case 8 + 2: GFN_CTA(2, 1); break;
            case 16 + 1: GFN_CTA(1, 2); break;
            case 16 + 2: GFN_CTA(2, 2); break;
            case 16 + 4: GFN_CTA(4, 2); break;
            case 32 + 1: GFN_CTA(1, 4); break;
            case 32 + 2: GFN_CTA(2, 4); break;
            case 32 + 4: GFN_CTA(4, 4); break;
            default: return gfn::fail(GFN_ERR_INVALID_ARG, "%s: no weight-gradient kernel for this shape", what);
        }
#undef GFN_CTA
        if (int rc = gfn::check_launch("cta_pw_wgrad_kernel")) return rc;
        hipLaunchKernelGGL(cta_pw_wgrad_sum_kernel, dim3((unsigned)((M * (C + 1) + 15) / 16)), dim3(256), 0, s, (const float *)part_pw,
                           p.wg_parts, M, C, d_pw_w, d_pw_b);
        if (int rc = gfn::check_launch("cta_pw_wgrad_sum_kernel")) return rc;
    }
    if (need & (GFN_CBT_NEED_X | GFN_CBT_NEED_DW)) {
        const int nparts = B * p.tiles;
        const dim3 grid((unsigned)(B * C * p.tiles));
        const float inv_n = 1.0f / ((float)B * (float)N);
        const int dw_need = need & (GFN_CBT_NEED_X | GFN_CBT_NEED_DW);
        if (x_dtype == GFN_F32)
            hipLaunchKernelGGL(cta_dw_bwd_kernel<float>, grid, dim3(256), 0, s, (const _Float16 *)gz, uh, static_cast<const float *>(x), dw_w,
                               bn_w, mean, invstd, (const float *)dgdb, static_cast<float *>(gx), part_dw, C, G, p.tiles_x, p.tiles, nparts,
                               inv_n, dw_need);
        else
            hipLaunchKernelGGL(cta_dw_bwd_kernel<_Float16>, grid, dim3(256), 0, s, (const _Float16 *)gz, uh, static_cast<const _Float16 *>(x),
                               dw_w, bn_w, mean, invstd, (const float *)dgdb, static_cast<_Float16 *>(gx), part_dw, C, G, p.tiles_x, p.tiles,
                               nparts, inv_n, dw_need);
        if (int rc = gfn::check_launch("cta_dw_bwd_kernel")) return rc;
        if (need & GFN_CBT_NEED_DW) {
            hipLaunchKernelGGL(cta_dw_wgrad_kernel, dim3((unsigned)C), dim3(256), 0, s, (const float *)part_dw, nparts, d_dw_w, d_dw_b);
            if (int rc = gfn::check_launch("cta_dw_wgrad_kernel")) return rc;
        }
    }
    return GFN_OK;
}
