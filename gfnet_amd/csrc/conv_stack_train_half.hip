// conv_stack_train_half.hip -- one refiner conv block in TRAINING mode in the reference's autocast class: fp16 maps in HBM.
//
// Reference: every ConvRefiner is built with amp=True (model/network.py:90-152) and trainer/train.py:29-43 drives the step with a
// GradScaler, so block1 + hidden_blocks (network.py:560-562) train under fp16 autocast.  The block is that of conv_stack_train.hip,
//   Conv2d(C, C, 5x5, padding 2, groups=C[, bias])  ->  BatchNorm2d (batch statistics)  ->  ReLU  ->  Conv2d(C, M, 1x1),
// and conv_train_common.h writes it once for both classes: the depthwise kernels, the small reductions, the prologues and epilogues
// of the 1x1 kernels, the workspace plan, the argument checks, the `need` mask and the launch sequence (train_fwd / train_bwd).
// This file is the fp16 class, F16Maps: its three GEMM kernels (ct_half_pw_fwd / _bwd / _wgrad_kernel), its split sum and the C
// entry points.  What the class means:
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

// the fp16 class: maps hold halves; a value is rounded where it is stored in a map or becomes an operand.  x is fp32 (a stack's
// first block: rounded on load, its gx written fp32) or fp16
struct F16Maps {
    using map_t = _Float16;
    template <typename T>
    static __device__ __forceinline__ float value(T v) { return as_half_value(v); }
    static int check_class(const char *what, int x_dtype, int C, int M);
    static int pw_fwd(const TrainPlan &p, hipStream_t s, const _Float16 *u, const float *bn_w, const float *bn_b, const float *mean,
                      const float *invstd, const float *pw_w, const float *pw_b, _Float16 *y, int B, int C, int M, int N);
    static int pw_bwd(const TrainPlan &p, hipStream_t s, const _Float16 *gy, const _Float16 *u, const float *bn_w, const float *bn_b,
                      const float *mean, const float *invstd, const float *pw_w, _Float16 *gz, float *part_bn, int B, int C, int M, int N);
    static int pw_wgrad(const char *what, const TrainPlan &p, hipStream_t s, const _Float16 *gy, const _Float16 *u, const float *bn_w,
                        const float *bn_b, const float *mean, const float *invstd, float *part_pw, int B, int C, int M, int N);
    static int pw_wgrad_sum(hipStream_t s, const float *part_pw, int nparts, int M, int C, float *d_pw_w, float *d_pw_b);
};

// ---- forward ---------------------------------------------------------------------------------------------------------------------
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
__global__ __launch_bounds__(256, 2) void ct_half_pw_fwd_kernel(const _Float16 *__restrict__ u, const float *__restrict__ gamma,
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
// gt[b] = W^T . gy[b] (rows = the C channels, k = the M output channels); pw_bwd_finish: gz = fp16(gt) where u*alpha + beta' > 0,
// written as a C map, and the per-workgroup partial sums of that rounded gz and of gz*u_hat.  part: (C, B * gridDim.x, 2).
__global__ __launch_bounds__(256, 2) void ct_half_pw_bwd_kernel(const _Float16 *__restrict__ gy, const _Float16 *__restrict__ u,
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
    stage_bn_rows(BM, c0, C, gamma, beta, mean, invstd, Al, Be, Mn, Is);  // read after the loop's barriers
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
    pw_bwd_finish<F16Maps>(acc, Al, Be, Mn, Is, red, u, gz, part, b, c0, n0, C, N, wave, col, kh);
}

// One split of dW[m, c] = sum_p gy[m, p] t[c, p], c = C being a row of ones (db_pw); the workgroup and wave shapes of
// ct_pw_wgrad_kernel.  Both operands have their k -- the cells -- contiguous in HBM: the tiles are plain copies of map rows
// (16 bytes at a time where vec says every piece is aligned), t recomputed from u on the way.
template <int MT, int CW>
__global__ __launch_bounds__(256) void ct_half_pw_wgrad_kernel(const _Float16 *__restrict__ gy, const _Float16 *__restrict__ u,
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
    stage_bn_rows(BC, c0, C, gamma, beta, mean, invstd, Al, Be);
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
    store_wgrad_partial(acc, part, (size_t)(blockIdx.z * KS + ks), m0, c0 + cw * 32 + col, kh, M, C);
}

// The partial (M, C+1) matrices summed in a fixed order; column C is db_pw.  A narrow block on a large grid leaves thousands of small
// partial matrices (C = 24 on 256 x 256 cells, batch 8: 2048 of 600 entries), so a workgroup takes 16 consecutive entries x 16 groups
// of parts: group g adds parts g, g + 16, ... in double, then the 16 groups are added in order.
__global__ __launch_bounds__(256) void ct_half_pw_wgrad_sum_kernel(const float *__restrict__ part, int nparts, int M, int C,
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

// ---- host: this class's check and four launches for train_fwd / train_bwd ----------------------------------------------------------
int F16Maps::check_class(const char *what, int x_dtype, int C, int M) {
    if (x_dtype != GFN_F32 && x_dtype != GFN_F16) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: x_dtype must be GFN_F32 or GFN_F16", what);
    if (C > 65535 * kHBM || M > 65535 * kHBM) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: more than %d channels", what, 65535 * kHBM);
    return GFN_OK;
}

int F16Maps::pw_fwd(const TrainPlan &p, hipStream_t s, const _Float16 *u, const float *bn_w, const float *bn_b, const float *mean,
                    const float *invstd, const float *pw_w, const float *pw_b, _Float16 *y, int B, int C, int M, int N) {
    const dim3 grid((unsigned)p.ntn, (unsigned)((M + kHBM - 1) / kHBM), (unsigned)B);
    hipLaunchKernelGGL(ct_half_pw_fwd_kernel, grid, dim3(256), 0, s, u, bn_w, bn_b, mean, invstd, pw_w, pw_b, y, M, C, N);
    return gfn::check_launch("ct_half_pw_fwd_kernel");
}

int F16Maps::pw_bwd(const TrainPlan &p, hipStream_t s, const _Float16 *gy, const _Float16 *u, const float *bn_w, const float *bn_b,
                    const float *mean, const float *invstd, const float *pw_w, _Float16 *gz, float *part_bn, int B, int C, int M, int N) {
    const dim3 grid((unsigned)p.ntn, (unsigned)((C + kHBM - 1) / kHBM), (unsigned)B);
    hipLaunchKernelGGL(ct_half_pw_bwd_kernel, grid, dim3(256), 0, s, gy, u, bn_w, bn_b, mean, invstd, pw_w, gz, part_bn, M, C, N);
    return gfn::check_launch("ct_half_pw_bwd_kernel");
}

int F16Maps::pw_wgrad(const char *what, const TrainPlan &p, hipStream_t s, const _Float16 *gy, const _Float16 *u, const float *bn_w,
                      const float *bn_b, const float *mean, const float *invstd, float *part_pw, int B, int C, int M, int N) {
    const dim3 grid((unsigned)p.wg_tc, (unsigned)p.wg_tm, (unsigned)(B * p.wg_s));
    // every 8-cell piece of a map row starts on 16 bytes: rows do when N % 8 == 0, pieces inside them always (chunks are
    // multiples of 32 cells)
    const int vec = N % 8 == 0 && !misaligned(gy) && !misaligned(u);
    const bool found = with_wgrad_shape(p, [&](auto sh) {
        hipLaunchKernelGGL((ct_half_pw_wgrad_kernel<decltype(sh)::mt, decltype(sh)::cw>), grid, dim3(256), 0, s, gy, u, bn_w, bn_b, mean, invstd,
                           part_pw, M, C, N, p.wg_s, p.wg_chunk, vec);
    });
    if (!found) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: no weight-gradient kernel for this shape", what);
    return gfn::check_launch("ct_half_pw_wgrad_kernel");
}

int F16Maps::pw_wgrad_sum(hipStream_t s, const float *part_pw, int nparts, int M, int C, float *d_pw_w, float *d_pw_b) {
    hipLaunchKernelGGL(ct_half_pw_wgrad_sum_kernel, dim3((unsigned)((M * (C + 1) + 15) / 16)), dim3(256), 0, s, part_pw, nparts, M, C, d_pw_w,
                       d_pw_b);
    return gfn::check_launch("ct_half_pw_wgrad_sum_kernel");
}

}  // namespace

GFN_EXPORT int64_t gfn_conv_block_train_half_ws_bytes(int B, int C, int M, int G, int backward) {
    return train_ws_bytes<F16Maps>(B, C, M, G, backward);
}

GFN_EXPORT int gfn_conv_block_train_half_fwd(const void *x, int x_dtype, const float *dw_w, const float *dw_b, const float *bn_w,
                                             const float *bn_b, float *running_mean, float *running_var, const float *pw_w,
                                             const float *pw_b, void *u, float *mean, float *invstd, void *y, int B, int C, int M, int G,
                                             double momentum, double eps, void *ws, int64_t ws_bytes, gfn_stream_t stream) {
    return train_fwd<F16Maps>("conv_block_train_half_fwd", x, x_dtype, dw_w, dw_b, bn_w, bn_b, running_mean, running_var, pw_w, pw_b, u, mean,
                              invstd, y, B, C, M, G, momentum, eps, ws, ws_bytes, stream);
}

GFN_EXPORT int gfn_conv_block_train_half_bwd(const void *gy, const void *x, int x_dtype, const void *u, const float *mean,
                                             const float *invstd, const float *dw_w, const float *bn_w, const float *bn_b,
                                             const float *pw_w, void *gx, float *d_dw_w, float *d_dw_b, float *d_bn_w, float *d_bn_b,
                                             float *d_pw_w, float *d_pw_b, int B, int C, int M, int G, int need, void *ws, int64_t ws_bytes,
                                             gfn_stream_t stream) {
    return train_bwd<F16Maps>("conv_block_train_half_bwd", gy, x, x_dtype, u, mean, invstd, dw_w, bn_w, bn_b, pw_w, gx, d_dw_w, d_dw_b, d_bn_w,
                              d_bn_b, d_pw_w, d_pw_b, B, C, M, G, need, ws, ws_bytes, stream);
}
