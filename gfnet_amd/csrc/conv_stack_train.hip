// conv_stack_train.hip -- one refiner conv block in TRAINING mode on gfx950: batch-statistic BatchNorm forward and the backward.
//
// Reference: ConvRefiner.create_block / forward, model/network.py:471-487 and :560-563, under model.train() -- per block
//   Conv2d(C, C, 5x5, padding 2, groups=C[, bias])  ->  BatchNorm2d (batch statistics)  ->  ReLU  ->  Conv2d(C, M, 1x1)
// differentiated by torch autograd there.  Everything is fp32 on contiguous (B, C, G, G) maps; the eval-mode kernels
// (conv_stack.hip) fold BatchNorm from the running statistics and cannot serve: here the statistics are the batch's own, the
// running buffers are updated, and the backward yields the input gradient and seven parameter gradients.
//
// The block is written once for this class and the fp16 autocast class (conv_stack_train_half.hip) in conv_train_common.h: the
// depthwise kernels, the small reductions, the prologues and epilogues of the 1x1 kernels, the workspace plan, the argument checks
// and the launch sequence (train_fwd / train_bwd).  This file is the fp32 class, F32Maps: its GEMM kernels on the fp32
// matrix-core tile of pw_gemm_tile.h, its split sum, and the C entry points.
//
// Forward (3 launches)
//   ct_dw_fwd_kernel       (common) u = dw5x5(x) + b_dw on 32x32 tiles staged with their halo in LDS; u goes to HBM -- the backward
//                          needs it -- and every workgroup leaves its tile's (mean, M2 = sum (u - mean)^2)
//   ct_stats_kernel        (common) per channel: Chan's merge of the tiles' (n, mean, M2) in double, in a fixed order; mean, invstd =
//                          1/sqrt(var + eps) with the biased variance, and the running buffers (unbiased variance) as torch
//   ct_pw_fwd_kernel       y = W_pw . relu(u*alpha + beta') + b_pw on the fp32 matrix-core tile (pw_gemm_kernel's too); alpha =
//                          gamma*invstd, beta' = beta - mean*alpha (bn_affine); t = relu(..) is formed while the B operand tile is
//                          staged and never reaches HBM
// Backward (up to 7 launches, each skipped when the `need` mask does not ask for what it makes)
//   ct_pw_bwd_kernel       gt = W_pw^T . gy on the same tile; then pw_bwd_finish: gz = gt where u*alpha + beta' > 0 (the forward's own
//                          expression, so both masks agree bit for bit), written as a C map; per-workgroup partial sums of gz and
//                          gz*u_hat
//   ct_bn_bwd_kernel       (common) dbeta = sum gz, dgamma = sum gz*u_hat from the partials (double, fixed order)
//   ct_pw_wgrad_kernel     dW_pw[m, c] = sum_p gy[m, p] t[c, p] on the matrix core (PwAcc; K runs over the cells), t recomputed from u;
//                          a column of ones appended to t makes db_pw the (C+1)-th column.  Split over the cells; every split writes
//                          its own partial matrix
//   ct_pw_wgrad_sum_kernel sums the partial matrices in a fixed order, one thread per entry.  The fp16 class sums by 16 groups of
//                          parts: another order, so the two stay apart for the sake of this class's bits
//   ct_dw_bwd_kernel       (common) gu = alpha*(gz - dbeta/N - u_hat*dgamma/N) formed while the gz / u halo tile is staged; gx = dw5x5
//                          of gu with flipped taps; per-workgroup partials of dW_dw[c, k] = sum_p gu[p] x[p + off_k] and db_dw = sum gu
//   ct_dw_wgrad_kernel     (common) sums those partials (double, fixed order)
// No floating-point atomics anywhere: two identical calls give identical bits.
#include "conv_train_common.h"

namespace {

// the fp32 class: maps hold floats and nothing is rounded.  x is fp32 too, so check_class has nothing to refuse
struct F32Maps {
    using map_t = float;
    static __device__ __forceinline__ float value(float v) { return v; }
    static int check_class(const char *, int, int, int) { return GFN_OK; }
    static int pw_fwd(const TrainPlan &p, hipStream_t s, const float *u, const float *bn_w, const float *bn_b, const float *mean,
                      const float *invstd, const float *pw_w, const float *pw_b, float *y, int B, int C, int M, int N);
    static int pw_bwd(const TrainPlan &p, hipStream_t s, const float *gy, const float *u, const float *bn_w, const float *bn_b,
                      const float *mean, const float *invstd, const float *pw_w, float *gz, float *part_bn, int B, int C, int M, int N);
    static int pw_wgrad(const char *what, const TrainPlan &p, hipStream_t s, const float *gy, const float *u, const float *bn_w,
                        const float *bn_b, const float *mean, const float *invstd, float *part_pw, int B, int C, int M, int N);
    static int pw_wgrad_sum(hipStream_t s, const float *part_pw, int nparts, int M, int C, float *d_pw_w, float *d_pw_b);
};

// ---- forward ---------------------------------------------------------------------------------------------------------------------
// y[b] = W . relu(u[b]*alpha + beta') + bias; W (M, K) row major, on the tile of pw_gemm_tile.h.
template <int MT>
__global__ __launch_bounds__(256, 2) void ct_pw_fwd_kernel(const float *__restrict__ u, const float *__restrict__ gamma,
                                                           const float *__restrict__ beta, const float *__restrict__ mean,
                                                           const float *__restrict__ invstd, const float *__restrict__ pw_w,
                                                           const float *__restrict__ pw_b, float *__restrict__ y, int M, int K, int N) {
    constexpr int BM = 32 * MT, AP = BM + 1;  // odd pitch: the transposing stores of the weight tile spread over the banks
    __shared__ float As[kKT][AP];
    __shared__ __attribute__((aligned(16))) float Bs[kKT][kBN];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.z, m0 = blockIdx.y * BM, n0 = blockIdx.x * kBN;
    const float *ub = u + (size_t)b * K * N;
    const int col = lane & 31, kh = lane >> 5;
    PwAcc<MT> acc;
    acc.zero();
    for (int k0 = 0; k0 < K; k0 += kKT) {
        for (int e = tid; e < kKT * BM; e += 256) {
            const int mm = e / kKT, k = e - mm * kKT;
            const bool ok = m0 + mm < M && k0 + k < K;
            const float v = pw_w[ok ? (size_t)(m0 + mm) * K + k0 + k : 0];
            As[k][mm] = ok ? v : 0.f;
        }
        stage_cells(Bs, ub, k0, K, n0, N, tid, [&](int kk) {
            float al, be;
            bn_affine(gamma[kk], beta[kk], mean[kk], invstd[kk], al, be);
            return [=](float v) { return fmaxf(bn_pre(v, al, be), 0.f); };
        });
        __syncthreads();
        acc.products(As, Bs, wave, col, kh);
        __syncthreads();
    }
    const int n = n0 + wave * 32 + col;
    if (n < N) {
        float *yb = y + (size_t)b * M * N + n;
        acc.each(kh, [&](int row, float v) {
            const int m = m0 + row;
            if (m < M) yb[(size_t)m * N] = v + pw_b[m];
        });
    }
}

// ---- backward --------------------------------------------------------------------------------------------------------------------
// gt[b] = W^T . gy[b] (rows = the C channels, k = the M output channels); pw_bwd_finish masks it by the forward's ReLU and leaves
// the partial sums BatchNorm's backward needs.  part: (C, B * gridDim.x, 2).
template <int MT>
__global__ __launch_bounds__(256, 2) void ct_pw_bwd_kernel(const float *__restrict__ gy, const float *__restrict__ u,
                                                           const float *__restrict__ gamma, const float *__restrict__ beta,
                                                           const float *__restrict__ mean, const float *__restrict__ invstd,
                                                           const float *__restrict__ pw_w, float *__restrict__ gz, float *__restrict__ part,
                                                           int M, int C, int N) {
    constexpr int BM = 32 * MT;
    __shared__ float As[kKT][BM];
    __shared__ __attribute__((aligned(16))) float Bs[kKT][kBN];
    __shared__ float Al[BM], Be[BM], Mn[BM], Is[BM];
    __shared__ float red[4][BM][2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.z, c0 = blockIdx.y * BM, n0 = blockIdx.x * kBN;
    const float *gb = gy + (size_t)b * M * N;
    const int col = lane & 31, kh = lane >> 5;
    stage_bn_rows(BM, c0, C, gamma, beta, mean, invstd, Al, Be, Mn, Is);  // read after the loop's barriers
    PwAcc<MT> acc;
    acc.zero();
    for (int k0 = 0; k0 < M; k0 += kKT) {
        for (int e = tid; e < kKT * BM; e += 256) {
            const int k = e / BM, cc = e - k * BM;
            const bool ok = k0 + k < M && c0 + cc < C;
            const float v = pw_w[ok ? (size_t)(k0 + k) * C + c0 + cc : 0];
            As[k][cc] = ok ? v : 0.f;
        }
        stage_cells(Bs, gb, k0, M, n0, N, tid, AsItIs());
        __syncthreads();
        acc.products(As, Bs, wave, col, kh);
        __syncthreads();
    }
    pw_bwd_finish<F32Maps>(acc, Al, Be, Mn, Is, red, u, gz, part, b, c0, n0, C, N, wave, col, kh);
}

// One split of dW[m, c] = sum_p gy[m, p] t[c, p], c = C being a row of ones (db_pw).  Workgroup: 32*MT rows m x 32*CW columns c;
// its 4 waves are CW column groups x KS = 4/CW cell groups, and every (split, cell group) leaves its own partial (M, C+1) matrix:
// narrow blocks (few columns) spread their waves over the cells instead of idling.  blockIdx.z = image x split.
template <int MT, int CW>
__global__ __launch_bounds__(256) void ct_pw_wgrad_kernel(const float *__restrict__ gy, const float *__restrict__ u,
                                                          const float *__restrict__ gamma, const float *__restrict__ beta,
                                                          const float *__restrict__ mean, const float *__restrict__ invstd,
                                                          float *__restrict__ part, int M, int C, int N, int S, int chunk) {
    constexpr int KS = 4 / CW, KTS = kWgCells * KS, BM = 32 * MT, BC = 32 * CW, P = KTS + 1;
    static_assert((BM + BC) * P * 4 <= 60 * 1024, "LDS");
    __shared__ float As[BM * P];
    __shared__ float Bs[BC * P];
    __shared__ float Al[BC], Be[BC];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cw = wave % CW, ks = wave / CW;
    const int col = lane & 31, kh = lane >> 5;
    const int c0 = blockIdx.x * BC, m0 = blockIdx.y * BM;
    const int b = blockIdx.z / S, sp = blockIdx.z - b * S;
    const int n_begin = sp * chunk, n_end = min(N, n_begin + chunk);
    const float *gb = gy + (size_t)b * M * N;
    const float *ub = u + (size_t)b * C * N;
    stage_bn_rows(BC, c0, C, gamma, beta, mean, invstd, Al, Be);
    __syncthreads();
    PwAcc<MT> acc;
    acc.zero();
    for (int nb = n_begin; nb < n_end; nb += KTS) {
        for (int e = tid; e < BM * KTS; e += 256) {
            const int row = e / KTS, kk = e - row * KTS;
            const bool ok = nb + kk < n_end && m0 + row < M;
            const float v = gb[ok ? (size_t)(m0 + row) * N + nb + kk : 0];
            As[row * P + kk] = ok ? v : 0.f;
        }
        for (int e = tid; e < BC * KTS; e += 256) {
            const int row = e / KTS, kk = e - row * KTS;
            const int c = c0 + row;
            const bool cell = nb + kk < n_end, ok = cell && c < C;
            const float v = ub[ok ? (size_t)c * N + nb + kk : 0];
            const float t = fmaxf(bn_pre(v, Al[row], Be[row]), 0.f);
            Bs[row * P + kk] = ok ? t : (cell && c == C ? 1.f : 0.f);
        }
        __syncthreads();
        const float *ap = &As[col * P + ks * kWgCells + kh];
        const float *bp = &Bs[(cw * 32 + col) * P + ks * kWgCells + kh];
#pragma unroll
        for (int s = 0; s < kWgCells / 2; ++s) {
            const float bv = bp[2 * s];
#pragma unroll
            for (int i = 0; i < MT; ++i) acc.a[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[i * 32 * P + 2 * s], bv, acc.a[i], 0, 0, 0);
        }
        __syncthreads();
    }
    store_wgrad_partial(acc, part, (size_t)(blockIdx.z * KS + ks), m0, c0 + cw * 32 + col, kh, M, C);
}

__global__ __launch_bounds__(256) void ct_pw_wgrad_sum_kernel(const float *__restrict__ part, int nparts, int M, int C,
                                                              float *__restrict__ d_pw_w, float *__restrict__ d_pw_b) {
    const int total = M * (C + 1);
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    double a = 0.0;
    for (int p = 0; p < nparts; ++p) a += (double)part[(size_t)p * total + idx];
    const int m = idx / (C + 1), c = idx - m * (C + 1);
    if (c < C) d_pw_w[(size_t)m * C + c] = (float)a;
    else d_pw_b[m] = (float)a;
}

// ---- host: this class's four launches for train_fwd / train_bwd ----------------------------------------------------------------------
int F32Maps::pw_fwd(const TrainPlan &p, hipStream_t s, const float *u, const float *bn_w, const float *bn_b, const float *mean,
                    const float *invstd, const float *pw_w, const float *pw_b, float *y, int B, int C, int M, int N) {
    int nblk, mt;
    slab_shape(M, &nblk, &mt);
    const dim3 grid((unsigned)p.ntn, (unsigned)nblk, (unsigned)B);
    with_row_tiles(mt, [&](auto MT) {
        hipLaunchKernelGGL((ct_pw_fwd_kernel<decltype(MT)::value>), grid, dim3(256), 0, s, u, bn_w, bn_b, mean, invstd, pw_w, pw_b, y, M, C, N);
    });
    return gfn::check_launch("ct_pw_fwd_kernel");
}

int F32Maps::pw_bwd(const TrainPlan &p, hipStream_t s, const float *gy, const float *u, const float *bn_w, const float *bn_b,
                    const float *mean, const float *invstd, const float *pw_w, float *gz, float *part_bn, int B, int C, int M, int N) {
    int nblk, mt;
    slab_shape(C, &nblk, &mt);
    const dim3 grid((unsigned)p.ntn, (unsigned)nblk, (unsigned)B);
    with_row_tiles(mt, [&](auto MT) {
        hipLaunchKernelGGL((ct_pw_bwd_kernel<decltype(MT)::value>), grid, dim3(256), 0, s, gy, u, bn_w, bn_b, mean, invstd, pw_w, gz, part_bn, M, C,
                           N);
    });
    return gfn::check_launch("ct_pw_bwd_kernel");
}

int F32Maps::pw_wgrad(const char *what, const TrainPlan &p, hipStream_t s, const float *gy, const float *u, const float *bn_w,
                      const float *bn_b, const float *mean, const float *invstd, float *part_pw, int B, int C, int M, int N) {
    const dim3 grid((unsigned)p.wg_tc, (unsigned)p.wg_tm, (unsigned)(B * p.wg_s));
    const bool found = with_wgrad_shape(p, [&](auto sh) {
        hipLaunchKernelGGL((ct_pw_wgrad_kernel<decltype(sh)::mt, decltype(sh)::cw>), grid, dim3(256), 0, s, gy, u, bn_w, bn_b, mean, invstd,
                           part_pw, M, C, N, p.wg_s, p.wg_chunk);
    });
    if (!found) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: no weight-gradient kernel for this shape", what);
    return gfn::check_launch("ct_pw_wgrad_kernel");
}

int F32Maps::pw_wgrad_sum(hipStream_t s, const float *part_pw, int nparts, int M, int C, float *d_pw_w, float *d_pw_b) {
    hipLaunchKernelGGL(ct_pw_wgrad_sum_kernel, dim3((unsigned)((M * (C + 1) + 255) / 256)), dim3(256), 0, s, part_pw, nparts, M, C, d_pw_w, d_pw_b);
    return gfn::check_launch("ct_pw_wgrad_sum_kernel");
}

}  // namespace

GFN_EXPORT int64_t gfn_conv_block_train_ws_bytes(int B, int C, int M, int G, int backward) {
    return train_ws_bytes<F32Maps>(B, C, M, G, backward);
}

GFN_EXPORT int gfn_conv_block_train_fwd(const float *x, const float *dw_w, const float *dw_b, const float *bn_w, const float *bn_b,
                                        float *running_mean, float *running_var, const float *pw_w, const float *pw_b, float *u,
                                        float *mean, float *invstd, float *y, int B, int C, int M, int G, double momentum, double eps,
                                        void *ws, int64_t ws_bytes, gfn_stream_t stream) {
    return train_fwd<F32Maps>("conv_block_train_fwd", x, GFN_F32, dw_w, dw_b, bn_w, bn_b, running_mean, running_var, pw_w, pw_b, u, mean,
                              invstd, y, B, C, M, G, momentum, eps, ws, ws_bytes, stream);
}

GFN_EXPORT int gfn_conv_block_train_bwd(const float *gy, const float *x, const float *u, const float *mean, const float *invstd,
                                        const float *dw_w, const float *bn_w, const float *bn_b, const float *pw_w, float *gx,
                                        float *d_dw_w, float *d_dw_b, float *d_bn_w, float *d_bn_b, float *d_pw_w, float *d_pw_b, int B,
                                        int C, int M, int G, int need, void *ws, int64_t ws_bytes, gfn_stream_t stream) {
    return train_bwd<F32Maps>("conv_block_train_bwd", gy, x, GFN_F32, u, mean, invstd, dw_w, bn_w, bn_b, pw_w, gx, d_dw_w, d_dw_b, d_bn_w,
                              d_bn_b, d_pw_w, d_pw_b, B, C, M, G, need, ws, ws_bytes, stream);
}
