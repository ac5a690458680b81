// conv_train_16bit.h -- the refiner's training-mode conv block in a class whose maps hold 16-bit floats, said once for fp16
// (conv_stack_train_half.hip) and bf16 (conv_stack_train_bf16.hip).  The element E, _Float16 or __bf16, tells the two apart, and
// elem16.h says what comes with it: V8<E> = Elem16<E>::vec8, a lane's operand fragment and a 16-byte access; Elem16<E>::round(v), the
// float a value becomes once it is rounded to E (to nearest even, no clamp: past the format's range it is inf); and mfma16, the
// 32x32x16 matrix instruction on two V8<E> fragments with fp32 accumulators.
// Maps16<E> is the class K of conv_train_common.h, which writes everything around the 1x1 products once for all classes.  Here: the
// matrix-core tile beside the exact-fp32 tile of pw_gemm_tile.h whose accumulators (PwAcc) and 128-cell workgroup tile it keeps, the
// three GEMM kernels (ct_half_pw_fwd / _bwd / _wgrad_kernel), the split sum of the weight gradient and the class's four launches.
//
// v_mfma_f32_32x32x16_{f16,bf16}: lane (col = lane & 31, kh = lane >> 5) supplies A[row col][k = 8 kh + j] and B[k = 8 kh + j][column
// col], j = 0 .. 7, as eight elements of one register quad, and receives D[row acc_row(r, kh)][column col].  So both operand tiles lie
// in LDS as [row or column][k] with k contiguous, and a lane's fragment is one 16-byte read.  The pitch is the K tile plus 8 elements:
// rows 80, 144 or 272 bytes apart start 20, 36 or 4 banks apart, and the 16 lanes a 16-byte read serves at a time cover all 64
// banks once.  Opens its own anonymous namespace.
#pragma once
#include "conv_train_common.h"
#include "elem16.h"

namespace {

using gfn::Elem16;
using gfn::mfma16;
template <typename E>
using V8 = typename Elem16<E>::vec8;

constexpr int kHKT = 32;  // channels per K tile of the forward and the input-gradient GEMM: two MFMA steps
constexpr int half_pitch(int kt) { return kt + 8; }

// One row tile per workgroup in the forward and the input-gradient GEMM: 32 rows x 128 cells.  The fp32 class's slabs of up to 7 row
// tiles leave a coarse grid with 128 workgroups for 256 CUs (417 rows on 32 x 32 cells, batch 8), one per CU and nothing to hide its
// loads behind; measured on the stack's step at the five widths, 1 row tile was the fastest or within 4 % of it.
constexpr int kHBM = 32;

// An operand tile T[ROWS][half_pitch(KT)]: every thread fills 16-byte pieces, piece(row, k8) handing back the eight elements
// T[row][k8 .. k8 + 7] (zeros where the source ends).  ROWS_FIRST: consecutive lanes take consecutive rows -- for a source whose
// rows are contiguous in memory and whose k is strided (a map's cells under its channels); otherwise consecutive lanes take
// consecutive pieces of one row (a source with k contiguous).
template <typename E, int ROWS, int KT, bool ROWS_FIRST, typename V>
__device__ __forceinline__ void stage_half_tile(E *T, int tid, V piece) {
    constexpr int P = half_pitch(KT), G8 = KT / 8;
    for (int e = tid; e < ROWS * G8; e += 256) {
        const int row = ROWS_FIRST ? e % ROWS : e / G8, k8 = (ROWS_FIRST ? e / ROWS : e % G8) * 8;
        *reinterpret_cast<V8<E> *>(&T[row * P + k8]) = piece(row, k8);
    }
}

// eight consecutive elements src[0 .. 7] of which the first `valid` exist; vec: src is 16-byte aligned (the caller's promise)
template <typename E>
__device__ __forceinline__ V8<E> load_half8(const E *src, int valid, bool vec) {
    if (vec && valid >= 8) return *reinterpret_cast<const V8<E> *>(src);
    V8<E> h;
#pragma unroll
    for (int j = 0; j < 8; ++j) h[j] = j < valid ? src[j] : (E)0.f;
    return h;
}

// STEPS MFMA steps of 16 k: a, b point at the lane's own fragment of the first step (row or column `col`, k = 8 kh) in tiles of
// pitch AP and BP; row tile i of A lies 32 rows further
template <typename E, int MT, int STEPS, int AP>
__device__ __forceinline__ void half_products(PwAcc<MT> &acc, const E *a, const E *b) {
#pragma unroll
    for (int s = 0; s < STEPS; ++s) {
        const V8<E> bv = *reinterpret_cast<const V8<E> *>(b + 16 * s);
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            const V8<E> av = *reinterpret_cast<const V8<E> *>(a + i * 32 * AP + 16 * s);
            acc.a[i] = mfma16(av, bv, acc.a[i]);
        }
    }
}

// the class: maps hold E; a value is rounded where it is stored in a map or becomes an operand.  x is fp32 (a stack's first
// block: rounded on load, its gx written fp32) or E
template <typename E>
struct Maps16 {
    using map_t = E;
    static __device__ __forceinline__ float value(float v) { return Elem16<E>::round(v); }
    static int check_class(const char *what, int x_dtype, int C, int M);
    static int pw_fwd(const TrainPlan &p, hipStream_t s, const map_t *u, const float *bn_w, const float *bn_b, const float *mean,
                      const float *invstd, const float *pw_w, const float *pw_b, map_t *y, int B, int C, int M, int N);
    static int pw_bwd(const TrainPlan &p, hipStream_t s, const map_t *gy, const map_t *u, const float *bn_w, const float *bn_b,
                      const float *mean, const float *invstd, const float *pw_w, map_t *gz, float *part_bn, int B, int C, int M, int N);
    static int pw_wgrad(const char *what, const TrainPlan &p, hipStream_t s, const map_t *gy, const map_t *u, const float *bn_w,
                        const float *bn_b, const float *mean, const float *invstd, float *part_pw, int B, int C, int M, int N);
    static int pw_wgrad_sum(hipStream_t s, const float *part_pw, int nparts, int M, int C, float *d_pw_w, float *d_pw_b);
};

// ---- forward ---------------------------------------------------------------------------------------------------------------------
// the B operand tile of a (K, N) map: Bs[cell][k] = f(k, map[k0 + k][n0 + cell]); channels past K and cells past N are zero
template <typename E, typename F>
__device__ __forceinline__ void stage_map_cells(E *Bs, const E *map, int k0, int K, int n0, int N, int tid, F f) {
    stage_half_tile<E, kBN, kHKT, true>(Bs, tid, [&](int cell, int k8) {
        const int n = n0 + cell;
        V8<E> h;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int kk = k0 + k8 + j;
            const bool ok = n < N && kk < K;
            const E v = map[ok ? (size_t)kk * N + n : 0];
            h[j] = ok ? f(k8 + j, v) : (E)0.f;
        }
        return h;
    });
}

// y[b] = elem(W . t + bias), t = elem(relu(u[b]*alpha + beta')); W (M, K) row major
template <typename E>
__global__ __launch_bounds__(256, 2) void ct_half_pw_fwd_kernel(const E *__restrict__ u, const float *__restrict__ gamma,
                                                                const float *__restrict__ beta, const float *__restrict__ mean,
                                                                const float *__restrict__ invstd, const float *__restrict__ pw_w,
                                                                const float *__restrict__ pw_b, E *__restrict__ y, int M, int K, int N) {
    constexpr int BM = kHBM, P = half_pitch(kHKT);
    __shared__ __attribute__((aligned(16))) E As[BM * P];
    __shared__ __attribute__((aligned(16))) E Bs[kBN * P];
    __shared__ float Al[2][kHKT], Be[2][kHKT];  // the K tile's alpha, beta': the next tile's are formed while this one is staged
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.z, m0 = blockIdx.y * BM, n0 = blockIdx.x * kBN;
    const E *ub = u + (size_t)b * K * N;
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
        stage_half_tile<E, BM, kHKT, false>(As, tid, [&](int row, int k8) {
            const int m = m0 + row;
            V8<E> h;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const bool ok = m < M && k0 + k8 + j < K;
                const float v = pw_w[ok ? (size_t)m * K + k0 + k8 + j : 0];
                h[j] = ok ? (E)v : (E)0.f;
            }
            return h;
        });
        stage_map_cells<E>(Bs, ub, k0, K, n0, N, tid,
                           [&](int k, E v) { return (E)fmaxf(bn_pre((float)v, Al[buf][k], Be[buf][k]), 0.f); });
        affine(buf ^ 1, k0 + kHKT);
        __syncthreads();
        half_products<E, 1, kHKT / 16, P>(acc, &As[col * P + 8 * kh], &Bs[(wave * 32 + col) * P + 8 * kh]);
        __syncthreads();
    }
    const int n = n0 + wave * 32 + col;
    if (n < N) {
        E *yb = y + (size_t)b * M * N + n;
        acc.each(kh, [&](int row, float v) {
            const int m = m0 + row;
            if (m < M) yb[(size_t)m * N] = (E)(v + pw_b[m]);
        });
    }
}

// ---- backward --------------------------------------------------------------------------------------------------------------------
// gt[b] = W^T . gy[b] (rows = the C channels, k = the M output channels); pw_bwd_finish: gz = elem(gt) where u*alpha + beta' > 0,
// written as a C map, and the per-workgroup partial sums of that rounded gz and of gz*u_hat.  part: (C, B * gridDim.x, 2).
template <typename E>
__global__ __launch_bounds__(256, 2) void ct_half_pw_bwd_kernel(const E *__restrict__ gy, const E *__restrict__ u, const float *__restrict__ gamma,
                                                                const float *__restrict__ beta, const float *__restrict__ mean,
                                                                const float *__restrict__ invstd, const float *__restrict__ pw_w,
                                                                E *__restrict__ gz, float *__restrict__ part, int M, int C, int N) {
    constexpr int BM = kHBM, P = half_pitch(kHKT);
    __shared__ __attribute__((aligned(16))) E As[BM * P];
    __shared__ __attribute__((aligned(16))) E Bs[kBN * P];
    __shared__ float Al[BM], Be[BM], Mn[BM], Is[BM];
    __shared__ float red[4][BM][2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.z, c0 = blockIdx.y * BM, n0 = blockIdx.x * kBN;
    const E *gb = gy + (size_t)b * M * N;
    const int col = lane & 31, kh = lane >> 5;
    stage_bn_rows(BM, c0, C, gamma, beta, mean, invstd, Al, Be, Mn, Is);  // read after the loop's barriers
    PwAcc<1> acc;
    acc.zero();
    for (int k0 = 0; k0 < M; k0 += kHKT) {
        stage_half_tile<E, BM, kHKT, true>(As, tid, [&](int cc, int k8) {  // A[c][m] = W[m][c]: consecutive lanes, consecutive c
            V8<E> h;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const bool ok = k0 + k8 + j < M && c0 + cc < C;
                const float v = pw_w[ok ? (size_t)(k0 + k8 + j) * C + c0 + cc : 0];
                h[j] = ok ? (E)v : (E)0.f;
            }
            return h;
        });
        stage_map_cells<E>(Bs, gb, k0, M, n0, N, tid, [](int, E v) { return v; });
        __syncthreads();
        half_products<E, 1, kHKT / 16, P>(acc, &As[col * P + 8 * kh], &Bs[(wave * 32 + col) * P + 8 * kh]);
        __syncthreads();
    }
    pw_bwd_finish<Maps16<E>>(acc, Al, Be, Mn, Is, red, u, gz, part, b, c0, n0, C, N, wave, col, kh);
}

// One split of dW[m, c] = sum_p gy[m, p] t[c, p], c = C being a row of ones (db_pw); the workgroup and wave shapes of
// ct_pw_wgrad_kernel.  Both operands have their k -- the cells -- contiguous in HBM: the tiles are plain copies of map rows
// (16 bytes at a time where vec says every piece is aligned), t recomputed from u on the way.
template <typename E, int MT, int CW>
__global__ __launch_bounds__(256) void ct_half_pw_wgrad_kernel(const E *__restrict__ gy, const E *__restrict__ u,
                                                               const float *__restrict__ gamma, const float *__restrict__ beta,
                                                               const float *__restrict__ mean, const float *__restrict__ invstd,
                                                               float *__restrict__ part, int M, int C, int N, int S, int chunk, int vec) {
    constexpr int KS = 4 / CW, KTS = kWgCells * KS, BM = 32 * MT, BC = 32 * CW, P = half_pitch(KTS);
    __shared__ __attribute__((aligned(16))) E As[BM * P];
    __shared__ __attribute__((aligned(16))) E Bs[BC * P];
    __shared__ float Al[BC], Be[BC];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cw = wave % CW, ks = wave / CW;
    const int col = lane & 31, kh = lane >> 5;
    const int c0 = blockIdx.x * BC, m0 = blockIdx.y * BM;
    const int b = blockIdx.z / S, sp = blockIdx.z - b * S;
    const int n_begin = sp * chunk, n_end = min(N, n_begin + chunk);
    const E *gb = gy + (size_t)b * M * N;
    const E *ub = u + (size_t)b * C * N;
    stage_bn_rows(BC, c0, C, gamma, beta, mean, invstd, Al, Be);
    __syncthreads();
    PwAcc<MT> acc;
    acc.zero();
    for (int nb = n_begin; nb < n_end; nb += KTS) {
        stage_half_tile<E, BM, KTS, false>(As, tid, [&](int row, int k8) {
            const int valid = m0 + row < M ? n_end - (nb + k8) : 0;
            return load_half8<E>(gb + (valid > 0 ? (size_t)(m0 + row) * N + nb + k8 : 0), valid, vec);
        });
        stage_half_tile<E, BC, KTS, false>(Bs, tid, [&](int row, int k8) {
            const int c = c0 + row, cells = n_end - (nb + k8);
            const int valid = c < C ? cells : 0;
            const V8<E> uu = load_half8<E>(ub + (valid > 0 ? (size_t)c * N + nb + k8 : 0), valid, vec);
            V8<E> h;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const E t = (E)fmaxf(bn_pre((float)uu[j], Al[row], Be[row]), 0.f);
                h[j] = j < valid ? t : (E)(c == C && j < cells ? 1.f : 0.f);
            }
            return h;
        });
        __syncthreads();
        half_products<E, MT, kWgCells / 16, P>(acc, &As[col * P + ks * kWgCells + 8 * kh], &Bs[(cw * 32 + col) * P + ks * kWgCells + 8 * kh]);
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

// ---- host: the class's check and four launches for train_fwd / train_bwd -----------------------------------------------------------
template <typename E>
int Maps16<E>::check_class(const char *what, int x_dtype, int C, int M) {
    if (x_dtype != GFN_F32 && x_dtype != Elem16<E>::kDtype) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: x_dtype must be GFN_F32 or %s", what, Elem16<E>::kDtypeName);
    if (C > 65535 * kHBM || M > 65535 * kHBM) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: more than %d channels", what, 65535 * kHBM);
    return GFN_OK;
}

template <typename E>
int Maps16<E>::pw_fwd(const TrainPlan &p, hipStream_t s, const map_t *u, const float *bn_w, const float *bn_b, const float *mean,
                      const float *invstd, const float *pw_w, const float *pw_b, map_t *y, int B, int C, int M, int N) {
    const dim3 grid((unsigned)p.ntn, (unsigned)((M + kHBM - 1) / kHBM), (unsigned)B);
    hipLaunchKernelGGL(ct_half_pw_fwd_kernel<E>, grid, dim3(256), 0, s, u, bn_w, bn_b, mean, invstd, pw_w, pw_b, y, M, C, N);
    return gfn::check_launch("ct_half_pw_fwd_kernel");
}

template <typename E>
int Maps16<E>::pw_bwd(const TrainPlan &p, hipStream_t s, const map_t *gy, const map_t *u, const float *bn_w, const float *bn_b,
                      const float *mean, const float *invstd, const float *pw_w, map_t *gz, float *part_bn, int B, int C, int M, int N) {
    const dim3 grid((unsigned)p.ntn, (unsigned)((C + kHBM - 1) / kHBM), (unsigned)B);
    hipLaunchKernelGGL(ct_half_pw_bwd_kernel<E>, grid, dim3(256), 0, s, gy, u, bn_w, bn_b, mean, invstd, pw_w, gz, part_bn, M, C, N);
    return gfn::check_launch("ct_half_pw_bwd_kernel");
}

template <typename E>
int Maps16<E>::pw_wgrad(const char *what, const TrainPlan &p, hipStream_t s, const map_t *gy, const map_t *u, const float *bn_w,
                        const float *bn_b, const float *mean, const float *invstd, float *part_pw, int B, int C, int M, int N) {
    const dim3 grid((unsigned)p.wg_tc, (unsigned)p.wg_tm, (unsigned)(B * p.wg_s));
    // every 8-cell piece of a map row starts on 16 bytes: rows do when N % 8 == 0, pieces inside them always (chunks are
    // multiples of 32 cells)
    const int vec = N % 8 == 0 && !misaligned(gy) && !misaligned(u);
    const bool found = with_wgrad_shape(p, [&](auto sh) {
        hipLaunchKernelGGL((ct_half_pw_wgrad_kernel<E, decltype(sh)::mt, decltype(sh)::cw>), grid, dim3(256), 0, s, gy, u, bn_w, bn_b, mean,
                           invstd, part_pw, M, C, N, p.wg_s, p.wg_chunk, vec);
    });
    if (!found) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: no weight-gradient kernel for this shape", what);
    return gfn::check_launch("ct_half_pw_wgrad_kernel");
}

template <typename E>
int Maps16<E>::pw_wgrad_sum(hipStream_t s, const float *part_pw, int nparts, int M, int C, float *d_pw_w, float *d_pw_b) {
    hipLaunchKernelGGL(ct_half_pw_wgrad_sum_kernel, dim3((unsigned)((M * (C + 1) + 15) / 16)), dim3(256), 0, s, part_pw, nparts, M, C, d_pw_w,
                       d_pw_b);
    return gfn::check_launch("ct_half_pw_wgrad_sum_kernel");
}

}  // namespace
