// conv_stack_train.hip -- one refiner conv block in TRAINING mode on gfx950: batch-statistic BatchNorm forward and the backward.
//
// Reference: ConvRefiner.create_block / forward, model/network.py:471-487 and :560-563, under model.train() -- per block
//   Conv2d(C, C, 5x5, padding 2, groups=C[, bias])  ->  BatchNorm2d (batch statistics)  ->  ReLU  ->  Conv2d(C, M, 1x1)
// differentiated by torch autograd there.  Everything is fp32 on contiguous (B, C, G, G) maps; the eval-mode kernels
// (conv_stack.hip) fold BatchNorm from the running statistics and cannot serve: here the statistics are the batch's own, the
// running buffers are updated, and the backward yields the input gradient and seven parameter gradients.
//
// Forward (3 launches)
//   ct_dw_fwd_kernel       u = dw5x5(x) + b_dw on 32x32 tiles staged with their halo in LDS (stage_halo; dw_taps: 25 fmas per cell in
//                          (dy, dx) order); u goes to HBM -- the backward needs it -- and every workgroup leaves its tile's
//                          (mean, M2 = sum (u - mean)^2): shifted sums, safe against cancellation
//   ct_stats_kernel        per channel: Chan's merge of the tiles' (n, mean, M2) in double, in a fixed order; mean, invstd =
//                          1/sqrt(var + eps) with the biased variance, and the running buffers (unbiased variance) as torch
//   ct_pw_fwd_kernel       y = W_pw . relu(u*alpha + beta') + b_pw on the fp32 matrix-core tile of pw_gemm_tile.h (pw_gemm_kernel's too);
//                          alpha = gamma*invstd, beta' = beta - mean*alpha (bn_affine); t = relu(..) is formed while the B operand
//                          tile is staged and never reaches HBM
// Backward (up to 7 launches, each skipped when the `need` mask does not ask for what it makes)
//   ct_pw_bwd_kernel       gt = W_pw^T . gy on the same tile; gz = gt where u*alpha + beta' > 0 (the forward's own expression, so
//                          both masks agree bit for bit), written as a C map; per-workgroup partial sums of gz and gz*u_hat
//   ct_bn_bwd_kernel       dbeta = sum gz, dgamma = sum gz*u_hat from the partials (double, fixed order)
//   ct_pw_wgrad_kernel     dW_pw[m, c] = sum_p gy[m, p] t[c, p] on the matrix core (PwAcc; K runs over the cells), t recomputed from u;
//                          a column of ones appended to t makes db_pw the (C+1)-th column.  Split over the cells; every split writes
//                          its own partial matrix
//   ct_pw_wgrad_sum_kernel sums the partial matrices in a fixed order
//   ct_dw_bwd_kernel       gu = alpha*(gz - dbeta/N - u_hat*dgamma/N) formed while the gz / u halo tile is staged; gx = dw5x5 of gu with
//                          flipped taps (the forward's stage_halo and dw_taps); per-workgroup partials of dW_dw[c, k] =
//                          sum_p gu[p] x[p + off_k] and db_dw = sum gu
//   ct_dw_wgrad_kernel     sums those partials (double, fixed order)
// No floating-point atomics anywhere: two identical calls give identical bits.
// The depthwise tile, bn_affine / bn_pre, the merge and three of the small reductions are conv_train_common.h's, shared with the fp16
// autocast class of conv_stack_train_half.hip.
#include "conv_train_common.h"

namespace {

// ---- forward ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ct_dw_fwd_kernel(const float *__restrict__ x, const float *__restrict__ dw_w,
                                                        const float *__restrict__ dw_b, float *__restrict__ u, float *__restrict__ part,
                                                        int C, int G, int tiles_x, int tiles, int nparts) {
    __shared__ __attribute__((aligned(16))) float Xs[kHalo * kHalo];
    __shared__ float red[4];
    const int tid = threadIdx.x;
    const TileId t = decode_tile(blockIdx.x, C, tiles_x, tiles);
    const float *xp = x + t.plane * (size_t)G * G;
    stage_halo(Xs, t, G, [&](bool ok, int off) {
        const float v = xp[off];
        return ok ? v : 0.f;
    });
    __syncthreads();
    const int r = tid >> 3, c4 = (tid & 7) * 4;
    float acc[4];
    dw_taps<false>(Xs, dw_w + (size_t)t.c * 25, r, c4, acc);
    const float bias = dw_b ? dw_b[t.c] : 0.f;
    const int gy = t.row0 + r, gx0 = t.col0 + c4;
    float *up = u + t.plane * (size_t)G * G + (size_t)gy * G + gx0;
    float uq[4], s = 0.f;
    bool ok[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        uq[q] = acc[q] + bias;
        ok[q] = gy < G && gx0 + q < G;
        if (ok[q]) up[q] = uq[q];
        s += ok[q] ? uq[q] : 0.f;
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

__global__ __launch_bounds__(64) void ct_stats_kernel(const float *__restrict__ part, float *__restrict__ mean, float *__restrict__ invstd,
                                                      float *__restrict__ running_mean, float *__restrict__ running_var, int G, int tiles_x,
                                                      int tiles, int nparts, double momentum, double eps) {
    stats_channel(part, mean, invstd, running_mean, running_var, G, tiles_x, tiles, nparts, momentum, eps);
}

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
// gt[b] = W^T . gy[b] (rows = the C channels, k = the M output channels), masked by the forward's ReLU, plus the partial sums
// BatchNorm's backward needs.  part: (C, B * gridDim.x, 2).
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
    if (tid < BM) {
        const int c = c0 + tid;
        float al = 0.f, be = 0.f, mn = 0.f, is = 0.f;
        if (c < C) {
            mn = mean[c], is = invstd[c];
            bn_affine(gamma[c], beta[c], mn, is, al, be);
        }
        Al[tid] = al, Be[tid] = be, Mn[tid] = mn, Is[tid] = is;
    }
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
    const int n = n0 + wave * 32 + col;
    const bool nok = n < N;
    const size_t base = (size_t)b * C * N + (nok ? n : 0);
    acc.each(kh, [&](int row, float a) {
        const int c = c0 + row;
        const bool ok = nok && c < C;
        const size_t at = base + (size_t)(ok ? c : 0) * N;
        const float uu = u[at];
        const float g = ok && bn_pre(uu, Al[row], Be[row]) > 0.f ? a : 0.f;
        if (ok) gz[at] = g;
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

__global__ __launch_bounds__(64) void ct_bn_bwd_kernel(const float *__restrict__ part, int nparts, int C, float *__restrict__ dgdb,
                                                       float *__restrict__ dgamma, float *__restrict__ dbeta) {
    bn_bwd_channel(part, nparts, C, dgdb, dgamma, dbeta);
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
    if (tid < BC) {
        float al = 0.f, be = 0.f;
        if (c0 + tid < C) bn_affine(gamma[c0 + tid], beta[c0 + tid], mean[c0 + tid], invstd[c0 + tid], al, be);
        Al[tid] = al, Be[tid] = be;
    }
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
    const int cidx = c0 + cw * 32 + col;
    if (cidx <= C) {
        float *pp = part + (size_t)(blockIdx.z * KS + ks) * M * (C + 1) + cidx;
        acc.each(kh, [&](int row, float v) {
            if (m0 + row < M) pp[(size_t)(m0 + row) * (C + 1)] = v;
        });
    }
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

// gu on the fly, gx and the partials of the depthwise parameter gradients; the tiling of ct_dw_fwd_kernel.  need bit 0: gx, bit 1:
// the partials.
__global__ __launch_bounds__(256) void ct_dw_bwd_kernel(const float *__restrict__ gz, const float *__restrict__ u, const float *__restrict__ x,
                                                        const float *__restrict__ dw_w, const float *__restrict__ gamma,
                                                        const float *__restrict__ mean, const float *__restrict__ invstd,
                                                        const float *__restrict__ dgdb, float *__restrict__ gx, float *__restrict__ part,
                                                        int C, int G, int tiles_x, int tiles, int nparts, float inv_n, int need) {
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
        const float g = gz[pbase + off], uu = u[pbase + off];
        return ok ? al * (g - k1 - ((uu - mn) * is) * k2) : 0.f;
    });
    if (want_w)
        stage_halo(Xs, t, G, [&](bool ok, int off) {
            const float xv = x[pbase + off];
            return ok ? xv : 0.f;
        });
    __syncthreads();
    const int r = tid >> 3, c4 = (tid & 7) * 4;
    if (want_x) {  // gx[q] = sum_k w[k] gu[q - off_k]: the forward's taps, flipped
        float acc[4];
        dw_taps<true>(Gs, dw_w + (size_t)t.c * 25, r, c4, acc);
        const int yy = t.row0 + r, xx0 = t.col0 + c4;
        float *gp = gx + pbase + (size_t)yy * G + xx0;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (yy < G && xx0 + q < G) gp[q] = acc[q];
    }
    if (want_w) dw_param_partials(Gs, Xs, r, c4, red, part + ((size_t)t.c * nparts + (size_t)t.b * tiles + t.tile) * kDwCols);
}

__global__ __launch_bounds__(256) void ct_dw_wgrad_kernel(const float *__restrict__ part, int nparts, float *__restrict__ d_dw_w,
                                                          float *__restrict__ d_dw_b) {
    dw_wgrad_channel(part, nparts, d_dw_w, d_dw_b);
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
// the tiling of TrainShape and where the partial sums and the gz map lie in the workspace, in floats
struct TrainPlan : TrainShape {
    int64_t fwd_floats;
    int64_t off_gz, off_bn, off_dgdb, off_dw, off_pw, bwd_floats;

    TrainPlan(int B, int C, int M, int G) : TrainShape(B, C, M, G) {
        const int64_t N = (int64_t)G * G;
        fwd_floats = align4((int64_t)C * B * tiles * 2);
        off_gz = 0;
        off_bn = off_gz + align4((int64_t)B * C * N);
        off_dgdb = off_bn + align4((int64_t)C * B * ntn * 2);
        off_dw = off_dgdb + align4(2 * (int64_t)C);
        off_pw = off_dw + align4((int64_t)C * B * tiles * kDwCols);
        bwd_floats = off_pw + align4((int64_t)wg_parts * M * (C + 1));
    }
};

}  // namespace

GFN_EXPORT int64_t gfn_conv_block_train_ws_bytes(int B, int C, int M, int G, int backward) {
    if (B <= 0 || C <= 0 || M <= 0 || G <= 0) return 0;
    const TrainPlan p(B, C, M, G);
    return (backward ? p.bwd_floats : p.fwd_floats) * (int64_t)sizeof(float);
}

GFN_EXPORT int gfn_conv_block_train_fwd(const float *x, const float *dw_w, const float *dw_b, const float *bn_w, const float *bn_b,
                                        float *running_mean, float *running_var, const float *pw_w, const float *pw_b, float *u,
                                        float *mean, float *invstd, float *y, int B, int C, int M, int G, double momentum, double eps,
                                        void *ws, int64_t ws_bytes, gfn_stream_t stream) {
    const char *what = "conv_block_train_fwd";
    if (!x || !dw_w || !bn_w || !bn_b || !running_mean || !running_var || !pw_w || !pw_b || !u || !mean || !invstd || !y)
        return gfn::fail(GFN_ERR_INVALID_ARG, "%s: null pointer", what);
    if (int rc = check_train_sizes(what, B, C, M, G)) return rc;
    if (x == u || x == y || u == y) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: x, u and y must be three different maps", what);
    if (!(momentum >= 0.0 && momentum <= 1.0) || !(eps >= 0.0)) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: momentum must lie in [0, 1] and eps be >= 0", what);
    if (B == 0) return GFN_OK;
    const TrainPlan p(B, C, M, G);
    if (!ws || misaligned(ws) || ws_bytes < p.fwd_floats * (int64_t)sizeof(float))
        return gfn::fail(GFN_ERR_SCRATCH, "%s: workspace missing, not 16-byte aligned or too small (%lld bytes needed)", what,
                         (long long)(p.fwd_floats * (int64_t)sizeof(float)));
    hipStream_t s = (hipStream_t)stream;
    float *part = static_cast<float *>(ws);
    const int nparts = B * p.tiles, N = G * G;
    hipLaunchKernelGGL(ct_dw_fwd_kernel, dim3((unsigned)(B * C * p.tiles)), dim3(256), 0, s, x, dw_w, dw_b, u, part, C, G, p.tiles_x, p.tiles,
                       nparts);
    if (int rc = gfn::check_launch("ct_dw_fwd_kernel")) return rc;
    hipLaunchKernelGGL(ct_stats_kernel, dim3((unsigned)C), dim3(64), 0, s, (const float *)part, mean, invstd, running_mean, running_var, G,
                       p.tiles_x, p.tiles, nparts, momentum, eps);
    if (int rc = gfn::check_launch("ct_stats_kernel")) return rc;
    int nblk, mt;
    slab_shape(M, &nblk, &mt);
    const dim3 grid((unsigned)p.ntn, (unsigned)nblk, (unsigned)B);
    with_row_tiles(mt, [&](auto MT) {
        hipLaunchKernelGGL((ct_pw_fwd_kernel<decltype(MT)::value>), grid, dim3(256), 0, s, (const float *)u, bn_w, bn_b, (const float *)mean,
                           (const float *)invstd, pw_w, pw_b, y, M, C, N);
    });
    return gfn::check_launch("ct_pw_fwd_kernel");
}

GFN_EXPORT int gfn_conv_block_train_bwd(const float *gy, const float *x, const float *u, const float *mean, const float *invstd,
                                        const float *dw_w, const float *bn_w, const float *bn_b, const float *pw_w, float *gx,
                                        float *d_dw_w, float *d_dw_b, float *d_bn_w, float *d_bn_b, float *d_pw_w, float *d_pw_b, int B,
                                        int C, int M, int G, int need, void *ws, int64_t ws_bytes, gfn_stream_t stream) {
    const char *what = "conv_block_train_bwd";
    if (!gy || !x || !u || !mean || !invstd || !dw_w || !bn_w || !bn_b || !pw_w) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: null pointer", what);
    if (int rc = check_train_sizes(what, B, C, M, G)) return rc;
    if (need < 0 || need > GFN_CBT_NEED_ALL) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: unknown need mask %d", what, need);
    if (((need & GFN_CBT_NEED_X) && !gx) || ((need & GFN_CBT_NEED_DW) && !d_dw_w) || ((need & GFN_CBT_NEED_BN) && (!d_bn_w || !d_bn_b)) ||
        ((need & GFN_CBT_NEED_PW) && (!d_pw_w || !d_pw_b)))
        return gfn::fail(GFN_ERR_INVALID_ARG, "%s: the need mask asks for a gradient whose pointer is null", what);
    if (B == 0 || need == 0) return GFN_OK;
    const TrainPlan p(B, C, M, G);
    if (!ws || misaligned(ws) || ws_bytes < p.bwd_floats * (int64_t)sizeof(float))
        return gfn::fail(GFN_ERR_SCRATCH, "%s: workspace missing, not 16-byte aligned or too small (%lld bytes needed)", what,
                         (long long)(p.bwd_floats * (int64_t)sizeof(float)));
    hipStream_t s = (hipStream_t)stream;
    float *w = static_cast<float *>(ws);
    float *gz = w + p.off_gz, *part_bn = w + p.off_bn, *dgdb = w + p.off_dgdb, *part_dw = w + p.off_dw, *part_pw = w + p.off_pw;
    const int N = G * G;
    if (need & (GFN_CBT_NEED_X | GFN_CBT_NEED_DW | GFN_CBT_NEED_BN)) {
        int nblk, mt;
        slab_shape(C, &nblk, &mt);
        const dim3 grid((unsigned)p.ntn, (unsigned)nblk, (unsigned)B);
        with_row_tiles(mt, [&](auto MT) {
            hipLaunchKernelGGL((ct_pw_bwd_kernel<decltype(MT)::value>), grid, dim3(256), 0, s, gy, u, bn_w, bn_b, mean, invstd, pw_w, gz, part_bn, M,
                               C, N);
        });
        if (int rc = gfn::check_launch("ct_pw_bwd_kernel")) return rc;
        const bool bn = need & GFN_CBT_NEED_BN;
        hipLaunchKernelGGL(ct_bn_bwd_kernel, dim3((unsigned)C), dim3(64), 0, s, (const float *)part_bn, B * p.ntn, C, dgdb, bn ? d_bn_w : nullptr,
                           bn ? d_bn_b : nullptr);
        if (int rc = gfn::check_launch("ct_bn_bwd_kernel")) return rc;
    }
    if (need & GFN_CBT_NEED_PW) {
        const dim3 grid((unsigned)p.wg_tc, (unsigned)p.wg_tm, (unsigned)(B * p.wg_s));
#define GFN_CT(MT, CW)                                                                                                                \
    hipLaunchKernelGGL((ct_pw_wgrad_kernel<MT, CW>), grid, dim3(256), 0, s, gy, u, bn_w, bn_b, mean, invstd, part_pw, M, C, N, p.wg_s, \
                       p.wg_chunk)
        switch (p.wg_cw * 8 + p.wg_mt) {
            case 8 + 1: GFN_CT(1, 1); break;
            case 8 + 2: GFN_CT(2, 1); break;
            case 16 + 1: GFN_CT(1, 2); break;
            case 16 + 2: GFN_CT(2, 2); break;
            case 16 + 4: GFN_CT(4, 2); break;
            case 32 + 1: GFN_CT(1, 4); break;
            case 32 + 2: GFN_CT(2, 4); break;
            case 32 + 4: GFN_CT(4, 4); break;
            default: return gfn::fail(GFN_ERR_INVALID_ARG, "%s: no weight-gradient kernel for this shape", what);
        }
#undef GFN_CT
        if (int rc = gfn::check_launch("ct_pw_wgrad_kernel")) return rc;
        hipLaunchKernelGGL(ct_pw_wgrad_sum_kernel, dim3((unsigned)((M * (C + 1) + 255) / 256)), dim3(256), 0, s, (const float *)part_pw,
                           p.wg_parts, M, C, d_pw_w, d_pw_b);
        if (int rc = gfn::check_launch("ct_pw_wgrad_sum_kernel")) return rc;
    }
    if (need & (GFN_CBT_NEED_X | GFN_CBT_NEED_DW)) {
        const int nparts = B * p.tiles;
        hipLaunchKernelGGL(ct_dw_bwd_kernel, dim3((unsigned)(B * C * p.tiles)), dim3(256), 0, s, (const float *)gz, u, x, dw_w, bn_w, mean, invstd,
                           (const float *)dgdb, gx, part_dw, C, G, p.tiles_x, p.tiles, nparts, 1.0f / ((float)B * (float)N),
                           need & (GFN_CBT_NEED_X | GFN_CBT_NEED_DW));
        if (int rc = gfn::check_launch("ct_dw_bwd_kernel")) return rc;
        if (need & GFN_CBT_NEED_DW) {
            hipLaunchKernelGGL(ct_dw_wgrad_kernel, dim3((unsigned)C), dim3(256), 0, s, (const float *)part_dw, nparts, d_dw_w, d_dw_b);
            if (int rc = gfn::check_launch("ct_dw_wgrad_kernel")) return rc;
        }
    }
    return GFN_OK;
}
