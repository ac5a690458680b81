// A block of the cross-view decoder around its attention core, inference in the fp16 autocast class (reference
// model/transformer/layers/block.py:327-328 with attention.py:236-238 and :255, mlp.py and layer_scale.py): what comes before
// gfn_cross_attn_fwd in one launch (norm1 and the three bias-free projections) and what comes after it in another (output
// projection, LayerScale, residual, norm2, fc1, GELU, fc2, LayerScale, residual).  Width 64, hidden width 256.
//
// Every product is computed transposed on v_mfma_f32_32x32x8_f16, Y^T = W X^T: the A operand is a Linear weight as PyTorch stores
// it, (out, in), read from LDS; a token is a column, so it sits on lane & 31 from the first product to the last, and lane half
// h = lane >> 5 holds its channels 8g + 4h + j (g = 0..7, j = 0..3).  That is the B operand of k-step g, and it is also where the
// accumulator leaves output row 8g + 4h + j (register 4g + j, common.h acc_row): a product's result is the next product's operand
// without moving between lanes, a LayerNorm is per-lane sums and one cross-half shuffle per statistic, and fc1 -> GELU -> fc2 never
// leaves the registers.  Workgroups are persistent: the weights are converted to fp16 into LDS once and the waves loop over
// 32-token tiles with no barrier in the loop.  No scratch, no atomics: identical calls give identical bits, and a token's result
// does not depend on where it sits in a tile or which tile it is in.
#include <climits>
#include <initializer_list>

#include "attn_common.h"

namespace {

using gfn::acc_row;
using gfn::f32x16;
using namespace gfn::attn;

constexpr int kC = 64, kHidden = 256;
constexpr int kQkvThreads = 256, kPostThreads = 512;
// LDS pitch of a weight row in halves: 4 more than its length, so the 32 rows an A-operand read touches (8 bytes each at one column)
// start 34 (K = 64) or 130 (K = 256) dwords apart and cover all 64 banks once; a 128-byte pitch would put them all in one bank pair
constexpr int kPitchC = kC + 4, kPitchH = kHidden + 4;

// rows * cols fp32 values as stored -> fp16 rows of `pitch` halves in LDS (cols a multiple of 4, src 16-byte aligned)
__device__ __forceinline__ void stage_weight(_Float16 *dst, const float *__restrict__ src, int rows, int cols, int pitch) {
    for (int i = threadIdx.x * 4; i < rows * cols; i += blockDim.x * 4) {
        const float4 f = *reinterpret_cast<const float4 *>(src + i);
        h4 o;
        o[0] = (_Float16)f.x, o[1] = (_Float16)f.y, o[2] = (_Float16)f.z, o[3] = (_Float16)f.w;
        *reinterpret_cast<h4 *>(dst + (i / cols) * pitch + (i % cols)) = o;
    }
}
__device__ __forceinline__ void stage_vector(float *dst, const float *__restrict__ src, int n) {
    for (int i = threadIdx.x; i < n; i += blockDim.x) dst[i] = src[i];
}

// the 32 values of a 64-wide row that lane half h holds: v[4g + j] is channel 8g + 4h + j
struct Tok {
    float v[32];
};

__device__ __forceinline__ Tok load_tok(const float *p, int h, bool ok) {
    Tok t;
#pragma unroll
    for (int g = 0; g < 8; ++g) {
        const float4 f = ok ? *reinterpret_cast<const float4 *>(p + 8 * g + 4 * h) : make_float4(0.f, 0.f, 0.f, 0.f);
        t.v[4 * g] = f.x, t.v[4 * g + 1] = f.y, t.v[4 * g + 2] = f.z, t.v[4 * g + 3] = f.w;
    }
    return t;
}
__device__ __forceinline__ void store_tok(float *p, int h, const Tok &t) {
#pragma unroll
    for (int g = 0; g < 8; ++g)
        *reinterpret_cast<float4 *>(p + 8 * g + 4 * h) = make_float4(t.v[4 * g], t.v[4 * g + 1], t.v[4 * g + 2], t.v[4 * g + 3]);
}

// a per-channel vector in LDS at the lane half's channels (every lane of a half reads one address: a broadcast)
__device__ __forceinline__ float4 chan4(const float *vec, int g, int h) { return *reinterpret_cast<const float4 *>(vec + 8 * g + 4 * h); }

// the B operands of the 8 k-steps: the values rounded to fp16 once
__device__ __forceinline__ void to_operand(const Tok &t, h4 b[8]) {
#pragma unroll
    for (int g = 0; g < 8; ++g)
#pragma unroll
        for (int j = 0; j < 4; ++j) b[g][j] = (_Float16)t.v[4 * g + j];
}

// LayerNorm of a token's row in fp32, two-pass over the values as held (mean, then squared distances from it), biased variance;
// both lane halves form the same two sums (a + b and b + a), so they agree on mean and rstd to the bit
__device__ __forceinline__ Tok layernorm(const Tok &t, const float *weight, const float *bias, float eps, int h) {
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < 32; ++i) sum += t.v[i];
    const float mean = (sum + other_half(sum)) / (float)kC;
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < 32; ++i) {
        const float d = t.v[i] - mean;
        sq = fmaf(d, d, sq);
    }
    const float rstd = 1.0f / sqrtf((sq + other_half(sq)) / (float)kC + eps);
    Tok r;
#pragma unroll
    for (int g = 0; g < 8; ++g) {
        const float4 w = chan4(weight, g, h), b = chan4(bias, g, h);
        r.v[4 * g] = fmaf((t.v[4 * g] - mean) * rstd, w.x, b.x);
        r.v[4 * g + 1] = fmaf((t.v[4 * g + 1] - mean) * rstd, w.y, b.y);
        r.v[4 * g + 2] = fmaf((t.v[4 * g + 2] - mean) * rstd, w.z, b.z);
        r.v[4 * g + 3] = fmaf((t.v[4 * g + 3] - mean) * rstd, w.w, b.w);
    }
    return r;
}

// acc += W[m0 .. m0 + 31][k0 .. k0 + 8 * KSTEPS - 1] * b: rows m0 + acc_row(r, h) of the product for the lane's token in acc[r]
template <int KSTEPS>
__device__ __forceinline__ f32x16 matmul(const _Float16 *w, int pitch, int m0, int k0, const h4 *b, f32x16 acc, int lane) {
    const _Float16 *row = w + (m0 + (lane & 31)) * pitch + k0 + 4 * (lane >> 5);
#pragma unroll
    for (int g = 0; g < KSTEPS; ++g) acc = __builtin_amdgcn_mfma_f32_32x32x8f16(*reinterpret_cast<const h4 *>(row + 8 * g), b[g], acc, 0, 0, 0);
    return acc;
}

// output rows m0 .. m0 + 31 of a projection, rounded to fp16 once, into the token's row of a (rows, 64) fp16 tensor: register
// 4g + j is channel m0 + 8g + 4h + j, so each g is one 8-byte store (the half of head m0 / 8 + g this lane half holds)
__device__ __forceinline__ void store_proj(_Float16 *p, int m0, int h, const f32x16 &acc) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        h4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = (_Float16)acc[4 * g + j];
        *reinterpret_cast<h4 *>(p + m0 + 8 * g + 4 * h) = o;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// before the attention: q = Wq fp16(LayerNorm(row)), k = Wk fp16(row), v = Wv fp16(row); k and v of row r land at row
// (r + rows / 2) mod rows, the other view's batch entry
__global__ __launch_bounds__(kQkvThreads) void decoder_qkv_kernel(const float *__restrict__ X, const float *__restrict__ norm_w,
                                                                  const float *__restrict__ norm_b, float eps,
                                                                  const float *__restrict__ wq, const float *__restrict__ wk,
                                                                  const float *__restrict__ wv, _Float16 *__restrict__ q,
                                                                  _Float16 *__restrict__ k, _Float16 *__restrict__ v, int64_t rows,
                                                                  int ntiles) {
    __shared__ alignas(16) _Float16 w[3][kC * kPitchC];
    __shared__ alignas(16) float nw[kC], nb[kC];
    stage_weight(w[0], wq, kC, kC, kPitchC);
    stage_weight(w[1], wk, kC, kC, kPitchC);
    stage_weight(w[2], wv, kC, kC, kPitchC);
    stage_vector(nw, norm_w, kC);
    stage_vector(nb, norm_b, kC);
    __syncthreads();
    const int lane = threadIdx.x & 63, h = lane >> 5, waves = kQkvThreads / 64;
    for (int tile = blockIdx.x * waves + (threadIdx.x >> 6); tile < ntiles; tile += gridDim.x * waves) {  // (no barrier in the loop)
        // the weights in LDS do not change between tiles, and a compiler that knows it reads them all into registers ahead of the
        // loop (245 VGPRs, one wave per SIMD; the second kernel spilled): every tile reads them again
        asm volatile("" ::: "memory");
        const int64_t row = (int64_t)tile * 32 + (lane & 31);
        const bool ok = row < rows;
        const Tok x = load_tok(X + (ok ? row : 0) * kC, h, ok);
        h4 xb[8], nx[8];
        to_operand(x, xb);
        to_operand(layernorm(x, nw, nb, eps, h), nx);
        const int64_t other = row + rows / 2 < rows ? row + rows / 2 : row - rows / 2;
#pragma unroll
        for (int m0 = 0; m0 < kC; m0 += 32) {
            const f32x16 z = {};
            const f32x16 aq = matmul<8>(w[0], kPitchC, m0, 0, nx, z, lane);
            if (ok) store_proj(q + row * kC, m0, h, aq);
            const f32x16 ak = matmul<8>(w[1], kPitchC, m0, 0, xb, z, lane);
            if (ok) store_proj(k + other * kC, m0, h, ak);
            const f32x16 av = matmul<8>(w[2], kPitchC, m0, 0, xb, z, lane);
            if (ok) store_proj(v + other * kC, m0, h, av);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// after the attention: x1 = x + g1 (Wproj a + bproj), x2 = x1 + g2 (W2 fp16(GELU(W1 fp16(LayerNorm(x1)) + b1)) + b2).  The proj, fc1
// and fc2 results stay fp32 in the accumulators; the hidden width goes by in chunks of 32, each chunk of fc1 feeding four k-steps of
// fc2.  x_out may be x: a lane reads its token's values before the loop body's products and writes the same addresses after them.
__device__ __forceinline__ float gelu(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)); }

__global__ __launch_bounds__(kPostThreads) void decoder_post_kernel(const float *X, const _Float16 *__restrict__ attn,
                                                                    const float *__restrict__ wproj, const float *__restrict__ bproj,
                                                                    const float *__restrict__ gamma1, const float *__restrict__ norm_w,
                                                                    const float *__restrict__ norm_b, float eps,
                                                                    const float *__restrict__ w1, const float *__restrict__ b1,
                                                                    const float *__restrict__ w2, const float *__restrict__ b2,
                                                                    const float *__restrict__ gamma2, float *X_out, int64_t rows,
                                                                    int ntiles) {
    __shared__ alignas(16) _Float16 wp[kC * kPitchC];
    __shared__ alignas(16) _Float16 wf1[kHidden * kPitchC];
    __shared__ alignas(16) _Float16 wf2[kC * kPitchH];
    __shared__ alignas(16) float bp[kC], g1[kC], nw[kC], nb[kC], bf2[kC], g2[kC], bf1[kHidden];
    stage_weight(wp, wproj, kC, kC, kPitchC);
    stage_weight(wf1, w1, kHidden, kC, kPitchC);
    stage_weight(wf2, w2, kC, kHidden, kPitchH);
    stage_vector(bp, bproj, kC);
    stage_vector(g1, gamma1, kC);
    stage_vector(nw, norm_w, kC);
    stage_vector(nb, norm_b, kC);
    stage_vector(bf2, b2, kC);
    stage_vector(g2, gamma2, kC);
    stage_vector(bf1, b1, kHidden);
    __syncthreads();
    const int lane = threadIdx.x & 63, h = lane >> 5, waves = kPostThreads / 64;
    for (int tile = blockIdx.x * waves + (threadIdx.x >> 6); tile < ntiles; tile += gridDim.x * waves) {  // (no barrier in the loop)
        // the weights in LDS do not change between tiles, and a compiler that knows it reads them all into registers ahead of the
        // loop (245 VGPRs, one wave per SIMD; the second kernel spilled): every tile reads them again
        asm volatile("" ::: "memory");
        const int64_t row = (int64_t)tile * 32 + (lane & 31);
        const bool ok = row < rows;
        const int64_t off = (ok ? row : 0) * kC;
        Tok x = load_tok(X + off, h, ok);
        h4 ab[8];
#pragma unroll
        for (int g = 0; g < 8; ++g) {
            const h4 zero = {};
            ab[g] = ok ? *reinterpret_cast<const h4 *>(attn + off + 8 * g + 4 * h) : zero;
        }
        // x1 = x + g1 * (Wproj a + bproj)
#pragma unroll
        for (int m0 = 0; m0 < kC; m0 += 32) {
            const f32x16 z = {};
            const f32x16 p = matmul<8>(wp, kPitchC, m0, 0, ab, z, lane);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int G = m0 / 8 + g;
                const float4 b = chan4(bp, G, h), s = chan4(g1, G, h);
                x.v[4 * G] = fmaf(s.x, p[4 * g] + b.x, x.v[4 * G]);
                x.v[4 * G + 1] = fmaf(s.y, p[4 * g + 1] + b.y, x.v[4 * G + 1]);
                x.v[4 * G + 2] = fmaf(s.z, p[4 * g + 2] + b.z, x.v[4 * G + 2]);
                x.v[4 * G + 3] = fmaf(s.w, p[4 * g + 3] + b.w, x.v[4 * G + 3]);
            }
        }
        h4 nx[8];
        to_operand(layernorm(x, nw, nb, eps, h), nx);
        f32x16 y0 = {}, y1 = {};  // fc2's output rows 0..31 and 32..63
#pragma unroll 1
        for (int c0 = 0; c0 < kHidden; c0 += 32) {
            const f32x16 z = {};
            const f32x16 u = matmul<8>(wf1, kPitchC, c0, 0, nx, z, lane);
            h4 gb[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float4 b = *reinterpret_cast<const float4 *>(bf1 + c0 + 8 * g + 4 * h);
                gb[g][0] = (_Float16)gelu(u[4 * g] + b.x);
                gb[g][1] = (_Float16)gelu(u[4 * g + 1] + b.y);
                gb[g][2] = (_Float16)gelu(u[4 * g + 2] + b.z);
                gb[g][3] = (_Float16)gelu(u[4 * g + 3] + b.w);
            }
            y0 = matmul<4>(wf2, kPitchH, 0, c0, gb, y0, lane);
            y1 = matmul<4>(wf2, kPitchH, 32, c0, gb, y1, lane);
        }
        // x2 = x1 + g2 * (y + b2)
#pragma unroll
        for (int G = 0; G < 8; ++G) {
            const float4 b = chan4(bf2, G, h), s = chan4(g2, G, h);
            const int r = 4 * (G & 3);
            x.v[4 * G] = fmaf(s.x, (G < 4 ? y0[r] : y1[r]) + b.x, x.v[4 * G]);
            x.v[4 * G + 1] = fmaf(s.y, (G < 4 ? y0[r + 1] : y1[r + 1]) + b.y, x.v[4 * G + 1]);
            x.v[4 * G + 2] = fmaf(s.z, (G < 4 ? y0[r + 2] : y1[r + 2]) + b.z, x.v[4 * G + 2]);
            x.v[4 * G + 3] = fmaf(s.w, (G < 4 ? y0[r + 3] : y1[r + 3]) + b.w, x.v[4 * G + 3]);
        }
        if (ok) store_tok(X_out + off, h, x);
    }
}

// the persistent grid: one workgroup per `per_group` tiles, at most `per_cu` workgroups per compute unit of the current device
int grid_for(int ntiles, int per_group, int per_cu, int *grid, const char *what) {
    static int cus[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return gfn::fail(GFN_ERR_LAUNCH, "%s: no current device", what);
    int n = dev >= 0 && dev < 64 ? cus[dev] : 0;
    if (n == 0) {
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1)
            return gfn::fail(GFN_ERR_LAUNCH, "%s: cannot read the device's compute unit count", what);
        if (dev >= 0 && dev < 64) cus[dev] = n;
    }
    const int groups = (ntiles + per_group - 1) / per_group;
    *grid = groups < n * per_cu ? groups : n * per_cu;
    return GFN_OK;
}

struct NamedPtr {
    const void *p;
    const char *name;
};

// widths and the row count first, then pointers (not looked at where rows = 0: there is nothing to do)
int check_args(const char *what, int64_t rows, int C, int hidden, float eps, std::initializer_list<NamedPtr> ptrs) {
    if (C != kC) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: C must be %d (8 heads of 8; a token's row is held across one lane pair), got %d", what, kC, C);
    if (hidden != kHidden) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: the hidden width must be %d, got %d", what, kHidden, hidden);
    if (rows < 0 || rows > (int64_t)INT_MAX - 31)
        return gfn::fail(GFN_ERR_INVALID_ARG, "%s: the number of rows must be 0 .. 2^31 - 32, got %lld", what, (long long)rows);
    if (!(eps >= 0.f) || !std::isfinite(eps)) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: eps must be finite and not negative", what);
    if (rows == 0) return GFN_OK;
    for (const NamedPtr &a : ptrs) {
        if (!a.p) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: null pointer (%s)", what, a.name);
        if ((uintptr_t)a.p & 15) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: %s must be 16-byte aligned (rows are read as vectors)", what, a.name);
    }
    return GFN_OK;
}

}  // namespace

GFN_EXPORT int gfn_decoder_qkv_fwd(const float *x, const float *norm_weight, const float *norm_bias, float eps, const float *wq,
                                   const float *wk, const float *wv, int B2, int N, int C, void *q, void *k, void *v,
                                   gfn_stream_t stream) {
    const char *what = "gfn_decoder_qkv_fwd";
    if (B2 < 0 || N < 1) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: bad size (batch %d, N %d)", what, B2, N);
    if (B2 & 1) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: the batch holds both views and must be even, got %d", what, B2);
    const int64_t rows = (int64_t)B2 * N;
    if (int rc = check_args(what, rows, C, kHidden, eps,
                            {{x, "x"}, {norm_weight, "norm_weight"}, {norm_bias, "norm_bias"}, {wq, "wq"}, {wk, "wk"}, {wv, "wv"}, {q, "q"}, {k, "k"}, {v, "v"}}))
        return rc;
    if (rows == 0) return GFN_OK;
    const int ntiles = (int)((rows + 31) / 32);
    int grid;
    if (int rc = grid_for(ntiles, kQkvThreads / 64, 2, &grid, what)) return rc;
    hipLaunchKernelGGL(decoder_qkv_kernel, dim3(grid), dim3(kQkvThreads), 0, (hipStream_t)stream, x, norm_weight, norm_bias, eps, wq, wk, wv,
                       (_Float16 *)q, (_Float16 *)k, (_Float16 *)v, rows, ntiles);
    return gfn::check_launch("decoder_qkv_kernel");
}

GFN_EXPORT int gfn_decoder_post_fwd(const float *x, const void *attn, const float *wproj, const float *bproj, const float *gamma1,
                                    const float *norm_weight, const float *norm_bias, float eps, const float *w1, const float *b1,
                                    const float *w2, const float *b2, const float *gamma2, int64_t rows, int C, int hidden, float *x_out,
                                    gfn_stream_t stream) {
    const char *what = "gfn_decoder_post_fwd";
    if (int rc = check_args(what, rows, C, hidden, eps,
                            {{x, "x"}, {attn, "attn"}, {wproj, "wproj"}, {bproj, "bproj"}, {gamma1, "gamma1"}, {norm_weight, "norm_weight"},
                             {norm_bias, "norm_bias"}, {w1, "w1"}, {b1, "b1"}, {w2, "w2"}, {b2, "b2"}, {gamma2, "gamma2"}, {x_out, "x_out"}}))
        return rc;
    if (rows == 0) return GFN_OK;
    const int ntiles = (int)((rows + 31) / 32);
    int grid;
    if (int rc = grid_for(ntiles, kPostThreads / 64, 1, &grid, what)) return rc;
    hipLaunchKernelGGL(decoder_post_kernel, dim3(grid), dim3(kPostThreads), 0, (hipStream_t)stream, x, (const _Float16 *)attn, wproj, bproj,
                       gamma1, norm_weight, norm_bias, eps, w1, b1, w2, b2, gamma2, x_out, rows, ntiles);
    return gfn::check_launch("decoder_post_kernel");
}
