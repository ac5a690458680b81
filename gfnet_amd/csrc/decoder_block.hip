// A block of the cross-view decoder around its attention core, in the fp16 or the bf16 autocast class (reference
// model/transformer/layers/block.py:327-328 with attention.py:236-238 and :255, mlp.py and layer_scale.py): what comes before
// gfn_cross_attn_fwd in one launch (norm1 and the three bias-free projections) and what comes after it in another (output
// projection, LayerScale, residual, norm2, fc1, GELU, fc2, LayerScale, residual).  Width 64, hidden width 256.
//
// Every product is computed transposed on v_mfma_f32_32x32x8_f16 (bf16 class: v_mfma_f32_32x32x8_bf16), Y^T = W X^T: the A operand
// is a Linear weight as PyTorch stores it, (out, in), read from LDS; a token is a column, so it sits on lane & 31 from the first
// product to the last, and lane half h = lane >> 5 holds its channels 8g + 4h + j (g = 0..7, j = 0..3).  That is the B operand of k-step g, and it is also where the
// accumulator leaves output row 8g + 4h + j (register 4g + j, common.h acc_row): a product's result is the next product's operand
// without moving between lanes, a LayerNorm is per-lane sums and one cross-half shuffle per statistic, and fc1 -> GELU -> fc2 never
// leaves the registers.  Workgroups are persistent: the weights are converted to the class's element into LDS once and the waves
// loop over 32-token tiles with no barrier in the loop.  No scratch, no atomics: identical calls give identical bits, and a token's result
// does not depend on where it sits in a tile or which tile it is in.  The second half of the file is the backward of both launches,
// for training in the same class (the forward kernels are the training forward as they are).
#include <climits>
#include <cmath>
#include <initializer_list>

#include "elem16.h"
#include "reduce.h"

namespace {

using namespace gfn;

constexpr int kC = 64, kHidden = 256;
constexpr int kQkvThreads = 256, kPostThreads = 512;
// LDS pitch of a weight row in halves: 4 more than its length, so the 32 rows an A-operand read touches (8 bytes each at one column)
// start 34 (K = 64) or 130 (K = 256) dwords apart and cover all 64 banks once; a 128-byte pitch would put them all in one bank pair
constexpr int kPitchC = kC + 4, kPitchH = kHidden + 4;

// The element E of a class, _Float16 (the fp16 autocast class) or __bf16 (the bf16 one), is a template parameter of everything below
// that touches an operand or a 16-bit tensor; what it brings with it (elem16.h): V4<E>, four elements as one register pair (an
// operand fragment, an 8-byte access); (E)float, the rounding to nearest even (v_cvt_f16_f32 / v_cvt_pk_bf16_f32; no clamp, NaN
// kept); and mfma8, v_mfma_f32_32x32x8_f16 / v_mfma_f32_32x32x8_bf16.  Both elements are 2 bytes, so LDS pitches, bank patterns and
// the workspace are one set of numbers.  "half" below is a 2-byte element, "fp16(x)" in a formula is (E)x.
template <typename E>
using V4 = typename Elem16<E>::vec4;

// rows * cols fp32 values as stored -> E rows of `pitch` halves in LDS (cols a multiple of 4, src 16-byte aligned)
template <typename E>
__device__ __forceinline__ void stage_weight(E *dst, const float *__restrict__ src, int rows, int cols, int pitch) {
    for (int i = threadIdx.x * 4; i < rows * cols; i += blockDim.x * 4) {
        const float4 f = *reinterpret_cast<const float4 *>(src + i);
        V4<E> o;
        o[0] = (E)f.x, o[1] = (E)f.y, o[2] = (E)f.z, o[3] = (E)f.w;
        *reinterpret_cast<V4<E> *>(dst + (i / cols) * pitch + (i % cols)) = o;
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

// the B operands of the 8 k-steps: the values rounded to E once
template <typename E>
__device__ __forceinline__ void to_operand(const Tok &t, V4<E> b[8]) {
#pragma unroll
    for (int g = 0; g < 8; ++g)
#pragma unroll
        for (int j = 0; j < 4; ++j) b[g][j] = (E)t.v[4 * g + j];
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
template <int KSTEPS, typename E>
__device__ __forceinline__ f32x16 matmul(const E *w, int pitch, int m0, int k0, const V4<E> *b, f32x16 acc, int lane) {
    const E *row = w + (m0 + (lane & 31)) * pitch + k0 + 4 * (lane >> 5);
#pragma unroll
    for (int g = 0; g < KSTEPS; ++g) acc = mfma8(*reinterpret_cast<const V4<E> *>(row + 8 * g), b[g], acc);
    return acc;
}

// output rows m0 .. m0 + 31 of a projection, rounded to E once, into the token's row of a (rows, 64) tensor of E: register
// 4g + j is channel m0 + 8g + 4h + j, so each g is one 8-byte store (the half of head m0 / 8 + g this lane half holds)
template <typename E>
__device__ __forceinline__ void store_proj(E *p, int m0, int h, const f32x16 &acc) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        V4<E> o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = (E)acc[4 * g + j];
        *reinterpret_cast<V4<E> *>(p + m0 + 8 * g + 4 * h) = o;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// before the attention: q = Wq fp16(LayerNorm(row)), k = Wk fp16(row), v = Wv fp16(row); k and v of row r land at row
// (r + rows / 2) mod rows, the other view's batch entry
template <typename E>
__global__ __launch_bounds__(kQkvThreads) void decoder_qkv_kernel(const float *__restrict__ X, const float *__restrict__ norm_w,
                                                                  const float *__restrict__ norm_b, float eps,
                                                                  const float *__restrict__ wq, const float *__restrict__ wk,
                                                                  const float *__restrict__ wv, E *__restrict__ q,
                                                                  E *__restrict__ k, E *__restrict__ v, int64_t rows,
                                                                  int ntiles) {
    __shared__ alignas(16) E w[3][kC * kPitchC];
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
        V4<E> xb[8], nx[8];
        to_operand<E>(x, xb);
        to_operand<E>(layernorm(x, nw, nb, eps, h), nx);
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

template <typename E>
__global__ __launch_bounds__(kPostThreads) void decoder_post_kernel(const float *X, const E *__restrict__ attn,
                                                                    const float *__restrict__ wproj, const float *__restrict__ bproj,
                                                                    const float *__restrict__ gamma1, const float *__restrict__ norm_w,
                                                                    const float *__restrict__ norm_b, float eps,
                                                                    const float *__restrict__ w1, const float *__restrict__ b1,
                                                                    const float *__restrict__ w2, const float *__restrict__ b2,
                                                                    const float *__restrict__ gamma2, float *X_out, int64_t rows,
                                                                    int ntiles) {
    __shared__ alignas(16) E wp[kC * kPitchC];
    __shared__ alignas(16) E wf1[kHidden * kPitchC];
    __shared__ alignas(16) E wf2[kC * kPitchH];
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
        V4<E> ab[8];
#pragma unroll
        for (int g = 0; g < 8; ++g) {
            const V4<E> zero = {};
            ab[g] = ok ? *reinterpret_cast<const V4<E> *>(attn + off + 8 * g + 4 * h) : zero;
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
        V4<E> nx[8];
        to_operand<E>(layernorm(x, nw, nb, eps, h), nx);
        f32x16 y0 = {}, y1 = {};  // fc2's output rows 0..31 and 32..63
#pragma unroll 1
        for (int c0 = 0; c0 < kHidden; c0 += 32) {
            const f32x16 z = {};
            const f32x16 u = matmul<8>(wf1, kPitchC, c0, 0, nx, z, lane);
            V4<E> gb[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float4 b = *reinterpret_cast<const float4 *>(bf1 + c0 + 8 * g + 4 * h);
                gb[g][0] = (E)gelu(u[4 * g] + b.x);
                gb[g][1] = (E)gelu(u[4 * g + 1] + b.y);
                gb[g][2] = (E)gelu(u[4 * g + 2] + b.z);
                gb[g][3] = (E)gelu(u[4 * g + 3] + b.w);
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

// the two forward entries, said once for both classes
template <typename E>
int qkv_fwd(const char *what, const float *x, const float *norm_weight, const float *norm_bias, float eps, const float *wq, const float *wk,
            const float *wv, int B2, int N, int C, void *q, void *k, void *v, gfn_stream_t stream) {
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
    hipLaunchKernelGGL(decoder_qkv_kernel<E>, dim3(grid), dim3(kQkvThreads), 0, (hipStream_t)stream, x, norm_weight, norm_bias, eps, wq, wk, wv,
                       (E *)q, (E *)k, (E *)v, rows, ntiles);
    return gfn::check_launch("decoder_qkv_kernel");
}

template <typename E>
int post_fwd(const char *what, const float *x, const void *attn, const float *wproj, const float *bproj, const float *gamma1,
             const float *norm_weight, const float *norm_bias, float eps, const float *w1, const float *b1, const float *w2, const float *b2,
             const float *gamma2, int64_t rows, int C, int hidden, float *x_out, gfn_stream_t stream) {
    if (int rc = check_args(what, rows, C, hidden, eps,
                            {{x, "x"}, {attn, "attn"}, {wproj, "wproj"}, {bproj, "bproj"}, {gamma1, "gamma1"}, {norm_weight, "norm_weight"},
                             {norm_bias, "norm_bias"}, {w1, "w1"}, {b1, "b1"}, {w2, "w2"}, {b2, "b2"}, {gamma2, "gamma2"}, {x_out, "x_out"}}))
        return rc;
    if (rows == 0) return GFN_OK;
    const int ntiles = (int)((rows + 31) / 32);
    int grid;
    if (int rc = grid_for(ntiles, kPostThreads / 64, 1, &grid, what)) return rc;
    hipLaunchKernelGGL(decoder_post_kernel<E>, dim3(grid), dim3(kPostThreads), 0, (hipStream_t)stream, x, (const E *)attn, wproj, bproj,
                       gamma1, norm_weight, norm_bias, eps, w1, b1, w2, b2, gamma2, x_out, rows, ntiles);
    return gfn::check_launch("decoder_post_kernel");
}

}  // namespace

GFN_EXPORT int gfn_decoder_qkv_fwd(const float *x, const float *norm_weight, const float *norm_bias, float eps, const float *wq,
                                   const float *wk, const float *wv, int B2, int N, int C, void *q, void *k, void *v,
                                   gfn_stream_t stream) {
    return qkv_fwd<_Float16>("gfn_decoder_qkv_fwd", x, norm_weight, norm_bias, eps, wq, wk, wv, B2, N, C, q, k, v, stream);
}
GFN_EXPORT int gfn_decoder_qkv_bf16_fwd(const float *x, const float *norm_weight, const float *norm_bias, float eps, const float *wq,
                                        const float *wk, const float *wv, int B2, int N, int C, void *q, void *k, void *v,
                                        gfn_stream_t stream) {
    return qkv_fwd<__bf16>("gfn_decoder_qkv_bf16_fwd", x, norm_weight, norm_bias, eps, wq, wk, wv, B2, N, C, q, k, v, stream);
}

GFN_EXPORT int gfn_decoder_post_fwd(const float *x, const void *attn, const float *wproj, const float *bproj, const float *gamma1,
                                    const float *norm_weight, const float *norm_bias, float eps, const float *w1, const float *b1,
                                    const float *w2, const float *b2, const float *gamma2, int64_t rows, int C, int hidden, float *x_out,
                                    gfn_stream_t stream) {
    return post_fwd<_Float16>("gfn_decoder_post_fwd", x, attn, wproj, bproj, gamma1, norm_weight, norm_bias, eps, w1, b1, w2, b2, gamma2, rows, C,
                              hidden, x_out, stream);
}
GFN_EXPORT int gfn_decoder_post_bf16_fwd(const float *x, const void *attn, const float *wproj, const float *bproj, const float *gamma1,
                                         const float *norm_weight, const float *norm_bias, float eps, const float *w1, const float *b1,
                                         const float *w2, const float *b2, const float *gamma2, int64_t rows, int C, int hidden,
                                         float *x_out, gfn_stream_t stream) {
    return post_fwd<__bf16>("gfn_decoder_post_bf16_fwd", x, attn, wproj, bproj, gamma1, norm_weight, norm_bias, eps, w1, b1, w2, b2, gamma2, rows,
                            C, hidden, x_out, stream);
}

// =================================================================================================================================
// Training: the backward of the two launches above, differentiating the forward as those kernels compute it with every fp16
// rounding taken as the identity (what autocast's backward does).  Tokens stay on lane & 31; a W^T g product takes the weight's
// other orientation, staged transposed, as its A operand.  A parameter gradient is a sum over tokens of g (x) operand, so there the
// tokens are the K dimension: both factors go through a wave-private [channel][token] fp16 tile in LDS and come back as 8-byte
// operand reads.  No atomics: every workgroup leaves fp32 partial sums in the caller's workspace and a later launch adds them in
// a fixed order, so identical calls give identical bits.  Nothing (rows, 256) leaves the chip.
namespace {

constexpr int kBwdThreads = 256, kBwdWaves = kBwdThreads / 64;  // one wave per SIMD: the accumulators take the register file
constexpr int kMaxGroups = 256;   // the persistent grids never exceed this, whatever the device: the workspace size is a function of rows alone
constexpr int kPitchT = 32 + 4;   // halves per row of a [channel][token] tile: 18 dwords, so 32 rows' 8-byte reads cover all 64 banks once
constexpr int kPartNorm = 4 * kC;                                                   // post, first launch: norm2 weight | bias | s2 = sum g | s1 = sum g1
constexpr int kOffW1 = kC * kHidden, kOffRp = 2 * kC * kHidden, kOffB1 = kOffRp + kC * kC;
constexpr int kPartPost = kOffB1 + kHidden;                                         // post, second launch: R2 | gW1 | Rp | gb1
constexpr int kPartQkv = 3 * kC * kC + 2 * kC;                                      // qkv: gWq | gWk | gWv | norm1 weight | bias

// W (rows, cols) fp32 as stored -> W^T, cols rows of `pitch` halves in LDS
template <typename E>
__device__ __forceinline__ void stage_weight_t(E *dst, const float *__restrict__ src, int rows, int cols, int pitch) {
    for (int i = threadIdx.x; i < rows * cols; i += blockDim.x) dst[(i % cols) * pitch + i / cols] = (E)src[i];
}

// LDS accesses of one wave complete in order; this keeps the compiler from moving a tile's reads across its writes
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// the first half of layernorm(): (row - mean) * rstd and rstd, the same sums in the same order
struct Normed {
    Tok xhat;
    float rstd;
};
__device__ __forceinline__ Normed normalise(const Tok &t, float eps) {
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
    Normed r;
    r.rstd = 1.0f / sqrtf((sq + other_half(sq)) / (float)kC + eps);
#pragma unroll
    for (int i = 0; i < 32; ++i) r.xhat.v[i] = (t.v[i] - mean) * r.rstd;
    return r;
}
// its second half as the B operands: fp16(xhat * weight + bias), layernorm()'s bits
template <typename E>
__device__ __forceinline__ void affine_operand(const Tok &xhat, const float *weight, const float *bias, int h, V4<E> b[8]) {
#pragma unroll
    for (int g = 0; g < 8; ++g) {
        const float4 w = chan4(weight, g, h), c = chan4(bias, g, h);
        b[g][0] = (E)fmaf(xhat.v[4 * g], w.x, c.x);
        b[g][1] = (E)fmaf(xhat.v[4 * g + 1], w.y, c.y);
        b[g][2] = (E)fmaf(xhat.v[4 * g + 2], w.z, c.z);
        b[g][3] = (E)fmaf(xhat.v[4 * g + 3], w.w, c.w);
    }
}
// gradient of the row given gn = dL/d(xhat * weight + bias): rstd * (gh - mean(gh) - xhat * mean(gh * xhat)), gh = gn * weight
__device__ __forceinline__ Tok layernorm_bwd(const Tok &gn, const Normed &n, const float *weight, int h) {
    Tok gh;
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int g = 0; g < 8; ++g) {
        const float4 w = chan4(weight, g, h);
        gh.v[4 * g] = gn.v[4 * g] * w.x, gh.v[4 * g + 1] = gn.v[4 * g + 1] * w.y;
        gh.v[4 * g + 2] = gn.v[4 * g + 2] * w.z, gh.v[4 * g + 3] = gn.v[4 * g + 3] * w.w;
    }
#pragma unroll
    for (int i = 0; i < 32; ++i) {
        s1 += gh.v[i];
        s2 = fmaf(gh.v[i], n.xhat.v[i], s2);
    }
    const float m1 = (s1 + other_half(s1)) / (float)kC, m2 = (s2 + other_half(s2)) / (float)kC;
    Tok r;
#pragma unroll
    for (int i = 0; i < 32; ++i) r.v[i] = n.rstd * (gh.v[i] - m1 - n.xhat.v[i] * m2);
    return r;
}

// two accumulators of a 64-row product (rows 0..31 and 32..63) as the token's row
__device__ __forceinline__ Tok as_tok(const f32x16 &lo, const f32x16 &hi) {
    Tok t;
#pragma unroll
    for (int i = 0; i < 16; ++i) t.v[i] = lo[i], t.v[16 + i] = hi[i];
    return t;
}

template <typename E>
__device__ __forceinline__ void load_operand(const E *p, int h, bool ok, V4<E> b[8]) {
#pragma unroll
    for (int g = 0; g < 8; ++g) {
        const V4<E> zero = {};
        b[g] = ok ? *reinterpret_cast<const V4<E> *>(p + 8 * g + 4 * h) : zero;
    }
}

// x += g1 * (Wproj a + bproj), as decoder_post_kernel forms x1
template <typename E>
__device__ __forceinline__ void add_proj(Tok &x, const V4<E> ab[8], const E *wp, const float *bp, const float *g1, int lane, int h) {
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
}

// the exact erf GELU and its derivative from one erf: GELU(x) = x Phi(x) (gelu()'s bits: a factor 1/2 is exact wherever it is
// applied), GELU'(x) = Phi(x) + x phi(x)
__device__ __forceinline__ float gelu_cdf(float x) { return 0.5f * (1.0f + erff(x * 0.70710678118654752440f)); }
__device__ __forceinline__ float gelu_grad(float x, float cdf) { return cdf + x * (0.39894228040143267794f * expf(-0.5f * x * x)); }

// G groups of 4 operand values (local channel 8g + 4h + j) of the lane's token into column lane & 31 of a [channel][token] tile;
// a lane past the last row writes zeros, so that it adds nothing to a sum over tokens whatever it computed
template <int G, typename E>
__device__ __forceinline__ void put_columns(E *T, int pitch, int token, const V4<E> *b, bool ok, int h) {
    E *col = T + 4 * h * pitch + token;
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
        for (int j = 0; j < 4; ++j) col[(8 * g + j) * pitch] = ok ? b[g][j] : (E)0.f;
}
// rows n0 .. n0 + 31 of a tile as the B operands of the KSTEPS k-steps over its 8 * KSTEPS tokens
template <int KSTEPS, typename E>
__device__ __forceinline__ void tile_operand(const E *T, int pitch, int n0, int lane, V4<E> *b) {
    const E *row = T + (n0 + (lane & 31)) * pitch + 4 * (lane >> 5);
#pragma unroll
    for (int s = 0; s < KSTEPS; ++s) b[s] = *reinterpret_cast<const V4<E> *>(row + 8 * s);
}
// acc[r] is element (m0 + acc_row(r, h), n0 + lane & 31) of a row-major matrix with `ld` columns
__device__ __forceinline__ void store_block(float *M, int ld, int m0, int n0, const f32x16 &acc, int lane) {
#pragma unroll
    for (int r = 0; r < 16; ++r) M[(m0 + acc_row(r, lane >> 5)) * ld + n0 + (lane & 31)] = acc[r];
}

// ---------------------------------------------------------------------------------------------------------------------------------
// post backward, first launch: gX, g_attn and the partial sums of everything 64-wide: norm2's gradients, s2 = sum g and s1 = sum g1.  Per token, g = gX_out:
//   gy = gamma2 g;  per hidden chunk: u = W1 n + b1 (recomputed), gu = (W2^T gy) GELU'(u), gn += W1^T gu;
//   g1 = g + LN2^T(gn);  gX = g1;  g_attn = fp16(Wproj^T (gamma1 g1))
template <typename E>
__global__ __launch_bounds__(kBwdThreads) void decoder_post_bwd_data_kernel(
    const float *__restrict__ X, const E *__restrict__ attn, const float *__restrict__ wproj, const float *__restrict__ bproj,
    const float *__restrict__ gamma1, const float *__restrict__ norm_w, const float *__restrict__ norm_b, float eps,
    const float *__restrict__ w1, const float *__restrict__ b1, const float *__restrict__ w2, const float *__restrict__ gamma2,
    const float *__restrict__ gX_out, float *__restrict__ gX, E *__restrict__ g_attn, float *__restrict__ part, int64_t rows,
    int ntiles) {
    __shared__ alignas(16) E wp[kC * kPitchC], wpt[kC * kPitchC];
    __shared__ alignas(16) E wf1[kHidden * kPitchC], w1t[kC * kPitchH];
    __shared__ alignas(16) E w2t[kHidden * kPitchC];
    __shared__ alignas(16) float bp[kC], g1[kC], nw[kC], nb[kC], g2[kC], bf1[kHidden];
    __shared__ float red[kBwdWaves][kPartNorm];
    stage_weight(wp, wproj, kC, kC, kPitchC);
    stage_weight_t(wpt, wproj, kC, kC, kPitchC);
    stage_weight(wf1, w1, kHidden, kC, kPitchC);
    stage_weight_t(w1t, w1, kHidden, kC, kPitchH);
    stage_weight_t(w2t, w2, kC, kHidden, kPitchC);
    stage_vector(bp, bproj, kC);
    stage_vector(g1, gamma1, kC);
    stage_vector(nw, norm_w, kC);
    stage_vector(nb, norm_b, kC);
    stage_vector(g2, gamma2, kC);
    stage_vector(bf1, b1, kHidden);
    __syncthreads();
    const int lane = threadIdx.x & 63, h = lane >> 5, wave = threadIdx.x >> 6;
    Tok acc_w = {}, acc_b = {}, s2 = {}, s1 = {};  // this lane's tokens' share of norm2's weight and bias gradients, of sum g and of sum g1
    for (int tile = blockIdx.x * kBwdWaves + wave; tile < ntiles; tile += gridDim.x * kBwdWaves) {  // (no barrier in the loop)
        asm volatile("" ::: "memory");  // (the weights are read again for every tile, as in the forward)
        const int64_t row = (int64_t)tile * 32 + (lane & 31);
        const bool ok = row < rows;
        const int64_t off = (ok ? row : 0) * kC;
        Tok x = load_tok(X + off, h, ok);
        const Tok g = load_tok(gX_out + off, h, ok);
        V4<E> ab[8], nx[8], gyb[8];
        load_operand(attn + off, h, ok, ab);
        add_proj(x, ab, wp, bp, g1, lane, h);
        const Normed n = normalise(x, eps);
        affine_operand<E>(n.xhat, nw, nb, h, nx);
#pragma unroll
        for (int G = 0; G < 8; ++G) {
            const float4 s = chan4(g2, G, h);
            gyb[G][0] = (E)(s.x * g.v[4 * G]), gyb[G][1] = (E)(s.y * g.v[4 * G + 1]);
            gyb[G][2] = (E)(s.z * g.v[4 * G + 2]), gyb[G][3] = (E)(s.w * g.v[4 * G + 3]);
        }
        f32x16 gn0 = {}, gn1 = {};  // W1^T gu, rows 0..31 and 32..63
#pragma unroll 1
        for (int c0 = 0; c0 < kHidden; c0 += 32) {
            const f32x16 z = {};
            const f32x16 u = matmul<8>(wf1, kPitchC, c0, 0, nx, z, lane);
            const f32x16 ga = matmul<8>(w2t, kPitchC, c0, 0, gyb, z, lane);
            V4<E> gub[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 b = *reinterpret_cast<const float4 *>(bf1 + c0 + 8 * q + 4 * h);
                const float bj[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float uu = u[4 * q + j] + bj[j];
                    gub[q][j] = (E)(ga[4 * q + j] * gelu_grad(uu, gelu_cdf(uu)));
                }
            }
            gn0 = matmul<4>(w1t, kPitchH, 0, c0, gub, gn0, lane);
            gn1 = matmul<4>(w1t, kPitchH, 32, c0, gub, gn1, lane);
        }
        const Tok gn = as_tok(gn0, gn1);
        if (ok) {
#pragma unroll
            for (int i = 0; i < 32; ++i) {
                acc_w.v[i] = fmaf(gn.v[i], n.xhat.v[i], acc_w.v[i]);
                acc_b.v[i] += gn.v[i];
            }
        }
        Tok gx = layernorm_bwd(gn, n, nw, h);
        V4<E> gpb[8];
#pragma unroll
        for (int G = 0; G < 8; ++G) {
            const float4 s = chan4(g1, G, h);
#pragma unroll
            for (int j = 0; j < 4; ++j) gx.v[4 * G + j] += g.v[4 * G + j];
            gpb[G][0] = (E)(s.x * gx.v[4 * G]), gpb[G][1] = (E)(s.y * gx.v[4 * G + 1]);
            gpb[G][2] = (E)(s.z * gx.v[4 * G + 2]), gpb[G][3] = (E)(s.w * gx.v[4 * G + 3]);
        }
        if (ok) {
            store_tok(gX + off, h, gx);
#pragma unroll
            for (int i = 0; i < 32; ++i) s2.v[i] += g.v[i], s1.v[i] += gx.v[i];
        }
#pragma unroll
        for (int m0 = 0; m0 < kC; m0 += 32) {
            const f32x16 z = {};
            const f32x16 ga = matmul<8>(wpt, kPitchC, m0, 0, gpb, z, lane);
            if (ok) store_proj(g_attn + off, m0, h, ga);
        }
    }
    // this workgroup's partial: tokens of a wave first, then the waves in order
#pragma unroll
    for (int i = 0; i < 32; ++i) {
        const float sw = half_wave_sum(acc_w.v[i]), sb = half_wave_sum(acc_b.v[i]), t2 = half_wave_sum(s2.v[i]), t1 = half_wave_sum(s1.v[i]);
        if ((lane & 31) == 0) {
            const int c = 8 * (i >> 2) + 4 * h + (i & 3);
            red[wave][c] = sw, red[wave][kC + c] = sb, red[wave][2 * kC + c] = t2, red[wave][3 * kC + c] = t1;
        }
    }
    __syncthreads();
    static_assert(kPartNorm <= kBwdThreads, "one thread per sum");
    if (threadIdx.x < kPartNorm) {
        float s = red[0][threadIdx.x];
        for (int w = 1; w < kBwdWaves; ++w) s += red[w][threadIdx.x];
        part[(int64_t)blockIdx.x * kPartNorm + threadIdx.x] = s;
    }
}

// post backward, second launch: the sums over tokens behind the parameter gradients, with x1, n, u recomputed and g1 = gX read back:
//   R2 = g (x) act, gW1 = gu (x) n, gb1 = sum gu, Rp = g1 (x) a
// A workgroup takes one 32-token tile at a time; its wave w owns hidden units 64w .. 64w + 63 (those columns of R2, rows of gW1) and
// one 32 x 32 block of Rp, so each sum has one owner and no wave waits for another.
template <typename E>
__global__ __launch_bounds__(kBwdThreads) void decoder_post_bwd_weight_kernel(
    const float *__restrict__ X, const E *__restrict__ attn, const float *__restrict__ wproj, const float *__restrict__ bproj,
    const float *__restrict__ gamma1, const float *__restrict__ norm_w, const float *__restrict__ norm_b, float eps,
    const float *__restrict__ w1, const float *__restrict__ b1, const float *__restrict__ w2, const float *__restrict__ gamma2,
    const float *__restrict__ gX_out, const float *__restrict__ gX, float *__restrict__ part, int64_t rows, int ntiles) {
    __shared__ alignas(16) E wp[kC * kPitchC];
    __shared__ alignas(16) E wf1[kHidden * kPitchC];
    __shared__ alignas(16) E w2t[kHidden * kPitchC];
    __shared__ alignas(16) float bp[kC], g1[kC], nw[kC], nb[kC], g2[kC], bf1[kHidden];
    __shared__ alignas(16) E tiles[kBwdWaves][(kC + kC + 32 + 32) * kPitchT];
    stage_weight(wp, wproj, kC, kC, kPitchC);
    stage_weight(wf1, w1, kHidden, kC, kPitchC);
    stage_weight_t(w2t, w2, kC, kHidden, kPitchC);
    stage_vector(bp, bproj, kC);
    stage_vector(g1, gamma1, kC);
    stage_vector(nw, norm_w, kC);
    stage_vector(nb, norm_b, kC);
    stage_vector(g2, gamma2, kC);
    stage_vector(bf1, b1, kHidden);
    __syncthreads();
    const int lane = threadIdx.x & 63, h = lane >> 5, wave = threadIdx.x >> 6;
    E *Tg = tiles[wave], *Tn = Tg + kC * kPitchT, *Ta = Tn + kC * kPitchT, *Tu = Ta + 32 * kPitchT;
    f32x16 r2[2][2] = {}, gw1[2][2] = {}, rp = {};  // [hidden chunk of the wave][32-channel block]
    float gb1[2][16] = {};
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {  // (no workgroup barrier in the loop)
        asm volatile("" ::: "memory");
        const int64_t row = (int64_t)tile * 32 + (lane & 31);
        const bool ok = row < rows;
        const int64_t off = (ok ? row : 0) * kC;
        Tok x = load_tok(X + off, h, ok);
        const Tok g = load_tok(gX_out + off, h, ok), gx = load_tok(gX + off, h, ok);
        V4<E> ab[8], nx[8], gyb[8], gb[8], g1b[8];
        load_operand(attn + off, h, ok, ab);
        add_proj(x, ab, wp, bp, g1, lane, h);
        const Normed n = normalise(x, eps);
        affine_operand<E>(n.xhat, nw, nb, h, nx);
#pragma unroll
        for (int G = 0; G < 8; ++G) {
            const float4 s = chan4(g2, G, h);
            gyb[G][0] = (E)(s.x * g.v[4 * G]), gyb[G][1] = (E)(s.y * g.v[4 * G + 1]);
            gyb[G][2] = (E)(s.z * g.v[4 * G + 2]), gyb[G][3] = (E)(s.w * g.v[4 * G + 3]);
        }
        to_operand<E>(g, gb);
        to_operand<E>(gx, g1b);
        wave_sync();  // the previous tile's reads are done
        put_columns<8>(Tg, kPitchT, lane & 31, gb, ok, h);
        put_columns<8>(Tn, kPitchT, lane & 31, nx, ok, h);
#pragma unroll
        for (int cc = 0; cc < 2; ++cc) {
            const int c0 = 64 * wave + 32 * cc;
            const f32x16 z = {};
            const f32x16 u = matmul<8>(wf1, kPitchC, c0, 0, nx, z, lane);
            const f32x16 ga = matmul<8>(w2t, kPitchC, c0, 0, gyb, z, lane);
            V4<E> actb[4], gub[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 b = *reinterpret_cast<const float4 *>(bf1 + c0 + 8 * q + 4 * h);
                const float bj[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float uu = u[4 * q + j] + bj[j];
                    const float cdf = gelu_cdf(uu);
                    const float gu = ok ? ga[4 * q + j] * gelu_grad(uu, cdf) : 0.f;
                    actb[q][j] = (E)(uu * cdf);
                    gub[q][j] = (E)gu;
                    gb1[cc][4 * q + j] += gu;
                }
            }
            wave_sync();  // the previous chunk's reads of Ta and Tu are done
            put_columns<4>(Ta, kPitchT, lane & 31, actb, ok, h);
            put_columns<4>(Tu, kPitchT, lane & 31, gub, ok, h);
            wave_sync();
            V4<E> b[4];
            tile_operand<4>(Ta, kPitchT, 0, lane, b);
            r2[cc][0] = matmul<4>(Tg, kPitchT, 0, 0, b, r2[cc][0], lane);
            r2[cc][1] = matmul<4>(Tg, kPitchT, 32, 0, b, r2[cc][1], lane);
            tile_operand<4>(Tn, kPitchT, 0, lane, b);
            gw1[cc][0] = matmul<4>(Tu, kPitchT, 0, 0, b, gw1[cc][0], lane);
            tile_operand<4>(Tn, kPitchT, 32, lane, b);
            gw1[cc][1] = matmul<4>(Tu, kPitchT, 0, 0, b, gw1[cc][1], lane);
        }
        // Rp's block (wave >> 1, wave & 1): rows from g1, columns from a
        wave_sync();
        if (wave >> 1) put_columns<4>(Ta, kPitchT, lane & 31, g1b + 4, ok, h);
        else put_columns<4>(Ta, kPitchT, lane & 31, g1b, ok, h);
        if (wave & 1) put_columns<4>(Tu, kPitchT, lane & 31, ab + 4, ok, h);
        else put_columns<4>(Tu, kPitchT, lane & 31, ab, ok, h);
        wave_sync();
        V4<E> b[4];
        tile_operand<4>(Tu, kPitchT, 0, lane, b);
        rp = matmul<4>(Ta, kPitchT, 0, 0, b, rp, lane);
    }
    float *P = part + (int64_t)blockIdx.x * kPartPost;
#pragma unroll
    for (int cc = 0; cc < 2; ++cc) {
        const int c0 = 64 * wave + 32 * cc;
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            store_block(P, kHidden, 32 * m, c0, r2[cc][m], lane);       // R2[c][hidden]
            store_block(P + kOffW1, kC, c0, 32 * m, gw1[cc][m], lane);  // gW1[hidden][c]
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const float s = half_wave_sum(gb1[cc][i]);
            if ((lane & 31) == 0) P[kOffB1 + c0 + 8 * (i >> 2) + 4 * h + (i & 3)] = s;
        }
    }
    store_block(P + kOffRp, kC, 32 * (wave >> 1), 32 * (wave & 1), rp, lane);
}

// the second stage of both backwards: sums[i] = sum over the workgroups g of part[g][i], for two sets of partials in one launch (a of
// na values from ga workgroups, then b).  A block takes 32 values; its 8 groups of 32 threads each add every 8th workgroup's partial
// in order, and the 8 sums meet in a fixed tree: the result depends on the number of workgroups, which depends on rows alone.
constexpr int kSumThreads = 256;
__global__ __launch_bounds__(kSumThreads) void decoder_bwd_sum_partials_kernel(const float *__restrict__ a, int ga, int na,
                                                                               const float *__restrict__ b, int gb, int nb,
                                                                               float *__restrict__ sums) {
    __shared__ float red[8][32];
    const int blocks_a = na / 32, e = threadIdx.x & 31, part = threadIdx.x >> 5;
    const bool first = (int)blockIdx.x < blocks_a;
    const float *p = first ? a : b;
    const int groups = first ? ga : gb, n = first ? na : nb, i = (first ? blockIdx.x : blockIdx.x - blocks_a) * 32 + e;
    float s = 0.f;
    for (int g = part; g < groups; g += 8) s += p[(int64_t)g * n + i];
    red[part][e] = s;
    __syncthreads();
    if (part == 0)
        sums[(first ? 0 : na) + i] = ((red[0][e] + red[1][e]) + (red[2][e] + red[3][e])) + ((red[4][e] + red[5][e]) + (red[6][e] + red[7][e]));
}

// post backward, last launch: the LayerScales taken out of the sums (pn and pw are now the totals of the first and second launch):
//   gW2 = gamma2_c R2, gb2 = gamma2_c s2, ggamma2_c = sum_h W2[c][h] R2[c][h] + b2_c s2_c, and the same for gamma1 with Wproj, bproj
// blocks 0..63: channel c of everything 64-wide; 64..127: gW1; 128: gb1
__global__ __launch_bounds__(256) void decoder_post_bwd_finish_kernel(const float *__restrict__ pn, const float *__restrict__ pw,
                                                                      const float *__restrict__ wproj, const float *__restrict__ bproj,
                                                                      const float *__restrict__ gamma1, const float *__restrict__ w2,
                                                                      const float *__restrict__ b2, const float *__restrict__ gamma2,
                                                                      float *__restrict__ g_wproj, float *__restrict__ g_bproj,
                                                                      float *__restrict__ g_gamma1, float *__restrict__ g_norm_w,
                                                                      float *__restrict__ g_norm_b, float *__restrict__ g_w1,
                                                                      float *__restrict__ g_b1, float *__restrict__ g_w2,
                                                                      float *__restrict__ g_b2, float *__restrict__ g_gamma2) {
    __shared__ float red[256];
    const int t = threadIdx.x, b = blockIdx.x;
    auto block_sum = [&](float v) {  // a fixed tree over the 256 threads
        red[t] = v;
        __syncthreads();
        for (int s = 128; s >= 1; s >>= 1) {
            if (t < s) red[t] += red[t + s];
            __syncthreads();
        }
        const float r = red[0];
        __syncthreads();
        return r;
    };
    if (b < kC) {
        const int c = b;
        const float r = pw[c * kHidden + t];
        g_w2[c * kHidden + t] = gamma2[c] * r;
        const float dot2 = block_sum(w2[c * kHidden + t] * r);
        float dp = 0.f;
        if (t < kC) {
            const float q = pw[kOffRp + c * kC + t];
            g_wproj[c * kC + t] = gamma1[c] * q;
            dp = wproj[c * kC + t] * q;
        }
        const float dot1 = block_sum(dp);
        if (t == 0) {
            const float s2 = pn[2 * kC + c], s1 = pn[3 * kC + c];
            g_b2[c] = gamma2[c] * s2;
            g_gamma2[c] = dot2 + b2[c] * s2;
            g_bproj[c] = gamma1[c] * s1;
            g_gamma1[c] = dot1 + bproj[c] * s1;
            g_norm_w[c] = pn[c];
            g_norm_b[c] = pn[kC + c];
        }
    } else if (b < 2 * kC) {
        const int i = (b - kC) * 256 + t;
        g_w1[i] = pw[kOffW1 + i];
    } else {
        g_b1[t] = pw[kOffB1 + t];
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// qkv backward: gX = LN1^T(Wq^T gq) + Wk^T gk' + Wv^T gv', with gk', gv' read where the forward wrote the row's k and v (the other
// view's batch entry), and the partial sums of gWq = gq (x) n, gWk = gk' (x) x, gWv = gv' (x) x and norm1's gradients.  A workgroup
// takes four tiles at a time: wave w computes gX of tile w and leaves its five operands in the shared [channel][128 tokens] images,
// then owns block (w >> 1, w & 1) of each of the three weight gradients over all 128 tokens.
constexpr int kPitchQ = 32 * kBwdWaves + 4;  // 66 dwords a row: 32 rows' 8-byte reads cover all 64 banks once
template <typename E>
__global__ __launch_bounds__(kBwdThreads) void decoder_qkv_bwd_kernel(const float *__restrict__ X, const float *__restrict__ norm_w,
                                                                      const float *__restrict__ norm_b, float eps,
                                                                      const float *__restrict__ wq, const float *__restrict__ wk,
                                                                      const float *__restrict__ wv, const E *__restrict__ gq,
                                                                      const E *__restrict__ gk, const E *__restrict__ gv,
                                                                      float *__restrict__ gX, float *__restrict__ part, int64_t rows,
                                                                      int ntiles) {
    __shared__ alignas(16) E wt[3][kC * kPitchC];
    __shared__ alignas(16) float nw[kC], nb[kC];
    __shared__ alignas(16) E T[5][kC * kPitchQ];  // gq | gk' | gv' | n | x
    __shared__ float red[kBwdWaves][2 * kC];
    stage_weight_t(wt[0], wq, kC, kC, kPitchC);
    stage_weight_t(wt[1], wk, kC, kC, kPitchC);
    stage_weight_t(wt[2], wv, kC, kC, kPitchC);
    stage_vector(nw, norm_w, kC);
    stage_vector(nb, norm_b, kC);
    const int lane = threadIdx.x & 63, h = lane >> 5, wave = threadIdx.x >> 6;
    const int m0 = 32 * (wave >> 1), n0 = 32 * (wave & 1);
    f32x16 gw[3] = {};  // this wave's block of gWq, gWk, gWv
    Tok acc_w = {}, acc_b = {};
    for (int first = blockIdx.x * kBwdWaves; first < ntiles; first += gridDim.x * kBwdWaves) {  // (every wave makes every trip)
        const int64_t row = (int64_t)(first + wave) * 32 + (lane & 31);
        const bool ok = row < rows;
        const int64_t off = (ok ? row : 0) * kC;
        const int64_t other = (ok ? (row + rows / 2 < rows ? row + rows / 2 : row - rows / 2) : 0) * kC;
        const Tok x = load_tok(X + off, h, ok);
        V4<E> xb[8], nx[8], gb[3][8];
        load_operand(gq + off, h, ok, gb[0]);
        load_operand(gk + other, h, ok, gb[1]);
        load_operand(gv + other, h, ok, gb[2]);
        to_operand<E>(x, xb);
        const Normed n = normalise(x, eps);
        affine_operand<E>(n.xhat, nw, nb, h, nx);
        __syncthreads();  // the weights are staged; the previous trip's reads of T are done
#pragma unroll
        for (int p = 0; p < 3; ++p) put_columns<8>(T[p], kPitchQ, 32 * wave + (lane & 31), gb[p], ok, h);
        put_columns<8>(T[3], kPitchQ, 32 * wave + (lane & 31), nx, ok, h);
        put_columns<8>(T[4], kPitchQ, 32 * wave + (lane & 31), xb, ok, h);
        const f32x16 z = {};
        const Tok gn = as_tok(matmul<8>(wt[0], kPitchC, 0, 0, gb[0], z, lane), matmul<8>(wt[0], kPitchC, 32, 0, gb[0], z, lane));
        if (ok) {
#pragma unroll
            for (int i = 0; i < 32; ++i) {
                acc_w.v[i] = fmaf(gn.v[i], n.xhat.v[i], acc_w.v[i]);
                acc_b.v[i] += gn.v[i];
            }
        }
        Tok gx = layernorm_bwd(gn, n, nw, h);
        const Tok gkv = as_tok(matmul<8>(wt[2], kPitchC, 0, 0, gb[2], matmul<8>(wt[1], kPitchC, 0, 0, gb[1], z, lane), lane),
                               matmul<8>(wt[2], kPitchC, 32, 0, gb[2], matmul<8>(wt[1], kPitchC, 32, 0, gb[1], z, lane), lane));
#pragma unroll
        for (int i = 0; i < 32; ++i) gx.v[i] += gkv.v[i];
        if (ok) store_tok(gX + off, h, gx);
        __syncthreads();  // all four tiles' operands are in T
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            V4<E> b[4 * kBwdWaves];
            tile_operand<4 * kBwdWaves>(T[p == 0 ? 3 : 4], kPitchQ, n0, lane, b);
            gw[p] = matmul<4 * kBwdWaves>(T[p], kPitchQ, m0, 0, b, gw[p], lane);
        }
    }
    float *P = part + (int64_t)blockIdx.x * kPartQkv;
#pragma unroll
    for (int p = 0; p < 3; ++p) store_block(P + p * kC * kC, kC, m0, n0, gw[p], lane);
#pragma unroll
    for (int i = 0; i < 32; ++i) {
        const float sw = half_wave_sum(acc_w.v[i]), sb = half_wave_sum(acc_b.v[i]);
        if ((lane & 31) == 0) {
            const int c = 8 * (i >> 2) + 4 * h + (i & 3);
            red[wave][c] = sw, red[wave][kC + c] = sb;
        }
    }
    __syncthreads();
    if (threadIdx.x < 2 * kC) {
        float s = red[0][threadIdx.x];
        for (int w = 1; w < kBwdWaves; ++w) s += red[w][threadIdx.x];  // wave order
        P[3 * kC * kC + threadIdx.x] = s;
    }
}

// qkv backward, last launch: the totals to where they belong
__global__ __launch_bounds__(256) void decoder_qkv_bwd_finish_kernel(const float *__restrict__ sums, float *__restrict__ g_wq,
                                                                     float *__restrict__ g_wk, float *__restrict__ g_wv,
                                                                     float *__restrict__ g_norm_w, float *__restrict__ g_norm_b) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= kPartQkv) return;
    const float s = sums[i];
    const int m = i / (kC * kC);
    if (m == 0) g_wq[i] = s;
    else if (m == 1) g_wk[i - kC * kC] = s;
    else if (m == 2) g_wv[i - 2 * kC * kC] = s;
    else if (i < 3 * kC * kC + kC) g_norm_w[i - 3 * kC * kC] = s;
    else g_norm_b[i - 3 * kC * kC - kC] = s;
}

// workgroups of a persistent backward grid: one per `per_group` tiles, kMaxGroups at most
int bwd_groups(int64_t rows, int per_group) {
    const int64_t groups = ((rows + 31) / 32 + per_group - 1) / per_group;
    return (int)(groups < kMaxGroups ? groups : kMaxGroups);
}
constexpr int kDataTiles = kBwdWaves, kWeightTiles = 4;  // tiles per workgroup before a grid stops growing
static_assert(kPartNorm % 32 == 0 && kPartPost % 32 == 0 && kPartQkv % 32 == 0, "decoder_bwd_sum_partials_kernel takes 32 values a block");
// the workgroups' partials, then their totals
int64_t bwd_ws_floats(int64_t rows) {
    const int64_t post = (int64_t)(bwd_groups(rows, kDataTiles) + 1) * kPartNorm + (int64_t)(bwd_groups(rows, kWeightTiles) + 1) * kPartPost;
    const int64_t qkv = (int64_t)(bwd_groups(rows, kDataTiles) + 1) * kPartQkv;
    return post > qkv ? post : qkv;
}
int check_ws(const char *what, int64_t rows, int64_t ws_bytes) {
    const int64_t need = bwd_ws_floats(rows) * (int64_t)sizeof(float);
    if (ws_bytes < need)
        return gfn::fail(GFN_ERR_INVALID_ARG, "%s: ws_bytes = %lld is too small, gfn_decoder_bwd_ws_bytes(%lld) = %lld", what, (long long)ws_bytes,
                         (long long)rows, (long long)need);
    return GFN_OK;
}

// the two backward entries, said once for both classes
template <typename E>
int qkv_bwd(const char *what, const float *x, const float *norm_weight, const float *norm_bias, float eps, const float *wq, const float *wk,
            const float *wv, const void *gq, const void *gk, const void *gv, int B2, int N, int C, float *gx, float *g_wq, float *g_wk,
            float *g_wv, float *g_norm_weight, float *g_norm_bias, void *ws, int64_t ws_bytes, gfn_stream_t stream) {
    if (B2 < 0 || N < 1) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: bad size (batch %d, N %d)", what, B2, N);
    if (B2 & 1) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: the batch holds both views and must be even, got %d", what, B2);
    const int64_t rows = (int64_t)B2 * N;
    if (int rc = check_args(what, rows, C, kHidden, eps,
                            {{x, "x"}, {norm_weight, "norm_weight"}, {norm_bias, "norm_bias"}, {wq, "wq"}, {wk, "wk"}, {wv, "wv"},
                             {gq, "gq"}, {gk, "gk"}, {gv, "gv"}, {gx, "gx"}, {g_wq, "g_wq"}, {g_wk, "g_wk"}, {g_wv, "g_wv"},
                             {g_norm_weight, "g_norm_weight"}, {g_norm_bias, "g_norm_bias"}, {ws, "ws"}}))
        return rc;
    if (rows == 0) return GFN_OK;
    if (int rc = check_ws(what, rows, ws_bytes)) return rc;
    const int ntiles = (int)((rows + 31) / 32), groups = bwd_groups(rows, kDataTiles);
    hipLaunchKernelGGL(decoder_qkv_bwd_kernel<E>, dim3(groups), dim3(kBwdThreads), 0, (hipStream_t)stream, x, norm_weight, norm_bias, eps, wq, wk,
                       wv, (const E *)gq, (const E *)gk, (const E *)gv, gx, (float *)ws, rows, ntiles);
    if (int rc = gfn::check_launch("decoder_qkv_bwd_kernel")) return rc;
    float *sums = (float *)ws + (int64_t)groups * kPartQkv;
    hipLaunchKernelGGL(decoder_bwd_sum_partials_kernel, dim3(kPartQkv / 32), dim3(kSumThreads), 0, (hipStream_t)stream, (const float *)ws, groups,
                       kPartQkv, (const float *)nullptr, 0, 0, sums);
    if (int rc = gfn::check_launch("decoder_bwd_sum_partials_kernel")) return rc;
    hipLaunchKernelGGL(decoder_qkv_bwd_finish_kernel, dim3((kPartQkv + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const float *)sums, g_wq,
                       g_wk, g_wv, g_norm_weight, g_norm_bias);
    return gfn::check_launch("decoder_qkv_bwd_finish_kernel");
}

template <typename E>
int post_bwd(const char *what, const float *x, const void *attn, const float *wproj, const float *bproj, const float *gamma1,
             const float *norm_weight, const float *norm_bias, float eps, const float *w1, const float *b1, const float *w2, const float *b2,
             const float *gamma2, const float *gx_out, int64_t rows, int C, int hidden, float *gx, void *g_attn, float *g_wproj,
             float *g_bproj, float *g_gamma1, float *g_norm_weight, float *g_norm_bias, float *g_w1, float *g_b1, float *g_w2, float *g_b2,
             float *g_gamma2, void *ws, int64_t ws_bytes, gfn_stream_t stream) {
    if (int rc = check_args(what, rows, C, hidden, eps,
                            {{x, "x"}, {attn, "attn"}, {wproj, "wproj"}, {bproj, "bproj"}, {gamma1, "gamma1"}, {norm_weight, "norm_weight"},
                             {norm_bias, "norm_bias"}, {w1, "w1"}, {b1, "b1"}, {w2, "w2"}, {b2, "b2"}, {gamma2, "gamma2"}, {gx_out, "gx_out"},
                             {gx, "gx"}, {g_attn, "g_attn"}, {g_wproj, "g_wproj"}, {g_bproj, "g_bproj"}, {g_gamma1, "g_gamma1"},
                             {g_norm_weight, "g_norm_weight"}, {g_norm_bias, "g_norm_bias"}, {g_w1, "g_w1"}, {g_b1, "g_b1"}, {g_w2, "g_w2"},
                             {g_b2, "g_b2"}, {g_gamma2, "g_gamma2"}, {ws, "ws"}}))
        return rc;
    if (rows == 0) return GFN_OK;
    if (int rc = check_ws(what, rows, ws_bytes)) return rc;
    const int ntiles = (int)((rows + 31) / 32), groups_n = bwd_groups(rows, kDataTiles), groups_w = bwd_groups(rows, kWeightTiles);
    float *pn = (float *)ws, *pw = pn + (int64_t)groups_n * kPartNorm, *sums = pw + (int64_t)groups_w * kPartPost;
    hipLaunchKernelGGL(decoder_post_bwd_data_kernel<E>, dim3(groups_n), dim3(kBwdThreads), 0, (hipStream_t)stream, x, (const E *)attn, wproj,
                       bproj, gamma1, norm_weight, norm_bias, eps, w1, b1, w2, gamma2, gx_out, gx, (E *)g_attn, pn, rows, ntiles);
    if (int rc = gfn::check_launch("decoder_post_bwd_data_kernel")) return rc;
    hipLaunchKernelGGL(decoder_post_bwd_weight_kernel<E>, dim3(groups_w), dim3(kBwdThreads), 0, (hipStream_t)stream, x, (const E *)attn,
                       wproj, bproj, gamma1, norm_weight, norm_bias, eps, w1, b1, w2, gamma2, gx_out, (const float *)gx, pw, rows, ntiles);
    if (int rc = gfn::check_launch("decoder_post_bwd_weight_kernel")) return rc;
    hipLaunchKernelGGL(decoder_bwd_sum_partials_kernel, dim3((kPartNorm + kPartPost) / 32), dim3(kSumThreads), 0, (hipStream_t)stream,
                       (const float *)pn, groups_n, kPartNorm, (const float *)pw, groups_w, kPartPost, sums);
    if (int rc = gfn::check_launch("decoder_bwd_sum_partials_kernel")) return rc;
    hipLaunchKernelGGL(decoder_post_bwd_finish_kernel, dim3(2 * kC + 1), dim3(256), 0, (hipStream_t)stream, (const float *)sums,
                       (const float *)(sums + kPartNorm), wproj, bproj, gamma1, w2, b2, gamma2, g_wproj, g_bproj, g_gamma1, g_norm_weight,
                       g_norm_bias, g_w1, g_b1, g_w2, g_b2, g_gamma2);
    return gfn::check_launch("decoder_post_bwd_finish_kernel");
}

}  // namespace

// (one size serves both classes: the partial sums are fp32 whatever the element)
GFN_EXPORT int64_t gfn_decoder_bwd_ws_bytes(int64_t rows) {
    if (rows <= 0 || rows > (int64_t)INT_MAX - 31) return 0;
    return bwd_ws_floats(rows) * (int64_t)sizeof(float);
}

#define GFN_DECODER_QKV_BWD(name, E)                                                                                                        \
    GFN_EXPORT int name(const float *x, const float *norm_weight, const float *norm_bias, float eps, const float *wq, const float *wk,      \
                        const float *wv, const void *gq, const void *gk, const void *gv, int B2, int N, int C, float *gx, float *g_wq,      \
                        float *g_wk, float *g_wv, float *g_norm_weight, float *g_norm_bias, void *ws, int64_t ws_bytes,                     \
                        gfn_stream_t stream) {                                                                                              \
        return qkv_bwd<E>(#name, x, norm_weight, norm_bias, eps, wq, wk, wv, gq, gk, gv, B2, N, C, gx, g_wq, g_wk, g_wv, g_norm_weight,     \
                          g_norm_bias, ws, ws_bytes, stream);                                                                               \
    }
GFN_DECODER_QKV_BWD(gfn_decoder_qkv_bwd, _Float16)
GFN_DECODER_QKV_BWD(gfn_decoder_qkv_bf16_bwd, __bf16)

#define GFN_DECODER_POST_BWD(name, E)                                                                                                       \
    GFN_EXPORT int name(const float *x, const void *attn, const float *wproj, const float *bproj, const float *gamma1,                      \
                        const float *norm_weight, const float *norm_bias, float eps, const float *w1, const float *b1, const float *w2,     \
                        const float *b2, const float *gamma2, const float *gx_out, int64_t rows, int C, int hidden, float *gx,              \
                        void *g_attn, float *g_wproj, float *g_bproj, float *g_gamma1, float *g_norm_weight, float *g_norm_bias,            \
                        float *g_w1, float *g_b1, float *g_w2, float *g_b2, float *g_gamma2, void *ws, int64_t ws_bytes,                    \
                        gfn_stream_t stream) {                                                                                              \
        return post_bwd<E>(#name, x, attn, wproj, bproj, gamma1, norm_weight, norm_bias, eps, w1, b1, w2, b2, gamma2, gx_out, rows, C,      \
                           hidden, gx, g_attn, g_wproj, g_bproj, g_gamma1, g_norm_weight, g_norm_bias, g_w1, g_b1, g_w2, g_b2, g_gamma2,    \
                           ws, ws_bytes, stream);                                                                                           \
    }
GFN_DECODER_POST_BWD(gfn_decoder_post_bwd, _Float16)
GFN_DECODER_POST_BWD(gfn_decoder_post_bf16_bwd, __bf16)
