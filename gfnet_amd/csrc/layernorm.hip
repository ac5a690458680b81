// The seam between two halves of a ViT block in one pass (reference model/transformer/layers/block.py:83-106 with
// layer_scale.py: x + ls(f(norm(x))), then the next norm): x_out = x + gamma * y, h_out = LayerNorm(x_out) * weight + bias.
// One wave per row; the row stays in registers between the residual update, the two statistics passes and the normalisation, so
// the stream is read once and written once.
#include <hip/hip_fp16.h>

#include <climits>
#include <cmath>

#include "elem16.h"
#include "reduce.h"

namespace {

using gfn::Elem16;
using gfn::wave_sum;

constexpr int kThreads = 256, kRowsPerBlock = kThreads / 64;
constexpr int kMaxC = 8192;

// 8 consecutive values of a row, widened
struct V8 {
    float e[8];
};

template <typename T>
__device__ __forceinline__ V8 load8(const T *p) {
    const auto v = *reinterpret_cast<const typename Elem16<T>::vec8 *>(p);
    V8 r;
#pragma unroll
    for (int j = 0; j < 8; ++j) r.e[j] = (float)v[j];
    return r;
}
__device__ __forceinline__ V8 load8(const float *p) {
    const float4 a = reinterpret_cast<const float4 *>(p)[0], b = reinterpret_cast<const float4 *>(p)[1];
    return {{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w}};
}
template <typename T>
__device__ __forceinline__ void store8(T *p, const V8 &r) {
    typename Elem16<T>::vec8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (T)r.e[j];  // to nearest even
    *reinterpret_cast<typename Elem16<T>::vec8 *>(p) = v;
}
__device__ __forceinline__ void store8(float *p, const V8 &r) {
    reinterpret_cast<float4 *>(p)[0] = make_float4(r.e[0], r.e[1], r.e[2], r.e[3]);
    reinterpret_cast<float4 *>(p)[1] = make_float4(r.e[4], r.e[5], r.e[6], r.e[7]);
}

// what the stream holds after a store: the value rounded to its storage type
template <typename T>
__device__ __forceinline__ float as_stored(float v, const T *) { return Elem16<T>::round(v); }
__device__ __forceinline__ float as_stored(float v, const float *) { return v; }

// VPL: 8-value vectors per lane; lane i holds vectors i, i + 64, ... of the row (those below C / 8)
template <typename T, int VPL>
__global__ __launch_bounds__(kThreads) void ls_add_layernorm_kernel(const T *x, const T *__restrict__ y, const T *__restrict__ gamma,
                                                                    const T *__restrict__ weight, const T *__restrict__ bias, float eps,
                                                                    int64_t rows, int C, T *x_out, T *__restrict__ h_out) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
    if (row >= rows) return;  // (whole waves; no barrier follows)
    const int nvec = C >> 3;
    const int64_t off = row * C;
    V8 v[VPL];
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
        const int vec = lane + 64 * i;
        if (vec < nvec) {
            v[i] = load8(x + off + 8 * vec);
            if (y) {
                const V8 yy = load8(y + off + 8 * vec), g = load8(gamma + 8 * vec);
#pragma unroll
                for (int j = 0; j < 8; ++j) v[i].e[j] = as_stored(fmaf(g.e[j], yy.e[j], v[i].e[j]), (const T *)nullptr);
                store8(x_out + off + 8 * vec, v[i]);  // (exact: the values are already representable)
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) sum += v[i].e[j];
        }
    }
    if (!h_out) return;
    // two passes over the registers: the mean, then the squared distances from it (never E[x^2] - mean^2)
    const float mean = wave_sum(sum) / (float)C;
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
        if (lane + 64 * i < nvec) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float d = v[i].e[j] - mean;
                sq = fmaf(d, d, sq);
            }
        }
    }
    const float rstd = 1.0f / sqrtf(wave_sum(sq) / (float)C + eps);
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
        const int vec = lane + 64 * i;
        if (vec < nvec) {
            const V8 w = load8(weight + 8 * vec), bb = load8(bias + 8 * vec);
            V8 r;
#pragma unroll
            for (int j = 0; j < 8; ++j) r.e[j] = fmaf((v[i].e[j] - mean) * rstd, w.e[j], bb.e[j]);
            store8(h_out + off + 8 * vec, r);
        }
    }
}

template <typename T, int VPL>
void launch(const void *x, const void *y, const void *gamma, const void *weight, const void *bias, float eps, int64_t rows, int C,
            void *x_out, void *h_out, hipStream_t s) {
    const unsigned grid = (unsigned)((rows + kRowsPerBlock - 1) / kRowsPerBlock);
    hipLaunchKernelGGL((ls_add_layernorm_kernel<T, VPL>), dim3(grid), dim3(kThreads), 0, s, (const T *)x, (const T *)y, (const T *)gamma,
                       (const T *)weight, (const T *)bias, eps, rows, C, (T *)x_out, (T *)h_out);
}

template <typename T>
void launch_for(int C, const void *x, const void *y, const void *gamma, const void *weight, const void *bias, float eps, int64_t rows,
                void *x_out, void *h_out, hipStream_t s) {
    const int vpl = (C / 8 + 63) / 64;  // 1..16
    if (vpl <= 1)
        launch<T, 1>(x, y, gamma, weight, bias, eps, rows, C, x_out, h_out, s);
    else if (vpl <= 2)
        launch<T, 2>(x, y, gamma, weight, bias, eps, rows, C, x_out, h_out, s);
    else if (vpl <= 4)
        launch<T, 4>(x, y, gamma, weight, bias, eps, rows, C, x_out, h_out, s);
    else if (vpl <= 8)
        launch<T, 8>(x, y, gamma, weight, bias, eps, rows, C, x_out, h_out, s);
    else
        launch<T, 16>(x, y, gamma, weight, bias, eps, rows, C, x_out, h_out, s);
}

// the checks and the launch of both entry points; dtype is one of the three storage types (the callers have seen to that)
int seam_fwd(const char *what, const void *x, const void *y, const void *gamma, const void *weight, const void *bias, float eps, int dtype,
             int64_t rows, int C, void *x_out, void *h_out, gfn_stream_t stream) {
    if (C < 8 || C > kMaxC || (C & 7))
        return gfn::fail(GFN_ERR_INVALID_ARG, "%s: C must be a multiple of 8 up to %d (a row is held in registers as 8-value vectors), got %d", what, kMaxC, C);
    if (rows < 0 || (rows + kRowsPerBlock - 1) / kRowsPerBlock > INT_MAX) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: bad rows %lld", what, (long long)rows);
    if (!(eps >= 0.f) || !std::isfinite(eps)) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: eps must be finite and not negative", what);
    if (!y && !h_out) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: nothing to compute (y and h_out are both NULL)", what);
    if (rows == 0) return GFN_OK;
    const struct {
        const void *p;
        const char *name;
        bool needed;
    } ptrs[] = {{x, "x", true},           {y, "y", false},         {gamma, "gamma", y != nullptr}, {x_out, "x_out", y != nullptr},
                {weight, "weight", h_out != nullptr}, {bias, "bias", h_out != nullptr}, {h_out, "h_out", false}};
    for (const auto &a : ptrs) {
        if (a.needed && !a.p) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: null pointer (%s)", what, a.name);
        if ((uintptr_t)a.p & 15) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: %s must be 16-byte aligned (rows are read as vectors)", what, a.name);
    }
    if (h_out && (h_out == x || h_out == x_out)) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: h_out must not alias x or x_out", what);
    hipStream_t s = (hipStream_t)stream;
    if (dtype == GFN_F16)
        launch_for<_Float16>(C, x, y, gamma, weight, bias, eps, rows, x_out, h_out, s);
    else if (dtype == GFN_BF16)
        launch_for<__bf16>(C, x, y, gamma, weight, bias, eps, rows, x_out, h_out, s);
    else
        launch_for<float>(C, x, y, gamma, weight, bias, eps, rows, x_out, h_out, s);
    return gfn::check_launch("ls_add_layernorm_kernel");
}

}  // namespace

GFN_EXPORT int gfn_ls_add_layernorm_fwd(const void *x, const void *y, const void *gamma, const void *weight, const void *bias, float eps,
                                        int dtype, int64_t rows, int C, void *x_out, void *h_out, gfn_stream_t stream) {
    const char *what = "gfn_ls_add_layernorm_fwd";
    if (dtype != GFN_F32 && dtype != GFN_F16)
        return gfn::fail(GFN_ERR_INVALID_ARG, "%s: dtype must be GFN_F32 or GFN_F16, got %d (bf16 tensors: gfn_ls_add_layernorm_bf16_fwd)", what, dtype);
    return seam_fwd(what, x, y, gamma, weight, bias, eps, dtype, rows, C, x_out, h_out, stream);
}

GFN_EXPORT int gfn_ls_add_layernorm_bf16_fwd(const void *x, const void *y, const void *gamma, const void *weight, const void *bias, float eps,
                                             int64_t rows, int C, void *x_out, void *h_out, gfn_stream_t stream) {
    return seam_fwd("gfn_ls_add_layernorm_bf16_fwd", x, y, gamma, weight, bias, eps, GFN_BF16, rows, C, x_out, h_out, stream);
}
