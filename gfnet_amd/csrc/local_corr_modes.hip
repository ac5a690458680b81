// local_corr_modes.hip -- local correlation for every sampling mode the reference accepts (gfx950).
//
// utils/local_correlation.py:4-72 passes `sample_mode` and `padding_mode` straight to F.grid_sample (:55-58, :66-68), and
// ConvRefiner forwards its own sample_mode (model/network.py:553-554).  The tiled kernels of local_corr.hip share one set of bilinear
// fractions among the taps of a cell, which holds for bilinear sampling with zeros padding only; every other combination of
// {nearest, bilinear, bicubic} x {zeros, border, reflection} runs here, in the form of local_corr_general_kernel: one thread per
// (cell, tap), channels unrolled, branch-free zero-weight reads (sample_modes.h).  Bilinear with zeros padding through this kernel
// is bit-identical to the general kernel of local_corr.hip.
#include "local_corr_common.h"
#include "sample_modes.h"

namespace {

// the window's end points in normalised units, as tap_general forms them
__device__ __forceinline__ void window_ends(const LcParams &p, float &xlo, float &xhi, float &ylo, float &yhi) {
    if (p.grid_based) {
        ylo = (float)(-2.0 * p.r / p.G); yhi = (float)(2.0 * p.r / p.G);
        xlo = ylo; xhi = yhi;
    } else {
        ylo = (float)(-2.0 * p.r / p.win_h); yhi = (float)(2.0 * p.r / p.win_h);
        xlo = (float)(-2.0 * p.r / p.win_w); xhi = (float)(2.0 * p.r / p.win_w);
    }
}

template <typename FT, int MODE, int PAD>
__global__ __launch_bounds__(256) void local_corr_mode_kernel(LcParams p) {
    using Taps = gfn_sm::Taps<MODE>;
    constexpr int UC = gfn_sm::group_channels<MODE>();
    const int D = 2 * p.r + 1, K = D * D;
    const long total = (long)p.B * K * p.G * p.G;
    float xlo, xhi, ylo, yhi;
    window_ends(p, xlo, xhi, ylo, yhi);
    const size_t plane = (size_t)p.H * p.W, cs = (size_t)p.G * p.G;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int j = (int)(idx % p.G);
        long t = idx / p.G;
        const int i = (int)(t % p.G);
        t /= p.G;
        const int k = (int)(t % K);
        const int b = (int)(t / K);
        float nx, ny;
        cell_coords(p, b, i, j, nx, ny);
        const float gx = nx + gfn::linspace_at(xlo, xhi, D, k % D);
        const float gy = ny + gfn::linspace_at(ylo, yhi, D, k / D);
        Taps tp;
        tp.template setup<PAD>(gx, gy, p.W, p.H);
        const float *f0p = p.f0 + (size_t)b * p.f0_bs + (size_t)i * p.G + j;
        const FT *f1p = f1_of<FT>(p, b);
        float acc = 0.f;
        for (int c0 = 0; c0 < p.C; c0 += UC) {
            float v[UC][Taps::N], q[UC];
#pragma unroll
            for (int u = 0; u < UC; ++u) {
                const int c = min(c0 + u, p.C - 1);
                tp.load(f1p + c * plane, v[u]);
                q[u] = f0p[c * cs];
            }
#pragma unroll
            for (int u = 0; u < UC; ++u)
                if (c0 + u < p.C) acc += (q[u] / p.sqrt_c) * tp.value(v[u]);
        }
        p.out[(size_t)b * p.out_bs + ((size_t)k * p.G + i) * p.G + j] = acc;
    }
}

// grad_f0[b,c,i,j] = (sum_k grad_out[b,k,i,j] * S_c(k)) / sqrt(C), S_c(k) the sample of f1[b,c] at tap k in this mode (the
// sampling runs under no_grad in the reference, local_correlation.py:54-60).  One thread per (cell, channel group), as
// local_corr_bwd_f0_kernel.
template <int MODE, int PAD>
__global__ __launch_bounds__(256) void local_corr_mode_bwd_f0_kernel(LcParams p, const float *__restrict__ gout, long gout_bs,
                                                                     float *__restrict__ gf0, long gf0_bs) {
    using Taps = gfn_sm::Taps<MODE>;
    constexpr int UC = gfn_sm::group_channels<MODE>();
    const int D = 2 * p.r + 1, K = D * D;
    const int groups = (p.C + UC - 1) / UC;
    const long total = (long)p.B * groups * p.G * p.G;
    float xlo, xhi, ylo, yhi;
    window_ends(p, xlo, xhi, ylo, yhi);
    const size_t plane = (size_t)p.H * p.W, cs = (size_t)p.G * p.G;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int j = (int)(idx % p.G);
        long t = idx / p.G;
        const int i = (int)(t % p.G);
        t /= p.G;
        const int cg = (int)(t % groups);
        const int b = (int)(t / groups);
        const int c0 = cg * UC;
        float nx, ny;
        cell_coords(p, b, i, j, nx, ny);
        const float *f1p = f1_of<float>(p, b);
        const float *g = gout + (size_t)b * gout_bs + (size_t)i * p.G + j;
        float acc[UC];
#pragma unroll
        for (int u = 0; u < UC; ++u) acc[u] = 0.f;
        for (int k = 0; k < K; ++k) {
            const float gx = nx + gfn::linspace_at(xlo, xhi, D, k % D);
            const float gy = ny + gfn::linspace_at(ylo, yhi, D, k / D);
            Taps tp;
            tp.template setup<PAD>(gx, gy, p.W, p.H);
            const float gk = g[(size_t)k * cs];
            float v[UC][Taps::N];
#pragma unroll
            for (int u = 0; u < UC; ++u) tp.load(f1p + min(c0 + u, p.C - 1) * plane, v[u]);
#pragma unroll
            for (int u = 0; u < UC; ++u) acc[u] = fmaf(gk, tp.value(v[u]), acc[u]);
        }
        float *dst = gf0 + (size_t)b * gf0_bs + (size_t)i * p.G + j;
#pragma unroll
        for (int u = 0; u < UC; ++u)
            if (c0 + u < p.C) dst[(size_t)(c0 + u) * cs] = acc[u] / p.sqrt_c;
    }
}

// the LcParams fields the per-tap kernels read
LcParams mode_params(const void *f1, const void *f1_second, bool f16, const float *flow, int B, int C, int G, int H, int W, int r,
                     int grid_based, int win_h, int win_w) {
    LcParams p{};
    p.f1 = f1; p.f1_second = f1_second; p.f16 = f16 ? 1 : 0; p.Bh = f1_second ? B / 2 : B;
    p.flow = flow;
    p.B = B; p.C = C; p.G = G; p.H = H; p.W = W;
    p.sqrt_c = (float)sqrt((double)C);
    p.inv_sqrt_c = (float)(1.0 / sqrt((double)C));
    p.r = r; p.win_h = win_h; p.win_w = win_w; p.grid_based = grid_based;
    return p;
}

// the argument checks of gfn_local_corr_fwd_dt / gfn_local_corr_bwd_f0, plus the two mode codes
int check_args(const char *what, bool null_ptr, bool odd_symmetric, int B, int C, int G, int H, int W, int r, int win_h, int win_w,
               int64_t in_bs, int64_t out_bs, bool has_flow, int sample_mode, int padding_mode) {
    if (!gfn_sm::valid_modes(sample_mode, padding_mode))
        return gfn::fail(GFN_ERR_INVALID_ARG, "%s: sample_mode %d / padding_mode %d is not a GFN_SAMPLE_* / GFN_PAD_* code", what,
                         sample_mode, padding_mode);
    if (null_ptr) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: null tensor pointer", what);
    if (odd_symmetric) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: symmetric batch must be even", what);
    if (B < 0 || C <= 0 || G <= 0 || H <= 0 || W <= 0 || r < 0 || win_h <= 0 || win_w <= 0)
        return gfn::fail(GFN_ERR_INVALID_ARG, "%s: bad size B=%d C=%d G=%d H=%d W=%d r=%d", what, B, C, G, H, W, r);
    const long K = (long)(2 * r + 1) * (2 * r + 1);
    if (in_bs < (long)C * G * G || out_bs < K * G * G)
        return gfn::fail(GFN_ERR_INVALID_ARG, "%s: batch stride smaller than one batch element", what);
    if (!has_flow && !(G == win_h && G == win_w))
        return gfn::fail(GFN_ERR_INVALID_ARG, "%s: flow=NULL needs num_grid == h == w (got G=%d h=%d w=%d)", what, G, win_h, win_w);
    if ((long)B * K * G * G >= (1L << 40) || (long)C * H * W >= (1L << 31)) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: tensor too large", what);
    return GFN_OK;
}

}  // namespace

// sample_mode / padding_mode: utils/local_correlation.py:4-16 (arguments), :55-58 and :66-68 (the F.grid_sample calls)
GFN_EXPORT int gfn_local_corr_mode_fwd(const float *f0, int64_t f0_bs, const void *f1, const void *f1_second, int f1_dtype,
                                       const float *flow, float *out, int64_t out_bs, int B, int C, int G, int H, int W, int r,
                                       int grid_based, int win_h, int win_w, int sample_mode, int padding_mode, gfn_stream_t stream) {
    if (f1_dtype != GFN_F32 && f1_dtype != GFN_F16) return gfn::fail(GFN_ERR_INVALID_ARG, "local_corr_mode: feature dtype must be GFN_F32 or GFN_F16");
    const int e = check_args("local_corr_mode", !f0 || !f1 || !out, f1_second && (B & 1), B, C, G, H, W, r, win_h, win_w, f0_bs, out_bs,
                             flow != nullptr, sample_mode, padding_mode);
    if (e != GFN_OK) return e;
    if (B == 0) return GFN_OK;
    LcParams p = mode_params(f1, f1_second, f1_dtype == GFN_F16, flow, B, C, G, H, W, r, grid_based, win_h, win_w);
    p.f0 = f0; p.out = out; p.f0_bs = f0_bs; p.out_bs = out_bs;
    const long total = (long)B * (2 * r + 1) * (2 * r + 1) * G * G;
    const dim3 grid((unsigned)((total + 255) / 256 < 16384 ? (total + 255) / 256 : 16384));
    const hipStream_t s = (hipStream_t)stream;
    return gfn_sm::with_modes(sample_mode, padding_mode, [&](auto m, auto pad) {
        constexpr int M = decltype(m)::value, P = decltype(pad)::value;
        if (p.f16) hipLaunchKernelGGL((local_corr_mode_kernel<_Float16, M, P>), grid, dim3(256), 0, s, p);
        else hipLaunchKernelGGL((local_corr_mode_kernel<float, M, P>), grid, dim3(256), 0, s, p);
        return gfn::check_launch("local_corr_mode_kernel");
    });
}

// the feature0 gradient of gfn_local_corr_mode_fwd (utils/local_correlation.py:54-60: feature1 and the coordinates under no_grad)
GFN_EXPORT int gfn_local_corr_mode_bwd_f0(const float *grad_out, int64_t grad_out_bs, const float *f1, const float *f1_second,
                                          const float *flow, float *grad_f0, int64_t grad_f0_bs, int B, int C, int G, int H, int W, int r,
                                          int grid_based, int win_h, int win_w, int sample_mode, int padding_mode, gfn_stream_t stream) {
    const int e = check_args("local_corr_mode_bwd", !grad_out || !f1 || !grad_f0, f1_second && (B & 1), B, C, G, H, W, r, win_h, win_w,
                             grad_f0_bs, grad_out_bs, flow != nullptr, sample_mode, padding_mode);
    if (e != GFN_OK) return e;
    if (B == 0) return GFN_OK;
    const LcParams p = mode_params(f1, f1_second, false, flow, B, C, G, H, W, r, grid_based, win_h, win_w);
    const hipStream_t s = (hipStream_t)stream;
    return gfn_sm::with_modes(sample_mode, padding_mode, [&](auto m, auto pad) {
        constexpr int M = decltype(m)::value, P = decltype(pad)::value;
        constexpr int UC = gfn_sm::group_channels<M>();
        const long total = (long)B * ((C + UC - 1) / UC) * G * G;
        const dim3 grid((unsigned)((total + 255) / 256 < 65536 ? (total + 255) / 256 : 65536));
        hipLaunchKernelGGL((local_corr_mode_bwd_f0_kernel<M, P>), grid, dim3(256), 0, s, p, grad_out, (long)grad_out_bs, grad_f0,
                           (long)grad_f0_bs);
        return gfn::check_launch("local_corr_mode_bwd_f0_kernel");
    });
}
