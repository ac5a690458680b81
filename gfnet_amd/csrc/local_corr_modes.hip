// local_corr_modes.hip -- the per-tap local correlation and its feature0 gradient, for every sampling mode the reference accepts
// (gfx950).
//
// utils/local_correlation.py:4-72 passes `sample_mode` and `padding_mode` straight to F.grid_sample (:55-58, :66-68), and
// ConvRefiner forwards its own sample_mode (model/network.py:553-554).  The tiled kernels of local_corr.hip share one set of bilinear
// fractions among the taps of a cell, which holds for bilinear sampling with zeros padding only; every other combination of
// {nearest, bilinear, bicubic} x {zeros, border, reflection} runs here: one thread per (cell, tap), channels unrolled, branch-free
// zero-weight reads (sample_modes.h; tap_dot in local_corr_common.h is the per-tap routine of the tiled kernels too).  The bilinear
// + zeros instantiation is also the general kernel of gfn_local_corr_fwd_dt (any C, radius, tap spacing: grid_based_correlation,
// pooled levels, calls without scratch) and the kernel of gfn_local_corr_bwd_f0.
#include "local_corr_common.h"
#include "sample_modes.h"

namespace {

template <typename FT, int MODE, int PAD>
__global__ __launch_bounds__(256) void local_corr_mode_kernel(LcParams p) {
    const int D = 2 * p.r + 1, K = D * D;
    const long total = (long)p.B * K * p.G * p.G;
    float xlo, xhi, ylo, yhi;
    window_ends(p, xlo, xhi, ylo, yhi);
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
        gfn_sm::Taps<MODE> tp;
        tp.template setup<PAD>(gx, gy, p.W, p.H);
        p.out[(size_t)b * p.out_bs + ((size_t)k * p.G + i) * p.G + j] = tap_dot<FT>(p, b, i, j, tp);
    }
}

// grad_f0[b,c,i,j] = (sum_k grad_out[b,k,i,j] * S_c(k)) / sqrt(C), S_c(k) the sample of f1[b,c] at tap k in this mode (the
// sampling runs under no_grad in the reference, local_correlation.py:54-60).  One thread per (cell, channel group) walks the K
// taps with the forward's own coordinate arithmetic.
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

}  // namespace

int gfn_lc_launch_taps(const LcParams &p, int sample_mode, int padding_mode, hipStream_t s) {
    const long total = (long)p.B * (2 * p.r + 1) * (2 * p.r + 1) * p.G * p.G;
    const dim3 grid((unsigned)((total + 255) / 256 < 16384 ? (total + 255) / 256 : 16384));
    return gfn_sm::with_modes(sample_mode, padding_mode, [&](auto m, auto pad) {
        constexpr int M = decltype(m)::value, P = decltype(pad)::value;
        if (p.f16) hipLaunchKernelGGL((local_corr_mode_kernel<_Float16, M, P>), grid, dim3(256), 0, s, p);
        else hipLaunchKernelGGL((local_corr_mode_kernel<float, M, P>), grid, dim3(256), 0, s, p);
        return gfn::check_launch("local_corr_mode_kernel");
    });
}

// sample_mode / padding_mode: utils/local_correlation.py:4-16 (arguments), :55-58 and :66-68 (the F.grid_sample calls)
GFN_EXPORT int gfn_local_corr_mode_fwd(const float *f0, int64_t f0_bs, const void *f1, const void *f1_second, int f1_dtype,
                                       const float *flow, float *out, int64_t out_bs, int B, int C, int G, int H, int W, int r,
                                       int grid_based, int win_h, int win_w, int sample_mode, int padding_mode, gfn_stream_t stream) {
    if (f1_dtype != GFN_F32 && f1_dtype != GFN_F16) return gfn::fail(GFN_ERR_INVALID_ARG, "local_corr_mode: feature dtype must be GFN_F32 or GFN_F16");
    const int e = check_args("local_corr_mode", !f0 || !f1 || !out, f1_second && (B & 1), B, C, G, H, W, r, win_h, win_w, f0_bs, out_bs,
                             flow != nullptr, sample_mode, padding_mode);
    if (e != GFN_OK) return e;
    if (B == 0) return GFN_OK;
    LcParams p = lc_params(f1, f1_second, f1_dtype == GFN_F16, flow, B, C, G, H, W, r, grid_based, win_h, win_w);
    p.f0 = f0; p.out = out; p.f0_bs = f0_bs; p.out_bs = out_bs;
    return gfn_lc_launch_taps(p, sample_mode, padding_mode, (hipStream_t)stream);
}

// the feature0 gradient of gfn_local_corr_mode_fwd (utils/local_correlation.py:54-60: feature1 and the coordinates under no_grad)
GFN_EXPORT int gfn_local_corr_mode_bwd_f0(const float *grad_out, int64_t grad_out_bs, const float *f1, const float *f1_second,
                                          const float *flow, float *grad_f0, int64_t grad_f0_bs, int B, int C, int G, int H, int W, int r,
                                          int grid_based, int win_h, int win_w, int sample_mode, int padding_mode, gfn_stream_t stream) {
    const int e = check_args("local_corr_mode_bwd", !grad_out || !f1 || !grad_f0, f1_second && (B & 1), B, C, G, H, W, r, win_h, win_w,
                             grad_f0_bs, grad_out_bs, flow != nullptr, sample_mode, padding_mode);
    if (e != GFN_OK) return e;
    if (B == 0) return GFN_OK;
    const LcParams p = lc_params(f1, f1_second, false, flow, B, C, G, H, W, r, grid_based, win_h, win_w);
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
