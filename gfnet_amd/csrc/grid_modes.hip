// grid_modes.hip -- grid_sample and the refiner-input assembly for every sampling mode the reference accepts (gfx950).
//
//   gfn_grid_sample_mode_fwd       F.grid_sample(mode = nearest | bilinear | bicubic, padding_mode = zeros | border | reflection,
//                                  align_corners=False)
//   gfn_refiner_input_mode_fwd_dt  ConvRefiner.forward's x_hat (model/network.py:537), grid_feature (:547) and displacement embedding
//                                  (:548-549) with ConvRefiner(sample_mode=...) (:464, 502); the reference's refiner always pads with zeros
//
// One thread per output pixel / grid cell: the sampling set-up (sample_modes.h) once, then the channels in groups with all loads
// of a group in flight.  gfn_grid_sample_fwd (bilinear, zeros, fp32) is gfn_grid_sample_mode_fwd; the bilinear refiner input of the
// product path keeps its own pair-gather kernel (grid_ops.hip, refiner_input.h), built on the same set-up.
#include "refiner_input.h"
#include "sample_modes.h"

namespace {

template <typename FT, int MODE, int PAD>
__global__ __launch_bounds__(256) void grid_sample_mode_kernel(const FT *__restrict__ in, const float *__restrict__ grid,
                                                               float *__restrict__ out, long out_bs, int B, int C, int H, int W, int Ho,
                                                               int Wo) {
    using Taps = gfn_sm::Taps<MODE>;
    constexpr int UC = gfn_sm::group_channels<MODE>();
    const long npix = (long)Ho * Wo, total = (long)B * npix;
    const size_t plane = (size_t)H * W;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int b = (int)(idx / npix);
        const long pix = idx - (long)b * npix;
        const float *g = grid + (size_t)idx * 2;
        Taps tp;
        tp.template setup<PAD>(g[0], g[1], W, H);
        const FT *src = in + (size_t)b * C * plane;
        float *dst = out + (size_t)b * out_bs + pix;
        for (int c0 = 0; c0 < C; c0 += UC) {
            float v[UC][Taps::N];
#pragma unroll
            for (int u = 0; u < UC; ++u) tp.load(src + min(c0 + u, C - 1) * plane, v[u]);
#pragma unroll
            for (int u = 0; u < UC; ++u)
                if (c0 + u < C) dst[(size_t)(c0 + u) * npix] = tp.value(v[u]);
        }
    }
}

// the body of refiner_input_cell (refiner_input.h) with a Taps<MODE> set-up per gather; grid (cell blocks, B), symmetric directions
// back to back as there (ri_direction)
template <typename FT, int MODE, bool KEEP>
__global__ __launch_bounds__(256) void refiner_input_mode_kernel(gfn_ri::RiArgs args) {
    using Taps = gfn_sm::Taps<MODE>;
    constexpr int UC = gfn_sm::group_channels<MODE>();
    const int b = gfn_ri::ri_direction(args.B, args.Bh, blockIdx.y);
    const int Bh = args.Bh, C = args.C, Hs = args.Hs, Ws = args.Ws, G = args.G;
    const unsigned GG = (unsigned)(G * G), cell = blockIdx.x * 256u + threadIdx.x;
    if (cell >= GG) return;
    const size_t plane = (size_t)Hs * Ws;
    const FT *__restrict__ fa = static_cast<const FT *>(args.fa);
    const FT *__restrict__ fb = static_cast<const FT *>(args.fb);
    const int i = (int)(cell / (unsigned)G), j = (int)(cell - (unsigned)i * (unsigned)G);
    const FT *q = (b < Bh ? fa + (size_t)b * C * plane : fb + (size_t)(b - Bh) * C * plane);   // query map
    const FT *sm = (b < Bh ? fb + (size_t)b * C * plane : fa + (size_t)(b - Bh) * C * plane);  // support map
    const float lo = (float)(-1 + 1.0 / G), hi = (float)(1 - 1.0 / G);
    const float cx = gfn::linspace_at(lo, hi, G, j), cy = gfn::linspace_at(lo, hi, G, i);  // network.py:539-546
    const float *fl = args.flow + (size_t)b * 2 * GG;
    const float fx = fl[cell], fy = fl[GG + cell];
    float *__restrict__ o = args.d + (size_t)b * args.d_bs;
    Taps sa, sb;
    if (!KEEP) sa.template setup<GFN_PAD_ZEROS>(cx, cy, Ws, Hs);  // grid_feature = grid_sample(x, im_A_coords)   network.py:547
    sb.template setup<GFN_PAD_ZEROS>(fx, fy, Ws, Hs);             // x_hat = grid_sample(y, flow)                 network.py:537
    for (int c0 = 0; c0 < C; c0 += UC) {
        float va[UC][Taps::N], vb[UC][Taps::N];
#pragma unroll
        for (int u = 0; u < UC; ++u) {
            const size_t off = (size_t)min(c0 + u, C - 1) * plane;
            if (!KEEP) sa.load(q + off, va[u]);
            sb.load(sm + off, vb[u]);
        }
#pragma unroll
        for (int u = 0; u < UC; ++u) {
            if (c0 + u < C) {
                if (!KEEP) o[(size_t)(c0 + u) * GG + cell] = sa.value(va[u]);
                o[(size_t)(C + c0 + u) * GG + cell] = sb.value(vb[u]);
            }
        }
    }
    // disp_emb(40/32 * scale_factor * (flow - im_A_coords))                                  network.py:548-549
    const float dx = args.disp_scale * (fx - cx), dy = args.disp_scale * (fy - cy);
    for (int k = 0; k < args.Dd; ++k) o[(size_t)(2 * C + k) * GG + cell] = args.dw[k * 2 + 0] * dx + args.dw[k * 2 + 1] * dy + args.db[k];
}

inline unsigned grid_blocks(long total, long cap) {
    const long g = (total + 255) / 256;
    return (unsigned)(g < 1 ? 1 : (g > cap ? cap : g));
}

}  // namespace

// F.grid_sample(in, grid, mode, padding_mode, align_corners=False): utils/local_correlation.py:55-58, model/network.py:537, 547
GFN_EXPORT int gfn_grid_sample_mode_fwd(const void *in, int in_dtype, const float *grid, float *out, int64_t out_bs, int B, int C, int H,
                                        int W, int Ho, int Wo, int sample_mode, int padding_mode, gfn_stream_t stream) {
    if (in_dtype != GFN_F32 && in_dtype != GFN_F16) return gfn::fail(GFN_ERR_INVALID_ARG, "grid_sample_mode: input dtype must be GFN_F32 or GFN_F16");
    if (!gfn_sm::valid_modes(sample_mode, padding_mode))
        return gfn::fail(GFN_ERR_INVALID_ARG, "grid_sample_mode: sample_mode %d / padding_mode %d is not a GFN_SAMPLE_* / GFN_PAD_* code",
                         sample_mode, padding_mode);
    if (!in || !grid || !out || B < 0 || C <= 0 || H <= 0 || W <= 0 || Ho <= 0 || Wo <= 0 || out_bs < (int64_t)C * Ho * Wo ||
        (long)H * W >= (1L << 31))
        return gfn::fail(GFN_ERR_INVALID_ARG, "grid_sample_mode: bad argument");
    if (B == 0) return GFN_OK;
    const dim3 grid_dim(grid_blocks((long)B * Ho * Wo, 16384));
    const hipStream_t s = (hipStream_t)stream;
    return gfn_sm::with_modes(sample_mode, padding_mode, [&](auto m, auto pad) {
        constexpr int M = decltype(m)::value, P = decltype(pad)::value;
        if (in_dtype == GFN_F16)
            hipLaunchKernelGGL((grid_sample_mode_kernel<_Float16, M, P>), grid_dim, dim3(256), 0, s, static_cast<const _Float16 *>(in), grid,
                               out, (long)out_bs, B, C, H, W, Ho, Wo);
        else
            hipLaunchKernelGGL((grid_sample_mode_kernel<float, M, P>), grid_dim, dim3(256), 0, s, static_cast<const float *>(in), grid, out,
                               (long)out_bs, B, C, H, W, Ho, Wo);
        return gfn::check_launch("grid_sample_mode_kernel");
    });
}

// ConvRefiner(sample_mode=...): model/network.py:464 (argument), :502 (stored), :537 and :547 (the two grid_samples)
GFN_EXPORT int gfn_refiner_input_mode_fwd_dt(const void *f0, const void *f1, int dtype, const float *flow, const float *disp_w,
                                             const float *disp_b, float *d, int64_t d_bs, int B, int C, int Hs, int Ws, int G, int disp_dim,
                                             float disp_scale, int symmetric, int sample_mode, gfn_stream_t stream) {
    if (!gfn_sm::valid_modes(sample_mode, GFN_PAD_ZEROS))
        return gfn::fail(GFN_ERR_INVALID_ARG, "refiner_input_mode: sample_mode %d is not a GFN_SAMPLE_* code", sample_mode);
    gfn_ri::RiArgs q;
    bool keep;
    if (int e = gfn_ri::ri_args("refiner_input_mode", f0, f1, dtype, flow, disp_w, disp_b, d, d_bs, B, C, Hs, Ws, G, disp_dim, disp_scale, symmetric, q, keep))
        return e;
    if (B == 0) return GFN_OK;
    const dim3 grid((unsigned)(((long)G * G + 255) / 256), (unsigned)B);
    const hipStream_t s = (hipStream_t)stream;
    return gfn_sm::with_modes(sample_mode, GFN_PAD_ZEROS, [&](auto m, auto) {
        constexpr int M = decltype(m)::value;
        if (dtype == GFN_F16) {
            if (keep) hipLaunchKernelGGL((refiner_input_mode_kernel<_Float16, M, true>), grid, dim3(256), 0, s, q);
            else hipLaunchKernelGGL((refiner_input_mode_kernel<_Float16, M, false>), grid, dim3(256), 0, s, q);
        } else {
            if (keep) hipLaunchKernelGGL((refiner_input_mode_kernel<float, M, true>), grid, dim3(256), 0, s, q);
            else hipLaunchKernelGGL((refiner_input_mode_kernel<float, M, false>), grid, dim3(256), 0, s, q);
        }
        return gfn::check_launch("refiner_input_mode_kernel");
    });
}
