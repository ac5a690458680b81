// sample_modes.h -- F.grid_sample's three interpolation modes (nearest, bilinear, bicubic) and three padding modes (zeros,
// border, reflection) with align_corners=False, as device helpers, following ATen's grid_sampler_2d
// (aten/src/ATen/native/GridSampler.h, cuda/GridSampler.cu).  The reference passes `sample_mode` and `padding_mode` straight to
// F.grid_sample (utils/local_correlation.py:55-58, 66-68; model/network.py:537, 547).
//
// A sampling point becomes a Taps<MODE> set-up once: the in-image offsets of its 1, 4 or 16 pixels (a pixel outside the image
// reads pixel 0, whose contribution is then dropped) and its weights; every channel plane is then read through the same set-up
// with all loads of a channel group in flight (load(), then value()).  For bilinear with zeros padding the arithmetic is
// exactly that of tap_general (local_corr_common.h) and bilin_setup (refiner_input.h), operation for operation.
//
// Coordinates whose floor lies 10^6 pixels or more outside the image, and non-finite ones, read zeros in every mode (the
// `sane` guard of the bilinear kernels); F.grid_sample's CPU and GPU implementations disagree with each other there.
#pragma once
#include <type_traits>

#include "common.h"
#include "refiner_input.h"

namespace gfn_sm {

using gfn_ri::unnorm;

__device__ __forceinline__ float ldf(const float *q) { return *q; }
__device__ __forceinline__ float ldf(const _Float16 *q) { return (float)*q; }

// clip_coordinates: into [0, size - 1]
__device__ __forceinline__ float clip_coord(float x, int size) { return fminf((float)(size - 1), fmaxf(x, 0.f)); }

// reflect_coordinates(x, twice_low = -1, twice_high = 2 size - 1): mirror about -0.5 and size - 0.5
__device__ __forceinline__ float reflect_coord(float x, int size) {
    const float mn = -0.5f, span = (float)size;
    const float in = fabsf(x - mn);
    const float extra = fmodf(in, span);
    const float flips = floorf(in / span);
    return fmodf(flips, 2.f) == 0.f ? extra + mn : span - extra + mn;
}

// compute_coordinates: the padding transform of an un-normalised coordinate
template <int PAD>
__device__ __forceinline__ float pad_coord(float x, int size) {
    if constexpr (PAD == GFN_PAD_BORDER) return clip_coord(x, size);
    else if constexpr (PAD == GFN_PAD_REFLECTION) return clip_coord(reflect_coord(x, size), size);
    else return x;
}

// the bilinear kernels' guard, on the floor of the un-padded coordinate (false for NaN)
__device__ __forceinline__ bool sane_floor(float fx, float fy) { return (fx > -1e6f) & (fx < 1e6f) & (fy > -1e6f) & (fy < 1e6f); }

// get_cubic_upsample_coefficients, A = -0.75 (the polynomials of cubic_coeffs in grid_ops.hip, ATen's argument order)
__device__ __forceinline__ float cubic_conv1(float x) { return ((-0.75f + 2.f) * x - (-0.75f + 3.f)) * x * x + 1.f; }
__device__ __forceinline__ float cubic_conv2(float x) { return ((-0.75f * x - 5.f * -0.75f) * x + 8.f * -0.75f) * x - 4.f * -0.75f; }
__device__ __forceinline__ void cubic_coeffs(float t, float c[4]) {
    c[0] = cubic_conv2(t + 1.f);
    c[1] = cubic_conv1(t);
    const float t2 = 1.f - t;
    c[2] = cubic_conv1(t2);
    c[3] = cubic_conv2(t2 + 1.f);
}

template <int MODE>
struct Taps;

// nearest: nearbyint of the padded coordinate (round half to even); outside the image reads 0
template <>
struct Taps<GFN_SAMPLE_NEAREST> {
    static constexpr int N = 1;
    int o[1];
    bool ok;
    template <int PAD>
    __device__ __forceinline__ void setup(float gx, float gy, int W, int H) {
        float ix = unnorm(gx, W), iy = unnorm(gy, H);
        const bool sane = sane_floor(floorf(ix), floorf(iy));
        ix = pad_coord<PAD>(sane ? ix : -8.f, W);
        iy = pad_coord<PAD>(sane ? iy : -8.f, H);
        const int x = (int)rintf(ix), y = (int)rintf(iy);
        ok = sane & ((unsigned)x < (unsigned)W) & ((unsigned)y < (unsigned)H);
        o[0] = ok ? y * W + x : 0;
    }
    template <typename FT>
    __device__ __forceinline__ void load(const FT *pl, float v[N]) const { v[0] = ldf(pl + o[0]); }
    __device__ __forceinline__ float value(const float v[N]) const { return ok ? v[0] : 0.f; }
};

// bilinear: corners nw, ne, sw, se of the padded coordinate, zero weight outside the image (tap_general's form)
template <>
struct Taps<GFN_SAMPLE_BILINEAR> {
    static constexpr int N = 4;
    int o[4];
    float w[4];
    template <int PAD>
    __device__ __forceinline__ void setup(float gx, float gy, int W, int H) {
        float ix = unnorm(gx, W), iy = unnorm(gy, H);
        const bool sane = sane_floor(floorf(ix), floorf(iy));
        ix = pad_coord<PAD>(ix, W);
        iy = pad_coord<PAD>(iy, H);
        const float fx = floorf(ix), fy = floorf(iy);
        const int x0 = sane ? (int)fx : -4, y0 = sane ? (int)fy : -4;
        const float w00 = (fx + 1.f - ix) * (fy + 1.f - iy), w01 = (ix - fx) * (fy + 1.f - iy);
        const float w10 = (fx + 1.f - ix) * (iy - fy), w11 = (ix - fx) * (iy - fy);
        const bool xa = (unsigned)x0 < (unsigned)W, xb = (unsigned)(x0 + 1) < (unsigned)W;
        const bool ya = (unsigned)y0 < (unsigned)H, yb = (unsigned)(y0 + 1) < (unsigned)H;
        o[0] = (ya & xa) ? y0 * W + x0 : 0;  // (each offset is formed only for a corner inside the image)
        o[1] = (ya & xb) ? y0 * W + x0 + 1 : 0;
        o[2] = (yb & xa) ? (y0 + 1) * W + x0 : 0;
        o[3] = (yb & xb) ? (y0 + 1) * W + x0 + 1 : 0;
        w[0] = (ya & xa) ? w00 : 0.f;
        w[1] = (ya & xb) ? w01 : 0.f;
        w[2] = (yb & xa) ? w10 : 0.f;
        w[3] = (yb & xb) ? w11 : 0.f;
    }
    template <typename FT>
    __device__ __forceinline__ void load(const FT *pl, float v[N]) const {
#pragma unroll
        for (int n = 0; n < 4; ++n) v[n] = ldf(pl + o[n]);
    }
    __device__ __forceinline__ float value(const float v[N]) const {
        float s = 0.f;
        s += v[0] * w[0];
        s += v[1] * w[1];
        s += v[2] * w[2];
        s += v[3] * w[3];
        return s;
    }
};

// bicubic: taps floor(ix) - 1 .. + 2 of the UN-padded coordinate, each tap padded on its own and read as 0 outside the image
// (get_value_bounded); rows interpolated along x first, then the four row values along y
template <>
struct Taps<GFN_SAMPLE_BICUBIC> {
    static constexpr int N = 16;
    int o[16];
    unsigned ok;  // bit 4 * row + column
    float cx[4], cy[4];
    template <int PAD>
    __device__ __forceinline__ void setup(float gx, float gy, int W, int H) {
        const float ix = unnorm(gx, W), iy = unnorm(gy, H);
        const float fx = floorf(ix), fy = floorf(iy);
        const bool sane = sane_floor(fx, fy);
        cubic_coeffs(sane ? ix - fx : 0.f, cx);  // (a non-finite fraction would turn the zeros below into NaN)
        cubic_coeffs(sane ? iy - fy : 0.f, cy);
        const float bx = sane ? fx : -8.f, by = sane ? fy : -8.f;
        int xs[4], ys[4];
        unsigned okx = 0, oky = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            xs[k] = (int)pad_coord<PAD>(bx - 1.f + (float)k, W);
            ys[k] = (int)pad_coord<PAD>(by - 1.f + (float)k, H);
            okx |= (sane & ((unsigned)xs[k] < (unsigned)W)) ? 1u << k : 0u;
            oky |= (sane & ((unsigned)ys[k] < (unsigned)H)) ? 1u << k : 0u;
        }
        ok = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const bool in = ((oky >> r) & (okx >> c) & 1u) != 0;
                o[4 * r + c] = in ? ys[r] * W + xs[c] : 0;
                ok |= in ? 1u << (4 * r + c) : 0u;
            }
        }
    }
    template <typename FT>
    __device__ __forceinline__ void load(const FT *pl, float v[N]) const {
#pragma unroll
        for (int n = 0; n < 16; ++n) v[n] = ldf(pl + o[n]);
    }
    __device__ __forceinline__ float value(const float v[N]) const {
        float row[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float t[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) t[c] = ((ok >> (4 * r + c)) & 1u) ? v[4 * r + c] : 0.f;
            row[r] = t[0] * cx[0] + t[1] * cx[1] + t[2] * cx[2] + t[3] * cx[3];
        }
        return row[0] * cy[0] + row[1] * cy[1] + row[2] * cy[2] + row[3] * cy[3];
    }
};

// channels unrolled per group: 8 for nearest and bilinear (as the general kernel), 4 for bicubic (16 loads per channel)
template <int MODE>
constexpr int group_channels() { return MODE == GFN_SAMPLE_BICUBIC ? 4 : 8; }

// f(std::integral_constant<int, MODE>, std::integral_constant<int, PAD>) for run-time codes the caller has validated
template <typename F>
int with_modes(int sample_mode, int padding_mode, F &&f) {
    using std::integral_constant;
    auto pad = [&](auto m) {
        if (padding_mode == GFN_PAD_BORDER) return f(m, integral_constant<int, GFN_PAD_BORDER>());
        if (padding_mode == GFN_PAD_REFLECTION) return f(m, integral_constant<int, GFN_PAD_REFLECTION>());
        return f(m, integral_constant<int, GFN_PAD_ZEROS>());
    };
    if (sample_mode == GFN_SAMPLE_NEAREST) return pad(integral_constant<int, GFN_SAMPLE_NEAREST>());
    if (sample_mode == GFN_SAMPLE_BICUBIC) return pad(integral_constant<int, GFN_SAMPLE_BICUBIC>());
    return pad(integral_constant<int, GFN_SAMPLE_BILINEAR>());
}

inline bool valid_modes(int sample_mode, int padding_mode) {
    return sample_mode >= GFN_SAMPLE_BILINEAR && sample_mode <= GFN_SAMPLE_BICUBIC && padding_mode >= GFN_PAD_ZEROS &&
           padding_mode <= GFN_PAD_REFLECTION;
}

}  // namespace gfn_sm
