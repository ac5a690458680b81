// sample_modes.h -- F.grid_sample's three interpolation modes (nearest, bilinear, bicubic) and three padding modes (zeros,
// border, reflection) with align_corners=False, as device helpers, following ATen's grid_sampler_2d
// (aten/src/ATen/native/GridSampler.h, cuda/GridSampler.cu).  The reference passes `sample_mode` and `padding_mode` straight to
// F.grid_sample (utils/local_correlation.py:55-58, 66-68; model/network.py:537, 547).
//
// A sampling point becomes a Taps<MODE> set-up once: the in-image offsets of its 1, 4 or 16 pixels (a pixel outside the image
// reads pixel 0, whose contribution is then dropped) and its weights; every channel plane is then read through the same set-up
// with all loads of a channel group in flight (load(), then value()).  This is the one definition of a sample: the per-tap
// routine of the tiled local-correlation kernels (tap_general, local_corr_common.h), every per-tap kernel (local_corr_modes.hip,
// grid_modes.hip) and the pair gathers of the refiner input (bilin_pairs, refiner_input.h) take their arithmetic from here.
// The zero-weight form reads pixel 0 of a plane for a corner outside the image and multiplies it by 0: exact for finite feature
// maps (include/gfnet_hip.h, conventions).
//
// Coordinates whose floor lies 10^6 pixels or more outside the image, and non-finite ones, read zeros in every mode (the
// `sane` guard of the bilinear kernels); F.grid_sample's CPU and GPU implementations disagree with each other there.
//
// tests/test_sampling_exact_gpu.py pins the decisions taken here -- the nearest ties (half to even), the mirrors at -0.5 and
// size - 0.5 and their multiples, the border clamp at size - 1, the corners and taps outside the image, the guard at +-10^6 -- by
// equality with a float64 oracle on data that leaves fp32 no rounding (tests/golden/sampling_cases.py).
#pragma once
#include <type_traits>

#include "common.h"

namespace gfn_sm {

// normalised -> pixel coordinate exactly as grid_sample(align_corners=False) un-normalises
__device__ __forceinline__ float unnorm(float g, int size) { return ((g + 1.f) * (float)size - 1.f) / 2.f; }

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

// get_cubic_upsample_coefficients, A = -0.75.  The polynomials of cubic_coeffs in grid_ops.hip (resize_normalise) in ATen's
// argument order -- cubic_conv2((1 - t) + 1) here, cubic2(2 - t) there: not the same bits, so the two stay apart.
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

// grid_sample's bilinear set-up (ATen grid_sampler_2d): the nw corner (x0, y0) of the padded coordinate, the weights of the corners
// nw, ne, sw, se and which corner columns / rows lie inside the image.  An insane coordinate has every corner outside.
struct Bilin {
    int x0, y0;
    float w00, w01, w10, w11;
    bool xa, xb, ya, yb;
};
template <int PAD>
__device__ __forceinline__ Bilin bilin_setup(float gx, float gy, int W, int H) {
    Bilin s;
    float ix = unnorm(gx, W), iy = unnorm(gy, H);
    const bool sane = sane_floor(floorf(ix), floorf(iy));
    ix = pad_coord<PAD>(ix, W);
    iy = pad_coord<PAD>(iy, H);
    const float fx = floorf(ix), fy = floorf(iy);
    s.x0 = sane ? (int)fx : -4;
    s.y0 = sane ? (int)fy : -4;
    s.w00 = (fx + 1.f - ix) * (fy + 1.f - iy);
    s.w01 = (ix - fx) * (fy + 1.f - iy);
    s.w10 = (fx + 1.f - ix) * (iy - fy);
    s.w11 = (ix - fx) * (iy - fy);
    s.xa = (unsigned)s.x0 < (unsigned)W;
    s.xb = (unsigned)(s.x0 + 1) < (unsigned)W;
    s.ya = (unsigned)s.y0 < (unsigned)H;
    s.yb = (unsigned)(s.y0 + 1) < (unsigned)H;
    return s;
}

// bilinear: four always-valid offsets and four weights that are zero for a corner outside the image, so the gathers need no
// branches (a zero weight times any finite value adds an exact 0; corner order nw, ne, sw, se is kept)
template <>
struct Taps<GFN_SAMPLE_BILINEAR> {
    static constexpr int N = 4;
    int o[4];
    float w[4];
    template <int PAD>
    __device__ __forceinline__ void setup(float gx, float gy, int W, int H) {
        const Bilin s = bilin_setup<PAD>(gx, gy, W, H);
        o[0] = (s.ya & s.xa) ? s.y0 * W + s.x0 : 0;  // (each offset is formed only for a corner inside the image)
        o[1] = (s.ya & s.xb) ? s.y0 * W + s.x0 + 1 : 0;
        o[2] = (s.yb & s.xa) ? (s.y0 + 1) * W + s.x0 : 0;
        o[3] = (s.yb & s.xb) ? (s.y0 + 1) * W + s.x0 + 1 : 0;
        w[0] = (s.ya & s.xa) ? s.w00 : 0.f;
        w[1] = (s.ya & s.xb) ? s.w01 : 0.f;
        w[2] = (s.yb & s.xa) ? s.w10 : 0.f;
        w[3] = (s.yb & s.xb) ? s.w11 : 0.f;
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

// channels unrolled per group: 8 for nearest and bilinear, 4 for bicubic (16 loads per channel)
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
