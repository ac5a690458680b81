// photometric.hip -- the reference's `initial_transforms` on gfx950: Resize, ColorJitter, RandomGrayscale, RandomGaussianBlur, ToTensor.
//
// Replaces train.py:74-79 / :88-93 of the reference, which run per image on host workers on PIL images (torchvision's PIL backend
// and datasets/homography_dataset_large_size.py:17-28).  What executes there is Pillow, so every stage here maps uint8 to uint8 with
// Pillow's arithmetic (pinned against Pillow 12.2.0, NOT against torchvision, which is a thin caller of it):
//   photo_resize_kernel : Image.resize(BILINEAR) -- both passes in one launch; the horizontally resized uint8 rows a tile needs are
//                         made in LDS, the vertical pass reads them there.  Taps and 22-bit fixed-point weights come from a table.
//   photo_stats_kernel  : the sum of L over each image as it stands when contrast's turn comes (ImageEnhance.Contrast's mean)
//   photo_jitter_blur_kernel : the per-image order of brightness / contrast / saturation / hue, the grey conversion, the three-pass
//                         box blur of ImageFilter.GaussianBlur and ToTensor, fused
// Tiles, stated once.  Resize: 32 x 32 output pixels per workgroup, 48 intermediate rows x 32 columns of packed RGBX dwords in LDS
// (6 KiB); a tile whose source rows exceed 48 walks them in chunks, accumulating in registers.  Jitter + blur: 64 x 32 output pixels,
// a halo of 3 (r + 1) <= 6 pixels per side (r = the integer box radius, 0 or 1), so at most 76 x 44 pixels, one packed RGBX dword
// each, in two buffers (2 x 13376 B = 26752 B of LDS): a lane reads and writes whole dwords at consecutive addresses, which is
// conflict-free, where byte planes would be 4 lanes to a bank.  Every box pass clamps its indices to the IMAGE (and to the staged
// region, whose outer ring a pass may spoil by r + 1 pixels: three passes per axis spoil exactly the halo).
// -ffp-contract=off: the float blends and the HSV conversions round in the order written, which is Pillow's.
#include "common.h"
#include "reduce.h"

namespace {

#define GFN_GLOBAL __attribute__((address_space(1)))
typedef unsigned char u8;

constexpr int kRzTile = 32, kRzRows = 48;
constexpr int kJbW = 64, kJbH = 32, kJbHalo = 6;
constexpr int kJbRegion = (kJbW + 2 * kJbHalo) * (kJbH + 2 * kJbHalo);
constexpr int kStatsPerBlock = 4096;

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ unsigned pack3(int r, int g, int b) { return (unsigned)r | ((unsigned)g << 8) | ((unsigned)b << 16); }

// Convert.c rgb2l
__device__ __forceinline__ int grey_l(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

// Blend.c: in1 + alpha * (in2 - in1) in float; truncated for alpha in [0, 1], clipped then truncated outside
__device__ __forceinline__ int blend(int a, int b, float f) {
    const float t = (float)a + f * (float)(b - a);
    if (f >= 0.f && f <= 1.f) return (int)t;
    return t <= 0.f ? 0 : (t >= 255.f ? 255 : (int)t);
}

// Convert.c rgb2hsv_row: float variables, double constants -- the mix is reproduced term by term
__device__ __forceinline__ void rgb2hsv(int r, int g, int b, int &uh, int &us, int &uv) {
    const int mx = max(r, max(g, b)), mn = min(r, min(g, b));
    uv = mx;
    if (mx == mn) { uh = 0; us = 0; return; }
    const float cr = (float)(mx - mn);
    const float s = cr / (float)mx;
    const float rc = (float)(mx - r) / cr, gc = (float)(mx - g) / cr, bc = (float)(mx - b) / cr;
    float h;
    if (r == mx) h = bc - gc;
    else if (g == mx) h = (float)((2.0 + (double)rc) - (double)bc);
    else h = (float)((4.0 + (double)gc) - (double)rc);
    const double t = (double)h / 6.0 + 1.0;     // in [5/6, 11/6]
    h = (float)(t - floor(t));                  // fmod(t, 1.0)
    uh = min((int)((double)h * 255.0), 255);
    us = min((int)((double)s * 255.0), 255);
}

// Convert.c hsv2rgb: double arithmetic on float f and fs, round() half away from zero
__device__ __forceinline__ void hsv2rgb(int h, int s, int v, int &r, int &g, int &b) {
    if (s == 0) { r = g = b = v; return; }
    const double hf = (double)(float)h * 6.0 / 255.0;
    const double fl = floor(hf);
    const double f = (double)(float)(hf - fl);
    const double fs = (double)(float)((double)(float)s / 255.0);
    const double vv = (double)v;
    const int p = clampi((int)floor(vv * (1.0 - fs) + 0.5), 0, 255);
    const int q = clampi((int)floor(vv * (1.0 - fs * f) + 0.5), 0, 255);
    const int t = clampi((int)floor(vv * (1.0 - fs * (1.0 - f)) + 0.5), 0, 255);
    switch ((int)fl % 6) {
        case 0: r = v; g = t; b = p; break;
        case 1: r = q; g = v; b = p; break;
        case 2: r = p; g = v; b = t; break;
        case 3: r = p; g = q; b = v; break;
        case 4: r = t; g = p; b = v; break;
        default: r = v; g = p; b = q; break;
    }
}

// one image's record (GFN_PHOTO_REC ints, include/gfnet_hip.h)
struct Chain {
    int order[4];
    float fb, fc, fs;
    int hue, grey, mask;
    float R;
};

__device__ __forceinline__ Chain load_chain(const int *__restrict__ params, int img) {
    const int *p = params + (long)img * GFN_PHOTO_REC;
    Chain c;
#pragma unroll
    for (int k = 0; k < 4; ++k) c.order[k] = p[k];
    c.fb = __int_as_float(p[4]); c.fc = __int_as_float(p[5]); c.fs = __int_as_float(p[6]);
    c.hue = p[7] & 255; c.grey = p[8]; c.R = __int_as_float(p[9]); c.mask = p[10];
    return c;
}

// The pointwise ops in the image's own order.  STATS: stop when contrast's turn comes (the pixel as ImageEnhance.Contrast sees it).
template <bool STATS>
__device__ __forceinline__ void apply_chain(int &r, int &g, int &b, const Chain &c, int mean) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int op = c.order[k];
        if (!((c.mask >> op) & 1)) continue;
        if (op == GFN_PHOTO_BRIGHTNESS) {
            r = blend(0, r, c.fb); g = blend(0, g, c.fb); b = blend(0, b, c.fb);
        } else if (op == GFN_PHOTO_CONTRAST) {
            if (STATS) return;
            r = blend(mean, r, c.fc); g = blend(mean, g, c.fc); b = blend(mean, b, c.fc);
        } else if (op == GFN_PHOTO_SATURATION) {
            const int l = grey_l(r, g, b);
            r = blend(l, r, c.fs); g = blend(l, g, c.fs); b = blend(l, b, c.fs);
        } else if (op == GFN_PHOTO_HUE) {
            int h, s, v;
            rgb2hsv(r, g, b, h, s, v);
            hsv2rgb((h + c.hue) & 255, s, v, r, g, b);
        }
    }
    if (!STATS && c.grey) r = g = b = grey_l(r, g, b);
}

// ---- gfn_photo_resize_u8 ---------------------------------------------------------------------------------------------------------
// Resample.c: a pass is clip8((sum_k w_k x_k + 2^21) >> 22), horizontal first into uint8, then vertical.
__device__ __forceinline__ int clip8_22(int ss) { return clampi(ss >> 22, 0, 255); }

__global__ __launch_bounds__(256) void photo_resize_kernel(const u8 *const *__restrict__ srcs, const int *__restrict__ src_dims,
                                                           u8 *const *__restrict__ dsts, const int *__restrict__ recs,
                                                           const int *__restrict__ coef) {
    __shared__ unsigned rows[kRzRows * kRzTile];
    const int img = blockIdx.y;
    const int *rec = recs + (long)img * GFN_PHOTO_RESIZE_REC;
    const int Ho = rec[0], Wo = rec[1];
    const int tiles_x = (Wo + kRzTile - 1) / kRzTile, tiles_y = (Ho + kRzTile - 1) / kRzTile;
    if ((int)blockIdx.x >= tiles_x * tiles_y) return;  // (an image that is not resized has Ho = 0)
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int ksx = rec[3], ksy = rec[5];
    const int *xb = coef + rec[2], *kx = xb + 2 * Wo;
    const int *yb = coef + rec[4], *ky = yb + 2 * Ho;
    const long stride = src_dims[img * 3 + 2];
    const GFN_GLOBAL u8 *src = (const GFN_GLOBAL u8 *)srcs[img];
    GFN_GLOBAL u8 *dst = (GFN_GLOBAL u8 *)dsts[img];

    const int ox0 = tx * kRzTile, oy0 = ty * kRzTile;
    const int oy_last = min(oy0 + kRzTile, Ho) - 1;
    const int ylo = yb[2 * oy0], yhi = yb[2 * oy_last] + yb[2 * oy_last + 1];  // the tile's source rows [ylo, yhi): bounds are monotone
    const int lx = threadIdx.x & 31, lyb = threadIdx.x >> 5;
    const int ox = ox0 + lx;
    int acc[4][3];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j][0] = acc[j][1] = acc[j][2] = 1 << 21;

    for (int cb = ylo; cb < yhi; cb += kRzRows) {
        for (int e = threadIdx.x; e < kRzRows * kRzTile; e += 256) {
            const int iy = cb + (e >> 5), cx = ox0 + (e & 31);
            if (iy < yhi && cx < Wo) {
                const int x0 = xb[2 * cx], n = xb[2 * cx + 1];
                const int *w = kx + (long)cx * ksx;
                const GFN_GLOBAL u8 *p = src + iy * stride + (long)x0 * 3;
                int s0 = 1 << 21, s1 = 1 << 21, s2 = 1 << 21;
                for (int k = 0; k < n; ++k) {
                    const int wk = w[k];
                    s0 += wk * p[3 * k]; s1 += wk * p[3 * k + 1]; s2 += wk * p[3 * k + 2];
                }
                rows[e] = pack3(clip8_22(s0), clip8_22(s1), clip8_22(s2));
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int oy = oy0 + lyb + 8 * j;
            if (oy < Ho && ox < Wo) {
                const int y0 = yb[2 * oy], n = yb[2 * oy + 1];
                const int *w = ky + (long)oy * ksy;
                const int k0 = max(cb - y0, 0), k1 = min(cb + kRzRows - y0, n);
                for (int k = k0; k < k1; ++k) {
                    const unsigned v = rows[(y0 + k - cb) * kRzTile + lx];
                    const int wk = w[k];
                    acc[j][0] += wk * (int)(v & 255u); acc[j][1] += wk * (int)((v >> 8) & 255u); acc[j][2] += wk * (int)((v >> 16) & 255u);
                }
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int oy = oy0 + lyb + 8 * j;
        if (oy < Ho && ox < Wo) {
            GFN_GLOBAL u8 *o = dst + ((long)oy * Wo + ox) * 3;
            o[0] = (u8)clip8_22(acc[j][0]); o[1] = (u8)clip8_22(acc[j][1]); o[2] = (u8)clip8_22(acc[j][2]);
        }
    }
}

// ---- gfn_photo_stats -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void photo_stats_kernel(const u8 *const *__restrict__ srcs, const int *__restrict__ dims,
                                                          const int *__restrict__ params, unsigned long long *__restrict__ sums) {
    const int img = blockIdx.y;
    const Chain c = load_chain(params, img);
    if (!((c.mask >> GFN_PHOTO_CONTRAST) & 1)) return;
    const int H = dims[img * 3], W = dims[img * 3 + 1];
    const long stride = dims[img * 3 + 2], total = (long)H * W;
    const long base = (long)blockIdx.x * kStatsPerBlock;
    if (base >= total) return;
    const GFN_GLOBAL u8 *src = (const GFN_GLOBAL u8 *)srcs[img];
    unsigned sum = 0;  // 16 pixels of at most 255 per lane
    for (int j = 0; j < kStatsPerBlock / 256; ++j) {
        const unsigned i = (unsigned)base + j * 256 + threadIdx.x;  // H * W <= 2^30: a 32-bit divide
        if (i < (unsigned)total) {
            const int y = (int)(i / (unsigned)W), x = (int)(i - (unsigned)y * (unsigned)W);
            const GFN_GLOBAL u8 *p = src + y * stride + (long)x * 3;
            int r = p[0], g = p[1], b = p[2];
            apply_chain<true>(r, g, b, c, 0);
            sum += (unsigned)grey_l(r, g, b);
        }
    }
    sum = gfn::wave_sum(sum);
    if ((threadIdx.x & 63) == 0) atomicAdd(sums + img, (unsigned long long)sum);  // integer: the total does not depend on the order
}

// ---- gfn_photo_jitter_blur -------------------------------------------------------------------------------------------------------
// BoxBlur.c ImagingLineBoxBlur8/32: out = (ww * sum_{|k| <= r} x[i + k] + fw * (x[i - r - 1] + x[i + r + 1]) + 2^23) >> 24
__device__ __forceinline__ unsigned box_tap(const unsigned *__restrict__ in, int base, int step, int i, int lo, int hi, int r,
                                            unsigned ww, unsigned fw) {
    unsigned s0 = 0, s1 = 0, s2 = 0;
    for (int k = -r; k <= r; ++k) {
        const unsigned v = in[base + clampi(i + k, lo, hi) * step];
        s0 += v & 255u; s1 += (v >> 8) & 255u; s2 += (v >> 16) & 255u;
    }
    const unsigned a = in[base + clampi(i - r - 1, lo, hi) * step], b = in[base + clampi(i + r + 1, lo, hi) * step];
    const unsigned f0 = (a & 255u) + (b & 255u), f1 = ((a >> 8) & 255u) + ((b >> 8) & 255u), f2 = ((a >> 16) & 255u) + ((b >> 16) & 255u);
    const unsigned o0 = (ww * s0 + fw * f0 + (1u << 23)) >> 24, o1 = (ww * s1 + fw * f1 + (1u << 23)) >> 24,
                   o2 = (ww * s2 + fw * f2 + (1u << 23)) >> 24;
    return o0 | (o1 << 8) | (o2 << 16);
}

template <bool U8OUT>
__device__ __forceinline__ void store_pixel(void *dstp, int H, int W, int y, int x, unsigned v) {
    if (U8OUT) {
        GFN_GLOBAL u8 *o = (GFN_GLOBAL u8 *)dstp + ((long)y * W + x) * 3;
        o[0] = (u8)(v & 255u); o[1] = (u8)((v >> 8) & 255u); o[2] = (u8)((v >> 16) & 255u);
    } else {  // ToTensor: a true division, planar
        GFN_GLOBAL float *o = (GFN_GLOBAL float *)dstp + ((long)y * W + x);
        const long plane = (long)H * W;
        o[0] = (float)(v & 255u) / 255.0f; o[plane] = (float)((v >> 8) & 255u) / 255.0f; o[2 * plane] = (float)((v >> 16) & 255u) / 255.0f;
    }
}

template <bool U8OUT>
__global__ __launch_bounds__(256) void photo_jitter_blur_kernel(const u8 *const *__restrict__ srcs, const int *__restrict__ dims,
                                                                const int *__restrict__ params,
                                                                const unsigned long long *__restrict__ sums,
                                                                void *const *__restrict__ dsts) {
    __shared__ unsigned bufA[kJbRegion], bufB[kJbRegion];
    const int img = blockIdx.y;
    const int H = dims[img * 3], W = dims[img * 3 + 1];
    const long stride = dims[img * 3 + 2];
    const int tiles_x = (W + kJbW - 1) / kJbW, tiles_y = (H + kJbH - 1) / kJbH;
    if ((int)blockIdx.x >= tiles_x * tiles_y) return;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int x0 = tx * kJbW, y0 = ty * kJbH;
    const Chain c = load_chain(params, img);
    // ImageEnhance.Contrast: int(mean(L) + 0.5), the mean a double division of the integer sum
    int mean = 0;
    if ((c.mask >> GFN_PHOTO_CONTRAST) & 1) mean = (int)((double)sums[img] / (double)((long)H * W) + 0.5);
    const GFN_GLOBAL u8 *src = (const GFN_GLOBAL u8 *)srcs[img];
    void *dst = dsts[img];

    if (!(c.R > 0.f)) {  // no blur: no halo, no LDS
        for (int e = threadIdx.x; e < kJbW * kJbH; e += 256) {
            const int y = y0 + (e >> 6), x = x0 + (e & 63);
            if (y < H && x < W) {
                const GFN_GLOBAL u8 *p = src + y * stride + (long)x * 3;
                int r = p[0], g = p[1], b = p[2];
                apply_chain<false>(r, g, b, c, mean);
                store_pixel<U8OUT>(dst, H, W, y, x, pack3(r, g, b));
            }
        }
        return;
    }
    const int r = min((int)c.R, 1);  // (the halo holds r <= 1, i.e. R < 2; the callers refuse more)
    const unsigned ww = (unsigned)(16777216.0f / (c.R * 2.0f + 1.0f));
    const unsigned fw = ((1u << 24) - (unsigned)(2 * r + 1) * ww) / 2u;
    const int h = 3 * (r + 1), rw = kJbW + 2 * h, rh = kJbH + 2 * h;
    const int rx0 = x0 - h, ry0 = y0 - h;
    // the staged pixels that lie in the image, in region coordinates: what every pass clamps to
    const int xlo = max(0, rx0) - rx0, xhi = min(W - 1, rx0 + rw - 1) - rx0;
    const int ylo = max(0, ry0) - ry0, yhi = min(H - 1, ry0 + rh - 1) - ry0;
    for (int e = threadIdx.x; e < rw * rh; e += 256) {
        const int ly = e / rw, lx = e - ly * rw;
        const int y = clampi(ly, ylo, yhi) + ry0, x = clampi(lx, xlo, xhi) + rx0;
        const GFN_GLOBAL u8 *p = src + y * stride + (long)x * 3;
        int rr = p[0], g = p[1], b = p[2];
        apply_chain<false>(rr, g, b, c, mean);
        bufA[e] = pack3(rr, g, b);
    }
    __syncthreads();
    unsigned *in = bufA, *out = bufB;
    for (int pass = 0; pass < 3; ++pass) {  // along rows
        for (int e = threadIdx.x; e < rw * rh; e += 256) {
            const int ly = e / rw, lx = e - ly * rw;
            out[e] = box_tap(in, ly * rw, 1, lx, xlo, xhi, r, ww, fw);
        }
        __syncthreads();
        unsigned *t = in; in = out; out = t;
    }
    for (int pass = 0; pass < 3; ++pass) {  // along columns, the tile's columns only
        for (int e = threadIdx.x; e < kJbW * rh; e += 256) {
            const int ly = e >> 6, lx = h + (e & 63);
            out[ly * rw + lx] = box_tap(in, lx, rw, ly, ylo, yhi, r, ww, fw);
        }
        __syncthreads();
        unsigned *t = in; in = out; out = t;
    }
    for (int e = threadIdx.x; e < kJbW * kJbH; e += 256) {
        const int ly = e >> 6, lx = e & 63;
        const int y = y0 + ly, x = x0 + lx;
        if (y < H && x < W) store_pixel<U8OUT>(dst, H, W, y, x, in[(ly + h) * rw + lx + h]);
    }
}

bool aligned(const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

int check_batch(const char *what, int N, int max_h, int max_w) {
    if (N < 0 || N > 65535 || max_h < 0 || max_w < 0 || max_h > 32768 || max_w > 32768)
        return gfn::fail(GFN_ERR_INVALID_ARG, "%s: bad size (N %d in [0, 65535], largest image %d x %d in [0, 32768])", what, N, max_h, max_w);
    return GFN_OK;
}

}  // namespace

GFN_EXPORT int gfn_photo_resize_u8(const void *const *src, const int *src_dims, void *const *dst, const int *recs, const int *coef, int N,
                                   int max_out_h, int max_out_w, gfn_stream_t stream) {
    if (int e = check_batch("photo_resize_u8", N, max_out_h, max_out_w)) return e;
    if (N == 0 || max_out_h == 0 || max_out_w == 0) return GFN_OK;
    if (!src || !src_dims || !dst || !recs || !coef) return gfn::fail(GFN_ERR_INVALID_ARG, "photo_resize_u8: null pointer");
    if (!aligned(src, 8) || !aligned(dst, 8) || !aligned(src_dims, 4) || !aligned(recs, 4) || !aligned(coef, 4))
        return gfn::fail(GFN_ERR_INVALID_ARG, "photo_resize_u8: misaligned table (pointer tables 8 bytes, int tables 4)");
    const unsigned tiles = (unsigned)(((max_out_w + kRzTile - 1) / kRzTile) * ((max_out_h + kRzTile - 1) / kRzTile));
    hipLaunchKernelGGL(photo_resize_kernel, dim3(tiles, (unsigned)N), dim3(256), 0, (hipStream_t)stream, (const u8 *const *)src, src_dims,
                       (u8 *const *)dst, recs, coef);
    return gfn::check_launch("photo_resize_kernel");
}

GFN_EXPORT int gfn_photo_stats(const void *const *src, const int *dims, const int *params, int64_t *sums, int N, int max_h, int max_w,
                               gfn_stream_t stream) {
    if (int e = check_batch("photo_stats", N, max_h, max_w)) return e;
    if (N == 0 || max_h == 0 || max_w == 0) return GFN_OK;
    if (!src || !dims || !params || !sums) return gfn::fail(GFN_ERR_INVALID_ARG, "photo_stats: null pointer");
    if (!aligned(src, 8) || !aligned(sums, 8) || !aligned(dims, 4) || !aligned(params, 4))
        return gfn::fail(GFN_ERR_INVALID_ARG, "photo_stats: misaligned table (pointers and sums 8 bytes, int tables 4)");
    const unsigned blocks = (unsigned)(((long)max_h * max_w + kStatsPerBlock - 1) / kStatsPerBlock);
    hipLaunchKernelGGL(photo_stats_kernel, dim3(blocks, (unsigned)N), dim3(256), 0, (hipStream_t)stream, (const u8 *const *)src, dims, params,
                       (unsigned long long *)sums);
    return gfn::check_launch("photo_stats_kernel");
}

GFN_EXPORT int gfn_photo_jitter_blur(const void *const *src, const int *dims, const int *params, const int64_t *sums, void *const *dst,
                                     int out_u8, int N, int max_h, int max_w, gfn_stream_t stream) {
    if (int e = check_batch("photo_jitter_blur", N, max_h, max_w)) return e;
    if (N == 0 || max_h == 0 || max_w == 0) return GFN_OK;
    if (!src || !dims || !params || !sums || !dst) return gfn::fail(GFN_ERR_INVALID_ARG, "photo_jitter_blur: null pointer");
    if (!aligned(src, 8) || !aligned(dst, 8) || !aligned(sums, 8) || !aligned(dims, 4) || !aligned(params, 4))
        return gfn::fail(GFN_ERR_INVALID_ARG, "photo_jitter_blur: misaligned table (pointers and sums 8 bytes, int tables 4)");
    const unsigned tiles = (unsigned)(((max_w + kJbW - 1) / kJbW) * ((max_h + kJbH - 1) / kJbH));
    const dim3 grid(tiles, (unsigned)N), block(256);
    if (out_u8)
        hipLaunchKernelGGL(photo_jitter_blur_kernel<true>, grid, block, 0, (hipStream_t)stream, (const u8 *const *)src, dims, params,
                           (const unsigned long long *)sums, dst);
    else
        hipLaunchKernelGGL(photo_jitter_blur_kernel<false>, grid, block, 0, (hipStream_t)stream, (const u8 *const *)src, dims, params,
                           (const unsigned long long *)sums, dst);
    return gfn::check_launch("photo_jitter_blur_kernel");
}
