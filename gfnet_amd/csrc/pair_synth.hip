// pair_synth.hip -- the training batch on gfx950: random homographies and fused perspective warps.
//
// Replaces datasets/generate_random_H_large_size.py:6-85 of the reference (random_four_points, randomH), which
// datasets/homography_dataset_large_size.py:148-228 runs per sample on host workers through kornia: a 640 x 640 crop of two images,
// two warp_perspective calls at 640 x 640, two centre crops, a third warp, three get_perspective_transform solves and a 3 x 3
// inverse, all in fp32.  Here:
//   pfp_kernel / rhp_kernel : the four-point solves, 8 lanes per problem on the elimination of ge_solve8.h, everything in double (the
//                             reference's fp32 solve of a system with entries up to 640^2 moves H_s2t by 6e-5 relative)
//   warp_perspective_kernel : crop + warp + centre crop are one projective map from output pixels to source pixels, so an image is
//                             gathered once, straight from its source, with the Normalize fused; the intermediates are never made
// -ffp-contract=off: the fp32 blend rounds in the order written, so a float64 restatement of it is unambiguous.
#include "elem16.h"
#include "ge_solve8.h"

namespace {

using gfn::f32x4;
using gfn::ge_solve8;
using gfn::lane_get;

#define GFN_GLOBAL __attribute__((address_space(1)))

// inverse of a 3 x 3 matrix as adjugate / determinant: exact for the identity and for integer translations (every product is exact
// and the determinant is 1).  A singular matrix gives non-finite entries, which the warp reads as "outside".
__device__ __forceinline__ void inv3(const double (&a)[9], double (&o)[9]) {
    const double c0 = a[4] * a[8] - a[5] * a[7], c1 = a[2] * a[7] - a[1] * a[8], c2 = a[1] * a[5] - a[2] * a[4];
    const double c3 = a[5] * a[6] - a[3] * a[8], c4 = a[0] * a[8] - a[2] * a[6], c5 = a[2] * a[3] - a[0] * a[5];
    const double c6 = a[3] * a[7] - a[4] * a[6], c7 = a[1] * a[6] - a[0] * a[7], c8 = a[0] * a[4] - a[1] * a[3];
    const double det = (a[0] * c0 + a[1] * c3) + a[2] * c6;
    o[0] = c0 / det; o[1] = c1 / det; o[2] = c2 / det;
    o[3] = c3 / det; o[4] = c4 / det; o[5] = c5 / det;
    o[6] = c6 / det; o[7] = c7 / det; o[8] = c8 / det;
}

__device__ __forceinline__ void matmul3(const double (&a)[9], const double (&b)[9], double (&o)[9]) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) o[3 * i + j] = (a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j]) + a[3 * i + 2] * b[6 + j];
}

// kornia's get_perspective_transform for one problem on the 8 lanes base .. base + 7 of a wave (row = lane & 7): lanes 2k and 2k + 1
// pass point k, (x, y) -> (u, v).  The system is kornia's; it is solved for H - identity: the right-hand side is then dst - src,
// which is exact, so src == dst gives the identity bit for bit and a near-identity H keeps its small part to full precision.  Every
// lane of the wave must call it (the elimination shuffles).  Returns ok (group-uniform) and H in every lane; H = identity when not
// ok or not `sound` (the caller's verdict on the source points, group-uniform).
__device__ __forceinline__ bool solve4(double x, double y, double u, double v, bool sound, int row, int base, double (&H)[9]) {
    double M[9];
    if (row & 1) {
        M[0] = 0; M[1] = 0; M[2] = 0; M[3] = x; M[4] = y; M[5] = 1; M[6] = -x * v; M[7] = -y * v; M[8] = v - y;
    } else {
        M[0] = x; M[1] = y; M[2] = 1; M[3] = 0; M[4] = 0; M[5] = 0; M[6] = -x * u; M[7] = -y * u; M[8] = u - x;
    }
    bool ok;
    const double g = ge_solve8<false>(M, row, base, ok);
    const unsigned long long fin = __ballot(isfinite(g));
    ok = ok && sound && (((fin >> base) & 0xFFull) == 0xFFull);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const double gi = lane_get<false>(g, base + i);
        H[i] = ok ? gi + ((i == 0 || i == 4) ? 1.0 : 0.0) : ((i == 0 || i == 4) ? 1.0 : 0.0);
    }
    H[8] = 1.0;
    return ok;
}

// No three of four points on a line (and no two coincident): otherwise there is no homography, and rounding can leave the
// elimination a tiny pivot instead of a zero.  Each cross product is held against the size of its two terms.
__device__ __forceinline__ bool quad_sound(const double (&px)[4], const double (&py)[4]) {
    auto bent = [&](int i, int j, int l) {
        const double p = (px[j] - px[i]) * (py[l] - py[i]), q = (py[j] - py[i]) * (px[l] - px[i]);
        return fabs(p - q) > 1e-12 * (fabs(p) + fabs(q));
    };
    return bent(0, 1, 2) && bent(0, 1, 3) && bent(0, 2, 3) && bent(1, 2, 3);
}

// ---- gfn_perspective_from_points -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pfp_kernel(const float *__restrict__ src, const float *__restrict__ dst, double *__restrict__ H,
                                                  int *__restrict__ okp, int n) {
    const int lane = threadIdx.x & 63, row = lane & 7, base = lane & ~7;
    const long gid = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 3;
    const bool live = gid < n;
    const long i = live ? gid : n - 1;  // a group past the end redoes the last problem and writes nothing: whole waves run the solve
    double sx[4], sy[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) { sx[k] = src[i * 8 + 2 * k]; sy[k] = src[i * 8 + 2 * k + 1]; }
    const int k = row >> 1;
    double h[9];
    const bool ok = solve4(src[i * 8 + 2 * k], src[i * 8 + 2 * k + 1], dst[i * 8 + 2 * k], dst[i * 8 + 2 * k + 1], quad_sound(sx, sy), row,
                           base, h);
    if (live && row == 0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) H[i * 9 + k] = h[k];
        if (okp) okp[i] = ok ? 1 : 0;
    }
}

// ---- gfn_random_h_params ---------------------------------------------------------------------------------------------------------
struct RhpParams {
    const int *draws;
    float *H32;
    double *H64, *MA, *MB;
    int *ok;
    int B, crop, deform, out_h, out_w, final_h, final_w;
};

// output pixel -> source-image pixel of one image: translate(cx, cy) Hinv translate(d2, d2)
__device__ __forceinline__ void pixel_map(const double (&Hinv)[9], double cx, double cy, double d2, double (&M)[9]) {
    double P[9];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        P[3 * r] = Hinv[3 * r];
        P[3 * r + 1] = Hinv[3 * r + 1];
        P[3 * r + 2] = (Hinv[3 * r] * d2 + Hinv[3 * r + 1] * d2) + Hinv[3 * r + 2];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        M[c] = P[c] + cx * P[6 + c];
        M[3 + c] = P[3 + c] + cy * P[6 + c];
        M[6 + c] = P[6 + c];
    }
}

__global__ __launch_bounds__(256) void rhp_kernel(RhpParams P) {
    const int lane = threadIdx.x & 63, row = lane & 7, base = lane & ~7;
    const long gid = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 3;
    const bool live = gid < P.B;
    const long b = live ? gid : P.B - 1;
    const int *d = P.draws + b * 18;
    const double cx = d[0], cy = d[1], d2 = P.deform / 2, w = P.crop, h = P.crop;
    const int k = row >> 1;  // this lane's point: 0 tl, 1 tr, 2 br, 3 bl
    // generate_random_H_large_size.py:23 -- the target point of both images
    const double tx = (k == 1 || k == 2) ? w - d2 - 1 : d2, ty = k >= 2 ? h - d2 - 1 : d2;
    double ax[4], ay[4], bx[4], by[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        ax[q] = d[2 + 2 * q]; ay[q] = d[3 + 2 * q];
        bx[q] = d[10 + 2 * q]; by[q] = d[11 + 2 * q];
    }
    double H1[9], H2[9], H1i[9], H2i[9], H12[9], Hs[9];
    bool ok = solve4(d[2 + 2 * k], d[3 + 2 * k], tx, ty, quad_sound(ax, ay), row, base, H1);          // :30, image 1
    ok = solve4(d[10 + 2 * k], d[11 + 2 * k], tx, ty, quad_sound(bx, by), row, base, H2) && ok;       // :30, image 2
    inv3(H1, H1i);
    inv3(H2, H2i);
    matmul3(H2, H1i, H12);                                  // :62
    // :64-69 -- kornia's transform_points (the homogeneous divide is a multiplication by 1 / z, by 1 where |z| <= 1e-8) of the
    // target point gives the flow of the centre crop's corner
    const double wc = P.out_w, hc = P.out_h;
    const double px = (k == 1 || k == 2) ? wc - 1 : 0.0, py = k >= 2 ? hc - 1 : 0.0;
    const double X = (H12[0] * tx + H12[1] * ty) + H12[2], Y = (H12[3] * tx + H12[4] * ty) + H12[5];
    const double Z = (H12[6] * tx + H12[7] * ty) + H12[8];
    const double s = fabs(Z) > 1e-8 ? 1.0 / Z : 1.0;
    ok = solve4(px, py, px + (X * s - tx), py + (Y * s - ty), true, row, base, Hs) && ok;             // :71 (a rectangle's corners)
    if (P.final_h != P.out_h || P.final_w != P.out_w) {     // :73-79, as written
        const double sl = (double)P.final_h / hc, ri = 1.0 / ((double)P.final_w / wc);
#pragma unroll
        for (int c = 0; c < 3; ++c) { Hs[c] = sl * Hs[c]; Hs[3 + c] = sl * Hs[3 + c]; }
#pragma unroll
        for (int r = 0; r < 3; ++r) { Hs[3 * r] = Hs[3 * r] * ri; Hs[3 * r + 1] = Hs[3 * r + 1] * ri; }
    }
    double MA[9], MB[9];
    pixel_map(H1i, cx, cy, d2, MA);
    pixel_map(H2i, cx, cy, d2, MB);
    if (live && row == 0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            if (P.H32) P.H32[b * 9 + k] = (float)Hs[k];
            if (P.H64) P.H64[b * 9 + k] = Hs[k];
            if (P.MA) P.MA[b * 9 + k] = MA[k];
            if (P.MB) P.MB[b * 9 + k] = MB[k];
        }
        if (P.ok) P.ok[b] = ok ? 1 : 0;
    }
}

// ---- gfn_warp_perspective_fwd ----------------------------------------------------------------------------------------------------
// A workgroup is a 32 x 32 tile of one sample's output (grid = tiles x B): the matrix and the source record are wave-uniform scalar
// loads.  A wave covers 16 x 16 pixels, a lane four consecutive pixels of a row, so that under a rotation the wave's source
// footprint stays a few cache lines tall; the four taps and weights of a pixel serve every channel.  All taps of a channel are
// loaded unconditionally from clamped (in-bounds) addresses and masked afterwards, so the loads issue back to back.
constexpr int kWarpTile = 32;

template <bool VEC>
__global__ __launch_bounds__(256) void warp_perspective_kernel(const float *const *__restrict__ planes, const int *__restrict__ dims,
                                                               const double *__restrict__ M, int invert, float *__restrict__ out,
                                                               long out_bs, int C, int Ho, int Wo, int tiles_x,
                                                               const float *__restrict__ mean, const float *__restrict__ stdv) {
    const int b = blockIdx.y;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int u0 = tx * kWarpTile + (wave & 1) * 16 + (lane & 3) * 4, v = ty * kWarpTile + (wave >> 1) * 16 + (lane >> 2);
    if (v >= Ho || u0 >= Wo) return;
    double m[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) m[k] = M[(long)b * 9 + k];
    if (invert) {
        double t[9];
        inv3(m, t);
#pragma unroll
        for (int k = 0; k < 9; ++k) m[k] = t[k];
    }
    const int H = dims[b * 3], W = dims[b * 3 + 1];
    const long cs = dims[b * 3 + 2];
    const GFN_GLOBAL float *p0 = (const GFN_GLOBAL float *)planes[b];
    const bool have = H > 0 && W > 0 && p0 != nullptr;

    int o00[4], o01[4], o10[4], o11[4];
    bool k00[4], k01[4], k10[4], k11[4];
    float fx[4], fy[4];
    const double dv = v;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const double du = u0 + j;
        const double X = (m[0] * du + m[1] * dv) + m[2], Y = (m[3] * du + m[4] * dv) + m[5], Z = (m[6] * du + m[7] * dv) + m[8];
        const double x = X / Z, y = Y / Z;
        // a pixel with no neighbour inside the source (or a non-finite coordinate: the comparisons fail) is zero
        const bool in = have && x > -1.0 && x < (double)W && y > -1.0 && y < (double)H;
        const double xs = in ? x : 0.0, ys = in ? y : 0.0;
        const double xf = floor(xs), yf = floor(ys);
        fx[j] = (float)(xs - xf);
        fy[j] = (float)(ys - yf);
        const int ix = (int)xf, iy = (int)yf;  // in [-1, W - 1] x [-1, H - 1]
        const bool x0 = ix >= 0, x1 = ix + 1 < W, y0 = iy >= 0, y1 = iy + 1 < H;
        k00[j] = in && x0 && y0; k01[j] = in && x1 && y0; k10[j] = in && x0 && y1; k11[j] = in && x1 && y1;
        const int xa = x0 ? ix : 0, xb = x1 ? ix + 1 : (W > 0 ? W - 1 : 0), ya = y0 ? iy : 0, yb = y1 ? iy + 1 : (H > 0 ? H - 1 : 0);
        o00[j] = ya * W + xa; o01[j] = ya * W + xb; o10[j] = yb * W + xa; o11[j] = yb * W + xb;
    }
    GFN_GLOBAL float *op = (GFN_GLOBAL float *)out + ((long)b * out_bs + (long)v * Wo + u0);
    for (int c = 0; c < C; ++c) {
        float r[4] = {0.f, 0.f, 0.f, 0.f};
        if (have) {
            const GFN_GLOBAL float *p = p0 + c * cs;
            float a00[4], a01[4], a10[4], a11[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) { a00[j] = p[o00[j]]; a01[j] = p[o01[j]]; a10[j] = p[o10[j]]; a11[j] = p[o11[j]]; }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float v00 = k00[j] ? a00[j] : 0.f, v01 = k01[j] ? a01[j] : 0.f, v10 = k10[j] ? a10[j] : 0.f, v11 = k11[j] ? a11[j] : 0.f;
                const float gx = 1.f - fx[j], gy = 1.f - fy[j];
                r[j] = gy * (gx * v00 + fx[j] * v01) + fy[j] * (gx * v10 + fx[j] * v11);
            }
        }
        if (mean) {
            const float mu = mean[c], sd = stdv[c];
#pragma unroll
            for (int j = 0; j < 4; ++j) r[j] = (r[j] - mu) / sd;
        }
        GFN_GLOBAL float *oc = op + (long)c * Ho * Wo;
        if (VEC) {
            *reinterpret_cast<GFN_GLOBAL f32x4 *>(oc) = f32x4{r[0], r[1], r[2], r[3]};
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (u0 + j < Wo) oc[j] = r[j];
        }
    }
}

}  // namespace

GFN_EXPORT int gfn_perspective_from_points(const float *src, const float *dst, double *H, int *ok, int n, gfn_stream_t stream) {
    if (n < 0 || n > (1 << 24)) return gfn::fail(GFN_ERR_INVALID_ARG, "perspective_from_points: n = %d out of range", n);
    if (n == 0) return GFN_OK;
    if (!src || !dst || !H) return gfn::fail(GFN_ERR_INVALID_ARG, "perspective_from_points: null pointer");
    hipLaunchKernelGGL(pfp_kernel, dim3((unsigned)(((long)n * 8 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, src, dst, H, ok, n);
    return gfn::check_launch("pfp_kernel");
}

GFN_EXPORT int gfn_random_h_params(const int *draws, int B, int crop_size, int deform_area, int out_h, int out_w, int final_h,
                                   int final_w, float *H_s2t32, double *H_s2t64, double *M_A, double *M_B, int *ok, gfn_stream_t stream) {
    if (B < 0 || B > (1 << 24)) return gfn::fail(GFN_ERR_INVALID_ARG, "random_h_params: B = %d out of range", B);
    if (crop_size < 2 || deform_area < 0 || final_h < 1 || final_w < 1)
        return gfn::fail(GFN_ERR_INVALID_ARG, "random_h_params: bad size (crop %d, deform_area %d, final %d x %d)", crop_size, deform_area,
                         final_h, final_w);
    const int centre = crop_size - 2 * (deform_area / 2);
    if (out_h != centre || out_w != centre || centre < 2)
        return gfn::fail(GFN_ERR_INVALID_ARG, "random_h_params: the centre crop of a %d crop with deform_area %d is %d x %d (>= 2), got %d x %d",
                         crop_size, deform_area, centre, centre, out_h, out_w);
    if (B == 0) return GFN_OK;
    if (!draws) return gfn::fail(GFN_ERR_INVALID_ARG, "random_h_params: null draws");
    RhpParams P;
    P.draws = draws; P.H32 = H_s2t32; P.H64 = H_s2t64; P.MA = M_A; P.MB = M_B; P.ok = ok;
    P.B = B; P.crop = crop_size; P.deform = deform_area; P.out_h = out_h; P.out_w = out_w; P.final_h = final_h; P.final_w = final_w;
    hipLaunchKernelGGL(rhp_kernel, dim3((unsigned)(((long)B * 8 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, P);
    return gfn::check_launch("rhp_kernel");
}

GFN_EXPORT int gfn_warp_perspective_fwd(const float *const *src_planes, const int *src_dims, const double *M, int invert, float *out,
                                        int64_t out_bs, int B, int C, int Ho, int Wo, const float *mean, const float *std,
                                        gfn_stream_t stream) {
    if (B < 0 || B > 65535 || C < 1 || Ho < 0 || Wo < 0 || Ho > 32768 || Wo > 32768)
        return gfn::fail(GFN_ERR_INVALID_ARG, "warp_perspective: bad size (B %d <= 65535, C %d, output %d x %d <= 32768)", B, C, Ho, Wo);
    if ((mean == nullptr) != (std == nullptr)) return gfn::fail(GFN_ERR_INVALID_ARG, "warp_perspective: mean and std go together");
    if (B == 0 || Ho == 0 || Wo == 0) return GFN_OK;
    if (!src_planes || !src_dims || !M || !out) return gfn::fail(GFN_ERR_INVALID_ARG, "warp_perspective: null pointer");
    if (out_bs < (int64_t)C * Ho * Wo) return gfn::fail(GFN_ERR_INVALID_ARG, "warp_perspective: out_bs %lld < C * Ho * Wo", (long long)out_bs);
    const int tiles_x = (Wo + kWarpTile - 1) / kWarpTile, tiles_y = (Ho + kWarpTile - 1) / kWarpTile;
    const dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)B), block(256);
    // one 16-byte store per plane and lane where every group of four pixels starts on a 16-byte boundary
    const bool vec = Wo % 4 == 0 && out_bs % 4 == 0 && ((uintptr_t)out & 15) == 0;
    if (vec)
        hipLaunchKernelGGL(warp_perspective_kernel<true>, grid, block, 0, (hipStream_t)stream, src_planes, src_dims, M, invert, out,
                           (long)out_bs, C, Ho, Wo, tiles_x, mean, std);
    else
        hipLaunchKernelGGL(warp_perspective_kernel<false>, grid, block, 0, (hipStream_t)stream, src_planes, src_dims, M, invert, out,
                           (long)out_bs, C, Ho, Wo, tiles_x, mean, std);
    return gfn::check_launch("warp_perspective_kernel");
}
