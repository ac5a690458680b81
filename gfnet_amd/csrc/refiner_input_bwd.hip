// refiner_input_bwd.hip -- gfn_refiner_input_bwd: the backward of the refiner-input assembly (gfn_refiner_input_fwd*,
// refiner_input.h; reference: ConvRefiner.forward prefix, model/network.py:537-555, differentiated by torch autograd there).
//
//   d = cat(grid_feature = sample(x, cell centres), x_hat = sample(y, flow), emb = W (disp_scale (flow - centres)) + b, local_corr)
//
// Three launches, each skipped when nobody asked for its outputs:
//   refiner_input_bwd_cell_kernel   one thread per (sample, grid cell), lanes = consecutive cells of a grid row.  dflow (the
//                                   x_hat sample's derivative with respect to its coordinate plus W^T g_emb), dy (the adjoint of
//                                   the x_hat gather: a scatter along the flow, fp32 atomicAdd, one channel plane per
//                                   instruction) and the workgroup's partial sums of dW / db (fixed order, no atomics).
//   refiner_input_bwd_sum_kernel    second stage of dW / db: one workgroup per entry sums the partials in a fixed order.
//   refiner_input_bwd_dx_kernel     dx, the adjoint of sampling x at the cell centres, as a gather: one thread per (pixel, block
//                                   of 8 channels) visits the cells whose centre can lie within one pixel of it and adds the ones
//                                   that have it as a corner, in row-major cell order.  No atomics.
// Every sample set-up is gfn_sm::bilin_setup / Taps<GFN_SAMPLE_BILINEAR> (sample_modes.h), the forward's own arithmetic, and the
// cell centres are the forward's linspace_at values.  On the plain entry point only dy depends on the order in which atomics
// arrive.
//
// gfn_refiner_input_bwd_det makes dy a function of the multiset of its terms: the same launches with the scatter in 64-bit fixed
// point (integer addition commutes; the KDE column sums of kde.hip do the same), around them
//   refiner_input_bwd_det_scale_kernel   M_b = the largest finite |g| of a sample's x_hat planes, an integer atomicMax on its bits
//   refiner_input_bwd_det_finish_kernel  dy = (float)(acc * 2^-k_b), NaN where a non-finite term arrived (a flag bitmap)
// with k_b = 62 - E_b - ceil(log2(G * G)) and M_b < 2^E_b: the bilinear weights lie in [0, 1] and a cell reaches an element at most
// once, so |sum of term * 2^k_b| < 2^62 whatever the flow.
#include <algorithm>

#include "common.h"
#include "reduce.h"
#include "refiner_input.h"
#include "sample_modes.h"

namespace {

using gfn::wave_sum;

constexpr int kEmbChunk = 16;  // displacement-embedding channels reduced per barrier pair
constexpr int kDxChannels = 8; // channels per thread of the dx gather

struct RibArgs {
    const float *g;  // grad_d (B, 2C + Dd + K, G, G), batch stride d_bs
    long d_bs;
    const void *y;   // (B, C, Hs, Ws), fp32 or fp16
    const float *flow, *dw, *gf0;
    float *dx, *dy, *dflow, *part;  // part: (3 Dd, B * blocks per sample) partial sums, NULL when dW / db are not wanted
    int B, C, Hs, Ws, G, Dd;
    float disp_scale;
    // the deterministic dy (DET kernels only): 64-bit accumulators and a non-finite flag bit per dy element, max |g| bits per sample
    unsigned long long *acc;
    unsigned *flags;
    unsigned *maxbits;
    int lgg;  // ceil(log2(G * G))
};

// k_b of a sample from the bits of M_b > 0 (finite): M_b < 2^E as frexp gives it, subnormals included
__device__ __forceinline__ int det_shift(unsigned maxbits, int lgg) {
    const int e = (int)(maxbits >> 23);
    const int E = e > 0 ? e - 126 : 32 - __clz((int)maxbits) - 149;
    return 62 - E - lgg;
}
// 2^k as a double, k within [-1022, 1023] (det_shift gives [-128, 210] and its negation)
__device__ __forceinline__ double det_pow2(int k) { return __longlong_as_double((long long)(1023 + k) << 52); }

template <typename FT, bool DET>
__global__ __launch_bounds__(256) void refiner_input_bwd_cell_kernel(RibArgs q) {
    const int C = q.C, Hs = q.Hs, Ws = q.Ws, G = q.G, Dd = q.Dd;
    const unsigned plane = (unsigned)(Hs * Ws), GG = (unsigned)(G * G);
    const int b = (int)blockIdx.y;
    const unsigned id = blockIdx.x * 256u + threadIdx.x;
    const bool live = id < GG;                 // (dead lanes stay for the barriers and add zeros)
    const unsigned cell = live ? id : GG - 1u;
    const int i = (int)(cell / (unsigned)G), j = (int)(cell - (unsigned)i * (unsigned)G);
    const float lo = (float)(-1 + 1.0 / G), hi = (float)(1 - 1.0 / G);
    const float cx = gfn::linspace_at(lo, hi, G, j), cy = gfn::linspace_at(lo, hi, G, i);  // as refiner_input_cell
    const float *fl = q.flow + (size_t)b * 2 * GG;
    const float fx = fl[cell], fy = fl[GG + cell];
    const float *__restrict__ g = q.g + (size_t)b * q.d_bs;

    float gfx = 0.f, gfy = 0.f;
    if (q.dy || q.dflow) {
        gfn_sm::Taps<GFN_SAMPLE_BILINEAR> t;
        t.setup<GFN_PAD_ZEROS>(fx, fy, Ws, Hs);
        const gfn_sm::Bilin s = gfn_sm::bilin_setup<GFN_PAD_ZEROS>(fx, fy, Ws, Hs);
        const bool in[4] = {s.ya && s.xa, s.ya && s.xb, s.yb && s.xa, s.yb && s.xb};
        const bool any = in[0] | in[1] | in[2] | in[3];  // false for an insane cell (sane_floor): it gets the embedding term only
        const float ix = gfn_sm::unnorm(fx, Ws), iy = gfn_sm::unnorm(fy, Hs);
        const float tx = any ? ix - floorf(ix) : 0.f, ty = any ? iy - floorf(iy) : 0.f;
        const FT *__restrict__ yb = static_cast<const FT *>(q.y) + (size_t)b * C * plane;
        float *__restrict__ dyb = q.dy ? q.dy + (size_t)b * C * plane : nullptr;
        double fix = 0.0;  // DET: 2^k_b, or 0 when the sample has no finite non-zero gradient (every finite term is then 0)
        if (DET && dyb) {
            const unsigned mb = q.maxbits[b];
            if (mb) fix = det_pow2(det_shift(mb, q.lgg));
        }
        float ax = 0.f, ay = 0.f;
        for (int c0 = 0; c0 < C; c0 += 4) {
            float gv[4], v[4][4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int c = min(c0 + k, C - 1);
                gv[k] = g[(size_t)(C + c) * GG + cell];
                if (q.dflow) t.load(yb + (size_t)c * plane, v[k]);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (c0 + k >= C) break;
                if (dyb && live) {  // lanes = consecutive cells: under a smooth flow the four adds of a wave fall on neighbouring pixels
                    float *pl = dyb + (size_t)(c0 + k) * plane;
#pragma unroll
                    for (int n = 0; n < 4; ++n) {
                        if (!in[n]) continue;
                        const float term = t.w[n] * gv[k];
                        if (!DET) {
                            atomicAdd(pl + t.o[n], term);
                        } else {
                            const size_t e = (size_t)(pl - q.dy) + (size_t)t.o[n];
                            if (!(fabsf(term) <= 3.402823466e38f)) atomicOr(q.flags + (e >> 5), 1u << (unsigned)(e & 31));
                            else if (fix != 0.0) atomicAdd(q.acc + e, (unsigned long long)llrint((double)term * fix));  // wraps: two's complement
                        }
                    }
                }
                if (q.dflow) {
                    const float v0 = in[0] ? v[k][0] : 0.f, v1 = in[1] ? v[k][1] : 0.f, v2 = in[2] ? v[k][2] : 0.f, v3 = in[3] ? v[k][3] : 0.f;
                    ax += gv[k] * ((v1 - v0) * (1.f - ty) + (v3 - v2) * ty);
                    ay += gv[k] * ((v2 - v0) * (1.f - tx) + (v3 - v1) * tx);
                }
            }
        }
        // grid_sample un-normalises with ((g + 1) W - 1) / 2: d ix / d g = W / 2
        gfx = any ? ax * (0.5f * (float)Ws) : 0.f;
        gfy = any ? ay * (0.5f * (float)Hs) : 0.f;
    }

    if (Dd > 0 && (q.dflow || q.part)) {
        __shared__ float red[4][3 * kEmbChunk];
        const float ex = fx - cx, ey = fy - cy;  // the forward's flow - im_A_coords
        const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
        const unsigned nblk = gridDim.x * gridDim.y, blk = (unsigned)b * gridDim.x + blockIdx.x;
        float ex_w = 0.f, ey_w = 0.f;
        for (int j0 = 0; j0 < Dd; j0 += kEmbChunk) {
            const int nj = min(kEmbChunk, Dd - j0);
            for (int jj = 0; jj < nj; ++jj) {
                const float ge = live ? g[(size_t)(2 * C + j0 + jj) * GG + cell] : 0.f;
                ex_w += q.dw[(j0 + jj) * 2 + 0] * ge;
                ey_w += q.dw[(j0 + jj) * 2 + 1] * ge;
                if (q.part) {
                    const float sx = wave_sum(ge * ex), sy = wave_sum(ge * ey), sb = wave_sum(ge);
                    if (lane == 0) {
                        red[wave][3 * jj + 0] = sx;
                        red[wave][3 * jj + 1] = sy;
                        red[wave][3 * jj + 2] = sb;
                    }
                }
            }
            if (q.part) {
                __syncthreads();
                if ((int)threadIdx.x < 3 * nj) {
                    const int jj = (int)threadIdx.x / 3, k = (int)threadIdx.x - 3 * jj;
                    const float sum = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
                    q.part[(size_t)(k * Dd + j0 + jj) * nblk + blk] = sum;
                }
                __syncthreads();
            }
        }
        gfx += q.disp_scale * ex_w;
        gfy += q.disp_scale * ey_w;
    }
    if (q.dflow && live) {
        float *o = q.dflow + (size_t)b * 2 * GG;
        o[cell] = gfx;
        o[GG + cell] = gfy;
    }
}

// M_b: the largest finite |g| over grad_d[b, C:2C] (contiguous), as its bit pattern -- unsigned order is magnitude order there
__global__ __launch_bounds__(256) void refiner_input_bwd_det_scale_kernel(RibArgs q) {
    const int b = (int)blockIdx.y;
    const size_t n = (size_t)q.C * (size_t)q.G * (size_t)q.G;
    const float *__restrict__ g = q.g + (size_t)b * q.d_bs + n;
    unsigned m = 0u;
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (size_t)gridDim.x * 256u) {
        const unsigned bits = __float_as_uint(g[i]) & 0x7fffffffu;
        if (bits < 0x7f800000u) m = max(m, bits);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o));
    if ((threadIdx.x & 63u) == 0 && m) atomicMax(q.maxbits + b, m);
}

__global__ __launch_bounds__(256) void refiner_input_bwd_det_finish_kernel(RibArgs q) {
    const size_t per = (size_t)q.C * (size_t)q.Hs * (size_t)q.Ws;
    const int b = (int)blockIdx.y;
    const unsigned mb = q.maxbits[b];
    const double inv = mb ? det_pow2(-det_shift(mb, q.lgg)) : 0.0;
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < per; i += (size_t)gridDim.x * 256u) {
        const size_t e = (size_t)b * per + i;
        const bool bad = (q.flags[e >> 5] >> (unsigned)(e & 31)) & 1u;
        const float v = (float)((double)(long long)q.acc[e] * inv);  // exact product (a power of two), one rounding to fp32
        q.dy[e] = bad ? __uint_as_float(0x7fc00000u) : v;
    }
}

// dW[j, k] = disp_scale * sum of row k * Dd + j (k = 0, 1), db[j] = sum of row 2 * Dd + j; one workgroup per row
__global__ __launch_bounds__(256) void refiner_input_bwd_sum_kernel(const float *__restrict__ part, unsigned nblk, int Dd, float disp_scale,
                                                                    float *__restrict__ ddw, float *__restrict__ ddb) {
    __shared__ float red[256];
    const unsigned row = blockIdx.x;
    const float *p = part + (size_t)row * nblk;
    float s = 0.f;
    for (unsigned n = threadIdx.x; n < nblk; n += 256u) s += p[n];
    red[threadIdx.x] = s;
    __syncthreads();
    for (unsigned m = 128; m >= 1; m >>= 1) {
        if (threadIdx.x < m) red[threadIdx.x] += red[threadIdx.x + m];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const int k = (int)row / Dd, j = (int)row - k * Dd;
        if (k < 2) {
            if (ddw) ddw[j * 2 + k] = disp_scale * red[0];
        } else if (ddb) {
            ddb[j] = red[0];
        }
    }
}

// The cell centres are ix(i) = (i + 1/2) Ws / G - 1/2 pixels (grid_sample's un-normalisation of linspace(-1 + 1/G, 1 - 1/G, G)),
// so the cells with a corner at pixel p are those with p - 1 < ix(i) < p + 1.  The range below is that interval in closed form,
// widened by one cell on each side against the rounding of the forward's fp32 centres; whether a candidate really has the pixel as
// a corner, and with which weight, is decided by the forward's own set-up.
__device__ __forceinline__ void dx_candidates(int p, int size, int G, int &first, int &last) {
    const float r = (float)G / (float)size;
    first = max(0, (int)floorf(((float)p - 0.5f) * r - 0.5f) - 1);
    last = min(G - 1, (int)ceilf(((float)p + 1.5f) * r - 0.5f) + 1);
}

__global__ __launch_bounds__(256) void refiner_input_bwd_dx_kernel(RibArgs q) {
    const int C = q.C, Hs = q.Hs, Ws = q.Ws, G = q.G;
    const unsigned plane = (unsigned)(Hs * Ws), GG = (unsigned)(G * G);
    const int b = (int)blockIdx.y, c0 = (int)blockIdx.z * kDxChannels;
    const unsigned pix = blockIdx.x * 256u + threadIdx.x;
    if (pix >= plane) return;
    const int py = (int)(pix / (unsigned)Ws), px = (int)(pix - (unsigned)py * (unsigned)Ws);
    const float lo = (float)(-1 + 1.0 / G), hi = (float)(1 - 1.0 / G);
    int i0, i1, j0, j1;
    dx_candidates(py, Hs, G, i0, i1);
    dx_candidates(px, Ws, G, j0, j1);
    const int nc = min(kDxChannels, C - c0);
    const float *__restrict__ g = q.g + (size_t)b * q.d_bs + (size_t)c0 * GG;
    const float *__restrict__ gf0 = q.gf0 ? q.gf0 + ((size_t)b * C + c0) * GG : nullptr;
    float acc[kDxChannels];
#pragma unroll
    for (int k = 0; k < kDxChannels; ++k) acc[k] = 0.f;
    for (int i = i0; i <= i1; ++i) {
        const float cy = gfn::linspace_at(lo, hi, G, i);
        for (int j = j0; j <= j1; ++j) {
            const float cx = gfn::linspace_at(lo, hi, G, j);
            const gfn_sm::Bilin s = gfn_sm::bilin_setup<GFN_PAD_ZEROS>(cx, cy, Ws, Hs);
            const unsigned ox = (unsigned)(px - s.x0), oy = (unsigned)(py - s.y0);  // 0 or 1: the pixel is a corner of this cell
            if (ox > 1u || oy > 1u) continue;
            const float w = oy ? (ox ? s.w11 : s.w10) : (ox ? s.w01 : s.w00);
            const unsigned cell = (unsigned)i * (unsigned)G + (unsigned)j;
#pragma unroll
            for (int k = 0; k < kDxChannels; ++k) {
                if (k < nc) {
                    float gv = g[(size_t)k * GG + cell];
                    if (gf0) gv += gf0[(size_t)k * GG + cell];
                    acc[k] += w * gv;
                }
            }
        }
    }
    float *o = q.dx + ((size_t)b * C + c0) * plane + pix;
#pragma unroll
    for (int k = 0; k < kDxChannels; ++k)
        if (k < nc) o[(size_t)k * plane] = acc[k];
}

inline unsigned cell_blocks(int G) { return (unsigned)(((long)G * G + 255) / 256); }

// The deterministic workspace: one 64-bit accumulator per dy element, one flag bit per element in 32-bit words, one 32-bit word per
// sample; each of the three parts a multiple of 8 bytes.
struct DetLayout {
    int64_t acc_bytes, flag_bytes, max_bytes;
    int64_t total() const { return acc_bytes + flag_bytes + max_bytes; }
};
inline DetLayout det_layout(int B, int C, int Hs, int Ws) {
    const int64_t n = (int64_t)B * C * Hs * Ws;
    return {n * 8, ((n + 31) / 32 * 4 + 7) / 8 * 8, ((int64_t)B * 4 + 7) / 8 * 8};
}

// Both entry points.  det: dy through the fixed-point accumulators of `ws`; everything else is the same launches on the same arguments.
int refiner_input_bwd_run(const char *what, bool det, const float *grad_d, int64_t d_bs, const void *f1, int dtype, const float *flow,
                          const float *disp_w, const float *gf0, float *dx, float *dy, float *dflow, float *ddisp_w, float *ddisp_b, int B,
                          int C, int Hs, int Ws, int G, int disp_dim, int K, float disp_scale, void *scratch, int64_t scratch_bytes, void *ws,
                          int64_t ws_bytes, gfn_stream_t stream) {
    if (dtype != GFN_F32 && dtype != GFN_F16) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: feature dtype must be GFN_F32 or GFN_F16", what);
    if (!grad_d || !f1 || !flow || (disp_dim > 0 && !disp_w)) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: null pointer", what);
    if (B < 0 || C <= 0 || Hs <= 0 || Ws <= 0 || G <= 0 || disp_dim < 0 || K < 0 || (long)C * Hs * Ws >= (1L << 31) ||
        d_bs < ((int64_t)2 * C + disp_dim + K) * G * G)
        return gfn::fail(GFN_ERR_INVALID_ARG, "%s: bad size", what);
    if (B > 0 && (B > 65535 || (long)G * G >= (1L << 31) || C > kDxChannels * 65535))
        return gfn::fail(GFN_ERR_INVALID_ARG, "%s: batch > 65535, grid too large or too many channels", what);
    const bool sums = disp_dim > 0 && (ddisp_w || ddisp_b);
    if (sums && (!scratch || scratch_bytes < gfn_refiner_input_bwd_scratch_bytes(B, G, disp_dim)))
        return gfn::fail(GFN_ERR_SCRATCH, "%s: scratch too small (%lld bytes needed)", what,
                         (long long)gfn_refiner_input_bwd_scratch_bytes(B, G, disp_dim));
    det = det && dy;
    const DetLayout lay = det_layout(B, C, Hs, Ws);
    if (det && B > 0 && (!ws || ((uintptr_t)ws & 7) || ws_bytes < lay.total()))
        return gfn::fail(GFN_ERR_SCRATCH, "%s: ws must be 8-byte aligned and hold %lld bytes", what, (long long)lay.total());
    if (B == 0) return GFN_OK;
    hipStream_t st = (hipStream_t)stream;
    RibArgs q;
    q.g = grad_d; q.d_bs = (long)d_bs; q.y = f1; q.flow = flow; q.dw = disp_w; q.gf0 = gf0;
    q.dx = dx; q.dy = dy; q.dflow = dflow; q.part = sums ? static_cast<float *>(scratch) : nullptr;
    q.B = B; q.C = C; q.Hs = Hs; q.Ws = Ws; q.G = G; q.Dd = disp_dim; q.disp_scale = disp_scale;
    q.acc = nullptr; q.flags = nullptr; q.maxbits = nullptr; q.lgg = 0;
    const unsigned qb = cell_blocks(G);
    if (det) {  // accumulators, flags and the per-sample maxima all start at zero
        char *w = static_cast<char *>(ws);
        q.acc = reinterpret_cast<unsigned long long *>(w);
        q.flags = reinterpret_cast<unsigned *>(w + lay.acc_bytes);
        q.maxbits = reinterpret_cast<unsigned *>(w + lay.acc_bytes + lay.flag_bytes);
        while ((1L << q.lgg) < (long)G * G) ++q.lgg;
        const hipError_t e = hipMemsetAsync(ws, 0, (size_t)lay.total(), st);
        if (e != hipSuccess) return gfn::fail(GFN_ERR_LAUNCH, "%s: hipMemsetAsync: %s", what, hipGetErrorString(e));
        const size_t n = (size_t)C * G * G;
        hipLaunchKernelGGL(refiner_input_bwd_det_scale_kernel, dim3((unsigned)std::min<size_t>((n + 1023) / 1024, 1024), (unsigned)B), dim3(256), 0,
                           st, q);
        if (int e2 = gfn::check_launch("refiner_input_bwd_det_scale_kernel")) return e2;
    } else if (dy) {  // the scatter adds into it
        const hipError_t e = hipMemsetAsync(dy, 0, (size_t)B * C * Hs * Ws * sizeof(float), st);
        if (e != hipSuccess) return gfn::fail(GFN_ERR_LAUNCH, "%s: hipMemsetAsync: %s", what, hipGetErrorString(e));
    }
    if (dy || dflow || sums) {
        const dim3 grid(qb, (unsigned)B);
        if (det) {
            if (dtype == GFN_F16) hipLaunchKernelGGL((refiner_input_bwd_cell_kernel<_Float16, true>), grid, dim3(256), 0, st, q);
            else hipLaunchKernelGGL((refiner_input_bwd_cell_kernel<float, true>), grid, dim3(256), 0, st, q);
        } else {
            if (dtype == GFN_F16) hipLaunchKernelGGL((refiner_input_bwd_cell_kernel<_Float16, false>), grid, dim3(256), 0, st, q);
            else hipLaunchKernelGGL((refiner_input_bwd_cell_kernel<float, false>), grid, dim3(256), 0, st, q);
        }
        if (int e = gfn::check_launch("refiner_input_bwd_cell_kernel")) return e;
    }
    if (det) {
        const size_t per = (size_t)C * Hs * Ws;
        hipLaunchKernelGGL(refiner_input_bwd_det_finish_kernel, dim3((unsigned)std::min<size_t>((per + 255) / 256, 4096), (unsigned)B), dim3(256),
                           0, st, q);
        if (int e = gfn::check_launch("refiner_input_bwd_det_finish_kernel")) return e;
    }
    if (sums) {
        hipLaunchKernelGGL(refiner_input_bwd_sum_kernel, dim3(3u * (unsigned)disp_dim), dim3(256), 0, st, q.part, qb * (unsigned)B, disp_dim,
                           disp_scale, ddisp_w, ddisp_b);
        if (int e = gfn::check_launch("refiner_input_bwd_sum_kernel")) return e;
    }
    if (dx) {
        const dim3 grid((unsigned)(((long)Hs * Ws + 255) / 256), (unsigned)B, (unsigned)((C + kDxChannels - 1) / kDxChannels));
        hipLaunchKernelGGL(refiner_input_bwd_dx_kernel, grid, dim3(256), 0, st, q);
        if (int e = gfn::check_launch("refiner_input_bwd_dx_kernel")) return e;
    }
    return GFN_OK;
}

}  // namespace

GFN_EXPORT int64_t gfn_refiner_input_bwd_scratch_bytes(int B, int G, int disp_dim) {
    if (B <= 0 || G <= 0 || disp_dim < 0) return 0;
    return (int64_t)B * cell_blocks(G) * 3 * (disp_dim > 0 ? disp_dim : 1) * (int64_t)sizeof(float);
}

GFN_EXPORT int gfn_refiner_input_bwd(const float *grad_d, int64_t d_bs, const void *f1, int dtype, const float *flow, const float *disp_w,
                                     const float *gf0, float *dx, float *dy, float *dflow, float *ddisp_w, float *ddisp_b, int B, int C,
                                     int Hs, int Ws, int G, int disp_dim, int K, float disp_scale, void *scratch, int64_t scratch_bytes,
                                     gfn_stream_t stream) {
    return refiner_input_bwd_run("refiner_input_bwd", false, grad_d, d_bs, f1, dtype, flow, disp_w, gf0, dx, dy, dflow, ddisp_w, ddisp_b, B, C,
                                 Hs, Ws, G, disp_dim, K, disp_scale, scratch, scratch_bytes, nullptr, 0, stream);
}

GFN_EXPORT int64_t gfn_refiner_input_bwd_det_ws_bytes(int B, int C, int Hs, int Ws) {
    if (B <= 0 || C <= 0 || Hs <= 0 || Ws <= 0) return 0;
    return det_layout(B, C, Hs, Ws).total();
}

GFN_EXPORT int gfn_refiner_input_bwd_det(const float *grad_d, int64_t d_bs, const void *f1, int dtype, const float *flow,
                                         const float *disp_w, const float *gf0, float *dx, float *dy, float *dflow, float *ddisp_w,
                                         float *ddisp_b, int B, int C, int Hs, int Ws, int G, int disp_dim, int K, float disp_scale,
                                         void *scratch, int64_t scratch_bytes, void *ws, int64_t ws_bytes, gfn_stream_t stream) {
    return refiner_input_bwd_run("refiner_input_bwd_det", true, grad_d, d_bs, f1, dtype, flow, disp_w, gf0, dx, dy, dflow, ddisp_w, ddisp_b, B,
                                 C, Hs, Ws, G, disp_dim, K, disp_scale, scratch, scratch_bytes, ws, ws_bytes, stream);
}
