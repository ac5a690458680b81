// One FPN layer in TRAINING mode, forward and backward (include/gfnet_hip.h: gfn_conv2d_bn_act_train_fwd / _bwd; reference
// model/FPN.py:95-128, :43-66 and model/network.py:66, 182 under model.train(), which torch autograd differentiates there):
//
//     u = conv(cat(x0, x1), weight)      mean, invstd of u over the batch      out = act(bn_w (u - mean) invstd + bn_b) + residual
//
// Only u is kept for the backward; the activation's derivative is recomputed from u, mean and invstd with the forward's expression.
// With up0 (the gfn_conv2d_up_bn_act_train_* entry points; stride 1) x0 is (B, C0, H/2, W/2) and stands for its 2x bilinear upsample
// x0' in both directions: the doubled map is never written, and gx0 comes back at the coarse size.
//
// Forward (5 launches): ones / zeros for the shared convolution kernels; u by fpn_conv.hip's kernels (fpn_conv_launch.h) with
// scale 1 and shift 0; ft_moments_kernel, a workgroup per 4096 values of one channel plane: (mean, M2) about its own mean;
// ft_stats_kernel, a wave per channel: Chan's merge in double (conv_train_common.h), mean, invstd and the running buffers;
// ft_apply_kernel, elementwise, float4 where the planes allow it.
// Backward, each launch only where `need` asks for what it makes:
//   ft_bn_bwd_part_kernel   per 4096 values of a plane: sum ga and sum ga x_hat with ga = gy act'(.)     -> ct_bn_bwd_kernel (double)
//   ft_gu_kernel            gu = bn_w invstd (ga - S1/n - x_hat S2/n), written once into the workspace
//   input gradient          stride 1: the forward convolution kernels on gu with the weights transposed and flipped on the device
//                           (ft_repack_kernel), one launch per input (gx0, gx1: the concatenation is never written); with up0 the
//                           launch for x0 writes the gradient of x0' into the workspace and ft_up2_adjoint_kernel gathers gx0 from
//                           it: the transposed upsample, 16 taps per coarse value in a fixed order;
//                           stride 2: ft_gather_s2_kernel, a workgroup per output parity class, so the taps it visits are uniform
//   weight gradient         ft_wgrad_kernel: a workgroup stages the halo tile of up to CIG input channels and the 8 x 32 tile of gu
//                           of 8 output channels in LDS; a thread owns one (ci, ky, kx) and 8 output channels, sums runs of 32
//                           positions in fp32 and adds the runs up; a workgroup walks every P-th tile and leaves one partial
//                           (Cout, Cin, K, K); ft_wsum_kernel adds the P partials in double, in order.  With up0 the coarse
//                           footprint of the tile goes into LDS first and the halo tile of an x0 channel is interpolated from it
//                           with up2_at's operations (fpn_conv_launch.h), so that it holds what the forward's staging held.
// Every sum has a fixed order and there are no floating-point atomics: identical calls give identical bits.
// The TF32 class (gfn_conv2d_bn_act_train_tf32_*): the same launches with u and the stride-1 input gradient by fpn_conv_tf32.hip's
// kernels wherever the launch's output channels are a multiple of 8 (conv() below), and the weight gradient under stride 1 without up0
// by that file's wgrad_tf32_kernel (the same partials, the same ft_wsum_kernel); ft_gather_s2_kernel, ft_wgrad_kernel under stride 2 and
// up0, and the BatchNorm passes are reused as they are, so those gradients stay exact fp32.
#include <algorithm>

#include "conv_train_common.h"
#include "fpn_conv_launch.h"

namespace {

using gfn::activate;
using gfn::ConvArgs;

constexpr int kEw = 1024;      // values per workgroup of the elementwise kernels (4 per thread)
constexpr int kRed = 4096;     // values per workgroup of the plane reductions (16 per thread)
constexpr int kWgTH = 8, kWgTW = 32, kWgPos = kWgTH * kWgTW, kWgCo = 8;  // weight gradient: output tile, output channels per workgroup
constexpr int kWgXFloats = 10240;                                          // ... and the LDS floats its input halo tiles may take
constexpr int kWgMaxParts = 512;                                           // partial weight gradients at most,
constexpr int64_t kWgPartFloats = (int64_t)4 << 20;                        // and floats of them at most (16 MiB)

// d act(z) / dz with the forward's own sigmoid expression
__device__ __forceinline__ float act_grad(float z, int act, float slope) {
    if (act == 1) return z > 0.f ? 1.f : slope;
    if (act == 2) {
        const float sg = 1.f / (1.f + expf(-z));
        return sg * (1.f + z * (1.f - sg));
    }
    return 1.f;
}

struct PlaneChunk {
    int c, b, chunk;
    int64_t base;  // of the plane (b, c) in a (B, C, HW) map
};
__device__ __forceinline__ PlaneChunk decode_chunk(unsigned bid, int C, int HW, int chunks) {
    PlaneChunk p;
    p.chunk = (int)(bid % (unsigned)chunks);
    const unsigned pl = bid / (unsigned)chunks;
    p.c = (int)(pl % (unsigned)C);
    p.b = (int)(pl / (unsigned)C);
    p.base = (int64_t)pl * HW;
    return p;
}

__global__ __launch_bounds__(64) void ft_identity_kernel(float *ident, int n) {  // ident[0 .. n) = 1, [n .. 2n) = 0
    for (int i = threadIdx.x; i < n; i += 64) ident[i] = 1.f, ident[n + i] = 0.f;
}

// (mean, M2 = sum (u - mean)^2) of up to kRed values of one plane: part (C, B * chunks, 2)
__global__ __launch_bounds__(256) void ft_moments_kernel(const float *__restrict__ u, float *__restrict__ part, int C, int HW, int chunks,
                                                         int nparts) {
    __shared__ float red[4];
    const int tid = threadIdx.x;
    const PlaneChunk pc = decode_chunk(blockIdx.x, C, HW, chunks);
    const int e0 = pc.chunk * kRed, cnt = min(kRed, HW - e0);
    const float *__restrict__ p = u + pc.base + e0;
    float v[kRed / 256], s = 0.f;
#pragma unroll
    for (int q = 0; q < kRed / 256; ++q) {
        const int i = tid + q * 256;
        v[q] = i < cnt ? p[i] : 0.f;
        s += v[q];
    }
    const float mt = block_sum(s, red) / (float)cnt;
    float d = 0.f;
#pragma unroll
    for (int q = 0; q < kRed / 256; ++q) d += tid + q * 256 < cnt ? (v[q] - mt) * (v[q] - mt) : 0.f;
    const float m2 = block_sum(d, red);
    if (tid == 0) {
        float *o = part + ((int64_t)pc.c * nparts + (int64_t)pc.b * chunks + pc.chunk) * 2;
        o[0] = mt, o[1] = m2;
    }
}

// one wave per channel: the chunks' moments -> mean, invstd (biased variance), the running buffers as torch updates them.  The conv
// bias is not in u: it shifts the batch mean that running_mean tracks and nothing else
__global__ __launch_bounds__(64) void ft_stats_kernel(const float *__restrict__ part, const float *__restrict__ conv_bias, float *__restrict__ mean,
                                                      float *__restrict__ invstd, float *__restrict__ running_mean, float *__restrict__ running_var,
                                                      int HW, int chunks, int nparts, double momentum, double eps) {
    __shared__ double sn[64], sm[64], s2[64];
    const int c = blockIdx.x, lane = threadIdx.x;
    Moments a = {0.0, 0.0, 0.0};
    for (int i = lane; i < nparts; i += 64) {
        const float *p = part + ((int64_t)c * nparts + i) * 2;
        const Moments b = {(double)min(kRed, HW - (i % chunks) * kRed), (double)p[0], (double)p[1]};
        merge(a, b);
    }
    sn[lane] = a.n, sm[lane] = a.mean, s2[lane] = a.m2;
    __syncthreads();
    for (int s = 32; s >= 1; s >>= 1) {
        if (lane < s) {
            Moments p = {sn[lane], sm[lane], s2[lane]};
            const Moments q = {sn[lane + s], sm[lane + s], s2[lane + s]};
            merge(p, q);
            sn[lane] = p.n, sm[lane] = p.mean, s2[lane] = p.m2;
        }
        __syncthreads();
    }
    if (lane == 0) {
        const double n = sn[0], mu = sm[0], var = s2[0] / n;
        mean[c] = (float)mu;
        invstd[c] = (float)(1.0 / sqrt(var + eps));
        const double bias = conv_bias ? (double)conv_bias[c] : 0.0;
        running_mean[c] = (float)((1.0 - momentum) * (double)running_mean[c] + momentum * (mu + bias));
        running_var[c] = (float)((1.0 - momentum) * (double)running_var[c] + momentum * (s2[0] / (n - 1.0)));
    }
}

// out = act(u alpha + beta') + residual; VEC: planes of a multiple of 4 values behind 16-byte aligned pointers
template <bool VEC>
__global__ __launch_bounds__(256) void ft_apply_kernel(const float *__restrict__ u, const float *__restrict__ bn_w, const float *__restrict__ bn_b,
                                                       const float *__restrict__ mean, const float *__restrict__ invstd,
                                                       const float *residual, float *out, int C, int HW, int chunks, int act, float slope) {
    const int tid = threadIdx.x;
    const PlaneChunk pc = decode_chunk(blockIdx.x, C, HW, chunks);
    float al, be;
    bn_affine(bn_w[pc.c], bn_b[pc.c], mean[pc.c], invstd[pc.c], al, be);
    if (VEC) {
        const int i = pc.chunk * kEw + tid * 4;
        if (i >= HW) return;
        const float4 uu = *reinterpret_cast<const float4 *>(u + pc.base + i);
        float4 r = {0.f, 0.f, 0.f, 0.f};
        if (residual) r = *reinterpret_cast<const float4 *>(residual + pc.base + i);
        float4 o;
        o.x = activate(bn_pre(uu.x, al, be), act, slope) + r.x;
        o.y = activate(bn_pre(uu.y, al, be), act, slope) + r.y;
        o.z = activate(bn_pre(uu.z, al, be), act, slope) + r.z;
        o.w = activate(bn_pre(uu.w, al, be), act, slope) + r.w;
        *reinterpret_cast<float4 *>(out + pc.base + i) = o;
    } else {
#pragma unroll
        for (int q = 0; q < kEw / 256; ++q) {
            const int i = pc.chunk * kEw + tid + q * 256;
            if (i >= HW) continue;
            float v = activate(bn_pre(u[pc.base + i], al, be), act, slope);
            if (residual) v += residual[pc.base + i];
            out[pc.base + i] = v;
        }
    }
}

// (sum ga, sum ga x_hat) of up to kRed values of one plane, ga = gy act'(u alpha + beta'): part (C, B * chunks, 2) as ct_bn_bwd_kernel reads it
__global__ __launch_bounds__(256) void ft_bn_bwd_part_kernel(const float *__restrict__ gy, const float *__restrict__ u, const float *__restrict__ bn_w,
                                                             const float *__restrict__ bn_b, const float *__restrict__ mean,
                                                             const float *__restrict__ invstd, float *__restrict__ part, int C, int HW, int chunks,
                                                             int nparts, int act, float slope) {
    __shared__ float red[4];
    const int tid = threadIdx.x;
    const PlaneChunk pc = decode_chunk(blockIdx.x, C, HW, chunks);
    const float mn = mean[pc.c], is = invstd[pc.c];
    float al, be;
    bn_affine(bn_w[pc.c], bn_b[pc.c], mn, is, al, be);
    const int e0 = pc.chunk * kRed, cnt = min(kRed, HW - e0);
    const float *__restrict__ gp = gy + pc.base + e0;
    const float *__restrict__ up = u + pc.base + e0;
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int q = 0; q < kRed / 256; ++q) {
        const int i = tid + q * 256;
        if (i < cnt) {
            const float uu = up[i], ga = gp[i] * act_grad(bn_pre(uu, al, be), act, slope);
            s1 += ga;
            s2 += ga * ((uu - mn) * is);
        }
    }
    s1 = block_sum(s1, red);
    s2 = block_sum(s2, red);
    if (tid == 0) {
        float *o = part + ((int64_t)pc.c * nparts + (int64_t)pc.b * chunks + pc.chunk) * 2;
        o[0] = s1, o[1] = s2;
    }
}

// gu = alpha (ga - dbeta / n - x_hat dgamma / n); dgdb (2, C) = dgamma, dbeta
__global__ __launch_bounds__(256) void ft_gu_kernel(const float *__restrict__ gy, const float *__restrict__ u, const float *__restrict__ bn_w,
                                                    const float *__restrict__ bn_b, const float *__restrict__ mean, const float *__restrict__ invstd,
                                                    const float *__restrict__ dgdb, float *__restrict__ gu, int C, int HW, int chunks, float inv_n,
                                                    int act, float slope) {
    const int tid = threadIdx.x;
    const PlaneChunk pc = decode_chunk(blockIdx.x, C, HW, chunks);
    const float mn = mean[pc.c], is = invstd[pc.c];
    float al, be;
    bn_affine(bn_w[pc.c], bn_b[pc.c], mn, is, al, be);
    const float k1 = dgdb[C + pc.c] * inv_n, k2 = dgdb[pc.c] * inv_n;
#pragma unroll
    for (int q = 0; q < kEw / 256; ++q) {
        const int i = pc.chunk * kEw + tid + q * 256;
        if (i >= HW) continue;
        const float uu = u[pc.base + i], ga = gy[pc.base + i] * act_grad(bn_pre(uu, al, be), act, slope);
        gu[pc.base + i] = al * (ga - k1 - ((uu - mn) * is) * k2);
    }
}

// wt (Cin, Cout, K, K) = weight (Cout, Cin, K, K) transposed, every plane turned by 180 degrees
__global__ __launch_bounds__(256) void ft_repack_kernel(const float *__restrict__ w, float *__restrict__ wt, int Cout, int Cin, int KK) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)Cout * Cin * KK) return;
    const int k = (int)(e % KK), ci = (int)(e / KK % Cin), co = (int)(e / ((int64_t)KK * Cin));
    wt[((int64_t)ci * Cout + co) * KK + (KK - 1 - k)] = w[e];
}

// The transposed 2x upsample along one axis: coarse index c of n gets the doubled grid's entries 2c - 1 .. 2c + 2 with the weights
// 1/4, 3/4, 3/4, 1/4 (up2_taps: entry 2m + 1 reads m and m + 1 with 3/4 and 1/4, entry 2m reads m - 1 and m with 1/4 and 3/4).  The
// two clamps fold the border onto the first and last index: entry 0 reads index 0 alone, entry 2n - 1 reads index n - 1 twice.  An
// entry outside the grid gets weight 0 and an index inside it.
__device__ __forceinline__ void up2_adjoint_taps(int c, int n, int idx[4], float wt[4]) {
    idx[0] = max(2 * c - 1, 0), wt[0] = c > 0 ? 0.25f : 0.f;
    idx[1] = 2 * c, wt[1] = c > 0 ? 0.75f : 1.f;
    idx[2] = 2 * c + 1, wt[2] = c < n - 1 ? 0.75f : 1.f;
    idx[3] = min(2 * c + 2, 2 * n - 1), wt[3] = c < n - 1 ? 0.25f : 0.f;
}

// gx (planes of h2 x w2) = the transposed upsample of gf (planes of 2 h2 x 2 w2): a thread per coarse value gathers its 4 x 4 taps,
// columns within a row, then the rows, always in that order.  The weights and their products are exact in fp32.
__global__ __launch_bounds__(256) void ft_up2_adjoint_kernel(const float *__restrict__ gf, float *__restrict__ gx, int64_t total, int h2, int w2) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int cx = (int)(e % w2), cy = (int)(e / w2 % h2);
    const float *__restrict__ p = gf + (e / ((int64_t)w2 * h2)) * (4 * (int64_t)h2 * w2);
    int iy[4], ix[4];
    float wy[4], wx[4];
    up2_adjoint_taps(cy, h2, iy, wy);
    up2_adjoint_taps(cx, w2, ix, wx);
    float acc = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float *__restrict__ row = p + (int64_t)iy[r] * (2 * w2);
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) s = fmaf(wx[k], row[ix[k]], s);
        acc = fmaf(wy[r], s, acc);
    }
    gx[e] = acc;
}

// Stride 2: gx[ci][y][x] = sum_co sum over the taps (ky, kx) with the parity of (y + pad, x + pad) of gu[co][(y + pad - ky) / 2][..]
// w[co][ci][ky][kx].  A workgroup serves 256 positions of ONE parity class (y & 1, x & 1) of one input plane, so its taps and with
// them its weight addresses are uniform.  Four output channels to a partial sum where there are more than 32 (fpn_conv.hip: SPLIT).
__global__ __launch_bounds__(256) void ft_gather_s2_kernel(const float *__restrict__ gu, const float *__restrict__ w, float *__restrict__ gx0,
                                                           float *__restrict__ gx1, int C0, int C1, int H, int W, int Cout, int Ho, int Wo,
                                                           int K, int chunks) {
    unsigned bid = blockIdx.x;
    const int chunk = (int)(bid % (unsigned)chunks);
    bid /= (unsigned)chunks;
    const int cls = (int)(bid & 3u);
    bid >>= 2;
    const int Cin = C0 + C1, ci = (int)(bid % (unsigned)Cin), b = (int)(bid / (unsigned)Cin);
    const int py = cls >> 1, px = cls & 1, pad = K / 2;
    const int Hp = (H - py + 1) >> 1, Wp = (W - px + 1) >> 1;  // rows and columns of this class
    const int i = chunk * 256 + (int)threadIdx.x;
    if (i >= Hp * Wp) return;
    const int y = 2 * (i / Wp) + py, x = 2 * (i % Wp) + px;
    const int ky0 = (y + pad) & 1, kx0 = (x + pad) & 1;  // uniform over the workgroup
    const float *__restrict__ gb = gu + (int64_t)b * Cout * Ho * Wo;
    float acc = 0.f, total = 0.f;
    for (int co = 0; co < Cout; ++co) {
        const float *__restrict__ wc = w + ((int64_t)co * Cin + ci) * (K * K);
        const float *__restrict__ gp = gb + (int64_t)co * Ho * Wo;
        for (int ky = ky0; ky < K; ky += 2) {
            const int ty = y + pad - ky;
            const int oy = ty >> 1;
            if (ty < 0 || oy >= Ho) continue;
            for (int kx = kx0; kx < K; kx += 2) {
                const int tx = x + pad - kx;
                const int ox = tx >> 1;
                if (tx < 0 || ox >= Wo) continue;
                acc = fmaf(gp[oy * Wo + ox], wc[ky * K + kx], acc);
            }
        }
        if (Cout > 32 && (co & 3) == 3) {
            total += acc;
            acc = 0.f;
        }
    }
    acc += total;
    if (ci < C0) gx0[((int64_t)b * C0 + ci) * H * W + (int64_t)y * W + x] = acc;
    else gx1[((int64_t)b * C1 + (ci - C0)) * H * W + (int64_t)y * W + x] = acc;
}

// how the weight gradient is cut up
struct WgradShape {
    int IH, IW, PITCH, coarse, cig, nci, nco, tiles_x, tiles_y, parts;
    int64_t ntiles, wn;

    WgradShape(int B, int Cin, int Cout, int Ho, int Wo, int K, int S, int up0) {
        IH = (kWgTH - 1) * S + K, IW = (kWgTW - 1) * S + K, PITCH = IW | 1;
        coarse = up0 ? (IH / 2 + 2) * (IW / 2 + 2) : 0;  // per channel: the coarse rows and columns that an IH x IW tile of x0' reads
        int cap = std::min(256 / (K * K), kWgXFloats / (IH * PITCH + coarse));
        if (cap < 1) cap = 1;
        nci = (Cin + cap - 1) / cap;
        cig = (Cin + nci - 1) / nci;
        nco = (Cout + kWgCo - 1) / kWgCo;
        tiles_x = (Wo + kWgTW - 1) / kWgTW, tiles_y = (Ho + kWgTH - 1) / kWgTH;
        ntiles = (int64_t)B * tiles_x * tiles_y;
        wn = (int64_t)Cout * Cin * K * K;
        int64_t p = kWgPartFloats / wn;
        if (p > kWgMaxParts) p = kWgMaxParts;
        if (p > ntiles) p = ntiles;
        parts = (int)(p < 1 ? 1 : p);
    }
    int lds_floats() const { return cig * (IH * PITCH + coarse) + kWgPos * kWgCo; }
};

// grid (parts, nci, nco).  Workgroup (slot, ci group, co group) walks tiles slot, slot + parts, ...: a tile is 8 x 32 outputs of one
// image.  Thread tid: item = tid / PG = (ci, ky, kx) of the group, pg = tid % PG takes positions pg, pg + PG, ... of the tile
// (PG = 256 / items).  Runs of 32 products in fp32, the runs added up in fp32, the PG threads of an item in order, the partial stored.
// UP (stride 1): x0 is (B, C0, H/2, W/2).  Behind gs lie CH x CW coarse values per x0 channel of the group, rows cy0 .. and columns
// cx0 .. clamped into the plane: every tap that up2_taps names for a position of the halo tile that lies inside the map.  KT: the
// kernel size at compile time, 0 to take it and what follows from it from the arguments; the UP instantiations fix it, which keeps
// the second staging pass's state within the scalar registers.
template <bool UP, int KT>
__global__ __launch_bounds__(256) void ft_wgrad_kernel(const float *__restrict__ x0, const float *__restrict__ x1, const float *__restrict__ gu,
                                                       float *__restrict__ part, int C0, int C1, int H, int W, int Cout, int Ho_, int Wo_, int K_,
                                                       int S_, int IH_, int IW_, int PITCH_, int cig, int tiles_x, int tiles_y,
                                                       int64_t ntiles) {
    static_assert(UP == (KT != 0), "the kernel size is fixed exactly where x0 is upsampled");
    const int K = KT ? KT : K_, S = UP ? 1 : S_, IH = KT ? kWgTH - 1 + KT : IH_, IW = KT ? kWgTW - 1 + KT : IW_;
    const int Ho = UP ? H : Ho_, Wo = UP ? W : Wo_;  // (stride 1)
    const int PITCH = KT ? ((kWgTW - 1 + KT) | 1) : PITCH_;
    extern __shared__ float lds[];
    float *xs = lds, *gs = lds + cig * IH * PITCH;  // gs[j * 256 + p]; afterwards the threads' totals
    const int tid = threadIdx.x, Cin = C0 + C1, KK = K * K, pad = K / 2;
    const int ci0 = blockIdx.y * cig, co0 = blockIdx.z * kWgCo;
    const int items = cig * KK, PG = 256 / items;
    const int item = tid / PG, pg = tid % PG;
    const bool active = item < items;
    const int ci_l = active ? item / KK : 0, k = active ? item % KK : 0;
    const float *xrow = xs + (ci_l * IH + k / K) * PITCH + k % K;
    const int niter = (kWgPos - pg + PG - 1) / PG;
    const int h2 = H >> 1, w2 = W >> 1, CH = IH / 2 + 2, CW = IW / 2 + 2;  // (UP only)
    float *cs = gs + kWgPos * kWgCo;
    const int nc0 = min(max(C0 - ci0, 0), cig);  // the group's x0 channels

    float total[kWgCo];
#pragma unroll
    for (int j = 0; j < kWgCo; ++j) total[j] = 0.f;

    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int tx = (int)(t % tiles_x), ty = (int)(t / tiles_x % tiles_y), b = (int)(t / ((int64_t)tiles_x * tiles_y));
        const int iy0 = ty * kWgTH * S - pad, ix0 = tx * kWgTW * S - pad;
        __syncthreads();  // the previous tile has been consumed
        const int cy0 = (iy0 - 1) >> 1, cx0 = (ix0 - 1) >> 1;  // (UP only) the first coarse row and column the tile can name
        if (UP) {
            for (int e = tid; e < nc0 * CH * CW; e += 256) {
                const int c = e / (CH * CW), rem = e - c * (CH * CW), r = rem / CW, xx = rem - r * CW;
                const int yy = min(max(cy0 + r, 0), h2 - 1), xc = min(max(cx0 + xx, 0), w2 - 1);
                cs[e] = x0[((int64_t)b * C0 + ci0 + c) * h2 * w2 + (int64_t)yy * w2 + xc];
            }
            __syncthreads();
        }
        for (int e = tid; e < cig * IH * IW; e += 256) {
            const int c = e / (IH * IW), rem = e - c * (IH * IW), r = rem / IW, xx = rem - r * IW;
            const int ci = ci0 + c, gy = iy0 + r, gx = ix0 + xx;
            float v = 0.f;
            if (ci < Cin && (unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W) {
                if (UP && ci < C0) {
                    const gfn::Up2Taps t = gfn::up2_taps(h2, w2, gy, gx);
                    const float *r0 = cs + (c * CH + (t.y0 - cy0)) * CW - cx0, *r1 = cs + (c * CH + (t.y1 - cy0)) * CW - cx0;
                    v = gfn::up2_blend(t, r0[t.x0], r0[t.x1], r1[t.x0], r1[t.x1]);
                } else {
                    v = ci < C0 ? x0[((int64_t)b * C0 + ci) * H * W + (int64_t)gy * W + gx]
                                : x1[((int64_t)b * C1 + (ci - C0)) * H * W + (int64_t)gy * W + gx];
                }
            }
            xs[(c * IH + r) * PITCH + xx] = v;
        }
        for (int e = tid; e < kWgPos * kWgCo; e += 256) {
            const int j = e / kWgPos, p = e % kWgPos;
            const int co = co0 + j, oy = ty * kWgTH + p / kWgTW, ox = tx * kWgTW + p % kWgTW;
            gs[e] = (co < Cout && oy < Ho && ox < Wo) ? gu[((int64_t)b * Cout + co) * Ho * Wo + (int64_t)oy * Wo + ox] : 0.f;
        }
        __syncthreads();
        if (active) {
            for (int i0 = 0; i0 < niter; i0 += 32) {
                float acc[kWgCo];
#pragma unroll
                for (int j = 0; j < kWgCo; ++j) acc[j] = 0.f;
                const int i1 = min(i0 + 32, niter);
                for (int i = i0; i < i1; ++i) {
                    const int p = pg + i * PG;
                    const float xv = xrow[(p / kWgTW) * S * PITCH + (p % kWgTW) * S];
#pragma unroll
                    for (int j = 0; j < kWgCo; ++j) acc[j] = fmaf(gs[j * kWgPos + p], xv, acc[j]);
                }
#pragma unroll
                for (int j = 0; j < kWgCo; ++j) total[j] += acc[j];
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kWgCo; ++j) gs[tid * kWgCo + j] = total[j];
    __syncthreads();
    float *dst = part + (int64_t)blockIdx.x * Cout * Cin * KK;
    for (int e = tid; e < items * kWgCo; e += 256) {
        const int it = e / kWgCo, j = e % kWgCo;
        const int co = co0 + j, ci = ci0 + it / KK;
        if (co >= Cout || ci >= Cin) continue;
        float s = 0.f;
        for (int g = 0; g < PG; ++g) s += gs[(it * PG + g) * kWgCo + j];
        dst[((int64_t)co * Cin + ci) * KK + it % KK] = s;
    }
}

// d_weight[e] = the sum of the partials in order, in double
__global__ __launch_bounds__(256) void ft_wsum_kernel(const float *__restrict__ part, int parts, int64_t wn, float *__restrict__ d_weight) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= wn) return;
    double s = 0.0;
    for (int p = 0; p < parts; ++p) s += (double)part[(int64_t)p * wn + e];
    d_weight[e] = (float)s;
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
struct Plan {
    int Cin, Ho, Wo, HW, red_chunks, nparts, ew_chunks, nident;
    WgradShape wg;
    int64_t off_ident, fwd_floats;                                        // forward: part, ident
    int64_t off_dgdb, off_gu, off_wt, off_wpart, off_gx0f, bwd_floats;    // backward: part, ident, dgdb, gu, wt, wpart; up0: the gradient of x0'
    int64_t off_pack_fwd, off_pack_bwd;                                   // the TF32 class: the split and packed weight, last in both

    Plan(int C0, int C1, int B, int H, int W, int Cout, int K, int S, int up0, int tf32)
        : Cin(C0 + C1), Ho((H + S - 1) / S), Wo((W + S - 1) / S), HW(Ho * Wo), red_chunks((HW + kRed - 1) / kRed), nparts(B * red_chunks),
          ew_chunks((HW + kEw - 1) / kEw), nident(std::max(Cout, std::max(C0, C1))), wg(B, C0 + C1, Cout, Ho, Wo, K, S, up0) {
        off_ident = align4((int64_t)Cout * nparts * 2);
        fwd_floats = off_ident + align4(2 * (int64_t)nident);
        off_dgdb = fwd_floats;  // (before the TF32 class's packed weight is added to it below)
        off_gu = off_dgdb + align4(2 * (int64_t)Cout);
        off_wt = off_gu + align4((int64_t)B * Cout * HW);
        off_wpart = off_wt + align4(wg.wn);
        off_gx0f = off_wpart + align4((int64_t)wg.parts * wg.wn);
        bwd_floats = off_gx0f + (up0 ? align4((int64_t)B * C0 * H * W) : 0);
        // one packed weight at a time: the forward's, then the input gradient's for x0 and for x1 (the roles of Cout and Cin swapped)
        const int64_t pack = !tf32 ? 0 : align4(std::max(gfn::fpn_conv_tf32_pack_bytes(Cout, Cin, K),
                                                         gfn::fpn_conv_tf32_pack_bytes(std::max(C0, C1), Cout, K)) / (int64_t)sizeof(float));
        off_pack_fwd = fwd_floats, off_pack_bwd = bwd_floats;
        fwd_floats += pack, bwd_floats += pack;
    }
};

// up0 reads x0 as its doubled image: what that needs of the sizes
bool up0_fits(int up0, int H, int W, int stride) { return !up0 || (stride == 1 && !((H | W) & 1)); }

// gfn_conv2d_bn_act_fwd's limits and batch statistics' own; 0 when fine.  With up0 the x0 bound is that of its doubled image, which
// the backward writes too (into the workspace)
int check_sizes(const char *what, int C0, int C1, int B, int H, int W, int Cout, int K, int stride, int act, int up0) {
    if (K != 1 && K != 3 && K != 5 && K != 7) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: kernel size %d is not supported, only 1, 3, 5, 7", what, K);
    if (stride != 1 && stride != 2) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: stride %d is not supported, only 1 and 2", what, stride);
    if (act < 0 || act > 2) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: act %d is not one of 0 (none), 1 (leaky ReLU), 2 (swish)", what, act);
    if (B < 0 || H < 1 || W < 1 || C0 < 1 || C1 < 0 || Cout < 1 || Cout > 256 || B > 65535)
        return gfn::fail(GFN_ERR_INVALID_ARG, "%s: bad size (B=%d H=%d W=%d C0=%d C1=%d Cout=%d; C0 >= 1, Cout <= 256, B <= 65535)", what, B,
                         H, W, C0, C1, Cout);
    if (up0 && stride != 1) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: up0 needs stride 1, got stride %d", what, stride);
    if (up0 && ((H | W) & 1)) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: up0 doubles x0, so H and W must be even (H=%d W=%d)", what, H, W);
    if (C0 + (int64_t)C1 > 65535) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: more than 65535 input channels (C0=%d C1=%d)", what, C0, C1);
    const int Ho = (H + stride - 1) / stride, Wo = (W + stride - 1) / stride;
    const int64_t limit = (int64_t)1 << 31;
    const int64_t in0 = (int64_t)C0 * H * W * 4, in1 = (int64_t)C1 * H * W * 4, outb = (int64_t)Cout * Ho * Wo * 4;
    if (in0 >= limit || in1 >= limit || outb >= limit)
        return gfn::fail(GFN_ERR_INVALID_ARG, "%s: a per-image map of 2^31 bytes or more (x0 %lld, x1 %lld, out %lld bytes)", what,
                         (long long)in0, (long long)in1, (long long)outb);
    if ((int64_t)(C0 + C1) * K * K * Cout * 4 >= limit) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: weight of 2^31 bytes or more", what);
    if (B > 0) {
        if ((int64_t)B * Ho * Wo < 2)
            return gfn::fail(GFN_ERR_INVALID_ARG, "%s: batch statistics need more than one value per channel (B*Ho*Wo = %lld)", what,
                             (long long)B * Ho * Wo);
        const int64_t ew = (int64_t)B * std::max(Cout, C0 + C1) * (((int64_t)std::max(Ho * Wo, H * W) + 255) / 256) * 4;
        if (ew > 0x7fffffffLL) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: %lld workgroups exceed the grid", what, (long long)ew);
    }
    return GFN_OK;
}

// The convolution of either class: with tf32 on the matrix core (fpn_conv_tf32.hip) where that class has a kernel, Cout a multiple of 8;
// every other Cout -- an input gradient's is C0 or C1 of the layer -- on the fp32 kernels, whose exact products lie within the class
int conv(const ConvArgs &a, int B, int K, int stride, int tf32, void *pack, hipStream_t s) {
    return tf32 && a.Cout % 8 == 0 ? gfn::fpn_conv_tf32_launch(a, B, K, stride, pack, s) : gfn::fpn_conv_launch(a, B, K, stride, s);
}

int64_t train_ws_bytes(int C0, int C1, int B, int H, int W, int Cout, int K, int stride, int backward, int up0, int tf32 = 0) {
    if (C0 < 1 || C1 < 0 || B < 1 || H < 1 || W < 1 || Cout < 1 || (K != 1 && K != 3 && K != 5 && K != 7) || (stride != 1 && stride != 2)) return 0;
    if (!up0_fits(up0, H, W, stride)) return 0;
    const Plan p(C0, C1, B, H, W, Cout, K, stride, up0, tf32);
    return (backward ? p.bwd_floats : p.fwd_floats) * (int64_t)sizeof(float);
}

int train_fwd(const char *what, const float *x0, int C0, int up0, const float *x1, int C1, const float *weight, const float *conv_bias,
              const float *bn_w, const float *bn_b, float *running_mean, float *running_var, const float *residual, float *u, float *mean,
              float *invstd, float *out, int B, int H, int W, int Cout, int K, int stride, int act, float slope, double momentum, double eps,
              void *ws, int64_t ws_bytes, gfn_stream_t stream, int tf32 = 0) {
    if (int rc = check_sizes(what, C0, C1, B, H, W, Cout, K, stride, act, up0)) return rc;
    if (!(momentum >= 0.0 && momentum <= 1.0) || !(eps >= 0.0))
        return gfn::fail(GFN_ERR_INVALID_ARG, "%s: momentum must lie in [0, 1] and eps be >= 0", what);
    if (B == 0) return GFN_OK;
    if (!x0 || !weight || !bn_w || !bn_b || !running_mean || !running_var || !u || !mean || !invstd || !out || (C1 > 0 && !x1))
        return gfn::fail(GFN_ERR_INVALID_ARG, "%s: null pointer", what);
    if (u == out || u == x0 || u == x1 || out == x0 || out == x1)
        return gfn::fail(GFN_ERR_INVALID_ARG, "%s: u and out must be maps of their own", what);
    const Plan p(C0, C1, B, H, W, Cout, K, stride, up0, tf32);
    if (int rc = check_workspace(what, ws, ws_bytes, p.fwd_floats)) return rc;
    hipStream_t s = (hipStream_t)stream;
    float *part = static_cast<float *>(ws), *ident = part + p.off_ident;

    hipLaunchKernelGGL(ft_identity_kernel, dim3(1), dim3(64), 0, s, ident, p.nident);
    if (int rc = gfn::check_launch("ft_identity_kernel")) return rc;
    const ConvArgs a{x0, x1, weight, ident, ident + p.nident, nullptr, u, C0, C1, up0, H, W, Cout, p.Ho, p.Wo, 0, 0.f};
    if (int rc = conv(a, B, K, stride, tf32, part + p.off_pack_fwd, s)) return rc;
    hipLaunchKernelGGL(ft_moments_kernel, dim3((unsigned)(Cout * p.nparts)), dim3(256), 0, s, (const float *)u, part, Cout, p.HW, p.red_chunks,
                       p.nparts);
    if (int rc = gfn::check_launch("ft_moments_kernel")) return rc;
    hipLaunchKernelGGL(ft_stats_kernel, dim3((unsigned)Cout), dim3(64), 0, s, (const float *)part, conv_bias, mean, invstd, running_mean,
                       running_var, p.HW, p.red_chunks, p.nparts, momentum, eps);
    if (int rc = gfn::check_launch("ft_stats_kernel")) return rc;
    const unsigned blocks = (unsigned)((int64_t)B * Cout * p.ew_chunks);
    const bool vec = p.HW % 4 == 0 && !misaligned(u) && !misaligned(out) && !(residual && misaligned(residual));
    if (vec)
        hipLaunchKernelGGL(ft_apply_kernel<true>, dim3(blocks), dim3(256), 0, s, (const float *)u, bn_w, bn_b, (const float *)mean,
                           (const float *)invstd, residual, out, Cout, p.HW, p.ew_chunks, act, slope);
    else
        hipLaunchKernelGGL(ft_apply_kernel<false>, dim3(blocks), dim3(256), 0, s, (const float *)u, bn_w, bn_b, (const float *)mean,
                           (const float *)invstd, residual, out, Cout, p.HW, p.ew_chunks, act, slope);
    return gfn::check_launch("ft_apply_kernel");
}

int train_bwd(const char *what, const float *gy, const float *x0, int C0, int up0, const float *x1, int C1, const float *weight,
              const float *bn_w, const float *bn_b, const float *u, const float *mean, const float *invstd, float *gx0, float *gx1,
              float *d_weight, float *d_bn_w, float *d_bn_b, int B, int H, int W, int Cout, int K, int stride, int act, float slope, int need,
              void *ws, int64_t ws_bytes, gfn_stream_t stream, int tf32 = 0) {
    if (int rc = check_sizes(what, C0, C1, B, H, W, Cout, K, stride, act, up0)) return rc;
    const int all = GFN_CBT_NEED_X | GFN_CBT_NEED_W | GFN_CBT_NEED_BN;
    if (need < 0 || (need & ~all)) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: unknown need mask %d", what, need);
    if (B == 0 || need == 0) return GFN_OK;
    if (!gy || !x0 || !weight || !bn_w || !bn_b || !u || !mean || !invstd || (C1 > 0 && !x1))
        return gfn::fail(GFN_ERR_INVALID_ARG, "%s: null pointer", what);
    if (((need & GFN_CBT_NEED_X) && (!gx0 || (C1 > 0 && !gx1))) || ((need & GFN_CBT_NEED_W) && !d_weight) ||
        ((need & GFN_CBT_NEED_BN) && (!d_bn_w || !d_bn_b)))
        return gfn::fail(GFN_ERR_INVALID_ARG, "%s: the need mask asks for a gradient whose pointer is null", what);
    const Plan p(C0, C1, B, H, W, Cout, K, stride, up0, tf32);
    if (int rc = check_workspace(what, ws, ws_bytes, p.bwd_floats)) return rc;
    hipStream_t s = (hipStream_t)stream;
    float *w = static_cast<float *>(ws);
    float *part = w, *ident = w + p.off_ident, *dgdb = w + p.off_dgdb, *gu = w + p.off_gu, *wt = w + p.off_wt, *wpart = w + p.off_wpart;
    const bool bn = need & GFN_CBT_NEED_BN;

    hipLaunchKernelGGL(ft_bn_bwd_part_kernel, dim3((unsigned)(Cout * p.nparts)), dim3(256), 0, s, gy, u, bn_w, bn_b, mean, invstd, part, Cout,
                       p.HW, p.red_chunks, p.nparts, act, slope);
    if (int rc = gfn::check_launch("ft_bn_bwd_part_kernel")) return rc;
    hipLaunchKernelGGL(ct_bn_bwd_kernel, dim3((unsigned)Cout), dim3(64), 0, s, (const float *)part, p.nparts, Cout, dgdb, bn ? d_bn_w : nullptr,
                       bn ? d_bn_b : nullptr);
    if (int rc = gfn::check_launch("ct_bn_bwd_kernel")) return rc;
    if (!(need & (GFN_CBT_NEED_X | GFN_CBT_NEED_W))) return GFN_OK;

    hipLaunchKernelGGL(ft_gu_kernel, dim3((unsigned)((int64_t)B * Cout * p.ew_chunks)), dim3(256), 0, s, gy, u, bn_w, bn_b, mean, invstd,
                       (const float *)dgdb, gu, Cout, p.HW, p.ew_chunks, 1.0f / ((float)B * (float)p.HW), act, slope);
    if (int rc = gfn::check_launch("ft_gu_kernel")) return rc;

    if (need & GFN_CBT_NEED_X) {
        if (stride == 1) {
            hipLaunchKernelGGL(ft_identity_kernel, dim3(1), dim3(64), 0, s, ident, p.nident);
            if (int rc = gfn::check_launch("ft_identity_kernel")) return rc;
            hipLaunchKernelGGL(ft_repack_kernel, dim3((unsigned)((p.wg.wn + 255) / 256)), dim3(256), 0, s, weight, wt, Cout, p.Cin, K * K);
            if (int rc = gfn::check_launch("ft_repack_kernel")) return rc;
            float *gx0f = up0 ? w + p.off_gx0f : gx0;  // the gradient of what the convolution read: x0, or with up0 its doubled image
            const ConvArgs a0{gu, nullptr, wt, ident, ident + p.nident, nullptr, gx0f, Cout, 0, 0, H, W, C0, H, W, 0, 0.f};
            if (int rc = conv(a0, B, K, 1, tf32, w + p.off_pack_bwd, s)) return rc;
            if (up0) {
                const int64_t total = (int64_t)B * C0 * (H / 2) * (W / 2);
                hipLaunchKernelGGL(ft_up2_adjoint_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (const float *)gx0f, gx0, total,
                                   H / 2, W / 2);
                if (int rc = gfn::check_launch("ft_up2_adjoint_kernel")) return rc;
            }
            if (C1 > 0) {
                const ConvArgs a1{gu, nullptr, wt + (int64_t)C0 * Cout * K * K, ident, ident + p.nident, nullptr, gx1, Cout, 0, 0, H, W, C1, H, W, 0, 0.f};
                if (int rc = conv(a1, B, K, 1, tf32, w + p.off_pack_bwd, s)) return rc;
            }
        } else {
            const int chunks = (((H + 1) / 2) * ((W + 1) / 2) + 255) / 256;
            hipLaunchKernelGGL(ft_gather_s2_kernel, dim3((unsigned)((int64_t)B * p.Cin * 4 * chunks)), dim3(256), 0, s, (const float *)gu, weight,
                               gx0, gx1, C0, C1, H, W, Cout, p.Ho, p.Wo, K, chunks);
            if (int rc = gfn::check_launch("ft_gather_s2_kernel")) return rc;
        }
    }
    if (need & GFN_CBT_NEED_W) {
        const WgradShape &g = p.wg;
        const dim3 grid((unsigned)g.parts, (unsigned)g.nci, (unsigned)g.nco);
        const size_t lds = (size_t)g.lds_floats() * sizeof(float);
        if (tf32 && stride == 1 && !up0) {  // the class's own weight gradient; stride 2 and up0 stay on ft_wgrad_kernel
            if (int rc = gfn::fpn_wgrad_tf32_launch(x0, x1, gu, wpart, C0, C1, H, W, Cout, K, g.IH, g.IW, g.PITCH, g.cig, g.nci, g.parts, g.tiles_x,
                                                    g.tiles_y, g.ntiles, s))
                return rc;
            hipLaunchKernelGGL(ft_wsum_kernel, dim3((unsigned)((g.wn + 255) / 256)), dim3(256), 0, s, (const float *)wpart, g.parts, g.wn, d_weight);
            return gfn::check_launch("ft_wsum_kernel");
        }
        auto kernel = ft_wgrad_kernel<false, 0>;
        if (up0) kernel = K == 1 ? ft_wgrad_kernel<true, 1> : K == 3 ? ft_wgrad_kernel<true, 3> : K == 5 ? ft_wgrad_kernel<true, 5> : ft_wgrad_kernel<true, 7>;
        hipLaunchKernelGGL(kernel, grid, dim3(256), lds, s, x0, x1, (const float *)gu, wpart, C0, C1, H, W, Cout, p.Ho, p.Wo, K, stride, g.IH,
                           g.IW, g.PITCH, g.cig, g.tiles_x, g.tiles_y, g.ntiles);
        if (int rc = gfn::check_launch("ft_wgrad_kernel")) return rc;
        hipLaunchKernelGGL(ft_wsum_kernel, dim3((unsigned)((g.wn + 255) / 256)), dim3(256), 0, s, (const float *)wpart, g.parts, g.wn, d_weight);
        if (int rc = gfn::check_launch("ft_wsum_kernel")) return rc;
    }
    return GFN_OK;
}

}  // namespace

GFN_EXPORT int64_t gfn_conv2d_bn_act_train_ws_bytes(int C0, int C1, int B, int H, int W, int Cout, int K, int stride, int backward) {
    return train_ws_bytes(C0, C1, B, H, W, Cout, K, stride, backward, 0);
}

GFN_EXPORT int64_t gfn_conv2d_up_bn_act_train_ws_bytes(int C0, int up0, int C1, int B, int H, int W, int Cout, int K, int stride,
                                                       int backward) {
    return train_ws_bytes(C0, C1, B, H, W, Cout, K, stride, backward, up0 ? 1 : 0);
}

GFN_EXPORT int gfn_conv2d_bn_act_train_fwd(const float *x0, int C0, const float *x1, int C1, const float *weight, const float *conv_bias,
                                           const float *bn_w, const float *bn_b, float *running_mean, float *running_var,
                                           const float *residual, float *u, float *mean, float *invstd, float *out, int B, int H, int W,
                                           int Cout, int K, int stride, int act, float slope, double momentum, double eps, void *ws,
                                           int64_t ws_bytes, gfn_stream_t stream) {
    return train_fwd("gfn_conv2d_bn_act_train_fwd", x0, C0, 0, x1, C1, weight, conv_bias, bn_w, bn_b, running_mean, running_var, residual, u,
                     mean, invstd, out, B, H, W, Cout, K, stride, act, slope, momentum, eps, ws, ws_bytes, stream);
}

GFN_EXPORT int gfn_conv2d_up_bn_act_train_fwd(const float *x0, int C0, int up0, const float *x1, int C1, const float *weight,
                                              const float *conv_bias, const float *bn_w, const float *bn_b, float *running_mean,
                                              float *running_var, const float *residual, float *u, float *mean, float *invstd, float *out,
                                              int B, int H, int W, int Cout, int K, int stride, int act, float slope, double momentum,
                                              double eps, void *ws, int64_t ws_bytes, gfn_stream_t stream) {
    return train_fwd("gfn_conv2d_up_bn_act_train_fwd", x0, C0, up0 ? 1 : 0, x1, C1, weight, conv_bias, bn_w, bn_b, running_mean, running_var,
                     residual, u, mean, invstd, out, B, H, W, Cout, K, stride, act, slope, momentum, eps, ws, ws_bytes, stream);
}

GFN_EXPORT int gfn_conv2d_bn_act_train_bwd(const float *gy, const float *x0, int C0, const float *x1, int C1, const float *weight,
                                           const float *bn_w, const float *bn_b, const float *u, const float *mean, const float *invstd,
                                           float *gx0, float *gx1, float *d_weight, float *d_bn_w, float *d_bn_b, int B, int H, int W,
                                           int Cout, int K, int stride, int act, float slope, int need, void *ws, int64_t ws_bytes,
                                           gfn_stream_t stream) {
    return train_bwd("gfn_conv2d_bn_act_train_bwd", gy, x0, C0, 0, x1, C1, weight, bn_w, bn_b, u, mean, invstd, gx0, gx1, d_weight, d_bn_w,
                     d_bn_b, B, H, W, Cout, K, stride, act, slope, need, ws, ws_bytes, stream);
}

GFN_EXPORT int gfn_conv2d_up_bn_act_train_bwd(const float *gy, const float *x0, int C0, int up0, const float *x1, int C1, const float *weight,
                                              const float *bn_w, const float *bn_b, const float *u, const float *mean, const float *invstd,
                                              float *gx0, float *gx1, float *d_weight, float *d_bn_w, float *d_bn_b, int B, int H, int W,
                                              int Cout, int K, int stride, int act, float slope, int need, void *ws, int64_t ws_bytes,
                                              gfn_stream_t stream) {
    return train_bwd("gfn_conv2d_up_bn_act_train_bwd", gy, x0, C0, up0 ? 1 : 0, x1, C1, weight, bn_w, bn_b, u, mean, invstd, gx0, gx1,
                     d_weight, d_bn_w, d_bn_b, B, H, W, Cout, K, stride, act, slope, need, ws, ws_bytes, stream);
}


// The TF32 class of the four pairs above in one set (include/gfnet_hip.h): the same launches with the forward convolution and the
// stride-1 input gradient on fpn_conv_tf32.hip's kernels
GFN_EXPORT int64_t gfn_conv2d_bn_act_train_tf32_ws_bytes(int C0, int up0, int C1, int B, int H, int W, int Cout, int K, int stride,
                                                         int backward) {
    return train_ws_bytes(C0, C1, B, H, W, Cout, K, stride, backward, up0 ? 1 : 0, 1);
}

GFN_EXPORT int gfn_conv2d_bn_act_train_tf32_fwd(const float *x0, int C0, int up0, const float *x1, int C1, const float *weight,
                                                const float *conv_bias, const float *bn_w, const float *bn_b, float *running_mean,
                                                float *running_var, const float *residual, float *u, float *mean, float *invstd, float *out,
                                                int B, int H, int W, int Cout, int K, int stride, int act, float slope, double momentum,
                                                double eps, void *ws, int64_t ws_bytes, gfn_stream_t stream) {
    return train_fwd("gfn_conv2d_bn_act_train_tf32_fwd", x0, C0, up0 ? 1 : 0, x1, C1, weight, conv_bias, bn_w, bn_b, running_mean, running_var,
                     residual, u, mean, invstd, out, B, H, W, Cout, K, stride, act, slope, momentum, eps, ws, ws_bytes, stream, 1);
}

GFN_EXPORT int gfn_conv2d_bn_act_train_tf32_bwd(const float *gy, const float *x0, int C0, int up0, const float *x1, int C1, const float *weight,
                                                const float *bn_w, const float *bn_b, const float *u, const float *mean, const float *invstd,
                                                float *gx0, float *gx1, float *d_weight, float *d_bn_w, float *d_bn_b, int B, int H, int W,
                                                int Cout, int K, int stride, int act, float slope, int need, void *ws, int64_t ws_bytes,
                                                gfn_stream_t stream) {
    return train_bwd("gfn_conv2d_bn_act_train_tf32_bwd", gy, x0, C0, up0 ? 1 : 0, x1, C1, weight, bn_w, bn_b, u, mean, invstd, gx0, gx1,
                     d_weight, d_bn_w, d_bn_b, B, H, W, Cout, K, stride, act, slope, need, ws, ws_bytes, stream, 1);
}
