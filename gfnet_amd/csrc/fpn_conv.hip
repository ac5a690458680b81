// Fused direct convolution of the FPN pyramid (reference model/FPN.py:5-69, 88-128; model/network.py:66, 182), inference only:
//
//     out = act(conv(cat(x0', x1), weight) * scale[c] + shift[c]) + residual          (include/gfnet_hip.h: gfn_conv2d_bn_act_fwd)
//
// where x0' is x0 or its 2x bilinear upsample (never written: interpolated while the halo tile is staged), BatchNorm and the conv
// bias arrive folded into scale / shift, and the decoder's residual add rides in the epilogue.  One launch per layer.
//
// conv_tile_kernel<K, S, COB, R, CI, SPLIT>: a 256-thread workgroup owns a 32 x 8R output tile of one image for COB output
// channels.  The input halo tile of CI input channels at a time goes through LDS; a lane owns one output column and R consecutive
// rows, so per input channel and kernel column it reads (R-1)S+K tile values once and uses each for up to K rows x COB channels of
// fmaf.  The weights are addressed uniformly over the wave (scalar loads, an SGPR operand per fmaf).  fp32 fmaf chains in the
// order (input channel, kernel column, output-channel octet, kernel row): the result depends on the arguments alone.  The layers
// with 32 and 64 output channels run here too, four to eight channel groups per tile: not yet on the matrix core.
// conv_general_kernel: one thread per output value straight from global memory, for Cout that is no multiple of 8.
#include "fpn_conv_launch.h"

namespace {

using gfn::activate;  // (ConvArgs and the activation: fpn_conv_launch.h, shared with the training path)
using gfn::ConvArgs;

constexpr int kThreads = 256;
constexpr int kTW = 32;                     // tile columns: the lanes of a half-wave
constexpr int kStrips = kThreads / kTW;     // row strips of a tile, R rows each
constexpr int kSplitAbove = 32;             // input channels above which the sum is split by stage (conv_tile_kernel, SPLIT)

using gfn::up2_at;  // (the 2x bilinear upsample as every reader of the doubled map evaluates it: fpn_conv_launch.h)

// channel ci of cat(x0', x1) of one image at (y, x), zero outside the map
__device__ __forceinline__ float input_at(const ConvArgs &a, const float *__restrict__ x0b, const float *__restrict__ x1b, int ci,
                                          int y, int x) {
    if ((unsigned)y >= (unsigned)a.H || (unsigned)x >= (unsigned)a.W) return 0.f;
    if (ci >= a.C0) return x1b[((ci - a.C0) * a.H + y) * a.W + x];
    if (a.up0) return up2_at(x0b + ci * (a.H >> 1) * (a.W >> 1), a.H >> 1, a.W >> 1, y, x);
    return x0b[(ci * a.H + y) * a.W + x];
}

// One input channel's halo tile into LDS: `fetch(y, x)` is called with coordinates clamped into the map, so its loads are
// unconditional and the unrolled loop can have many of them in flight; what lies outside the map is then replaced by zero.
template <int IH, int IW, typename Fetch, typename Place>
__device__ __forceinline__ void stage_plane(float *__restrict__ dst, int tid, int iy0, int ix0, int H, int W, Fetch fetch, Place place) {
    constexpr int N = IH * IW, U = 4;  // U values per lane in flight (each up to four loads)
#pragma unroll 1
    for (int i0 = tid; i0 < N; i0 += U * kThreads) {
        float v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = min(i0 + u * kThreads, N - 1), r = i / IW, x = i - r * IW;
            const int gy = iy0 + r, gx = ix0 + x;
            const bool inside = (unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W;
            v[u] = fetch(min(max(gy, 0), H - 1), min(max(gx, 0), W - 1));
            v[u] = inside ? v[u] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = i0 + u * kThreads, r = i / IW, x = i - r * IW;
            if (i < N) dst[place(r, x)] = v[u];
        }
    }
}

template <int K, int S, int COB, int R, int CI, bool SPLIT>
__global__ __launch_bounds__(kThreads) void conv_tile_kernel(const ConvArgs a, const int tiles_x, const int tiles_y, const int groups) {
    constexpr int TH = kStrips * R, IH = (TH - 1) * S + K, IW = (kTW - 1) * S + K, NIN = (R - 1) * S + K, PAD = K / 2;
    // stride 2: a tile row holds its even columns first, then its odd ones from HALF on, so that the lanes of a half-wave, which
    // want every second column, read consecutive words (no two on one LDS bank)
    constexpr int HALF = (IW + 1) / 2, PITCH = S == 1 ? (IW | 1) : (2 * HALF + 1);
    __shared__ float tile[CI * IH * PITCH];

    unsigned bid = blockIdx.x;
    const int tx = bid % tiles_x;
    bid /= tiles_x;
    const int ty = bid % tiles_y;
    bid /= tiles_y;
    const int co0 = (bid % groups) * COB;
    const int b = bid / groups;

    const int Cin = a.C0 + a.C1;
    const int H0 = a.up0 ? a.H >> 1 : a.H, W0 = a.up0 ? a.W >> 1 : a.W;
    const float *__restrict__ x0b = a.x0 + (int64_t)b * a.C0 * H0 * W0;
    const float *__restrict__ x1b = a.x1 + (int64_t)b * a.C1 * a.H * a.W;  // (never read when C1 = 0)
    const float *__restrict__ w = a.weight;

    const int tid = threadIdx.x, lx = tid % kTW, strip = tid / kTW;
    const int iy0 = ty * TH * S - PAD, ix0 = tx * kTW * S - PAD;

    float acc[R][COB];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int j = 0; j < COB; ++j) acc[r][j] = 0.f;
    // SPLIT (more than 32 input channels): every stage's CI K K terms are summed on their own and then added to `total`, so no
    // chain is longer than a stage plus one addition per stage (a single chain over 128 x 9 terms measured 5 x the error of the
    // library's blocked sums, 1.2 x at 16 channels)
    float total[SPLIT ? R : 1][SPLIT ? COB : 1];
    if (SPLIT) {
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int j = 0; j < COB; ++j) total[r][j] = 0.f;
    }

    for (int c0 = 0; c0 < Cin; c0 += CI) {
        __syncthreads();  // the previous chunk has been consumed
        const int nc = min(CI, Cin - c0);
        const auto place = [](int r, int x) { return r * PITCH + (S == 1 ? x : (x & 1) * HALF + (x >> 1)); };
        for (int c = 0; c < nc; ++c) {  // (the channels past Cin of the last stage are not read below)
            const int ci = c0 + c;
            float *dst = tile + c * IH * PITCH;
            if (ci >= a.C0) {
                const float *__restrict__ p = x1b + (ci - a.C0) * a.H * a.W;
                stage_plane<IH, IW>(dst, tid, iy0, ix0, a.H, a.W, [&](int y, int x) { return p[y * a.W + x]; }, place);
            } else if (a.up0) {
                const float *__restrict__ p = x0b + ci * H0 * W0;
                stage_plane<IH, IW>(dst, tid, iy0, ix0, a.H, a.W, [&](int y, int x) { return up2_at(p, H0, W0, y, x); }, place);
            } else {
                const float *__restrict__ p = x0b + ci * a.H * a.W;
                stage_plane<IH, IW>(dst, tid, iy0, ix0, a.H, a.W, [&](int y, int x) { return p[y * a.W + x]; }, place);
            }
        }
        __syncthreads();
#pragma unroll 1
        for (int c = 0; c < nc; ++c) {
            const float *__restrict__ wc = w + ((int64_t)co0 * Cin + (c0 + c)) * (K * K);
            const float *t = tile + (c * IH + strip * R * S) * PITCH + lx;
#pragma unroll
            for (int kx = 0; kx < K; ++kx) {
                float in[NIN];
#pragma unroll
                for (int j = 0; j < NIN; ++j) in[j] = t[j * PITCH + (S == 1 ? kx : (kx & 1) * HALF + (kx >> 1))];
                // eight output channels at a time, fenced: left alone, the scheduler hoists a whole channel's scalar weight loads
                // (up to 16 K K of them) above the fmaf and spills SGPRs through v_readlane, more of those than fmaf
#pragma unroll
                for (int j0 = 0; j0 < COB; j0 += 8) {
#pragma unroll
                    for (int ky = 0; ky < K; ++ky)
#pragma unroll
                        for (int j = j0; j < j0 + 8; ++j) {
                            const float wv = wc[j * Cin * (K * K) + ky * K + kx];
#pragma unroll
                            for (int r = 0; r < R; ++r) acc[r][j] = fmaf(in[r * S + ky], wv, acc[r][j]);
                        }
                    if (K * K * COB > 160) __builtin_amdgcn_sched_barrier(0);  // (3 x 3 x 16 weights fit: fenced, it measured 5-19 % slower)
                }
            }
        }
        if (SPLIT) {
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int j = 0; j < COB; ++j) {
                    total[r][j] += acc[r][j];
                    acc[r][j] = 0.f;
                }
        }
    }

    const int ox = tx * kTW + lx;
    if (ox >= a.Wo) return;
    const int64_t ob = (int64_t)b * a.Cout * a.Ho * a.Wo;
#pragma unroll
    for (int j = 0; j < COB; ++j) {
        const int co = co0 + j;
        const float sc = a.scale[co], sh = a.shift[co];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int oy = ty * TH + strip * R + r;
            if (oy >= a.Ho) continue;
            const int64_t o = ob + ((int64_t)co * a.Ho + oy) * a.Wo + ox;
            float v = activate(fmaf(SPLIT ? total[r][j] : acc[r][j], sc, sh), a.act, a.slope);
            if (a.residual) v += a.residual[o];
            a.out[o] = v;
        }
    }
}

// One thread per output value: any Cout, any K and stride of the ABI.  The tile kernel's summation order.
__global__ __launch_bounds__(kThreads) void conv_general_kernel(const ConvArgs a, const int K, const int S, const int64_t per_image) {
    const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= per_image) return;
    const int b = blockIdx.y;
    const int ox = (int)(idx % a.Wo), oy = (int)(idx / a.Wo % a.Ho), co = (int)(idx / ((int64_t)a.Wo * a.Ho));
    const int Cin = a.C0 + a.C1, pad = K / 2;
    const int H0 = a.up0 ? a.H >> 1 : a.H, W0 = a.up0 ? a.W >> 1 : a.W;
    const float *__restrict__ x0b = a.x0 + (int64_t)b * a.C0 * H0 * W0;
    const float *__restrict__ x1b = a.x1 + (int64_t)b * a.C1 * a.H * a.W;
    float acc = 0.f, total = 0.f;
    for (int ci = 0; ci < Cin; ++ci) {
        const float *__restrict__ wc = a.weight + ((int64_t)co * Cin + ci) * (K * K);
        for (int kx = 0; kx < K; ++kx)
            for (int ky = 0; ky < K; ++ky)
                acc = fmaf(input_at(a, x0b, x1b, ci, oy * S - pad + ky, ox * S - pad + kx), wc[ky * K + kx], acc);
        if (Cin > kSplitAbove && (ci & 3) == 3) {  // as the tile kernel: four channels to a partial sum
            total += acc;
            acc = 0.f;
        }
    }
    acc += total;
    const int64_t o = (int64_t)b * per_image + idx;
    float v = activate(fmaf(acc, a.scale[co], a.shift[co]), a.act, a.slope);
    if (a.residual) v += a.residual[o];
    a.out[o] = v;
}

template <int K, int S, int COB>
int launch_tile(const ConvArgs &a, int B, hipStream_t s) {
    // rows per lane and input channels per stage: every weight (a scalar load) should feed many fmaf -- 8 rows where a lane holds 8
    // channels, 4 where it holds 16 (64 accumulators either way) -- within some 20 KiB of LDS for the halo tile, whose area under
    // stride 2 is four times the output's
    constexpr int R = (S == 1 && COB == 8) ? 8 : 4, CI = S == 2 ? 1 : (COB == 8 ? 2 : 4), TH = kStrips * R;
    const int tiles_x = (a.Wo + kTW - 1) / kTW, tiles_y = (a.Ho + TH - 1) / TH, groups = a.Cout / COB;
    const int64_t blocks = (int64_t)tiles_x * tiles_y * groups * B;
    if (blocks > 0x7fffffffLL) return gfn::fail(GFN_ERR_INVALID_ARG, "gfn_conv2d_bn_act_fwd: %lld workgroups exceed the grid", (long long)blocks);
    if (a.C0 + a.C1 > kSplitAbove)
        hipLaunchKernelGGL((conv_tile_kernel<K, S, COB, R, CI, true>), dim3((unsigned)blocks), dim3(kThreads), 0, s, a, tiles_x, tiles_y, groups);
    else
        hipLaunchKernelGGL((conv_tile_kernel<K, S, COB, R, CI, false>), dim3((unsigned)blocks), dim3(kThreads), 0, s, a, tiles_x, tiles_y, groups);
    return gfn::check_launch("conv_tile_kernel");
}

template <int K, int S>
int launch_tile_cob(const ConvArgs &a, int B, hipStream_t s) {
    return a.Cout % 16 == 0 ? launch_tile<K, S, 16>(a, B, s) : launch_tile<K, S, 8>(a, B, s);
}

template <int K>
int launch_tile_stride(const ConvArgs &a, int S, int B, hipStream_t s) {
    return S == 1 ? launch_tile_cob<K, 1>(a, B, s) : launch_tile_cob<K, 2>(a, B, s);
}

}  // namespace

int gfn::fpn_conv_launch(const ConvArgs &a, int B, int K, int stride, hipStream_t s) {
    if (a.Cout % 8 == 0) {
        switch (K) {
            case 1: return launch_tile_stride<1>(a, stride, B, s);
            case 3: return launch_tile_stride<3>(a, stride, B, s);
            case 5: return launch_tile_stride<5>(a, stride, B, s);
            default: return launch_tile_stride<7>(a, stride, B, s);
        }
    }
    const int64_t per_image = (int64_t)a.Cout * a.Ho * a.Wo;
    hipLaunchKernelGGL(conv_general_kernel, dim3((unsigned)((per_image + kThreads - 1) / kThreads), (unsigned)B), dim3(kThreads), 0, s, a,
                       K, stride, per_image);
    return gfn::check_launch("conv_general_kernel");
}

GFN_EXPORT int gfn_conv2d_bn_act_fwd(const float *x0, int C0, int up0, const float *x1, int C1, const float *weight, const float *scale,
                                     const float *shift, const float *residual, float *out, int B, int H, int W, int Cout, int K,
                                     int stride, int act, float slope, gfn_stream_t stream) {
    const char *what = "gfn_conv2d_bn_act_fwd";
    if (K != 1 && K != 3 && K != 5 && K != 7) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: kernel size %d is not supported, only 1, 3, 5, 7", what, K);
    if (stride != 1 && stride != 2) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: stride %d is not supported, only 1 and 2", what, stride);
    if (act < 0 || act > 2) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: act %d is not one of 0 (none), 1 (leaky ReLU), 2 (swish)", what, act);
    if (B < 0 || H < 1 || W < 1 || C0 < 1 || C1 < 0 || Cout < 1 || Cout > 256 || B > 65535)
        return gfn::fail(GFN_ERR_INVALID_ARG, "%s: bad size (B=%d H=%d W=%d C0=%d C1=%d Cout=%d; C0 >= 1, Cout <= 256, B <= 65535)", what, B,
                         H, W, C0, C1, Cout);
    if (up0 && ((H | W) & 1)) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: up0 doubles x0, so H and W must be even (H=%d W=%d)", what, H, W);
    const int Ho = (H + stride - 1) / stride, Wo = (W + stride - 1) / stride;
    const int64_t limit = (int64_t)1 << 31;
    const int64_t in0 = (int64_t)C0 * (up0 ? H / 2 : H) * (up0 ? W / 2 : W) * 4, in1 = (int64_t)C1 * H * W * 4,
                  outb = (int64_t)Cout * Ho * Wo * 4;
    if (in0 >= limit || in1 >= limit || outb >= limit)
        return gfn::fail(GFN_ERR_INVALID_ARG, "%s: a per-image map of 2^31 bytes or more (x0 %lld, x1 %lld, out %lld bytes)", what,
                         (long long)in0, (long long)in1, (long long)outb);
    if ((int64_t)(C0 + C1) * K * K * Cout * 4 >= limit) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: weight of 2^31 bytes or more", what);
    if (B == 0) return GFN_OK;
    if (!x0 || !weight || !scale || !shift || !out || (C1 > 0 && !x1)) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: null pointer", what);

    const ConvArgs a{x0, x1, weight, scale, shift, residual, out, C0, C1, up0 ? 1 : 0, H, W, Cout, Ho, Wo, act, slope};
    return gfn::fpn_conv_launch(a, B, K, stride, (hipStream_t)stream);
}
