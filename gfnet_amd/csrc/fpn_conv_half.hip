// The FPN layer of fpn_conv.hip in an fp16 class: fp16 maps in HBM, the convolution an implicit GEMM on the matrix core
// (include/gfnet_hip.h: gfn_conv2d_bn_act_half_fwd), inference only:
//
//     out = act(conv(cat(x0', x1), weight) * scale[c] + shift[c]) + residual
//
// The GEMM: rows are output pixels (16 or 32 consecutive columns of one output row), columns are output channels, and the summed
// index is k = (cg * UP + ky * K + kx) * 8 + c over the channel groups cg of eight input channels -- a UNIT is the eight channels
// of one tap, 16 bytes, one MFMA fragment of a lane.  v_mfma_f32_16x16x32_f16 sums four units per instruction (Cout < 32: at worst
// half of its columns idle), v_mfma_f32_32x32x16_f16 two (Cout >= 32).
//
// conv_half_kernel<K, S, WIDE, NT, NG>: a 256-thread workgroup owns a 16 x 32 output tile of one image for NT column tiles of
// output channels; each wave owns four of its rows.  The halo tile of NG channel groups at a time is staged in LDS channel-innermost,
// [group][row][column][8 channels]: a lane gathers its pixel's eight channels from the planes (with up0: interpolates them in
// fp32 and rounds once) and writes them with ONE 16-byte store, so there is no 2-byte LDS store anywhere, and a lane's A fragment of
// any tap is one ds_read_b128 whose 16 lanes of a pixel run read consecutive slots.  Under stride 2 a tile row holds its even
// columns first and its odd ones from HALF on, as in fpn_conv.hip, so those reads stay consecutive.  The weights come packed
// (ops.conv2d_pack_half) so that a lane's B fragment is one aligned 16-byte read from global memory, the same for every workgroup.
// Padded units and padded channels multiply zeros by zeros: an A fragment past the last tap is set to zero, never read (an inf in
// the map times a zero weight would be NaN).
//
// Epilogue: scale, shift, activation and residual in fp32 on the accumulators, one rounding to fp16, four consecutive pixels of a
// lane as one 8-byte LDS write into a [channel][16 x 32 pixels] image of the tile; the workgroup then stores that image as row
// segments, 16 bytes per lane where the rows allow it.  No atomics, a fixed order of sums: identical calls give identical bits.
#include "elem16.h"
#include "fpn_conv_launch.h"

namespace {

using gfn::activate;
using gfn::f16x4;
using gfn::f16x8;
using gfn::f32x16;
using gfn::f32x4;
using gfn::up2_blend;
using gfn::up2_taps;
using gfn::Up2Taps;

struct HalfArgs {
    const _Float16 *x0, *x1, *weight;
    const float *scale, *shift;
    const _Float16 *residual;
    _Float16 *out;
    int C0, C1, up0, H, W, Cout, Ho, Wo, act;
    float slope;
};

constexpr int kThreads = 256;
constexpr int kTW = 32, kTH = 16;                 // the output tile
constexpr int kWaveRows = kTH / (kThreads / 64);  // rows of it per wave
constexpr int kOutPitch = kTH * kTW + 4;          // fp16 values per channel of the staged output tile: 8 bytes of padding

constexpr int units_padded(int K) { return (K * K + 3) / 4 * 4; }  // UP: units per channel group in the packed weight
constexpr int cout_padded(int Cout) { return Cout < 32 ? (Cout + 15) / 16 * 16 : (Cout + 31) / 32 * 32; }  // its rows

template <int K, int S>
struct Halo {
    static constexpr int IH = (kTH - 1) * S + K, IW = (kTW - 1) * S + K, HALF = (IW + 1) / 2, PITCH = S == 1 ? IW : 2 * HALF;
    static constexpr int SLOTS = IH * PITCH;  // 16-byte slots per channel group
    // channel groups per stage: what fits in some 36 KiB, four at the most
    static constexpr int NG = 36 * 1024 / (SLOTS * 16) < 1 ? 1 : (36 * 1024 / (SLOTS * 16) > 4 ? 4 : 36 * 1024 / (SLOTS * 16));
    static __device__ __forceinline__ int place(int x) { return S == 1 ? x : (x & 1) * HALF + (x >> 1); }
};

template <bool WIDE>
struct Acc {
    typedef f32x4 type;
};
template <>
struct Acc<true> {
    typedef f32x16 type;
};
__device__ __forceinline__ f32x4 mma(f16x8 a, f16x8 b, f32x4 c) { return gfn::mfma32(a, b, c); }
__device__ __forceinline__ f32x16 mma(f16x8 a, f16x8 b, f32x16 c) { return gfn::mfma16(a, b, c); }

// (two column tiles of the 32-wide instruction are 128 accumulator registers: bounded to two workgroups per CU the compiler fits
// them in 256 registers without scratch; left alone it takes 276-280 and one workgroup runs alone, nothing covering its staging)
template <int K, int S, bool WIDE, int NT, int NG>
__global__ __launch_bounds__(kThreads, (WIDE && NT == 2) ? 2 : 1) void conv_half_kernel(const HalfArgs a, const int tiles_x, const int tiles_y, const int groups,
                                                             const int CG) {
    typedef Halo<K, S> T;
    typedef typename Acc<WIDE>::type acc_t;
    constexpr int NW = WIDE ? 32 : 16;            // pixels and output channels of one MFMA tile
    constexpr int G = WIDE ? 2 : 4;               // units per MFMA
    constexpr int KK = K * K, UP = units_padded(K), NSTEP = (KK + G - 1) / G;
    constexpr int MPR = kTW / NW, MT = kWaveRows * MPR;  // pixel tiles per row and per wave
    constexpr int PAD = K / 2;
    constexpr int HALO_BYTES = NG * T::SLOTS * 16, OUT_BYTES = NW * kOutPitch * 2;
    __shared__ __attribute__((aligned(16))) unsigned char smem[HALO_BYTES > OUT_BYTES ? HALO_BYTES : OUT_BYTES];
    f16x8 *tile = reinterpret_cast<f16x8 *>(smem);
    _Float16 *stage = reinterpret_cast<_Float16 *>(smem);

    unsigned bid = blockIdx.x;
    const int tx = bid % tiles_x;
    bid /= tiles_x;
    const int ty = bid % tiles_y;
    bid /= tiles_y;
    const int co0 = (bid % groups) * (NT * NW);
    const int b = bid / groups;

    const int Cin = a.C0 + a.C1;
    const int H0 = a.up0 ? a.H >> 1 : a.H, W0 = a.up0 ? a.W >> 1 : a.W;
    const _Float16 *__restrict__ x0b = a.x0 + (int64_t)b * a.C0 * H0 * W0;
    const _Float16 *__restrict__ x1b = a.x1 + (int64_t)b * a.C1 * a.H * a.W;  // (never read when C1 = 0)

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = lane & (NW - 1), g = lane / NW;  // the lane's pixel (A) and output channel (B) within a tile; its unit of a step
    const int iy0 = ty * kTH * S - PAD, ix0 = tx * kTW * S - PAD;

    acc_t acc[MT][NT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[m][t] = acc_t(0.f);

    // the lane's pixel of pixel tile m in the halo tile (tap 0, 0), in slots
    int base[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) base[m] = (wave * kWaveRows + m / MPR) * S * T::PITCH + (m % MPR) * NW + n;

    for (int cg0 = 0; cg0 < CG; cg0 += NG) {
        const int ng = min(NG, CG - cg0);
        __syncthreads();  // the previous stage has been consumed
        for (int i = tid; i < ng * T::IH * T::IW; i += kThreads) {
            const int cgl = i / (T::IH * T::IW), rem = i - cgl * (T::IH * T::IW), r = rem / T::IW, x = rem - r * T::IW;
            const int gy = iy0 + r, gx = ix0 + x;
            f16x8 v = f16x8((_Float16)0.f);
            if ((unsigned)gy < (unsigned)a.H && (unsigned)gx < (unsigned)a.W) {
                const int c0 = (cg0 + cgl) * 8;
                const Up2Taps t = up2_taps(H0, W0, gy, gx);  // (used with up0 only)
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int ci = c0 + j;
                    if (ci >= Cin) continue;  // the padded channels of the last group stay zero
                    if (ci >= a.C0) {
                        v[j] = x1b[((ci - a.C0) * a.H + gy) * a.W + gx];
                    } else if (a.up0) {
                        const _Float16 *__restrict__ p = x0b + ci * H0 * W0;
                        v[j] = (_Float16)up2_blend(t, (float)p[t.y0 * W0 + t.x0], (float)p[t.y0 * W0 + t.x1], (float)p[t.y1 * W0 + t.x0],
                                                   (float)p[t.y1 * W0 + t.x1]);
                    } else {
                        v[j] = x0b[(ci * a.H + gy) * a.W + gx];
                    }
                }
            }
            tile[(cgl * T::IH + r) * T::PITCH + T::place(x)] = v;
        }
        __syncthreads();
#pragma unroll 1
        for (int cgl = 0; cgl < ng; ++cgl) {
            const f16x8 *tl = tile + cgl * T::SLOTS;
            // row co0 + n of the packed weight, channel group cg0 + cgl: UP units of 8
            const _Float16 *__restrict__ wrow = a.weight + ((int64_t)(co0 + n) * CG + (cg0 + cgl)) * (UP * 8);
#pragma unroll
            for (int s = 0; s < NSTEP; ++s) {
                const int u = s * G + g, uc = min(u, KK - 1), ky = uc / K, kx = uc - ky * K;
                const bool valid = u < KK;
                const int off = ky * T::PITCH + (S == 1 ? kx : (kx & 1) * T::HALF + (kx >> 1));
                f16x8 bf[NT];
#pragma unroll
                for (int t = 0; t < NT; ++t) bf[t] = *reinterpret_cast<const f16x8 *>(wrow + (int64_t)t * NW * CG * (UP * 8) + u * 8);
#pragma unroll
                for (int m = 0; m < MT; ++m) {
                    f16x8 af = tl[base[m] + off];
                    if (!valid) af = f16x8((_Float16)0.f);
#pragma unroll
                    for (int t = 0; t < NT; ++t) acc[m][t] = mma(af, bf[t], acc[m][t]);
                }
            }
        }
    }

    const int64_t ob = (int64_t)b * a.Cout * a.Ho * a.Wo;
    const bool vec = (a.Wo & 7) == 0;  // every 8-pixel segment of a row is then whole and 16-byte aligned
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        __syncthreads();  // the halo tile, or the previous channel tile's image, has been read
        const int co = co0 + t * NW + n;
        if (co < a.Cout) {
            const float sc = a.scale[co], sh = a.shift[co];
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                const int rl = wave * kWaveRows + m / MPR, oy = ty * kTH + rl;
#pragma unroll
                for (int q = 0; q < (WIDE ? 4 : 1); ++q) {
                    // registers 4q .. 4q+3 of the lane: four consecutive pixels of one row (common.h: acc_row)
                    const int px = (m % MPR) * NW + (WIDE ? 8 * q + 4 * g : 4 * g);
                    f16x4 h;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float v = activate(fmaf(acc[m][t][4 * q + r], sc, sh), a.act, a.slope);
                        const int ox = tx * kTW + px + r;
                        if (a.residual && oy < a.Ho && ox < a.Wo) v += (float)a.residual[ob + ((int64_t)co * a.Ho + oy) * a.Wo + ox];
                        h[r] = (_Float16)v;
                    }
                    *reinterpret_cast<f16x4 *>(stage + n * kOutPitch + rl * kTW + px) = h;
                }
            }
        }
        __syncthreads();
        for (int i = tid; i < NW * kTH * (kTW / 8); i += kThreads) {
            const int seg = i % (kTW / 8), rl = i / (kTW / 8) % kTH, c = i / (kTW / 8 * kTH);
            const int co = co0 + t * NW + c, oy = ty * kTH + rl, ox = tx * kTW + seg * 8;
            if (co >= a.Cout || oy >= a.Ho || ox >= a.Wo) continue;
            const _Float16 *src = stage + c * kOutPitch + rl * kTW + seg * 8;
            const f16x4 lo = *reinterpret_cast<const f16x4 *>(src), hi = *reinterpret_cast<const f16x4 *>(src + 4);
            _Float16 *dst = a.out + ob + ((int64_t)co * a.Ho + oy) * a.Wo + ox;
            if (vec) {
                *reinterpret_cast<f16x8 *>(dst) = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (ox + j < a.Wo) dst[j] = lo[j];
                    if (ox + 4 + j < a.Wo) dst[4 + j] = hi[j];
                }
            }
        }
    }
}

template <int K, int S, bool WIDE, int NT>
int launch(const HalfArgs &a, int B, int CG, hipStream_t s) {
    constexpr int NG = Halo<K, S>::NG;
    const int tiles_x = (a.Wo + kTW - 1) / kTW, tiles_y = (a.Ho + kTH - 1) / kTH;
    const int cout_pad = cout_padded(a.Cout), groups = cout_pad / (NT * (WIDE ? 32 : 16));
    const int64_t blocks = (int64_t)tiles_x * tiles_y * groups * B;
    if (blocks > 0x7fffffffLL)
        return gfn::fail(GFN_ERR_INVALID_ARG, "gfn_conv2d_bn_act_half_fwd: %lld workgroups exceed the grid", (long long)blocks);
    hipLaunchKernelGGL((conv_half_kernel<K, S, WIDE, NT, NG>), dim3((unsigned)blocks), dim3(kThreads), 0, s, a, tiles_x, tiles_y, groups, CG);
    return gfn::check_launch("conv_half_kernel");
}

// 16-wide tiles below 32 output channels, 32-wide from there; two column tiles per workgroup where the padded Cout divides
template <int K, int S>
int launch_shape(const HalfArgs &a, int B, int CG, hipStream_t s) {
    const int cout_pad = cout_padded(a.Cout);
    if (a.Cout < 32) return cout_pad == 32 ? launch<K, S, false, 2>(a, B, CG, s) : launch<K, S, false, 1>(a, B, CG, s);
    return cout_pad % 64 == 0 ? launch<K, S, true, 2>(a, B, CG, s) : launch<K, S, true, 1>(a, B, CG, s);
}

template <int K>
int launch_stride(const HalfArgs &a, int S, int B, int CG, hipStream_t s) {
    return S == 1 ? launch_shape<K, 1>(a, B, CG, s) : launch_shape<K, 2>(a, B, CG, s);
}

}  // namespace

GFN_EXPORT int gfn_conv2d_bn_act_half_fwd(const void *x0, int C0, int up0, const void *x1, int C1, const void *weight, const float *scale,
                                          const float *shift, const void *residual, void *out, int B, int H, int W, int Cout, int K,
                                          int stride, int act, float slope, gfn_stream_t stream) {
    const char *what = "gfn_conv2d_bn_act_half_fwd";
    if (K != 1 && K != 3 && K != 5 && K != 7) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: kernel size %d is not supported, only 1, 3, 5, 7", what, K);
    if (stride != 1 && stride != 2) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: stride %d is not supported, only 1 and 2", what, stride);
    if (act < 0 || act > 2) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: act %d is not one of 0 (none), 1 (leaky ReLU), 2 (swish)", what, act);
    if (B < 0 || H < 1 || W < 1 || C0 < 1 || C1 < 0 || Cout < 1 || Cout > 256 || B > 65535)
        return gfn::fail(GFN_ERR_INVALID_ARG, "%s: bad size (B=%d H=%d W=%d C0=%d C1=%d Cout=%d; C0 >= 1, Cout <= 256, B <= 65535)", what, B,
                         H, W, C0, C1, Cout);
    if (Cout % 8) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: Cout %d is not a multiple of 8 (this class has no general kernel)", what, Cout);
    if (up0 && ((H | W) & 1)) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: up0 doubles x0, so H and W must be even (H=%d W=%d)", what, H, W);
    const int Ho = (H + stride - 1) / stride, Wo = (W + stride - 1) / stride;
    const int64_t limit = (int64_t)1 << 31;
    const int64_t in0 = (int64_t)C0 * (up0 ? H / 2 : H) * (up0 ? W / 2 : W) * 2, in1 = (int64_t)C1 * H * W * 2,
                  outb = (int64_t)Cout * Ho * Wo * 2;
    if (in0 >= limit || in1 >= limit || outb >= limit)
        return gfn::fail(GFN_ERR_INVALID_ARG, "%s: a per-image map of 2^31 bytes or more (x0 %lld, x1 %lld, out %lld bytes)", what,
                         (long long)in0, (long long)in1, (long long)outb);
    const int CG = (int)(((int64_t)C0 + C1 + 7) / 8);
    if ((int64_t)cout_padded(Cout) * CG * units_padded(K) * 16 >= limit)
        return gfn::fail(GFN_ERR_INVALID_ARG, "%s: packed weight of 2^31 bytes or more", what);
    if (B == 0) return GFN_OK;
    if (!x0 || !weight || !scale || !shift || !out || (C1 > 0 && !x1)) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: null pointer", what);

    const HalfArgs a{(const _Float16 *)x0, (const _Float16 *)x1, (const _Float16 *)weight, scale, shift, (const _Float16 *)residual,
                     (_Float16 *)out,      C0, C1, up0 ? 1 : 0, H, W, Cout, Ho, Wo, act, slope};
    hipStream_t s = (hipStream_t)stream;
    switch (K) {
        case 1: return launch_stride<1>(a, stride, B, CG, s);
        case 3: return launch_stride<3>(a, stride, B, CG, s);
        case 5: return launch_stride<5>(a, stride, B, CG, s);
        default: return launch_stride<7>(a, stride, B, CG, s);
    }
}
