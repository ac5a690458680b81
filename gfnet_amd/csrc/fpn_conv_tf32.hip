// The FPN layer of fpn_conv.hip in the reference's TF32 CLASS (include/gfnet_hip.h: gfn_conv2d_bn_act_tf32_fwd and, through
// fpn_conv_launch.h, the convolutions of gfn_conv2d_bn_act_train_tf32_*): fp32 maps in HBM exactly as on the fp32 path, the
// convolution an implicit GEMM on the matrix core with SPLIT-bf16 operands.  gfx950 has no TF32 matrix instruction; its bf16 one
// at a third of its rate carries 16 significant bits of each operand against TF32's 11:
//
//     v = hi + lo + r      hi = bf16(v) to nearest even, lo = bf16(v - hi), lo = 0 where hi is not finite (an inf stays an inf)
//     a b ~= a_hi b_hi + a_hi b_lo + a_lo b_hi          each product exact in fp32, summed in fp32 by the instruction; a_lo b_lo dropped
//
// tf32_pack_kernel splits the fp32 weight (Cout, Cin, K, K) -- the layer's own, or the transposed and flipped one that the input
// gradient reads -- into a hi and a lo image in ops.conv2d_pack_half's fragment order [co][cg][unit][8], zeros past Cout, Cin and
// K K: one small launch in front of every convolution, since in training the weights change every step.
//
// conv_tf32_kernel<K, S, WIDE, NT, NG> is fpn_conv_half.hip's conv_half_kernel in this class: a 256-thread workgroup owns a 16 x 32
// output tile of one image for NT column tiles of output channels, each wave four of its rows.  The halo tile of NG channel groups
// is staged channel-innermost from the fp32 planes: a lane gathers its pixel's eight channels (with up0: interpolates them in fp32
// with up2_taps / up2_blend, as the fp32 kernels do), splits them and writes a hi slot and a lo slot, 16 bytes each, so a lane's A
// fragment of any tap is one ds_read_b128 per slot and there is no 2-byte LDS store.  A step is three matrix instructions per
// accumulator: hi hi, hi lo, lo hi, always in that order; a channel group's steps sum into a partial accumulator and the groups'
// partials into the result (two levels, so that no chain of roundings is longer than a group's).  An A fragment past the last tap
// is set to zero, never read.
// Epilogue: scale, shift, activation and residual in fp32 on the accumulators, NO rounding: the tile goes through LDS as fp32 and is
// stored as row segments, 16 bytes per lane where the rows allow it.  No atomics, a fixed order of sums: identical calls give
// identical bits.
#include "elem16.h"
#include "fpn_conv_launch.h"

namespace {

using gfn::activate;
using gfn::bf16x8;
using gfn::ConvArgs;
using gfn::f32x16;
using gfn::f32x4;
using gfn::up2_blend;
using gfn::up2_taps;
using gfn::Up2Taps;

constexpr int kThreads = 256;
constexpr int kTW = 32, kTH = 16;                 // the output tile
constexpr int kWaveRows = kTH / (kThreads / 64);  // rows of it per wave
constexpr int kOutPitch = kTH * kTW + 4;          // floats per channel of the staged output tile: 16 bytes of padding

// (fpn_conv_half.hip's packing)
constexpr int units_padded(int K) { return (K * K + 3) / 4 * 4; }  // UP: units per channel group in the packed weight
constexpr int cout_padded(int Cout) { return Cout < 32 ? (Cout + 15) / 16 * 16 : (Cout + 31) / 32 * 32; }  // its rows

// the class's split of one operand
__device__ __forceinline__ void split(float v, __bf16 &hi, __bf16 &lo) {
    hi = (__bf16)v;
    const float h = (float)hi;
    lo = (__bf16)(__builtin_isfinite(h) ? v - h : 0.f);
}

// packed[e] = hi, packed[total + e] = lo of weight[co][8 cg + c][u], e = ((co CG + cg) UP + u) 8 + c; zero past Cout, Cin and KK
__global__ __launch_bounds__(256) void tf32_pack_kernel(const float *__restrict__ w, __bf16 *__restrict__ packed, int Cout, int Cin, int KK,
                                                        int CG, int UP, int total) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int c = e & 7, u = (e >> 3) % UP, cg = (e >> 3) / UP % CG, co = (e >> 3) / UP / CG;
    const int ci = cg * 8 + c;
    const float v = (co < Cout && ci < Cin && u < KK) ? w[((int64_t)co * Cin + ci) * KK + u] : 0.f;
    __bf16 hi, lo;
    split(v, hi, lo);
    packed[e] = hi;
    packed[total + e] = lo;
}

template <int K, int S>
struct Halo {
    static constexpr int IH = (kTH - 1) * S + K, IW = (kTW - 1) * S + K, HALF = (IW + 1) / 2, PITCH = S == 1 ? IW : 2 * HALF;
    static constexpr int SLOTS = IH * PITCH;  // 16-byte slots per channel group, for hi and again for lo
    // channel groups per stage: what fits in some 64 KiB, four at the most
    static constexpr int FIT = 64 * 1024 / (SLOTS * 32);
    static constexpr int NG = FIT < 1 ? 1 : (FIT > 4 ? 4 : FIT);
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
__device__ __forceinline__ f32x4 mma(bf16x8 a, bf16x8 b, f32x4 c) { return gfn::mfma32(a, b, c); }
__device__ __forceinline__ f32x16 mma(bf16x8 a, bf16x8 b, f32x16 c) { return gfn::mfma16(a, b, c); }

template <int K, int S, bool WIDE, int NT, int NG>
__global__ __launch_bounds__(kThreads) void conv_tf32_kernel(const ConvArgs a, const __bf16 *__restrict__ wpack, const int lo_off,
                                                             const int tiles_x, const int tiles_y, const int groups, const int CG) {
    typedef Halo<K, S> T;
    typedef typename Acc<WIDE>::type acc_t;
    constexpr int NW = WIDE ? 32 : 16;            // pixels and output channels of one MFMA tile
    constexpr int G = WIDE ? 2 : 4;               // units per MFMA
    constexpr int KK = K * K, UP = units_padded(K), NSTEP = (KK + G - 1) / G;
    constexpr int MPR = kTW / NW, MT = kWaveRows * MPR;  // pixel tiles per row and per wave
    constexpr int PAD = K / 2;
    constexpr int HALO_BYTES = NG * 2 * T::SLOTS * 16, OUT_BYTES = NW * kOutPitch * 4;
    __shared__ __attribute__((aligned(16))) unsigned char smem[HALO_BYTES > OUT_BYTES ? HALO_BYTES : OUT_BYTES];
    bf16x8 *tile = reinterpret_cast<bf16x8 *>(smem);  // [group][hi, lo][row][column]
    float *stage = reinterpret_cast<float *>(smem);

    unsigned bid = blockIdx.x;
    const int tx = bid % tiles_x;
    bid /= tiles_x;
    const int ty = bid % tiles_y;
    bid /= tiles_y;
    const int co0 = (bid % groups) * (NT * NW);
    const int b = bid / groups;

    const int Cin = a.C0 + a.C1;
    const int H0 = a.up0 ? a.H >> 1 : a.H, W0 = a.up0 ? a.W >> 1 : a.W;
    const float *__restrict__ x0b = a.x0 + (int64_t)b * a.C0 * H0 * W0;
    const float *__restrict__ x1b = a.x1 + (int64_t)b * a.C1 * a.H * a.W;  // (never read when C1 = 0)

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
            bf16x8 vh = bf16x8((__bf16)0.f), vl = bf16x8((__bf16)0.f);
            if ((unsigned)gy < (unsigned)a.H && (unsigned)gx < (unsigned)a.W) {
                const int c0 = (cg0 + cgl) * 8;
                const Up2Taps t = up2_taps(H0, W0, gy, gx);  // (used with up0 only)
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int ci = c0 + j;
                    if (ci >= Cin) continue;  // the padded channels of the last group stay zero
                    float v;
                    if (ci >= a.C0) {
                        v = x1b[((ci - a.C0) * a.H + gy) * a.W + gx];
                    } else if (a.up0) {
                        const float *__restrict__ p = x0b + ci * H0 * W0;
                        v = up2_blend(t, p[t.y0 * W0 + t.x0], p[t.y0 * W0 + t.x1], p[t.y1 * W0 + t.x0], p[t.y1 * W0 + t.x1]);
                    } else {
                        v = x0b[(ci * a.H + gy) * a.W + gx];
                    }
                    __bf16 hi, lo;
                    split(v, hi, lo);
                    vh[j] = hi, vl[j] = lo;
                }
            }
            const int slot = (cgl * 2 * T::IH + r) * T::PITCH + T::place(x);
            tile[slot] = vh;
            tile[slot + T::SLOTS] = vl;
        }
        __syncthreads();
#pragma unroll 1
        for (int cgl = 0; cgl < ng; ++cgl) {
            const bf16x8 *th = tile + cgl * 2 * T::SLOTS, *tl = th + T::SLOTS;
            // row co0 + n of the packed weight's hi image, channel group cg0 + cgl: UP units of 8; the lo image lies lo_off further
            const __bf16 *__restrict__ wrow = wpack + ((co0 + n) * CG + (cg0 + cgl)) * (UP * 8);
            // the sums are two-level: a channel group's 3 NSTEP instructions chain into `part`, the groups' parts into acc.  One chain
            // over all of them (120 links at 64 input channels, 3 x 3) walks some sqrt(120) roundings away from the sum; torch's own fp32
            // convolution, the unit the training tests measure in, stays nearer than a quarter of that
            acc_t part[MT][NT];
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int t = 0; t < NT; ++t) part[m][t] = acc_t(0.f);
#pragma unroll
            for (int s = 0; s < NSTEP; ++s) {
                const int u = s * G + g, uc = min(u, KK - 1), ky = uc / K, kx = uc - ky * K;
                const bool valid = u < KK;
                const int off = ky * T::PITCH + (S == 1 ? kx : (kx & 1) * T::HALF + (kx >> 1));
                bf16x8 bh[NT], bl[NT];
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    bh[t] = *reinterpret_cast<const bf16x8 *>(wrow + t * NW * CG * (UP * 8) + u * 8);
                    bl[t] = *reinterpret_cast<const bf16x8 *>(wrow + lo_off + t * NW * CG * (UP * 8) + u * 8);
                }
#pragma unroll
                for (int m = 0; m < MT; ++m) {
                    bf16x8 ah = th[base[m] + off], al = tl[base[m] + off];
                    if (!valid) ah = bf16x8((__bf16)0.f), al = bf16x8((__bf16)0.f);
#pragma unroll
                    for (int t = 0; t < NT; ++t) {
                        part[m][t] = mma(ah, bh[t], part[m][t]);
                        part[m][t] = mma(ah, bl[t], part[m][t]);
                        part[m][t] = mma(al, bh[t], part[m][t]);
                    }
                }
            }
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int t = 0; t < NT; ++t) acc[m][t] += part[m][t];
        }
    }

    const int64_t ob = (int64_t)b * a.Cout * a.Ho * a.Wo;
    // every 4-pixel segment of a row is then whole and 16-byte aligned
    const bool vec = (a.Wo & 3) == 0 && (reinterpret_cast<uintptr_t>(a.out) & 15u) == 0;
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
                    f32x4 h;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float v = activate(fmaf(acc[m][t][4 * q + r], sc, sh), a.act, a.slope);
                        const int ox = tx * kTW + px + r;
                        if (a.residual && oy < a.Ho && ox < a.Wo) v += a.residual[ob + ((int64_t)co * a.Ho + oy) * a.Wo + ox];
                        h[r] = v;
                    }
                    *reinterpret_cast<f32x4 *>(stage + n * kOutPitch + rl * kTW + px) = h;
                }
            }
        }
        __syncthreads();
        for (int i = tid; i < NW * kTH * (kTW / 4); i += kThreads) {
            const int seg = i % (kTW / 4), rl = i / (kTW / 4) % kTH, c = i / (kTW / 4 * kTH);
            const int co = co0 + t * NW + c, oy = ty * kTH + rl, ox = tx * kTW + seg * 4;
            if (co >= a.Cout || oy >= a.Ho || ox >= a.Wo) continue;
            const f32x4 v = *reinterpret_cast<const f32x4 *>(stage + c * kOutPitch + rl * kTW + seg * 4);
            float *dst = a.out + ob + ((int64_t)co * a.Ho + oy) * a.Wo + ox;
            if (vec) {
                *reinterpret_cast<f32x4 *>(dst) = v;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (ox + j < a.Wo) dst[j] = v[j];
            }
        }
    }
}

template <int K, int S, bool WIDE, int NT>
int launch(const ConvArgs &a, int B, int CG, const __bf16 *wpack, int lo_off, hipStream_t s) {
    constexpr int NG = Halo<K, S>::NG;
    const int tiles_x = (a.Wo + kTW - 1) / kTW, tiles_y = (a.Ho + kTH - 1) / kTH;
    const int cout_pad = cout_padded(a.Cout), groups = cout_pad / (NT * (WIDE ? 32 : 16));
    const int64_t blocks = (int64_t)tiles_x * tiles_y * groups * B;
    if (blocks > 0x7fffffffLL) return gfn::fail(GFN_ERR_INVALID_ARG, "fpn_conv_tf32_launch: %lld workgroups exceed the grid", (long long)blocks);
    hipLaunchKernelGGL((conv_tf32_kernel<K, S, WIDE, NT, NG>), dim3((unsigned)blocks), dim3(kThreads), 0, s, a, wpack, lo_off, tiles_x, tiles_y,
                       groups, CG);
    return gfn::check_launch("conv_tf32_kernel");
}

// 16-wide tiles below 32 output channels (two column tiles where the padded Cout is 32), 32-wide from there
template <int K, int S>
int launch_shape(const ConvArgs &a, int B, int CG, const __bf16 *wpack, int lo_off, hipStream_t s) {
    if (a.Cout < 32)
        return cout_padded(a.Cout) == 32 ? launch<K, S, false, 2>(a, B, CG, wpack, lo_off, s) : launch<K, S, false, 1>(a, B, CG, wpack, lo_off, s);
    return launch<K, S, true, 1>(a, B, CG, wpack, lo_off, s);
}

template <int K>
int launch_stride(const ConvArgs &a, int S, int B, int CG, const __bf16 *wpack, int lo_off, hipStream_t s) {
    return S == 1 ? launch_shape<K, 1>(a, B, CG, wpack, lo_off, s) : launch_shape<K, 2>(a, B, CG, wpack, lo_off, s);
}

// ---- the weight gradient, stride 1 without up0 -----------------------------------------------------------------------------------
// d_weight[co][ci, ky, kx] = sum over b, y, x of gu[b, co, y, x] x[b, ci, y + ky - p, x + kx - p] as a GEMM on v_mfma_f32_16x16x32_bf16:
// M = Cout (A: gu), N = Cin K K (B: the shifted x), the summed index the pixels; a fragment of either operand is eight consecutive
// pixels of one plane row, both split as above.  Grid (parts, input-channel groups, blocks of 16 output channels) -- fpn_conv_train.hip's
// WgradShape, so the partials and ft_wsum_kernel are the fp32 path's.  A workgroup walks the 8 x 32 pixel tiles slot, slot + parts, ...:
// it stages the zero-padded halo rows of its `cig` input channels in LDS, one 32-bit word per pixel holding hi (low half) and lo, so
// that a B fragment at any shift is eight aligned 4-byte reads; the A fragment of a tile row comes straight from memory and serves every
// item.  Wave w owns the 16-item column tiles w, w + 4, ... (items = cig K K <= 256: four at the most).  A tile's 24 instructions chain
// into a partial accumulator, the tiles' partials into the total (two levels, as in the convolution); the total is stored once, every
// (co, ci, ky, kx) of the partial by exactly one lane.  No atomics, a fixed order.
constexpr int kWgRows = 8, kWgCols = 32, kWgJ = 4;

__global__ __launch_bounds__(256) void wgrad_tf32_kernel(const float *__restrict__ x0, const float *__restrict__ x1, const float *__restrict__ gu,
                                                         float *__restrict__ part, int C0, int C1, int H, int W, int Cout, int K, int IH, int IW,
                                                         int PITCH, int cig, int tiles_x, int tiles_y, int64_t ntiles) {
    extern __shared__ unsigned xs[];  // [channel of the group][halo row][halo column]: bf16 hi | bf16 lo << 16
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = lane & 15, g = lane >> 4;
    const int Cin = C0 + C1, KK = K * K, pad = K / 2;
    const int ci0 = blockIdx.y * cig, co0 = blockIdx.z * 16;
    const int items = cig * KK, njt = (items + 15) / 16;

    // the lane's item of its wave's q-th column tile: where its tap (0, 0) pixel of tile row 0, unit g lies in xs
    int off[kWgJ], ci_l[kWgJ], tap[kWgJ];
    bool valid[kWgJ];
#pragma unroll
    for (int q = 0; q < kWgJ; ++q) {
        const int item = (wave + 4 * q) * 16 + n;
        valid[q] = item < items;
        ci_l[q] = valid[q] ? item / KK : 0;
        tap[q] = valid[q] ? item % KK : 0;
        off[q] = (ci_l[q] * IH + tap[q] / K) * PITCH + tap[q] % K + 8 * g;
    }
    f32x4 total[kWgJ];
#pragma unroll
    for (int q = 0; q < kWgJ; ++q) total[q] = f32x4(0.f);

    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int tx = (int)(t % tiles_x), ty = (int)(t / tiles_x % tiles_y), b = (int)(t / ((int64_t)tiles_x * tiles_y));
        const int iy0 = ty * kWgRows - pad, ix0 = tx * kWgCols - pad;
        __syncthreads();  // the previous tile has been consumed
        for (int e = tid; e < cig * IH * IW; e += 256) {
            const int c = e / (IH * IW), rem = e - c * (IH * IW), r = rem / IW, xx = rem - r * IW;
            const int ci = ci0 + c, gy = iy0 + r, gx = ix0 + xx;
            float v = 0.f;
            if (ci < Cin && (unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W)
                v = ci < C0 ? x0[((int64_t)b * C0 + ci) * H * W + (int64_t)gy * W + gx] : x1[((int64_t)b * C1 + (ci - C0)) * H * W + (int64_t)gy * W + gx];
            __bf16 hi, lo;
            split(v, hi, lo);
            xs[(c * IH + r) * PITCH + xx] = (unsigned)__builtin_bit_cast(unsigned short, hi) | ((unsigned)__builtin_bit_cast(unsigned short, lo) << 16);
        }
        __syncthreads();
        f32x4 acc[kWgJ];
#pragma unroll
        for (int q = 0; q < kWgJ; ++q) acc[q] = f32x4(0.f);
        const int co = co0 + n;
#pragma unroll 1
        for (int r = 0; r < kWgRows; ++r) {
            const int oy = ty * kWgRows + r;
            bf16x8 ah = bf16x8((__bf16)0.f), al = bf16x8((__bf16)0.f);
            if (co < Cout && oy < H) {
                const float *__restrict__ gp = gu + ((int64_t)b * Cout + co) * H * W + (int64_t)oy * W;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int ox = tx * kWgCols + 8 * g + j;
                    if (ox >= W) continue;
                    __bf16 hi, lo;
                    split(gp[ox], hi, lo);
                    ah[j] = hi, al[j] = lo;
                }
            }
#pragma unroll
            for (int q = 0; q < kWgJ; ++q) {
                if (wave + 4 * q >= njt) continue;  // (uniform over the wave)
                bf16x8 bh = bf16x8((__bf16)0.f), bl = bf16x8((__bf16)0.f);
                if (valid[q]) {
                    const unsigned *p = xs + off[q] + r * PITCH;
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const unsigned w2 = p[j];
                        bh[j] = __builtin_bit_cast(__bf16, (unsigned short)(w2 & 0xffffu));
                        bl[j] = __builtin_bit_cast(__bf16, (unsigned short)(w2 >> 16));
                    }
                }
                acc[q] = gfn::mfma32(ah, bh, acc[q]);
                acc[q] = gfn::mfma32(ah, bl, acc[q]);
                acc[q] = gfn::mfma32(al, bh, acc[q]);
            }
        }
#pragma unroll
        for (int q = 0; q < kWgJ; ++q) total[q] += acc[q];
    }

    // the lane holds rows 4 g .. 4 g + 3 (output channels) of column n (its item) of every tile (common.h: acc_row)
    float *dst = part + (int64_t)blockIdx.x * Cout * Cin * KK;
#pragma unroll
    for (int q = 0; q < kWgJ; ++q) {
        const int ci = ci0 + ci_l[q];
        if (!valid[q] || wave + 4 * q >= njt || ci >= Cin) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int co = co0 + 4 * g + r;
            if (co < Cout) dst[((int64_t)co * Cin + ci) * KK + tap[q]] = total[q][r];
        }
    }
}

}  // namespace

int gfn::fpn_wgrad_tf32_launch(const float *x0, const float *x1, const float *gu, float *part, int C0, int C1, int H, int W, int Cout, int K,
                               int IH, int IW, int PITCH, int cig, int nci, int parts, int tiles_x, int tiles_y, int64_t ntiles, hipStream_t s) {
    if (cig * K * K > 16 * 4 * kWgJ)
        return gfn::fail(GFN_ERR_INVALID_ARG, "fpn_wgrad_tf32_launch: %d items per input-channel group exceed %d", cig * K * K, 16 * 4 * kWgJ);
    const dim3 grid((unsigned)parts, (unsigned)nci, (unsigned)((Cout + 15) / 16));
    hipLaunchKernelGGL(wgrad_tf32_kernel, grid, dim3(256), (size_t)cig * IH * PITCH * sizeof(unsigned), s, x0, x1, gu, part, C0, C1, H, W, Cout, K,
                       IH, IW, PITCH, cig, tiles_x, tiles_y, ntiles);
    return gfn::check_launch("wgrad_tf32_kernel");
}

int64_t gfn::fpn_conv_tf32_pack_bytes(int Cout, int Cin, int K) {
    return (int64_t)cout_padded(Cout) * ((Cin + 7) / 8) * units_padded(K) * 8 * 2 * (int64_t)sizeof(__bf16);
}

int gfn::fpn_conv_tf32_launch(const ConvArgs &a, int B, int K, int stride, void *pack, hipStream_t s) {
    const int Cin = a.C0 + a.C1, CG = (Cin + 7) / 8, UP = units_padded(K);
    const int64_t total = fpn_conv_tf32_pack_bytes(a.Cout, Cin, K) / (2 * (int64_t)sizeof(__bf16));
    if (a.Cout % 8 || 2 * total > 0x7fffffffLL)
        return gfn::fail(GFN_ERR_INVALID_ARG, "fpn_conv_tf32_launch: Cout %d is not a multiple of 8, or a packed weight of 2^31 values or more", a.Cout);
    __bf16 *packed = static_cast<__bf16 *>(pack);
    hipLaunchKernelGGL(tf32_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a.weight, packed, a.Cout, Cin, K * K, CG, UP,
                       (int)total);
    if (int rc = gfn::check_launch("tf32_pack_kernel")) return rc;
    switch (K) {
        case 1: return launch_stride<1>(a, stride, B, CG, packed, (int)total, s);
        case 3: return launch_stride<3>(a, stride, B, CG, packed, (int)total, s);
        case 5: return launch_stride<5>(a, stride, B, CG, packed, (int)total, s);
        default: return launch_stride<7>(a, stride, B, CG, packed, (int)total, s);
    }
}

GFN_EXPORT int64_t gfn_conv2d_bn_act_tf32_ws_bytes(int C0, int C1, int Cout, int K) {
    if (C0 < 1 || C1 < 0 || Cout < 1 || Cout > 256 || Cout % 8 || (K != 1 && K != 3 && K != 5 && K != 7) || (int64_t)C0 + C1 > 0x7fffffffLL) return 0;
    return gfn::fpn_conv_tf32_pack_bytes(Cout, C0 + C1, K);
}

GFN_EXPORT int gfn_conv2d_bn_act_tf32_fwd(const float *x0, int C0, int up0, const float *x1, int C1, const float *weight, const float *scale,
                                          const float *shift, const float *residual, float *out, int B, int H, int W, int Cout, int K,
                                          int stride, int act, float slope, void *ws, int64_t ws_bytes, gfn_stream_t stream) {
    const char *what = "gfn_conv2d_bn_act_tf32_fwd";
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
    const int64_t in0 = (int64_t)C0 * (up0 ? H / 2 : H) * (up0 ? W / 2 : W) * 4, in1 = (int64_t)C1 * H * W * 4,
                  outb = (int64_t)Cout * Ho * Wo * 4;
    if (in0 >= limit || in1 >= limit || outb >= limit)
        return gfn::fail(GFN_ERR_INVALID_ARG, "%s: a per-image map of 2^31 bytes or more (x0 %lld, x1 %lld, out %lld bytes)", what,
                         (long long)in0, (long long)in1, (long long)outb);
    if ((int64_t)(C0 + C1) * K * K * Cout * 4 >= limit) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: weight of 2^31 bytes or more", what);
    const int64_t need = gfn::fpn_conv_tf32_pack_bytes(Cout, C0 + C1, K);
    if (need >= limit) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: packed weight of 2^31 bytes or more", what);
    if (B == 0) return GFN_OK;
    if (!x0 || !weight || !scale || !shift || !out || (C1 > 0 && !x1)) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: null pointer", what);
    if (!ws || (reinterpret_cast<uintptr_t>(ws) & 15u) || ws_bytes < need)
        return gfn::fail(GFN_ERR_SCRATCH, "%s: workspace missing, not 16-byte aligned or too small (%lld bytes needed)", what, (long long)need);

    const ConvArgs a{x0, x1, weight, scale, shift, residual, out, C0, C1, up0 ? 1 : 0, H, W, Cout, Ho, Wo, act, slope};
    return gfn::fpn_conv_tf32_launch(a, B, K, stride, ws, (hipStream_t)stream);
}
