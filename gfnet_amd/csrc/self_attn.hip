// Self-attention forward of the DINOv2 ViT at head dim 64 (reference model/transformer/layers/attention.py:77-101, where
// F.scaled_dot_product_attention does this work): out = softmax(scale * Q K^T) V per (batch, head) on the PACKED projection,
// qkv (B, N, 3, H, 64) fp16 as `self.qkv(x).reshape(B, N, 3, H, C // H)` leaves it -> out (B, N, H, 64).  Forward only: the ViT is
// frozen.  Nothing N x N is written, no scratch, no atomics.  The kernel is written once over the 16-bit element T, _Float16 or __bf16
// (the bf16 autocast class): only the two products' instruction and the two roundings (P, out) know the format; staging, the permuted
// k order, the pitches, the tail selects and the fp32 softmax between the products are the same text for both.
//
// Orientation (as 4.7): S^T = K Q^T, so a query sits on a lane (column = lane & 31) and the 32 keys of a tile in the
// lane's 16 accumulator registers (rows acc_row(r, lane >> 5)): running maximum and sum are per-lane registers.  The tile of
// weights P^T is then ALREADY the B operand of the next product O^T = V^T P^T, which sums over its row index: registers 8s..8s+7,
// rounded to T, are the fragment of k-step s, with no trip through LDS.  Inside such a step the k order is permuted -- element j
// of lane half h is key 16s + 8(j >> 2) + 4h + (j & 3) of the tile -- so the V^T fragment is gathered in that same order
// (vt_frag); tests/test_self_attn_gpu.py::test_layout_exact fails for any other order.
#include <climits>

#include "attn_common.h"

namespace {

using namespace gfn;
using namespace gfn::attn;

constexpr int kD = 64;         // head dim: four k-steps of v_mfma_f32_32x32x16_{f16,bf16} per score tile
constexpr int kThreads = 256;  // 4 waves, 32 queries each
constexpr int kOwn = 128;      // queries per workgroup
constexpr int kChunk = 64;     // keys staged per step (2 tiles)
// LDS pitches in elements.  K rows (read as 16 bytes at [key][16s + 8h]): 128-byte rows would put every key in the same banks; 144
// bytes moves consecutive keys 36 banks on, so 16 lanes' reads cover all 64 banks once.  V^T rows (read as 8 bytes at
// [d][key 16s + 4h] and + 8): 136 bytes moves consecutive d 34 banks on, 32 lanes' reads cover 64 banks once.
constexpr int kKPitch = 72, kVPitch = 68;

// the 16-byte piece of a staged chunk that piece index p (0..511) names: key p >> 3 of the chunk, values 8 (p & 7) ...
template <typename T>
__device__ __forceinline__ typename Elem16<T>::vec8 load_piece(const T *__restrict__ base, int64_t token_stride, int key0, int N, int p) {
    using t8 = typename Elem16<T>::vec8;
    const int key = key0 + (p >> 3);
    t8 z = {};
    return key < N ? *reinterpret_cast<const t8 *>(base + key * token_stride + 8 * (p & 7)) : z;  // a key past N is staged as zeros
}

template <typename T>
__global__ __launch_bounds__(kThreads) void self_attn_fwd_kernel(const T *__restrict__ qkv, T *__restrict__ out, int N, int H, int nqb,
                                                                 float scale) {
    using t4 = typename Elem16<T>::vec4;
    using t8 = typename Elem16<T>::vec8;
    __shared__ alignas(16) T ks[kChunk * kKPitch];  // K rows as stored: the A operand of S^T = K Q^T
    __shared__ alignas(16) T vt[kD * kVPitch];      // V transposed, [d][key]: the A operand of O^T = V^T P^T
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, c = lane & 31;
    const int qb = blockIdx.x % nqb, bh = blockIdx.x / nqb, b = bh / H, hd = bh % H;
    const int64_t token_stride = (int64_t)3 * H * kD;
    const T *qbase = qkv + (int64_t)b * N * token_stride + hd * kD;
    const T *kbase = qbase + H * kD, *vbase = kbase + H * kD;

    const int qi = qb * kOwn + wave * 32 + c;
    const bool qok = qi < N;
    t8 qf[4];  // B operand of k-step s: Q[query c][16s + 8h + j]
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        t8 z = {};
        qf[s] = qok ? *reinterpret_cast<const t8 *>(qbase + qi * token_stride + 16 * s + 8 * h) : z;
    }

    float m = -INFINITY, l = 0.f;
    f32x16 o[2] = {};  // O^T: register r of tile dt is value d = 32 dt + acc_row(r, h) of query c

    t8 kreg[2], vreg[2];  // the next chunk on its way: pieces tid and tid + 256 of K and of V
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        kreg[i] = load_piece(kbase, token_stride, 0, N, tid + kThreads * i);
        vreg[i] = load_piece(vbase, token_stride, 0, N, tid + kThreads * i);
    }

    for (int k0 = 0; k0 < N; k0 += kChunk) {
        __syncthreads();  // the previous chunk has been consumed
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int p = tid + kThreads * i, key = p >> 3, g = p & 7;
            *reinterpret_cast<t8 *>(&ks[key * kKPitch + 8 * g]) = kreg[i];
#pragma unroll
            for (int e = 0; e < 8; ++e) vt[(8 * g + e) * kVPitch + key] = vreg[i][e];
        }
        __syncthreads();
        if (k0 + kChunk < N) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                kreg[i] = load_piece(kbase, token_stride, k0 + kChunk, N, tid + kThreads * i);
                vreg[i] = load_piece(vbase, token_stride, k0 + kChunk, N, tid + kThreads * i);
            }
        }
        const int left = N - k0, ntile = left >= kChunk ? kChunk / 32 : (left + 31) / 32;
#pragma unroll 1
        for (int t = 0; t < ntile; ++t) {
            f32x16 s = {};
#pragma unroll
            for (int st = 0; st < 4; ++st) {
                const t8 kf = *reinterpret_cast<const t8 *>(&ks[(t * 32 + c) * kKPitch + 16 * st + 8 * h]);
                s = mfma16(kf, qf[st], s);
            }
            // The loop is bound by its vector instructions, not by its 8 matrix instructions, so the two things only some tiles need
            // sit behind wave-uniform tests: the selects on the key index (only a tile that reaches past N: `tail`), and the
            // rescale of l and of the 32 results (only where some query's maximum moved; multiplying by 1 changes no bit).
            const bool tail = t * 32 + 32 > left;
            // scaled scores are rounded once, as the definition's `s * scale` is
            float tv[16], mx = m;
#pragma unroll
            for (int r = 0; r < 16; ++r) tv[r] = s[r] * scale;
            if (tail) {
                // a key past the end is left out of the maximum and given -inf: exp2 then makes its weight exactly zero, by its
                // index and not by a finite sentinel (a select per row, never a branch per row)
#pragma unroll
                for (int r = 0; r < 16; ++r) tv[r] = t * 32 + acc_row(r, h) < left ? tv[r] : -INFINITY;
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) mx = fmaxf(mx, tv[r]);
            // the two lane halves of a query hold different keys of the tile but feed ONE product: they share the maximum (every tile
            // has a key below `left` in half 0, so mx is finite from the first tile on)
            mx = fmaxf(mx, other_half(mx));
            const float alpha = (m == -INFINITY) ? 0.f : hw_exp2((m - mx) * kLog2e);
            if (__any(alpha != 1.f)) {
                l *= alpha;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    o[0][r] *= alpha;
                    o[1][r] *= alpha;
                }
            }
            t8 pf[2];  // B operand of k-step s of O^T = V^T P^T: registers 8s..8s+7 as they are (permuted k order, see vt_frag below)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float p = hw_exp2((tv[r] - mx) * kLog2e);  // (-inf - mx) * c = -inf: exactly 0 for a key past the end
                l += p;
                pf[r >> 3][r & 7] = (T)p;  // rounded to nearest even once; in fp16 it is lost below 2^-25
            }
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) {
#pragma unroll
                for (int st = 0; st < 2; ++st) {
                    // vt_frag: element j of lane half h must be the V of the key that element j of pf[st] weighs,
                    // key 16 st + 8 (j >> 2) + 4h + (j & 3) of the tile: two runs of four keys
                    const T *row = &vt[(32 * dt + c) * kVPitch + t * 32 + 16 * st + 4 * h];
                    const t4 lo = *reinterpret_cast<const t4 *>(row), hi = *reinterpret_cast<const t4 *>(row + 8);
                    const t8 vf = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                    o[dt] = mfma16(vf, pf[st], o[dt]);
                }
            }
            m = mx;
        }
    }
    l += other_half(l);  // both halves summed their keys' weights under the shared maximum
    if (qok) {
        T *orow = out + (((int64_t)b * N + qi) * H + hd) * kD;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {  // registers 4g..4g+3 are values d = 32 dt + 8g + 4h + 0..3; rounded once, fp16 overflow to inf
                t4 v;
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = (T)(o[dt][4 * g + j] / l);
                *reinterpret_cast<t4 *>(orow + 32 * dt + 8 * g + 4 * h) = v;
            }
        }
    }
}

template <typename T>
void launch(const void *qkv, void *out, int B, int N, int H, int nqb, float scale, hipStream_t s) {
    hipLaunchKernelGGL(self_attn_fwd_kernel<T>, dim3((unsigned)(B * H * nqb)), dim3(kThreads), 0, s, (const T *)qkv, (T *)out, N, H, nqb, scale);
}

}  // namespace

GFN_EXPORT int gfn_self_attn_fwd(const void *qkv, int dtype, int B, int N, int H, int D, float scale, void *out, gfn_stream_t stream) {
    const char *what = "gfn_self_attn_fwd";
    if (D != kD) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: head dim %d is not supported, only D = 64 (four 32x32x16 matrix steps per score tile)", what, D);
    if (dtype != GFN_F16 && dtype != GFN_BF16) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: dtype must be GFN_F16 or GFN_BF16, got %d", what, dtype);
    if (B < 0 || N < 1 || H < 1) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: bad size (B=%d N=%d H=%d)", what, B, N, H);
    if (!std::isfinite(scale)) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: scale must be finite", what);
    if (B == 0) return GFN_OK;
    const int nqb = (N + kOwn - 1) / kOwn;
    if ((int64_t)B * H * nqb > INT_MAX)
        return gfn::fail(GFN_ERR_INVALID_ARG, "%s: B * H * ceil(N / %d) is the grid, at most 2^31 - 1 (B=%d N=%d H=%d)", what, kOwn, B, N, H);
    if (!qkv || !out) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: null pointer (%s)", what, !qkv ? "qkv" : "out");
    if (((uintptr_t)qkv | (uintptr_t)out) & 15) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: qkv and out must be 16-byte aligned (rows are read as vectors)", what);
    return with_elem16(dtype, [&](auto e) {
        launch<decltype(e)>(qkv, out, B, N, H, nqb, scale, (hipStream_t)stream);
        return gfn::check_launch("self_attn_fwd_kernel");
    });
}
