// pw_gemm_tile.h -- what the refiner conv kernels say about the fp32 matrix-core tile of a 1x1 conv, once: a workgroup of 4 waves
// owns 32*MT output rows x 128 cells of one map and walks K in tiles of 16; per K tile the A operand tile (weights) and the B
// operand tile Bs[k][cell] sit in LDS, and every wave multiplies its 32 cells into MT accumulators with v_mfma_f32_32x32x2_f32,
// k ascending.  Users: pw_gemm_kernel (conv_stack.hip), ct_pw_fwd_kernel, ct_pw_bwd_kernel and -- accumulators only --
// ct_pw_wgrad_kernel (conv_stack_train.hip); the fused block (conv_block_fused.h) takes the constants.  The kernels differ in how
// the operands reach LDS and in what their epilogues do with a (row, value).  Opens its own anonymous namespace.
#pragma once
#include <type_traits>

#include "common.h"

namespace {

using gfn::f32x16;

constexpr int kKT = 16;   // channels per K tile
constexpr int kBN = 128;  // cells per workgroup tile: 4 waves x 32

// four cells of a map row (any N: the tail cell by cell); cells past N read as zero
__device__ __forceinline__ float4 load_cells(const float *src, int n, int N) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if ((N & 3) == 0) {
        if (n < N) v = *reinterpret_cast<const float4 *>(src);
    } else {
        if (n < N) v.x = src[0];
        if (n + 1 < N) v.y = src[1];
        if (n + 2 < N) v.z = src[2];
        if (n + 3 < N) v.w = src[3];
    }
    return v;
}

// B operand tile of K tile k0: Bs[k][cell] = row(k0 + k)(map[k0 + k][n0 + cell]) of a (K, N) map -- row(kk) hands back the
// per-element functor of channel kk; rows past K and cells past N are zero whatever that functor makes of a zero
template <typename R>
__device__ __forceinline__ void stage_cells(float (*Bs)[kBN], const float *map, int k0, int K, int n0, int N, int tid, R row) {
    for (int e = tid; e < kKT * (kBN / 4); e += 256) {
        const int k = e / (kBN / 4), n4 = e - k * (kBN / 4);
        const int kk = k0 + k, n = n0 + n4 * 4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (kk < K) {
            const auto f = row(kk);
            const float4 raw = load_cells(map + (size_t)kk * N + n, n, N);
            v.x = n < N ? f(raw.x) : 0.f;
            v.y = n + 1 < N ? f(raw.y) : 0.f;
            v.z = n + 2 < N ? f(raw.z) : 0.f;
            v.w = n + 3 < N ? f(raw.w) : 0.f;
        }
        *reinterpret_cast<float4 *>(&Bs[k][n4 * 4]) = v;
    }
}
// the functor of a map that is staged as it is
struct AsItIs {
    __device__ __forceinline__ auto operator()(int) const {
        return [](float v) { return v; };
    }
};

// the accumulators of a wave: MT row tiles of 32 rows x its 32 cells; lane (col = lane & 31, kh = lane >> 5)
template <int MT>
struct PwAcc {
    f32x16 a[MT];

    __device__ __forceinline__ void zero() {
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) a[i][r] = 0.f;
    }
    // one K tile: A operand As[k][row] at the kernel's own pitch AP, B operand Bs[k][wave * 32 + cell]
    template <int AP>
    __device__ __forceinline__ void products(const float (*As)[AP], const float (*Bs)[kBN], int wave, int col, int kh) {
#pragma unroll
        for (int s = 0; s < kKT / 2; ++s) {
            const float bv = Bs[2 * s + kh][wave * 32 + col];
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                const float av = As[2 * s + kh][i * 32 + col];
                a[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, a[i], 0, 0, 0);
            }
        }
    }
    // f(row of the 32*MT, value) for the 16*MT values of this lane; their cell is the lane's col
    template <typename F>
    __device__ __forceinline__ void each(int kh, F f) const {
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) f(i * 32 + gfn::acc_row(r, kh), a[i][r]);
    }
};

// rows of a 1x1 GEMM's output: as few workgroups along them as possible with <= 7 row tiles (112 accumulators) each
inline void slab_shape(int rows, int *nblk, int *mt) {
    const int tiles = (rows + 31) / 32;
    *nblk = (tiles + 6) / 7;
    *mt = (tiles + *nblk - 1) / *nblk;
}

// f(std::integral_constant<int, MT>) for the mt = 1 .. 7 of slab_shape
template <int MT = 7, typename F>
void with_row_tiles(int mt, F &&f) {
    if (MT > 1 && mt < MT) return with_row_tiles<(MT > 1 ? MT - 1 : 1)>(mt, f);
    f(std::integral_constant<int, MT>());
}

}  // namespace
