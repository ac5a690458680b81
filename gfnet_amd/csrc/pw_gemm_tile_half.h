// pw_gemm_tile_half.h -- the fp16 matrix-core tile of a 1x1 conv in the training class with fp16 maps (conv_stack_train_half.hip),
// beside the exact-fp32 tile of pw_gemm_tile.h whose accumulators (PwAcc) and 128-cell workgroup tile it keeps.
// v_mfma_f32_32x32x16_f16: lane (col = lane & 31, kh = lane >> 5) supplies A[row col][k = 8 kh + j] and B[k = 8 kh + j][column col],
// j = 0 .. 7, as eight halves of one register quad, and receives D[row acc_row(r, kh)][column col].  So both operand tiles lie in
// LDS as [row or column][k] with k contiguous, and a lane's fragment is one 16-byte read.  The pitch is the K tile plus 8 halves:
// rows 80, 144 or 272 bytes apart start 20, 36 or 4 banks apart, and the 16 lanes a 16-byte read serves at a time cover all 64
// banks once.  Opens its own anonymous namespace.
#pragma once
#include "pw_gemm_tile.h"

namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

constexpr int kHKT = 32;  // channels per K tile of the forward and the input-gradient GEMM: two MFMA steps
constexpr int half_pitch(int kt) { return kt + 8; }

// float -> fp16 is v_cvt_f16_f32: to nearest even, and past 65504 to inf -- never a clamp, or overflow would be hidden from the
// loss scaler.  as_half_value: the float a map of either type holds once it is an fp16 operand
__device__ __forceinline__ float as_half_value(float v) { return (float)(_Float16)v; }
__device__ __forceinline__ float as_half_value(_Float16 v) { return (float)v; }

// An operand tile T[ROWS][half_pitch(KT)]: every thread fills 16-byte pieces, piece(row, k8) handing back the eight halves
// T[row][k8 .. k8 + 7] (zeros where the source ends).  ROWS_FIRST: consecutive lanes take consecutive rows -- for a source whose
// rows are contiguous in memory and whose k is strided (a map's cells under its channels); otherwise consecutive lanes take
// consecutive pieces of one row (a source with k contiguous).
template <int ROWS, int KT, bool ROWS_FIRST, typename V>
__device__ __forceinline__ void stage_half_tile(_Float16 *T, int tid, V piece) {
    constexpr int P = half_pitch(KT), G8 = KT / 8;
    for (int e = tid; e < ROWS * G8; e += 256) {
        const int row = ROWS_FIRST ? e % ROWS : e / G8, k8 = (ROWS_FIRST ? e / ROWS : e % G8) * 8;
        *reinterpret_cast<f16x8 *>(&T[row * P + k8]) = piece(row, k8);
    }
}

// eight consecutive halves src[0 .. 7] of which the first `valid` exist; vec: src is 16-byte aligned (the caller's promise)
__device__ __forceinline__ f16x8 load_half8(const _Float16 *src, int valid, bool vec) {
    if (vec && valid >= 8) return *reinterpret_cast<const f16x8 *>(src);
    f16x8 h;
#pragma unroll
    for (int j = 0; j < 8; ++j) h[j] = j < valid ? src[j] : (_Float16)0.f;
    return h;
}

// STEPS MFMA steps of 16 k: a, b point at the lane's own fragment of the first step (row or column `col`, k = 8 kh) in tiles of
// pitch AP and BP; row tile i of A lies 32 rows further
template <int MT, int STEPS, int AP>
__device__ __forceinline__ void half_products(PwAcc<MT> &acc, const _Float16 *a, const _Float16 *b) {
#pragma unroll
    for (int s = 0; s < STEPS; ++s) {
        const f16x8 bv = *reinterpret_cast<const f16x8 *>(b + 16 * s);
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            const f16x8 av = *reinterpret_cast<const f16x8 *>(a + i * 32 * AP + 16 * s);
            acc.a[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(av, bv, acc.a[i], 0, 0, 0);
        }
    }
}

}  // namespace
