// What the two attention files (cross_attn.hip at head dim 8, self_attn.hip at head dim 64) both need in their kernels: the base-2
// exponential and its constants, the cross-half shuffle and the 16-bit vector types with their 32x32x8 and 32x32x16 matrix
// instructions.
#pragma once
#include <hip/hip_fp16.h>

#include <cmath>

#include "common.h"

namespace gfn {
namespace attn {

constexpr float kLog2e = 1.4426950408889634f;
constexpr float kLn2 = 0.6931471805599453f;

typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef __bf16 b4 __attribute__((ext_vector_type(4)));
typedef __bf16 b8 __attribute__((ext_vector_type(8)));

// four values of a 16-bit element as one register pair: an operand fragment of the 32x32x8 step and an 8-byte access
template <typename T>
struct Vec4;
template <>
struct Vec4<_Float16> {
    typedef h4 type;
};
template <>
struct Vec4<__bf16> {
    typedef b4 type;
};

// eight values as one register quad: an operand fragment of the 32x32x16 step and a 16-byte access
template <typename T>
struct Vec8;
template <>
struct Vec8<_Float16> {
    typedef h8 type;
};
template <>
struct Vec8<__bf16> {
    typedef b8 type;
};

// acc += A B over 8 values on v_mfma_f32_32x32x8_f16 / v_mfma_f32_32x32x8_bf16 (the _1k form: four bf16 per lane, the builtin takes
// them as shorts)
__device__ __forceinline__ f32x16 mfma8(h4 a, h4 b, f32x16 acc) { return __builtin_amdgcn_mfma_f32_32x32x8f16(a, b, acc, 0, 0, 0); }
__device__ __forceinline__ f32x16 mfma8(b4 a, b4 b, f32x16 acc) {
    typedef short s4 __attribute__((ext_vector_type(4)));
    return __builtin_amdgcn_mfma_f32_32x32x8bf16_1k(__builtin_bit_cast(s4, a), __builtin_bit_cast(s4, b), acc, 0, 0, 0);
}

// acc += A B over 16 values on v_mfma_f32_32x32x16_f16 / v_mfma_f32_32x32x16_bf16
__device__ __forceinline__ f32x16 mfma16(h8 a, h8 b, f32x16 acc) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, acc, 0, 0, 0); }
__device__ __forceinline__ f32x16 mfma16(b8 a, b8 b, f32x16 acc) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0); }

__device__ __forceinline__ float hw_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

// the value the other lane half (lane ^ 32) holds
__device__ __forceinline__ float other_half(float x) { return __shfl_xor(x, 32, 64); }

}  // namespace attn
}  // namespace gfn
