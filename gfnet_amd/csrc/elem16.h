// elem16.h -- the 16-bit element of a precision class, said once: which type it is, how a float is rounded into it, which vector
// types carry it and which matrix instruction multiplies it.  Beside it the vector typedefs every kernel file shares (f32x16, the
// 32x32 accumulator, is in common.h).
#pragma once
#include "common.h"

namespace gfn {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

// Elem16<T>, T = _Float16 or __bf16:
//   vec2        two values as one register: a channel pair of a 16-bit map
//   vec4        four values as one register pair: an operand fragment of the 32x32x8 step and an 8-byte access
//   vec8        eight values as one register quad: an operand fragment of the 32x32x16 and 16x16x32 steps and a 16-byte access
//   kDtype      the GFN_* constant of a tensor of T;  kDtypeName: its name in messages
//   round(v)    the float v becomes once it is stored as T: to nearest even, no clamp
template <typename T>
struct Elem16;
// float -> fp16 is v_cvt_f16_f32: to nearest even, and past 65504 to inf -- never a clamp, or overflow would be hidden from the
// loss scaler
template <>
struct Elem16<_Float16> {
    typedef f16x2 vec2;
    typedef f16x4 vec4;
    typedef f16x8 vec8;
    static constexpr int kDtype = GFN_F16;
    static constexpr const char *kDtypeName = "GFN_F16";
    static __device__ __forceinline__ float round(float v) { return (float)(_Float16)v; }
};
// float -> bf16 (v_cvt_pk_bf16_f32): fp32's exponent range, so nothing overflows that was finite in fp32; inf and NaN stay what they are
template <>
struct Elem16<__bf16> {
    typedef bf16x2 vec2;
    typedef bf16x4 vec4;
    typedef bf16x8 vec8;
    static constexpr int kDtype = GFN_BF16;
    static constexpr const char *kDtypeName = "GFN_BF16";
    static __device__ __forceinline__ float round(float v) { return (float)(__bf16)v; }
};

// acc += A B over 8 values on v_mfma_f32_32x32x8_f16 / v_mfma_f32_32x32x8_bf16 (the _1k form: four bf16 per lane, the builtin takes
// them as shorts)
__device__ __forceinline__ f32x16 mfma8(f16x4 a, f16x4 b, f32x16 acc) { return __builtin_amdgcn_mfma_f32_32x32x8f16(a, b, acc, 0, 0, 0); }
__device__ __forceinline__ f32x16 mfma8(bf16x4 a, bf16x4 b, f32x16 acc) {
    typedef short s4 __attribute__((ext_vector_type(4)));
    return __builtin_amdgcn_mfma_f32_32x32x8bf16_1k(__builtin_bit_cast(s4, a), __builtin_bit_cast(s4, b), acc, 0, 0, 0);
}

// acc += A B over 16 values on v_mfma_f32_32x32x16_f16 / v_mfma_f32_32x32x16_bf16
__device__ __forceinline__ f32x16 mfma16(f16x8 a, f16x8 b, f32x16 acc) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, acc, 0, 0, 0); }
__device__ __forceinline__ f32x16 mfma16(bf16x8 a, bf16x8 b, f32x16 acc) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0); }

// acc += A B over 32 values on v_mfma_f32_16x16x32_f16 / v_mfma_f32_16x16x32_bf16 (the 16x16 tile: four accumulator values per lane)
__device__ __forceinline__ f32x4 mfma32(f16x8 a, f16x8 b, f32x4 acc) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, acc, 0, 0, 0); }
__device__ __forceinline__ f32x4 mfma32(bf16x8 a, bf16x8 b, f32x4 acc) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0); }

// host: f(T()) for the element T that dtype names; the caller has checked that it is GFN_F16 or GFN_BF16
template <typename F>
int with_elem16(int dtype, F f) {
    return dtype == GFN_BF16 ? f(__bf16()) : f(_Float16());
}

}  // namespace gfn
