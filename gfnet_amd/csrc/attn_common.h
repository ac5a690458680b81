// What the two attention files (cross_attn.hip at head dim 8, self_attn.hip at head dim 64) both need in their kernels: the base-2
// exponential and its constants, the cross-half shuffle and the fp16 vector types.
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

__device__ __forceinline__ float hw_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

// the value the other lane half (lane ^ 32) holds
__device__ __forceinline__ float other_half(float x) { return __shfl_xor(x, 32, 64); }

}  // namespace attn
}  // namespace gfn
