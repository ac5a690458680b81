// What the two attention files (cross_attn.hip at head dim 8, self_attn.hip at head dim 64) both need in their kernels beyond the
// element (elem16.h) and the cross-half shuffle (reduce.h): the base-2 exponential and its constants.
#pragma once
#include <cmath>

#include "elem16.h"
#include "reduce.h"

namespace gfn {
namespace attn {

constexpr float kLog2e = 1.4426950408889634f;
constexpr float kLn2 = 0.6931471805599453f;

__device__ __forceinline__ float hw_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

}  // namespace attn
}  // namespace gfn
