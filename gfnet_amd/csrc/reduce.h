// reduce.h -- sums over a wave of 64 lanes and over a workgroup of four.  The two wave forms associate differently and are not
// interchangeable: a call site that must keep its bits keeps its form.
#pragma once
#include "common.h"

namespace gfn {

// the value the other lane half (lane ^ 32) holds
template <typename T>
__device__ __forceinline__ T other_half(T v) { return __shfl_xor(v, 32, 64); }

// the xor butterfly: both partners of every exchange form the same sum, so every lane ends with the same bits
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}
// the same over the 32 lanes that share lane >> 5
template <typename T>
__device__ __forceinline__ T half_wave_sum(T v) {
#pragma unroll
    for (int m = 16; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}
// the shift-down tree: only lane 0 ends with the sum
template <typename T>
__device__ __forceinline__ T wave_sum_lane0(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// sum over the workgroup's 256 threads in a fixed order, returned to every thread; red: 4 floats of LDS
__device__ __forceinline__ float block_sum(float v, float *red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

}  // namespace gfn
