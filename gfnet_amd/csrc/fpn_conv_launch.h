// fpn_conv_launch.h -- what the FPN's training path (fpn_conv_train.hip) shares with its inference path (fpn_conv.hip): the argument
// block of the direct convolution, the activation as both directions evaluate it, and the launch of the convolution kernels
// (conv_tile_kernel for Cout a multiple of 8, conv_general_kernel otherwise).  The kernels themselves are instantiated once, in
// fpn_conv.hip; the training path runs them with scale = 1 and shift = 0 (fmaf(acc, 1, 0) is acc, bit for bit) for the raw
// convolution output u and, on the stride-1 layers, for the input gradient (the same convolution of gu with repacked weights).
#pragma once
#include <cmath>

#include "common.h"

namespace gfn {

struct ConvArgs {
    const float *x0, *x1, *weight, *scale, *shift, *residual;
    float *out;
    int C0, C1, up0, H, W, Cout, Ho, Wo, act;
    float slope;
};

__device__ __forceinline__ float activate(float v, int act, float slope) {
    if (act == 1) return v > 0.f ? v : v * slope;
    if (act == 2) return v * (1.f / (1.f + expf(-v)));
    return v;
}

// the kernel for (K, stride, a.Cout) on stream s; the caller has checked the sizes (gfn_conv2d_bn_act_fwd's limits)
int fpn_conv_launch(const ConvArgs &a, int B, int K, int stride, hipStream_t s);

}  // namespace gfn
