// fpn_conv_launch.h -- what the FPN's training path (fpn_conv_train.hip) shares with its inference path (fpn_conv.hip): the argument
// block of the direct convolution, the activation as both directions evaluate it, and the launch of the convolution kernels
// (conv_tile_kernel for Cout a multiple of 8, conv_general_kernel otherwise).  The kernels themselves are instantiated once, in
// fpn_conv.hip; the training path runs them with scale = 1 and shift = 0 (fmaf(acc, 1, 0) is acc, bit for bit) for the raw
// convolution output u and, on the stride-1 layers, for the input gradient (the same convolution of gu with repacked weights).
// fpn_conv_tf32_launch is the same seam in the TF32 class (fpn_conv_tf32.hip), which the gfn_conv2d_bn_act_train_tf32_* entry points take.
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

// F.interpolate(scale_factor=2, mode="bilinear", align_corners=False) of the (h2, w2) plane p at (y, x) of the doubled grid: the
// source coordinate 0.5 (dst + 0.5) - 0.5 clamped at 0, the far neighbour clamped to the plane, weights and sum in ATen's order
__device__ __forceinline__ float up2_at(const float *__restrict__ p, int h2, int w2, int y, int x) {
    const float sy = fmaxf(0.5f * ((float)y + 0.5f) - 0.5f, 0.f), sx = fmaxf(0.5f * ((float)x + 0.5f) - 0.5f, 0.f);
    const int y0 = (int)sy, x0 = (int)sx;
    const int y1 = min(y0 + 1, h2 - 1), x1 = min(x0 + 1, w2 - 1);
    const float ly = sy - (float)y0, lx = sx - (float)x0;
    const float hy = 1.f - ly, hx = 1.f - lx;
    return hy * (hx * p[y0 * w2 + x0] + lx * p[y0 * w2 + x1]) + ly * (hx * p[y1 * w2 + x0] + lx * p[y1 * w2 + x1]);
}

// up2_at in two halves, for a reader whose four values lie elsewhere than in the plane itself (the weight gradient's LDS copy of a
// tile's coarse footprint): the same operations on the same operands in the same order, and the library is built without FMA
// contraction, so both directions of the training path see the same x0' bit for bit.
struct Up2Taps {
    int y0, y1, x0, x1;
    float ly, lx;
};
__device__ __forceinline__ Up2Taps up2_taps(int h2, int w2, int y, int x) {
    const float sy = fmaxf(0.5f * ((float)y + 0.5f) - 0.5f, 0.f), sx = fmaxf(0.5f * ((float)x + 0.5f) - 0.5f, 0.f);
    Up2Taps t;
    t.y0 = (int)sy, t.x0 = (int)sx;
    t.y1 = min(t.y0 + 1, h2 - 1), t.x1 = min(t.x0 + 1, w2 - 1);
    t.ly = sy - (float)t.y0, t.lx = sx - (float)t.x0;
    return t;
}
__device__ __forceinline__ float up2_blend(const Up2Taps &t, float v00, float v01, float v10, float v11) {
    const float hy = 1.f - t.ly, hx = 1.f - t.lx;
    return hy * (hx * v00 + t.lx * v01) + t.ly * (hx * v10 + t.lx * v11);
}

// the kernel for (K, stride, a.Cout) on stream s; the caller has checked the sizes (gfn_conv2d_bn_act_fwd's limits)
int fpn_conv_launch(const ConvArgs &a, int B, int K, int stride, hipStream_t s);

// The same convolution in the TF32 class (fpn_conv_tf32.hip): split-bf16 operands on the matrix core, fp32 maps, fp32 sums and epilogue.
// a.weight is the plain fp32 (a.Cout, a.C0 + a.C1, K, K) weight; it is split and packed into `pack` (fpn_conv_tf32_pack_bytes bytes of
// 16-byte aligned device memory) by one small launch in front of the convolution.  a.Cout must be a multiple of 8.
int64_t fpn_conv_tf32_pack_bytes(int Cout, int Cin, int K);
int fpn_conv_tf32_launch(const ConvArgs &a, int B, int K, int stride, void *pack, hipStream_t s);
// The stride-1 weight gradient in that class: `parts` partial (Cout, C0 + C1, K, K) gradients into `part`, cut up as fpn_conv_train.hip's
// WgradShape says (8 x 32 pixel tiles, `cig` input channels per workgroup, cig K K <= 256), for ft_wsum_kernel to add up
int fpn_wgrad_tf32_launch(const float *x0, const float *x1, const float *gu, float *part, int C0, int C1, int H, int W, int Cout, int K, int IH,
                          int IW, int PITCH, int cig, int nci, int parts, int tiles_x, int tiles_y, int64_t ntiles, hipStream_t s);

}  // namespace gfn
