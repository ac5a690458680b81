// conv_stack_train_bf16.hip -- one refiner conv block in TRAINING mode in the bf16 autocast class: bf16 maps in HBM.
//
// A ConvRefiner takes amp_dtype as the reference's does (model/network.py:444-564); with amp_dtype = torch.bfloat16 its block1 +
// hidden_blocks (network.py:560-562) train under bf16 autocast.  bf16 keeps fp32's exponent range: nothing overflows at 65504 and
// the step needs no loss scale.  The block is that of conv_stack_train.hip,
//   Conv2d(C, C, 5x5, padding 2, groups=C[, bias])  ->  BatchNorm2d (batch statistics)  ->  ReLU  ->  Conv2d(C, M, 1x1),
// conv_train_common.h writes it once for all classes and conv_train_16bit.h the classes with 16-bit maps once over their element
// (elem16.h): the three GEMM kernels, the split sum and the four launches.  This file is the bf16 class, BF16Maps = Maps16<__bf16>,
// beside F16Maps of conv_stack_train_half.hip: its C entry points.  What the class means:
//   * maps in HBM are plain contiguous (B, C, G, G) bf16: x (the previous block's y), u, y, the backward's gz and gx.  Any C, any
//     G: with odd G a plane starts on a 2-byte boundary, so maps are read and written 2 bytes at a time unless G % 4 == 0 (G % 8 == 0
//     for the 16-byte loads of the weight gradient) makes a wider access aligned.  A stack's first block reads the fp32 concat and
//     rounds it on load (XT = float); its gx is then written fp32, unrounded, for the refiner input's backward
//   * parameters, their gradients, mean, invstd and every sum are fp32; depthwise taps and 1x1 weights are rounded to bf16 where
//     they become operands.  bf16 x bf16 products are exact in fp32, so the depthwise forward is the fp32 tap loop on rounded values
//   * u is rounded once; statistics, normalisation and backward all read the rounded u, so the block is an exact function of what
//     it stored.  t = relu(u*alpha + beta') is rounded as the B operand; alpha, beta' come from bn_affine / bn_pre in both
//     directions, so both ReLU masks agree bit for bit
//   * the three 1x1 products (y = W.t, gt = W^T.gy, dW = gy.t^T with its column of ones) run on v_mfma_f32_32x32x16_bf16 with fp32
//     accumulators
//   * every rounding is to nearest even ((__bf16)float); there is no clamp, and inf and NaN propagate
// No floating-point atomics: two identical calls give identical bits.
#include "conv_train_16bit.h"

namespace {

using BF16Maps = Maps16<__bf16>;

}  // namespace

GFN_EXPORT int64_t gfn_conv_block_train_bf16_ws_bytes(int B, int C, int M, int G, int backward) {
    return train_ws_bytes<BF16Maps>(B, C, M, G, backward);
}

GFN_EXPORT int gfn_conv_block_train_bf16_fwd(const void *x, int x_dtype, const float *dw_w, const float *dw_b, const float *bn_w,
                                             const float *bn_b, float *running_mean, float *running_var, const float *pw_w,
                                             const float *pw_b, void *u, float *mean, float *invstd, void *y, int B, int C, int M, int G,
                                             double momentum, double eps, void *ws, int64_t ws_bytes, gfn_stream_t stream) {
    return train_fwd<BF16Maps>("conv_block_train_bf16_fwd", x, x_dtype, dw_w, dw_b, bn_w, bn_b, running_mean, running_var, pw_w, pw_b, u, mean,
                               invstd, y, B, C, M, G, momentum, eps, ws, ws_bytes, stream);
}

GFN_EXPORT int gfn_conv_block_train_bf16_bwd(const void *gy, const void *x, int x_dtype, const void *u, const float *mean,
                                             const float *invstd, const float *dw_w, const float *bn_w, const float *bn_b,
                                             const float *pw_w, void *gx, float *d_dw_w, float *d_dw_b, float *d_bn_w, float *d_bn_b,
                                             float *d_pw_w, float *d_pw_b, int B, int C, int M, int G, int need, void *ws, int64_t ws_bytes,
                                             gfn_stream_t stream) {
    return train_bwd<BF16Maps>("conv_block_train_bf16_bwd", gy, x, x_dtype, u, mean, invstd, dw_w, bn_w, bn_b, pw_w, gx, d_dw_w, d_dw_b, d_bn_w,
                               d_bn_b, d_pw_w, d_pw_b, B, C, M, G, need, ws, ws_bytes, stream);
}
