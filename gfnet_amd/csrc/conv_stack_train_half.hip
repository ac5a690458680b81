// conv_stack_train_half.hip -- one refiner conv block in TRAINING mode in the reference's autocast class: fp16 maps in HBM.
//
// Reference: every ConvRefiner is built with amp=True (model/network.py:90-152) and trainer/train.py:29-43 drives the step with a
// GradScaler, so block1 + hidden_blocks (network.py:560-562) train under fp16 autocast.  The block is that of conv_stack_train.hip,
//   Conv2d(C, C, 5x5, padding 2, groups=C[, bias])  ->  BatchNorm2d (batch statistics)  ->  ReLU  ->  Conv2d(C, M, 1x1),
// and conv_train_common.h writes it once for all classes: the depthwise kernels, the small reductions, the prologues and epilogues
// of the 1x1 kernels, the workspace plan, the argument checks, the `need` mask and the launch sequence (train_fwd / train_bwd).
// conv_train_16bit.h writes the classes with 16-bit maps once over their element (elem16.h): the three GEMM kernels (ct_half_pw_fwd /
// _bwd / _wgrad_kernel), the split sum and the four launches.  This file is the fp16 class, F16Maps = Maps16<_Float16>: its C entry
// points (conv_stack_train_bf16.hip is the bf16 class).  What the class means:
//   * maps in HBM are plain contiguous (B, C, G, G) fp16: x (the previous block's y), u, y, the backward's gz and gx.  Any C, any
//     G: with odd G a plane starts on a 2-byte boundary, so maps are read and written half by half unless G % 4 == 0 (G % 8 == 0
//     for the 16-byte loads of the weight gradient) makes a wider access aligned.  A stack's first block reads the fp32 concat and
//     rounds it on load (XT = float); its gx is then written fp32, unrounded, for the refiner input's backward
//   * parameters, their gradients, mean, invstd and every sum are fp32; depthwise taps and 1x1 weights are rounded to fp16 where
//     they become operands.  fp16 x fp16 products are exact in fp32, so the depthwise forward is the fp32 tap loop on rounded values
//   * u is rounded once; statistics, normalisation and backward all read the rounded u, so the block is an exact function of what
//     it stored.  t = relu(u*alpha + beta') is rounded as the B operand; alpha, beta' come from bn_affine / bn_pre in both
//     directions, so both ReLU masks agree bit for bit
//   * the three 1x1 products (y = W.t, gt = W^T.gy, dW = gy.t^T with its column of ones) run on v_mfma_f32_32x32x16_f16 with fp32
//     accumulators
//   * every rounding is to nearest even and overflows to inf (Elem16<_Float16>::round): a loss scale that is too large shows as inf / nan
// No floating-point atomics: two identical calls give identical bits.
#include "conv_train_16bit.h"

namespace {

using F16Maps = Maps16<_Float16>;

}  // namespace

GFN_EXPORT int64_t gfn_conv_block_train_half_ws_bytes(int B, int C, int M, int G, int backward) {
    return train_ws_bytes<F16Maps>(B, C, M, G, backward);
}

GFN_EXPORT int gfn_conv_block_train_half_fwd(const void *x, int x_dtype, const float *dw_w, const float *dw_b, const float *bn_w,
                                             const float *bn_b, float *running_mean, float *running_var, const float *pw_w,
                                             const float *pw_b, void *u, float *mean, float *invstd, void *y, int B, int C, int M, int G,
                                             double momentum, double eps, void *ws, int64_t ws_bytes, gfn_stream_t stream) {
    return train_fwd<F16Maps>("conv_block_train_half_fwd", x, x_dtype, dw_w, dw_b, bn_w, bn_b, running_mean, running_var, pw_w, pw_b, u, mean,
                              invstd, y, B, C, M, G, momentum, eps, ws, ws_bytes, stream);
}

GFN_EXPORT int gfn_conv_block_train_half_bwd(const void *gy, const void *x, int x_dtype, const void *u, const float *mean,
                                             const float *invstd, const float *dw_w, const float *bn_w, const float *bn_b,
                                             const float *pw_w, void *gx, float *d_dw_w, float *d_dw_b, float *d_bn_w, float *d_bn_b,
                                             float *d_pw_w, float *d_pw_b, int B, int C, int M, int G, int need, void *ws, int64_t ws_bytes,
                                             gfn_stream_t stream) {
    return train_bwd<F16Maps>("conv_block_train_half_bwd", gy, x, x_dtype, u, mean, invstd, dw_w, bn_w, bn_b, pw_w, gx, d_dw_w, d_dw_b, d_bn_w,
                              d_bn_b, d_pw_w, d_pw_b, B, C, M, G, need, ws, ws_bytes, stream);
}
