// conv_stack_half.hip -- the refiners' conv blocks on fp16 maps (the reference's amp=True class).
//
// Reference: ConvRefiner.forward, model/network.py:560-562 -- `with torch.autocast("cuda", enabled=self.amp, dtype=self.amp_dtype)`
// around block1 + hidden_blocks: every map between two blocks is a float16 tensor there.  Same fused kernel as
// csrc/conv_stack.hip's fp16-operand variant (csrc/conv_block_fused.h: depthwise, BatchNorm and accumulation in fp32, 1x1
// operands fp16) with the maps between blocks stored as fp16 in HBM, channel pairs side by side ((B, ceil(C/2), G, G) half2):
// the blocks of the fine scales (C = 24, 73 on 128^2 .. 320^2 maps) are bound by that traffic, and it halves.
// The first block of a stack reads the fp32 concat `d`, the last one (out_conv folded in) writes fp32.
#include "conv_block_fused.h"

namespace {

template <bool HIN, bool HOUT>
int launch_half(const ConvRoute &r, const void *x, const float *packed, void *y, int C, int M, int G, hipStream_t s) {
    const float *xf = (const float *)x;
    float *yf = (float *)y;
    if constexpr (HIN && HOUT) {  // blocks between two half maps, wide enough for more than three accumulator row tiles
        if (r.KW == 2) return launch_fused_tw<true, HIN, HOUT, true, 2>(r, xf, packed, yf, M, C, G, s);
    }
    if (r.KW != 1) return no_fused_kernel(r);
    return launch_fused_tw<true, HIN, HOUT, true>(r, xf, packed, yf, M, C, G, s);
}

}  // namespace

GFN_EXPORT int gfn_conv_block_half_fwd(const void *x, int x_dtype, const float *packed, void *y, int y_dtype, int B, int C, int M,
                                       int G, gfn_stream_t stream) {
    if (!x || !packed || !y) return gfn::fail(GFN_ERR_INVALID_ARG, "conv_block_half: bad argument");
    if (x == y) return gfn::fail(GFN_ERR_INVALID_ARG, "conv_block_half: in-place is not supported (cells read their neighbours)");
    ConvRoute r;
    if (int rc = conv_route(GFN_CBR_ENTRY_HALF, x_dtype, y_dtype, B, C, M, G, &r)) return rc;
    if (B == 0) return GFN_OK;
    hipStream_t s = (hipStream_t)stream;
    if (!r.HIN) return launch_half<false, true>(r, x, packed, y, C, M, G, s);
    if (!r.HOUT) return launch_half<true, false>(r, x, packed, y, C, M, G, s);
    return launch_half<true, true>(r, x, packed, y, C, M, G, s);
}
