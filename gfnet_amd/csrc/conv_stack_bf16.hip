// conv_stack_bf16.hip -- the refiners' conv blocks on bf16 maps: the inference twin of csrc/conv_stack_half.hip for a model that
// was trained in the bf16 autocast class (csrc/conv_stack_train_bf16.hip) and was never held inside fp16's range.
//
// Reference: ConvRefiner.forward, model/network.py:560-562 -- `with torch.autocast("cuda", enabled=self.amp, dtype=self.amp_dtype)`
// around block1 + hidden_blocks with amp_dtype=torch.bfloat16: every map between two blocks is a bfloat16 tensor there.  The
// kernel is csrc/conv_block_fused.h's, instantiated with the 16-bit element __bf16 (csrc/elem16.h): the depthwise 5x5 on
// v_mfma_f32_16x16x32_bf16, the 1x1 conv on v_mfma_f32_32x32x16_bf16, BatchNorm, ReLU and every sum in fp32, the maps between
// blocks bf16 in HBM in the half map's layout ((B, ceil(C/2), G, G) of bf16 pairs).  Same tile shapes and routes as the fp16
// class (conv_route answers GFN_CBR_ENTRY_BF16 with what it answers GFN_CBR_ENTRY_HALF).  The packed block comes from
// gfn_conv_block_pack_bf16 (csrc/conv_stack.hip): same layout, the 1x1 weights and the banded taps rounded to bf16.
// The first block of a stack reads the fp32 concat `d`, the last one (out_conv folded in) writes fp32.
#include "conv_block_fused.h"

namespace {

template <bool HIN, bool HOUT>
int launch_bf16(const ConvRoute &r, const void *x, const float *packed, void *y, int C, int M, int G, hipStream_t s) {
    const float *xf = (const float *)x;
    float *yf = (float *)y;
    if constexpr (HIN && HOUT) {  // blocks between two bf16 maps, wide enough for more than three accumulator row tiles
        if (r.KW == 2) return launch_fused_tw<true, HIN, HOUT, true, 2, __bf16>(r, xf, packed, yf, M, C, G, s);
    }
    if (r.KW != 1) return no_fused_kernel(r);
    return launch_fused_tw<true, HIN, HOUT, true, 1, __bf16>(r, xf, packed, yf, M, C, G, s);
}

}  // namespace

GFN_EXPORT int gfn_conv_block_bf16_fwd(const void *x, int x_dtype, const float *packed, void *y, int y_dtype, int B, int C, int M,
                                       int G, gfn_stream_t stream) {
    if (!x || !packed || !y) return gfn::fail(GFN_ERR_INVALID_ARG, "conv_block_bf16: bad argument");
    if (x == y) return gfn::fail(GFN_ERR_INVALID_ARG, "conv_block_bf16: in-place is not supported (cells read their neighbours)");
    ConvRoute r;
    if (int rc = conv_route(GFN_CBR_ENTRY_BF16, x_dtype, y_dtype, B, C, M, G, &r)) return rc;
    if (B == 0) return GFN_OK;
    hipStream_t s = (hipStream_t)stream;
    if (!r.HIN) return launch_bf16<false, true>(r, x, packed, y, C, M, G, s);
    if (!r.HOUT) return launch_bf16<true, false>(r, x, packed, y, C, M, G, s);
    return launch_bf16<true, true>(r, x, packed, y, C, M, G, s);
}
