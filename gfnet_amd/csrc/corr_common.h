// corr_common.h -- what the global-correlation kernels (corr_softargmax.hip, corr_softargmax_bwd.hip) say about a 32 x 32 tile, once:
// the B-grid cell of a position, the fp32 tile product, the virtual symmetric direction and the host-side argument checks (the
// accumulator layout, f32x16 and acc_row, is common.h's: the 1x1 conv tile reads it too).  split3 also serves kde.hip.
#pragma once
#include "elem16.h"
#include "reduce.h"

namespace gfn {

// x = h + m + l exactly (three round-to-nearest bf16 pieces of 8 significant bits each cover the 24 of an fp32 value)
__device__ __forceinline__ void split3(float v, __bf16 &h, __bf16 &m, __bf16 &l) {
    h = (__bf16)v;
    const float r1 = v - (float)h;
    m = (__bf16)r1;
    l = (__bf16)(r1 - (float)m);
}

// B-grid cell (jx, jy) of position j = jy W1 + jx, inv_w1 = 1.0f / W1.  The float quotient is off by one row for some j >= 2^22
// (j + 0.5 and the product round); one integer step either way makes (jx, jy) exact for every j < 2^24 (tests/test_host_cpu.py
// runs this formula over all of them)
__device__ __forceinline__ void cell_of(int j, int W1, float inv_w1, int &jx, int &jy) {
    jy = (int)(((float)j + 0.5f) * inv_w1);
    jx = j - jy * W1;
    if (jx < 0) { --jy; jx += W1; }
    else if (jx >= W1) { ++jy; jx -= W1; }
}

// centre of that cell (torch.linspace as the reference fills its grid); a padded j >= H1 W1 takes the last row
__device__ __forceinline__ void cell_centre(int j, int H1, int W1, float inv_w1, float &gx, float &gy) {
    int jx, jy;
    cell_of(j, W1, inv_w1, jx, jy);
    gx = linspace_at((float)(-1 + 1.0 / W1), (float)(1 - 1.0 / W1), W1, jx);
    gy = linspace_at((float)(-1 + 1.0 / H1), (float)(1 - 1.0 / H1), H1, min(jy, H1 - 1));
}

// S[q][p] = sum_c Y[c][q] X[c][p] for one tile on the exact-fp32 matrix core: y = the lane's KS values Y[2 s + h][q0 + col],
// x = X[2 s + h][p0 + col] (zero for channels >= C).
// two independent accumulation chains (even / odd k-steps): a single chain left the matrix pipe waiting on its own
// result between issues (0.152 -> 0.122 ms for 64 directions; four chains: 0.131); summed at the end
template <int KS>
__device__ __forceinline__ f32x16 corr_tile(const float (&y)[KS], const float (&x)[KS]) {
    f32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, acc2 = acc;
#pragma unroll
    for (int s = 0; s < KS; s += 2) {
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(y[s], x[s], acc, 0, 0, 0);
        if (s + 1 < KS) acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(y[s + 1], x[s + 1], acc2, 0, 0, 0);
    }
    return acc + acc2;
}

// symmetric batches are virtual (Bh = B/2 images per side): direction b >= Bh swaps the roles of the two arrays instead of
// reading a concatenated copy (model/network.py:213-222).  Image of direction b in `fwd` (b < Bh) or `rev`, `stride` elements each.
template <typename T>
__device__ __forceinline__ T *dir_image(T *fwd, T *rev, int b, int Bh, size_t stride) {
    return b < Bh ? fwd + (size_t)b * stride : rev + (size_t)(b - Bh) * stride;
}

// the argument checks every global-correlation entry point shares, in the order they refuse; `out` = the flow (or volume) array
inline int corr_check(const char *who, const void *f0, const void *f1, const void *out, int B, int C, int H0, int W0, int H1, int W1,
                      int symmetric) {
    if (!f0 || !f1) return fail(GFN_ERR_INVALID_ARG, "%s: null feature pointer", who);
    if (B < 0 || C <= 0 || H0 <= 0 || W0 <= 0 || H1 <= 0 || W1 <= 0)
        return fail(GFN_ERR_INVALID_ARG, "%s: bad size B=%d C=%d %dx%d vs %dx%d", who, B, C, H0, W0, H1, W1);
    if (C > 128) return fail(GFN_ERR_INVALID_ARG, "%s: C=%d > 128 channels not supported", who, C);
    if ((long)H0 * W0 >= (1L << 24) || (long)H1 * W1 >= (1L << 24)) return fail(GFN_ERR_INVALID_ARG, "%s: map too large", who);
    if (!out) return fail(GFN_ERR_INVALID_ARG, "%s: null flow / volume", who);
    if (symmetric && ((B & 1) || H0 != H1 || W0 != W1))
        return fail(GFN_ERR_INVALID_ARG, "%s: symmetric needs an even batch and equal map sizes", who);
    return GFN_OK;
}

}  // namespace gfn
