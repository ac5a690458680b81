// local_corr_common.h -- what every local-correlation kernel shares: the launch constants, the kernel argument block (LcParams)
// with its host-side checks and filler, and the device helpers of the per-tap routine, the cell coordinates and the wave reductions.
#pragma once
#include "elem16.h"
#include "sample_modes.h"

struct LcParams {
    const float *f0;
    const void *f1;          // feature maps (B or Bh, C, H, W), fp32 or fp16 (f16 != 0): BASELINE config 5 stores the pyramids in fp16
    const void *f1_second;   // symmetric batches: f1 of directions b >= Bh (NULL: f1 holds all B maps)
    int f16;
    int Bh;
    const float *flow;
    float *out;
    long f0_bs, out_bs;
    int B, C, G, H, W;
    int tiles_x, tiles_y;
    float sqrt_c, inv_sqrt_c;
    int r, win_h, win_w, grid_based;  // general path / flagged cells
    float win_xhi, win_yhi;           // tiled path: linspace end points 2r/W, 2r/H rounded to fp32
    float win_xstep, win_ystep;       // ... and the linspace steps (hi - lo) / (2r), fp32 division done on the host
    int *todo;                        // [kTodoHdr + B*tiles]: header (see kTodoHdr), then the ids of the tiles left to the second launch
    long todo_ints;
    int planned;                      // lean path: the plan is already in scratch (gfn_refiner_input_plan_fwd_dt wrote it)
    int mq;                           // r >= 5: the first launch is the matrix-core tile kernel (local_corr_mq.h)
    int *plan;                        // lean path: [4 * B*tiles] per-tile staging regions written by the plan launch (16-byte aligned)
};

// host: launches the per-(cell, tap) kernel of local_corr_modes.hip for validated mode codes; the general route of
// gfn_local_corr_fwd_dt (bilinear, zeros) and gfn_local_corr_mode_fwd end here
int gfn_lc_launch_taps(const LcParams &p, int sample_mode, int padding_mode, hipStream_t s);

namespace {

constexpr int kThreads = 512;
constexpr int kWaves = kThreads / 64;
constexpr int kChunk = 16;                // channels staged per pass
constexpr int kSlotV4 = kChunk / 4 + 1;   // float4s per staged pixel: 4 data + 1 pad = 80 B
constexpr int kStageBytes = 68 * 1024;    // stage buffer (aliased by the D buffer in the epilogue)
constexpr int kCapSlots = kStageBytes / (kSlotV4 * 16) - 1;  // pixels that fit, minus the zero slot
static_assert((kCapSlots + 1) * kSlotV4 < 65536, "stage indices are packed in 16 bits");
constexpr int kTileW = 16;
constexpr int kMaxLds = 150 * 1024;       // dynamic LDS a tiled launch may ask for
constexpr int kFar = 1 << 28;             // patch origin of a cell that samples nothing
constexpr int kTodoHdr = 8;               // ints in front of the tile list in scratch: [0] tiles left to the second launch, [1] its queue head,
                                          // [2] its finished workgroups, [3] last call's [0], [4] cells redone per tap (running call),
                                          // [5] last call's [4], [6] tiles staged in halves (running call), [7] last call's [6]; [0..2], [4] and [6] are zero between calls

// f1 map of direction b.  Symmetric batches are virtual: the second half of the directions reads
// the other image's features (f1_second) instead of a concatenated copy (model/network.py:213-222).
template <typename FT>
__device__ __forceinline__ const FT *f1_of(const LcParams &p, int b) {
    const size_t chw = (size_t)p.C * p.H * p.W;
    return (b < p.Bh) ? static_cast<const FT *>(p.f1) + (size_t)b * chw : static_cast<const FT *>(p.f1_second) + (size_t)(b - p.Bh) * chw;
}
// a feature value as fp32 (fp16 storage is widened in registers; every sum stays fp32)
using gfn_sm::ldf;

// lane -> (b128 hardware lane group, index inside the group).  ds_read_b128 is serviced in four
// 16-lane groups {0-3,12-15,20-27}, {4-11,16-19,28-31}, and the same +32.
__device__ __forceinline__ void lane_group(int lane, int &g, int &s) {
    const int m = lane & 31;
    const bool even = (m < 4) | ((m >= 12) & (m < 16)) | ((m >= 20) & (m < 28));
    if (even)
        s = (m < 4) ? m : (m < 16 ? m - 8 : m - 12);
    else
        s = (m < 12) ? m - 4 : (m < 20 ? m - 8 : m - 16);
    g = ((lane >> 5) << 1) | (even ? 0 : 1);
}


// min over each row of 16 lanes (a 2 x 8-cell group), valid in lane 15 of the row
__device__ __forceinline__ int row_min_i32(int v) {
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x111, 0xf, 0xf, false));  // row_shr:1
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x112, 0xf, 0xf, false));  // row_shr:2
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x114, 0xf, 0xf, false));  // row_shr:4
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x118, 0xf, 0xf, false));  // row_shr:8
    return v;
}

// min over the 64 lanes of a wave, returned to every lane (scalar): the row minimum, then the two row broadcasts of the GFX9 DPP
// set; lanes without a source keep their own value (min is idempotent).
__device__ __forceinline__ int wave_min_i32(int v) {
    v = row_min_i32(v);
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x142, 0xa, 0xf, false));  // row_bcast:15 -> rows 1, 3
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x143, 0xc, 0xf, false));  // row_bcast:31 -> rows 2, 3
    return __builtin_amdgcn_readlane(v, 63);
}

// Normalised -> pixel coordinate exactly as grid_sample(align_corners=False) un-normalises.
using gfn_sm::unnorm;

// the window's end points in normalised units: +-2r / G (grid_based) or +-2r / (win_w, win_h)
__device__ __forceinline__ void window_ends(const LcParams &p, float &xlo, float &xhi, float &ylo, float &yhi) {
    if (p.grid_based) {
        ylo = (float)(-2.0 * p.r / p.G); yhi = (float)(2.0 * p.r / p.G);
        xlo = ylo; xhi = yhi;
    } else {
        ylo = (float)(-2.0 * p.r / p.win_h); yhi = (float)(2.0 * p.r / p.win_h);
        xlo = (float)(-2.0 * p.r / p.win_w); xhi = (float)(2.0 * p.r / p.win_w);
    }
}

// sum_c f0[b,c,i,j] / sqrt(C) * (the sample of f1[b,c] through the set-up tp), as the reference forms it op for op: channels in
// groups with all gathers of a group in flight -- a corner outside the image reads pixel 0 with weight 0 (adds an exact 0), the
// branchy form exposed one L2 round trip per channel
template <typename FT, int MODE>
__device__ __forceinline__ float tap_dot(const LcParams &p, int b, int i, int j, const gfn_sm::Taps<MODE> &tp) {
    constexpr int UC = gfn_sm::group_channels<MODE>();
    const float *f0p = p.f0 + (size_t)b * p.f0_bs + (size_t)i * p.G + j;
    const FT *f1p = f1_of<FT>(p, b);
    const size_t plane = (size_t)p.H * p.W, cs = (size_t)p.G * p.G;
    float acc = 0.f;
    for (int c0 = 0; c0 < p.C; c0 += UC) {
        float v[UC][gfn_sm::Taps<MODE>::N], q[UC];
#pragma unroll
        for (int u = 0; u < UC; ++u) {
            const int c = min(c0 + u, p.C - 1);
            tp.load(f1p + c * plane, v[u]);
            q[u] = f0p[c * cs];
        }
#pragma unroll
        for (int u = 0; u < UC; ++u)
            if (c0 + u < p.C) acc += (q[u] / p.sqrt_c) * tp.value(v[u]);
    }
    return acc;
}

// ---- general per-tap evaluation of the tiled kernels (flagged cells, rounds that do not fit the stage): bilinear, zeros ---------
template <typename FT>
__device__ __forceinline__ float tap_general(const LcParams &p, int b, int i, int j, int ky, int kx, int D, float nx, float ny) {
    float xlo, xhi, ylo, yhi;
    window_ends(p, xlo, xhi, ylo, yhi);
    gfn_sm::Taps<GFN_SAMPLE_BILINEAR> tp;
    tp.setup<GFN_PAD_ZEROS>(nx + gfn::linspace_at(xlo, xhi, D, kx), ny + gfn::linspace_at(ylo, yhi, D, ky), p.W, p.H);
    return tap_dot<FT>(p, b, i, j, tp);
}

__device__ __forceinline__ void cell_coords(const LcParams &p, int b, int i, int j, float &nx, float &ny) {
    if (p.flow) {
        nx = p.flow[(((size_t)b * 2 + 0) * p.G + i) * p.G + j];
        ny = p.flow[(((size_t)b * 2 + 1) * p.G + i) * p.G + j];
    } else {  // identity grid (local_correlation.py:21-30)
        nx = gfn::linspace_at((float)(-1 + 1.0 / p.win_w), (float)(1 - 1.0 / p.win_w), p.win_w, j);
        ny = gfn::linspace_at((float)(-1 + 1.0 / p.win_h), (float)(1 - 1.0 / p.win_h), p.win_h, i);
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------
// the argument checks of the local-correlation entry points (`what` names the caller in the error text); in / out: the tensor
// of C and of K planes per batch element (f0 and out forwards, grad_f0 and grad_out backwards)
inline int check_args(const char *what, bool null_ptr, bool odd_symmetric, int B, int C, int G, int H, int W, int r, int win_h, int win_w,
                      int64_t in_bs, int64_t out_bs, bool has_flow, int sample_mode, int padding_mode) {
    if (!gfn_sm::valid_modes(sample_mode, padding_mode))
        return gfn::fail(GFN_ERR_INVALID_ARG, "%s: sample_mode %d / padding_mode %d is not a GFN_SAMPLE_* / GFN_PAD_* code", what,
                         sample_mode, padding_mode);
    if (null_ptr) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: null tensor pointer", what);
    if (odd_symmetric) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: symmetric batch must be even", what);
    if (B < 0 || C <= 0 || G <= 0 || H <= 0 || W <= 0 || r < 0 || win_h <= 0 || win_w <= 0)
        return gfn::fail(GFN_ERR_INVALID_ARG, "%s: bad size B=%d C=%d G=%d H=%d W=%d r=%d", what, B, C, G, H, W, r);
    const long K = (long)(2 * r + 1) * (2 * r + 1);
    if (in_bs < (long)C * G * G || out_bs < K * G * G)
        return gfn::fail(GFN_ERR_INVALID_ARG, "%s: batch stride smaller than one batch element", what);
    if (!has_flow && !(G == win_h && G == win_w))
        return gfn::fail(GFN_ERR_INVALID_ARG, "%s: flow=NULL needs num_grid == h == w (got G=%d h=%d w=%d)", what, G, win_h, win_w);
    if ((long)B * K * G * G >= (1L << 40) || (long)C * H * W >= (1L << 31)) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: tensor too large", what);
    return GFN_OK;
}

// what the forward, backward and plan entry points fill alike
inline LcParams lc_params(const void *f1, const void *f1_second, bool f16, const float *flow, int B, int C, int G, int H, int W, int r,
                          int grid_based, int win_h, int win_w) {
    LcParams p{};
    p.f1 = f1; p.f1_second = f1_second; p.f16 = f16 ? 1 : 0; p.Bh = f1_second ? B / 2 : B;
    p.flow = flow;
    p.B = B; p.C = C; p.G = G; p.H = H; p.W = W;
    p.sqrt_c = (float)sqrt((double)C);
    p.inv_sqrt_c = (float)(1.0 / sqrt((double)C));
    p.r = r; p.win_h = win_h; p.win_w = win_w; p.grid_based = grid_based;
    return p;
}

}  // namespace
