// local_corr_common.h -- what every local-correlation kernel shares: the launch constants, the kernel argument block (LcParams),
// and the device helpers of the per-tap routine, the cell coordinates and the wave reductions.
#pragma once
#include "common.h"
#include "refiner_input.h"

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

// f1 map of direction b.  Symmetric batches are virtual: the second half of the directions reads
// the other image's features (f1_second) instead of a concatenated copy (model/network.py:213-222).
template <typename FT>
__device__ __forceinline__ const FT *f1_of(const LcParams &p, int b) {
    const size_t chw = (size_t)p.C * p.H * p.W;
    return (b < p.Bh) ? static_cast<const FT *>(p.f1) + (size_t)b * chw : static_cast<const FT *>(p.f1_second) + (size_t)(b - p.Bh) * chw;
}
// a feature value as fp32 (fp16 storage is widened in registers; every sum stays fp32)
__device__ __forceinline__ float ldf(const float *q) { return *q; }
__device__ __forceinline__ float ldf(const _Float16 *q) { return (float)*q; }

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

// Normalised -> pixel coordinate exactly as grid_sample(align_corners=False) un-normalises (refiner_input.h).
using gfn_ri::unnorm;

// ---- general per-tap evaluation (mirrors the reference op for op) ---------------------------
template <typename FT>
__device__ __forceinline__ float tap_general(const LcParams &p, int b, int i, int j, int ky, int kx, int D, float nx, float ny) {
    float ylo, yhi, xlo, xhi;
    if (p.grid_based) {
        ylo = (float)(-2.0 * p.r / p.G); yhi = (float)(2.0 * p.r / p.G);
        xlo = ylo; xhi = yhi;
    } else {
        ylo = (float)(-2.0 * p.r / p.win_h); yhi = (float)(2.0 * p.r / p.win_h);
        xlo = (float)(-2.0 * p.r / p.win_w); xhi = (float)(2.0 * p.r / p.win_w);
    }
    const float gx = nx + gfn::linspace_at(xlo, xhi, D, kx);
    const float gy = ny + gfn::linspace_at(ylo, yhi, D, ky);
    const float ix = unnorm(gx, p.W), iy = unnorm(gy, p.H);
    float fx = floorf(ix), fy = floorf(iy);
    const bool sane = (fx > -1e6f) & (fx < 1e6f) & (fy > -1e6f) & (fy < 1e6f);
    const int x0 = sane ? (int)fx : -4, y0 = sane ? (int)fy : -4;
    const float w00 = (fx + 1.f - ix) * (fy + 1.f - iy), w01 = (ix - fx) * (fy + 1.f - iy);
    const float w10 = (fx + 1.f - ix) * (iy - fy), w11 = (ix - fx) * (iy - fy);
    const bool xa = (unsigned)x0 < (unsigned)p.W, xb = (unsigned)(x0 + 1) < (unsigned)p.W;
    const bool ya = (unsigned)y0 < (unsigned)p.H, yb = (unsigned)(y0 + 1) < (unsigned)p.H;
    const float *f0p = p.f0 + (size_t)b * p.f0_bs + (size_t)i * p.G + j;
    const FT *f1p = f1_of<FT>(p, b);
    const size_t plane = (size_t)p.H * p.W, cs = (size_t)p.G * p.G;
    const long o00 = (long)y0 * p.W + x0;
    // zero padding without branches: a corner outside the image reads pixel 0 with weight 0 (adds an exact 0), so the
    // gathers of 8 channels can all be in flight at once -- the branchy form exposed one L2 round trip per channel
    const long oa = (ya & xa) ? o00 : 0, ob = (ya & xb) ? o00 + 1 : 0, oc = (yb & xa) ? o00 + p.W : 0, od = (yb & xb) ? o00 + p.W + 1 : 0;
    const float wa = (ya & xa) ? w00 : 0.f, wb = (ya & xb) ? w01 : 0.f, wc = (yb & xa) ? w10 : 0.f, wd = (yb & xb) ? w11 : 0.f;
    float acc = 0.f;
    constexpr int UC = 8;
    for (int c0 = 0; c0 < p.C; c0 += UC) {
        float va[UC], vb[UC], vc[UC], vd[UC], q[UC];
#pragma unroll
        for (int u = 0; u < UC; ++u) {
            const int c = min(c0 + u, p.C - 1);
            const FT *pl = f1p + c * plane;
            va[u] = ldf(pl + oa); vb[u] = ldf(pl + ob); vc[u] = ldf(pl + oc); vd[u] = ldf(pl + od);
            q[u] = f0p[c * cs];
        }
#pragma unroll
        for (int u = 0; u < UC; ++u) {
            if (c0 + u < p.C) {
                float s = 0.f;
                s += va[u] * wa;
                s += vb[u] * wb;
                s += vc[u] * wc;
                s += vd[u] * wd;
                acc += (q[u] / p.sqrt_c) * s;
            }
        }
    }
    return acc;
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

}  // namespace
