// local_corr_tile.h -- the round-1 tile routine of the local correlation (process_tile), its tile kernel and the second launch
// that finishes the tiles a first launch could not stage.  The lean and matrix-core kernels hand tiles to the same routine.
#pragma once
#include "local_corr_common.h"
#include "local_corr_stage.h"

namespace {

struct Region {
    int x0, y0, w, h, pitch;
};

// tiles of the round-1 routine: 2 * ROUNDS x 16 cells (r <= 4: 4 x 16, as the lean kernel's; r >= 5: 2 x 16, as the matrix-core kernel's)
constexpr int round1_rounds(int r) { return r <= 4 ? 2 : 1; }

// dynamic LDS of the round-1 routine (tile kernel, second launch): stage, cell arrays, (r <= 2) a fraction table of its own, f0 block
constexpr size_t round1_lds(int r, int C) {
    const int NC = 32 * round1_rounds(r);
    return kStageBytes + ((NC * 20 + 32 + 15) & ~15) + (r <= 2 ? ((NC * (2 * (2 * r + 1) + 1) * 4 + 15) & ~15) : 0) + (size_t)NC * (C + 4) * 4;
}

// ---- fast tiled kernel -----------------------------------------------------------------------
// Stage traffic: wave-iteration wi covers channel group (wi & 3) of the 64 region pixels starting
// at (wi >> 2) * 64: four coalesced row-segment loads (one per channel) and one 16-byte LDS write
// per lane.  Issue and commit are separate so that a whole chunk's loads are in flight at once and
// the NEXT chunk's loads stay in flight across the D-stage.  Addresses are clamped instead of
// branched around (a conditional load becomes a branch + wait per element).
template <int N, typename FT>
struct StageRegs {
    FT v[N][4];  // as stored: fp16 values are widened at the commit (widening at the load makes hipcc wait for the loads in
                 // small groups instead of keeping a chunk's worth in flight)
    int dst[N];  // float4 index in the stage, or -1
};

template <int N, typename FT>
__device__ __forceinline__ void stage_issue(StageRegs<N, FT> &r, const FT *f1c, int H, int W, const Region &rg, int wave,
                                            int lane, int wi_begin) {
    const int npx = rg.w * rg.h;
    const int nwi = ((npx + 63) >> 6) * 4;
    const float inv_w = __builtin_amdgcn_rcpf((float)rg.w);  // 1 ulp is plenty: (q + 0.5) / w stays >= 0.5 / w away from an integer
    const unsigned pl32 = (unsigned)(H * W);
#pragma unroll
    for (int u = 0; u < N; ++u) {
        const int wi = wi_begin + wave + u * kWaves;
        const int cg = wi & 3;
        const int q = ((wi >> 2) << 6) + lane;
        const bool ok = (wi < nwi) & (q < npx);
        const int y = (int)(((float)q + 0.5f) * inv_w);  // exact for q < 2^16, w < 2^10
        const int x = q - y * rg.w;
        // 32-bit element offsets from the wave-uniform chunk base (C*H*W < 2^31 is checked on the host):
        // one VGPR per address instead of a 64-bit pair
        const unsigned off = ok ? (unsigned)(cg * 4) * pl32 + (unsigned)((rg.y0 + y) * W + (rg.x0 + x)) : 0u;
        const unsigned st = ok ? pl32 : 0u;
        r.v[u][0] = f1c[off];
        r.v[u][1] = f1c[off + st];
        r.v[u][2] = f1c[off + 2 * st];
        r.v[u][3] = f1c[off + 3 * st];
        r.dst[u] = ok ? (y * rg.pitch + x) * kSlotV4 + cg : -1;
    }
}

template <int N, typename FT>
__device__ __forceinline__ void stage_commit(float4 *s4, const StageRegs<N, FT> &r) {
#pragma unroll
    for (int u = 0; u < N; ++u)
        if (r.dst[u] >= 0) s4[r.dst[u]] = make_float4((float)r.v[u][0], (float)r.v[u][1], (float)r.v[u][2], (float)r.v[u][3]);
}

// whatever of the region the first `done` wave-iterations per wave did not cover
template <int N, typename FT>
__device__ __forceinline__ void stage_rest(float4 *s4, const FT *f1c, int H, int W, const Region &rg, int wave, int lane,
                                           int done) {
    const int nwi = ((rg.w * rg.h + 63) >> 6) * 4;
    for (int wi0 = done * kWaves; wi0 < nwi; wi0 += kWaves * N) {
        StageRegs<N, FT> r;
        stage_issue(r, f1c, H, W, rg, wave, lane, wi0);
        stage_commit(s4, r);
    }
}

// One tile of 2*ROUNDS x 16 cells.
//   STAGED = true : regular path -- the tile's windows are staged in LDS; a tile whose windows do
//                   not fit is appended to p.todo and left to the second launch.
//   STAGED = false: irregular path -- same arithmetic, patch pixels gathered straight from f1 (L2).
// Geometry: the tile's NC = 32*ROUNDS cells form a block TW cells wide whose top-left cell is
// (row0, col0) of image b's grid; only its first `rows` rows belong to it (sub-tiles of a 2-row tile).
//   SECOND = false: first launch (TW = 16, one tile per workgroup).
//   SECOND = true : second launch -- an irregular tile is cut into 4 x 8 sub-tiles, each staged on
//                   its own (half the footprint along the grid row, so twice the magnification
//                   fits); a sub-tile that still does not fit falls through to the gather variant.
//   QOK: the r >= 5 staging may use the 16-byte quad loads (fp16 maps: only with an even width -- 4-byte aligned 8-byte quads; the
//        host picks the instantiation.  As a run-time flag both staging forms' registers were live at once: the fp16 kernels spilled
//        16-39 registers at 128)
template <int R, int ROUNDS, bool STAGED, int TW, bool SECOND, typename FT, int STAGE = 68 * 1024, bool QOK = true>
__device__ __forceinline__ void process_tile(const LcParams &p, int b, int row0, int col0, int rows, unsigned wid,
                                             unsigned char *smem) {
    constexpr int kStageBytes = STAGE;       // shadow the file-level defaults: the lean kernel runs this path inside its own,
    constexpr int kCapSlots = STAGE / (kSlotV4 * 16) - 1;  // smaller LDS allocation
    constexpr int PW = 2 * R + 2;            // patch width: taps -R..R plus the +1 bilinear neighbour
    constexpr int P = PW * PW;               // patch positions per cell
    constexpr int NP = (P + 15) / 16;        // positions per lane
    constexpr int D = 2 * R + 1, K = D * D;
    constexpr int NC = 32 * ROUNDS;          // cells per tile (2 * ROUNDS rows of 16)
    constexpr int DS = P + 1;                // D-buffer cell stride (odd: conflict-free epilogue reads)
    constexpr int TS = 2 * D + 1;            // fraction-table cell stride (odd)
    // small windows (r <= 2, 16-channel maps) leave LDS for a fraction table of its own next to the stage: it is then filled
    // under the first chunk's stage loads instead of after the D-stage (9 % of the r = 2 kernel)
    constexpr bool kEarlyTab = R <= 2;
    static_assert((NC * DS + (kEarlyTab ? 0 : NC * TS)) * 4 <= kStageBytes, "D buffer (+ fraction table) must fit in the stage they alias");

    float4 *s4 = reinterpret_cast<float4 *>(smem);
    float *dbuf = reinterpret_cast<float *>(smem);
    int *cellX0 = reinterpret_cast<int *>(smem + kStageBytes);
    int *cellY0 = cellX0 + NC;
    float *cellNx = reinterpret_cast<float *>(cellY0 + NC);  // normalised centre (flow) of the cell
    float *cellNy = cellNx + NC;
    int *cellSlow = reinterpret_cast<int *>(cellNy + NC);    // [NC] 1 = redo this cell with the per-tap routine
    int *bbox = cellSlow + NC;                                // x0,y0,x1,y1 of the tile's windows
    int *nSlow = bbox + 4;                                    // number of flagged cells in the tile
    int *allInside = bbox + 5;                                // 1 = no window of the tile touches the image border
    constexpr int kCellBytes = (NC * 20 + 32 + 15) & ~15;
    constexpr int kTabBytes = kEarlyTab ? (NC * TS * 4 + 15) & ~15 : 0;
    float *tab = kEarlyTab ? reinterpret_cast<float *>(smem + kStageBytes + kCellBytes)  // [NC][TS] per-tap fractions
                           : dbuf + NC * DS;                                               // ... or aliasing the stage
    float *f0s = reinterpret_cast<float *>(smem + kStageBytes + kCellBytes + kTabBytes);  // [NC][C+4]: the tile's f0, cell-major
    const int CS = p.C + 4;                                   // +4: the 4 cells a wave reads hit different banks

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int G = p.G, H = p.H, W = p.W;
    auto cell_gi = [&](int cell) { return row0 + cell / TW; };
    auto cell_gj = [&](int cell) { return col0 + cell % TW; };
    auto cell_ok = [&](int cell) { return (cell / TW < rows) & (row0 + cell / TW < G) & (col0 + cell % TW < G); };

    // ---- per-cell setup: patch origin, bounding box -------------------------------------------
    if (tid < 4) bbox[tid] = (tid & 2) ? -kFar : kFar;
    if (tid == 0) { *nSlow = 0; *allInside = 1; }
    __syncthreads();
    const float xhi = p.win_xhi, xlo = -xhi, yhi = p.win_yhi, ylo = -yhi;  // +-2r/W, +-2r/H as fp32
    // the cell's flow: requested before the f0 block below so that the two DRAM round trips of the set-up overlap
    float pre_nx = 0.f, pre_ny = 0.f;
    if (tid < NC && cell_ok(tid)) cell_coords(p, b, cell_gi(tid), cell_gj(tid), pre_nx, pre_ny);
    // the tile's f0 block (NC cells x C channels, 8-16 KB): coalesced 64-byte row segments -> LDS,
    // cell-major.  (Loading f0 per lane would issue 16 loads per round and chunk that fetch 16 bytes each.)
    {
        const float *f0b = p.f0 + (size_t)b * p.f0_bs;
        const int total = p.C * NC;
        constexpr int UF = 4;
        for (int e0 = tid; e0 < total; e0 += kThreads * UF) {
            float v[UF];
#pragma unroll
            for (int q = 0; q < UF; ++q) {
                const int e = e0 + q * kThreads;
                const int c = e / NC, cell = e - c * NC;
                const int gi = cell_gi(cell), gj = cell_gj(cell);
                const bool ok = (e < total) & cell_ok(cell);
                v[q] = f0b[ok ? (size_t)c * G * G + (size_t)gi * G + gj : 0];  // clamped address, select below
                v[q] = ok ? v[q] : 0.f;
            }
#pragma unroll
            for (int q = 0; q < UF; ++q) {
                const int e = e0 + q * kThreads;
                const int c = e / NC, cell = e - c * NC;
                if (e < total) f0s[cell * CS + c] = v[q];
            }
        }
    }
    int bx0 = kFar, by0 = kFar, bx1 = -kFar, by1 = -kFar;  // this cell's window clipped to the image
    bool inside = true;                                      // ... and whether clipping changed nothing
    if (tid < NC) {
        int X0 = kFar, Y0 = kFar, slow = 0;
        float nx = 0.f, ny = 0.f;
        if (cell_ok(tid)) {
            nx = pre_nx; ny = pre_ny;
            // patch origin = floor of the reference's own fp32 coordinate of tap 0:
            // taps kx=0..2R then read columns kx and kx+1 of the patch
            const float fx = floorf(unnorm(nx + xlo, W));  // linspace(lo, hi, D)[0] == lo
            const float fy = floorf(unnorm(ny + ylo, H));
            if ((fx > -1e6f) & (fx < 1e6f) & (fy > -1e6f) & (fy < 1e6f)) {  // false for nan/inf
                X0 = (int)fx;
                Y0 = (int)fy;
                if (STAGED) {
                    const int x0 = max(X0, 0), x1 = min(X0 + PW, W), y0 = max(Y0, 0), y1 = min(Y0 + PW, H);
                    if (x0 < x1 && y0 < y1) { bx0 = x0; by0 = y0; bx1 = x1; by1 = y1; }
                    inside = (X0 >= 0) & (X0 + PW <= W) & (Y0 >= 0) & (Y0 + PW <= H);
                }
            } else {
                slow = 1;  // non-finite / absurd flow: let the per-tap routine decide
                atomicAdd(nSlow, 1);
                inside = false;
            }
        }
        cellX0[tid] = X0;
        cellY0[tid] = Y0;
        cellNx[tid] = nx;
        cellNy[tid] = ny;
        cellSlow[tid] = slow;
    }
    if (STAGED && wave < (NC + 63) / 64) {  // bounding box: reduce inside the wave (all 64 lanes take
        // part, idle ones with the identity) with DPP row shifts / broadcasts -- the ds_bpermute butterfly took 1500+ cycles
        // of every tile's critical path -- then one LDS update per wave and bound
        bx0 = wave_min_i32(bx0); by0 = wave_min_i32(by0);
        bx1 = -wave_min_i32(-bx1); by1 = -wave_min_i32(-by1);
        // cells off the grid or with absurd flow have inside == true but an empty box: harmless
        const bool all_in = __all(inside || tid >= NC);
        if (lane == 0) {
            if (NC <= 64) {  // a single wave holds every cell: plain stores
                bbox[0] = bx0; bbox[1] = by0; bbox[2] = bx1; bbox[3] = by1;
            } else {
                atomicMin(bbox + 0, bx0);
                atomicMin(bbox + 1, by0);
                atomicMax(bbox + 2, bx1);
                atomicMax(bbox + 3, by1);
            }
            if (!all_in) *allInside = 0;
        }
    }
    // the zero slot (index kCapSlots) is what every out-of-image tap reads
    if (STAGED && tid < kSlotV4) s4[kCapSlots * kSlotV4 + tid] = make_float4(0.f, 0.f, 0.f, 0.f);
    __syncthreads();

    // ---- the staging region (block-uniform) -----------------------------------------------------
    Region u;
    u.x0 = bbox[0]; u.y0 = bbox[1];
    u.w = max(bbox[2] - u.x0, 0); u.h = max(bbox[3] - u.y0, 0);
    // Round 3, r >= 5 (64-channel maps): the stage loads are 16-byte quads through a buffer descriptor (local_corr_stage.h) instead
    // of 4-byte loads -- a 2 x 16-cell tile at r = 6 issued ~750 wave-level loads, the whole kernel's time in the CU's
    // vector-memory issue path.  A row is then whole quads (the last one may hang over the region's right edge: its pixels land in
    // pad slots nobody reads; past the tensor the descriptor returns zeros).  fp16 maps need even x0 and even rows (4-byte aligned
    // 8-byte quads); odd-width fp16 maps keep the narrow loads.
    constexpr bool quads = STAGED && R >= 5 && QOK;  // a compile-time constant: no branch around the loads, one staging form's registers
    if (quads && sizeof(FT) == 2 && (u.x0 & 1)) { u.x0 -= 1; u.w += 1; }
    const int w4 = quads ? ((u.w + 3) & ~3) : u.w;
    u.pitch = w4 + ((PW - w4) & 15);  // pitch == patch width (mod 16): conflict-free b128 reads across patch rows
    // a region that only fits without that padding is staged unpadded: some bank conflicts in the D-stage cost far less
    // than the second launch
    if (STAGED && (long)u.pitch * u.h > kCapSlots && (long)w4 * u.h <= kCapSlots) u.pitch = w4;
    if (STAGED && (long)u.pitch * u.h > kCapSlots) {
        // strong magnification / rotation / scattered flow: the windows do not fit the stage
        if (!SECOND) {
            if (tid == 0) p.todo[kTodoHdr + atomicAdd(p.todo, 1)] = (int)wid;
        } else {
            __syncthreads();
            process_tile<R, ROUNDS, false, TW, true, FT, STAGE, QOK>(p, b, row0, col0, rows, wid, smem);  // gather from L2
        }
        return;
    }

    // the first chunk's stage loads go out before the per-lane addressing below: ~2.5 k cycles of index arithmetic under the
    // round trip instead of in front of it
    const FT *f1b = f1_of<FT>(p, b);
    constexpr int PRE = 4;  // wave-iterations of stage loads kept in flight (48 x 64 px x 4 ch = a 768-pixel region)
    StageRegs<PRE, FT> pre;
    constexpr int PRE0 = R <= 2 ? 4 : 6;  // the first chunk is requested before the D-stage registers exist: more of it in flight at
                                          // once (r <= 2 regions need 3.5 iterations; unused ones still cost their index math)
    StageRegs<PRE0, FT> pre0;
    // the quad form (r >= 5): the region as a RowPlan, two items per lane in flight
    RowPlan up;
    up.x0 = u.x0; up.y0 = u.y0; up.w = u.w; up.h = u.h; up.pitch = u.pitch; up.nq = (u.w + 3) >> 2;
    up.nitems = ((up.h * up.nq + 15) / 16 + 7) & ~7;
    QuadLane qlq;
    QuadRegs<kQuadPre, FT> preq;
    const rsrc_t f1r = make_rsrc(f1b, (unsigned)p.C * (unsigned)(H * W) * (unsigned)sizeof(FT));
    if (quads) {
#pragma unroll
        for (int n = 0; n < kQuadPre; ++n) qlq.it[n] = quad_item<false, FT, kSlotV4, true>(up, H, W, wave, lane, n);
        quad_issue<kQuadPre, false, FT, kSlotV4, true>(preq, f1r, 0u, H, W, up, wave, lane, qlq, 0);
    } else if (STAGED) {
        stage_issue(pre0, f1b, H, W, u, wave, lane, 0);
    }

    // fraction table: the reference's fp32 coordinate of every tap column / row of every cell
    // (local_correlation.py:55 adds window offsets in normalised units, grid_sample un-normalises)
    auto fill_table = [&]() {
        for (int e = tid; e < NC * 2 * D; e += kThreads) {
            const int cell = e / (2 * D), a = e - cell * (2 * D);
            const bool isy = a >= D;
            const int k = isy ? a - D : a;
            const float n = isy ? cellNy[cell] : cellNx[cell];
            const float pix = unnorm(n + (isy ? gfn::linspace_step_at(ylo, yhi, p.win_ystep, D, k) : gfn::linspace_step_at(xlo, xhi, p.win_xstep, D, k)),
                                     isy ? H : W);
            const float fl = floorf(pix);
            const int origin = isy ? cellY0[cell] : cellX0[cell];
            // tap k must start at patch column/row k; if rounding moved its floor(), redo the cell per tap
            if (origin != kFar && !(fl == (float)(origin + k))) {
                cellSlow[cell] = 1;
                atomicAdd(nSlow, 1);
            }
            tab[cell * TS + a] = pix - fl;
        }
    };
    if (kEarlyTab) fill_table();

    // ---- per-lane D-stage addressing -----------------------------------------------------------
    int g, s16;
    lane_group(lane, g, s16);
    const int cr = wave * 4 + g;  // cell inside a round (0..31): row cr>>4, column cr&15
    const bool interior = STAGED && *allInside != 0;  // block-uniform
    unsigned apk[ROUNDS][(NP + 1) / 2];  // staged: float4 index (< 2^16) of each (round, pass) patch pixel, two per register
    float acc[ROUNDS][NP];
#pragma unroll
    for (int rd = 0; rd < ROUNDS; ++rd) {
        const int cell = rd * 32 + cr;
        const int X0 = cellX0[cell], Y0 = cellY0[cell];
        // interior tiles (no window touches the border, every cell on the grid): no per-pixel tests
        const int base = (Y0 - u.y0) * u.pitch + (X0 - u.x0);
#pragma unroll
        for (int t = 0; t < NP; ++t) {
            acc[rd][t] = 0.f;
            if (STAGED) {
                const int pp = s16 + 16 * t;
                const int yy = pp / PW, xx = pp - yy * PW;
                int slot;
                if (interior) {
                    slot = (pp < P && X0 != kFar) ? base + yy * u.pitch + xx : kCapSlots;
                } else {
                    const int X = X0 + xx, Y = Y0 + yy;
                    const bool in = (pp < P) & ((unsigned)X < (unsigned)W) & ((unsigned)Y < (unsigned)H);
                    slot = in ? (Y - u.y0) * u.pitch + (X - u.x0) : kCapSlots;
                }
                const unsigned a = (unsigned)(slot * kSlotV4);
                if (t & 1)
                    apk[rd][t >> 1] |= a << 16;
                else
                    apk[rd][t >> 1] = a;
            }
        }
    }

    // ---- main loop: 16 channels at a time ----------------------------------------------------
    const size_t cs = (size_t)G * G;
    if (quads) {
        quad_commit<kQuadPre, false, FT>(s4, preq, H, W, up, wave, lane, qlq, 0);
        quad_rest<false, FT>(s4, f1r, 0u, H, W, up, wave, lane, qlq, kQuadPre);
    } else if (STAGED) {
        stage_commit(s4, pre0);
        stage_rest<2>(s4, f1b, H, W, u, wave, lane, PRE0);
    }
    if (STAGED) __syncthreads();
    for (int c0 = 0; c0 < p.C; c0 += kChunk) {
        const FT *f1c = f1b + (size_t)c0 * H * W;
        const bool more = c0 + kChunk < p.C;
        if (STAGED) {
            // keep the packed indices packed: without this the unpacking is hoisted out of the loop and
            // the unpacked copies cost NP more registers per round
#pragma unroll
            for (int rd = 0; rd < ROUNDS; ++rd)
#pragma unroll
                for (int h = 0; h < (NP + 1) / 2; ++h) asm volatile("" : "+v"(apk[rd][h]));
            // next chunk's loads: in flight across this chunk's D-stage
            const unsigned next_off = (unsigned)(c0 + kChunk) * (unsigned)(H * W) * (unsigned)sizeof(FT);
            if (more && quads) quad_issue<kQuadPre, false, FT, kSlotV4, true>(preq, f1r, next_off, H, W, up, wave, lane, qlq, 0);
            else if (more) stage_issue(pre, f1c + (size_t)kChunk * H * W, H, W, u, wave, lane, 0);
        }
#pragma unroll
        for (int rd = 0; rd < ROUNDS; ++rd) {
            float f[kChunk];
            {   // this lane's cell, 16 channels: 4 LDS reads (the 16 lanes of a cell read the same address)
                const float4 *fq = reinterpret_cast<const float4 *>(f0s + (rd * 32 + cr) * CS + c0);
                const float4 a0 = fq[0], a1 = fq[1], a2 = fq[2], a3 = fq[3];
                f[0] = a0.x; f[1] = a0.y; f[2] = a0.z; f[3] = a0.w; f[4] = a1.x; f[5] = a1.y; f[6] = a1.z; f[7] = a1.w;
                f[8] = a2.x; f[9] = a2.y; f[10] = a2.z; f[11] = a2.w; f[12] = a3.x; f[13] = a3.y; f[14] = a3.z; f[15] = a3.w;
            }
            if (STAGED) {
#pragma unroll
                for (int t = 0; t < NP; ++t) {
                    const float4 *q = s4 + ((t & 1) ? (apk[rd][t >> 1] >> 16) : (apk[rd][t >> 1] & 0xFFFFu));
                    const float4 v0 = q[0], v1 = q[1], v2 = q[2], v3 = q[3];
                    float a = acc[rd][t];
                    a = fmaf(f[0], v0.x, a);  a = fmaf(f[1], v0.y, a);  a = fmaf(f[2], v0.z, a);  a = fmaf(f[3], v0.w, a);
                    a = fmaf(f[4], v1.x, a);  a = fmaf(f[5], v1.y, a);  a = fmaf(f[6], v1.z, a);  a = fmaf(f[7], v1.w, a);
                    a = fmaf(f[8], v2.x, a);  a = fmaf(f[9], v2.y, a);  a = fmaf(f[10], v2.z, a); a = fmaf(f[11], v2.w, a);
                    a = fmaf(f[12], v3.x, a); a = fmaf(f[13], v3.y, a); a = fmaf(f[14], v3.z, a); a = fmaf(f[15], v3.w, a);
                    acc[rd][t] = a;
                }
            } else {
                const size_t plane = (size_t)H * W;
                const int cX0 = cellX0[rd * 32 + cr], cY0 = cellY0[rd * 32 + cr];
                // TG patch positions x 16 channels = 64 gathers in flight per lane: this path is pure L2 latency
                // (one position at a time left a sub-tile of scattered flow at 150-200 us)
                constexpr int TG = 4;
#pragma unroll
                for (int t0 = 0; t0 < NP; t0 += TG) {
                    FT v[TG][kChunk];  // as stored: fp16 values are widened at their use (widening at the load made hipcc wait for
                                       // the gathers in small groups: the scattered-flow path ran 2x slower on fp16 maps)
                    bool in[TG];
#pragma unroll
                    for (int tt = 0; tt < TG; ++tt) {
                        if (t0 + tt < NP) {
                            const int pp = s16 + 16 * (t0 + tt);
                            const int yy = pp / PW, xx = pp - yy * PW;
                            const int X = cX0 + xx, Y = cY0 + yy;
                            in[tt] = (pp < P) & ((unsigned)X < (unsigned)W) & ((unsigned)Y < (unsigned)H);
                            const unsigned off = in[tt] ? (unsigned)(Y * W + X) : 0u;  // offset 0 when outside: valid memory, masked below
#pragma unroll
                            for (int k = 0; k < kChunk; ++k) v[tt][k] = f1c[k * plane + off];  // scalar plane base + 32-bit lane offset
                        }
                    }
#pragma unroll
                    for (int tt = 0; tt < TG; ++tt) {
                        if (t0 + tt < NP) {
                            float a = acc[rd][t0 + tt];
#pragma unroll
                            for (int k = 0; k < kChunk; ++k) a = fmaf(f[k], in[tt] ? (float)v[tt][k] : 0.f, a);
                            acc[rd][t0 + tt] = a;
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);  // one group of loads in flight at a time (register budget)
                }
            }
        }
        // do not let the scheduler sink this chunk's FMAs below the barrier (it would keep every
        // LDS read result of the chunk live across it: hundreds of spills)
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int rd = 0; rd < ROUNDS; ++rd)
#pragma unroll
            for (int t = 0; t < NP; ++t) asm volatile("" : "+v"(acc[rd][t]));  // pins the FMAs above this point
        if (STAGED && more) {
            __syncthreads();  // everyone is done reading this chunk
            if (quads) {
                const unsigned next_off = (unsigned)(c0 + kChunk) * (unsigned)(H * W) * (unsigned)sizeof(FT);
                quad_commit<kQuadPre, false, FT>(s4, preq, H, W, up, wave, lane, qlq, 0);
                quad_rest<false, FT>(s4, f1r, next_off, H, W, up, wave, lane, qlq, kQuadPre);
            } else {
                stage_commit(s4, pre);
                stage_rest<2>(s4, f1c + (size_t)kChunk * H * W, H, W, u, wave, lane, PRE);
            }
            __syncthreads();
        }
    }

    // ---- epilogue: D -> LDS, per-tap fractions, bilinear combination, coalesced stores -------
    __syncthreads();
#pragma unroll
    for (int rd = 0; rd < ROUNDS; ++rd) {
        const int cell = rd * 32 + cr;
#pragma unroll
        for (int t = 0; t < NP; ++t) {
            const int pp = s16 + 16 * t;
            if (pp < P) dbuf[cell * DS + pp] = acc[rd][t];
        }
    }
    if (!kEarlyTab) fill_table();
    __syncthreads();
    {
        // each wave combines CW cells x a strided subset of the K taps: lane -> cell (so that stores run
        // along the grid row), taps strided over the waves (and over lane halves when NC == 32)
        constexpr int CW = NC >= 64 ? 64 : 32;          // cells per wave-instruction
        constexpr int NCB = NC / CW;                    // groups of CW cells per tile
        constexpr int WPB = kWaves / NCB * (64 / CW);   // tap phases sharing one group of cells
        const int cell = (wave / (kWaves / NCB)) * CW + (lane & (CW - 1));
        const int kphase = (wave % (kWaves / NCB)) * (64 / CW) + (lane / CW);
        const int gi = cell_gi(cell), gj = cell_gj(cell);
        if (cell_ok(cell) && !cellSlow[cell]) {
            // one tap ROW (ky) at a time: the two D rows it needs are read once (2*PW LDS reads for D
            // outputs), the column fractions of the cell stay in registers
            const float *dc = dbuf + cell * DS;
            const float *tc = tab + cell * TS;
            float *o = p.out + (size_t)b * p.out_bs + (size_t)gi * G + gj;
            float wx1[D], wx0[D];
#pragma unroll
            for (int kx = 0; kx < D; ++kx) { wx1[kx] = tc[kx]; wx0[kx] = 1.f - wx1[kx]; }
            constexpr int NR = (D + WPB - 1) / WPB;
#pragma unroll
            for (int n = 0; n < NR; ++n) {
                const int ky = kphase + n * WPB;
                if (ky < D) {
                    // separable bilinear: the PW patch columns are blended vertically once (1/sqrt(C) folded into the row
                    // weights), every tap is then two instructions -- 4 per output instead of the 12 of the four-corner
                    // form (the combine was ~28 % of a tile's vector instructions at r = 4)
                    const float wy1 = tc[D + ky];
                    const float wy1s = wy1 * p.inv_sqrt_c, wy0s = (1.f - wy1) * p.inv_sqrt_c;
                    const float *d = dc + ky * PW;
                    float m[PW];
#pragma unroll
                    for (int x = 0; x < PW; ++x) m[x] = fmaf(d[PW + x], wy1s, d[x] * wy0s);
                    float *ok = o + (size_t)(ky * D) * cs;
#pragma unroll
                    for (int kx = 0; kx < D; ++kx)
                        __builtin_nontemporal_store(fmaf(m[kx + 1], wx1[kx], m[kx] * wx0[kx]),
                                                    ok + (size_t)kx * cs);  // streamed: nothing on the hot path reads it back
                }
            }
        }
    }

    // ---- flagged cells: general per-tap routine (about one cell in 10^4) ------------------------
    if (*nSlow != 0) {  // block-uniform, rare
        // compact the flagged cells (cellX0 is free now), then spread (cell, tap) pairs over the whole workgroup
        __syncthreads();
        if (tid == 0) {
            int n = 0;
            for (int cell = 0; cell < NC; ++cell)
                if (cellSlow[cell] && cell_ok(cell)) cellX0[n++] = cell;
            *nSlow = n;
        }
        __syncthreads();
        const int total = *nSlow * K;
        for (int e = tid; e < total; e += kThreads) {
            const int cell = cellX0[e / K], k = e % K;
            const int gi = cell_gi(cell), gj = cell_gj(cell);
            p.out[(size_t)b * p.out_bs + ((size_t)k * G + gi) * G + gj] =
                tap_general<FT>(p, b, gi, gj, k / D, k % D, D, cellNx[cell], cellNy[cell]);
        }
    }
}

template <int R, int ROUNDS, typename FT, bool QOK = true>
__global__ __launch_bounds__(kThreads, 4) void local_corr_tile_kernel(LcParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const unsigned wid = gfn::xcd_remap(blockIdx.x, gridDim.x);
    const int tiles = p.tiles_x * p.tiles_y;
    const int b = wid / tiles, tile = wid - b * tiles;
    const int ty = tile / p.tiles_x, tx = tile - ty * p.tiles_x;
    process_tile<R, ROUNDS, true, kTileW, false, FT, 68 * 1024, QOK>(p, b, ty * 2 * ROUNDS, tx * kTileW, 2 * ROUNDS, wid, smem);
}

// second launch: the tiles the staged kernel left in p.todo (their number is only known on the
// device), re-cut into sub-tiles 8 cells wide and up to 4 rows high
// worker `me` of `nworkers`: the separate second launch (round-1 path: a workgroup of its own), or the first workgroups of the
// lean tile kernel (which finishes the plan launch's list inside its own launch, with its own -- smaller -- stage)
template <int R, int ROUNDS, typename FT, int STAGE, bool QOK = true>
__device__ __forceinline__ void second_launch_worker(const LcParams &p, unsigned char *smem, int me, int nworkers) {
    constexpr int TH = 2 * ROUNDS, SH = TH < 4 ? TH : 4;  // sub-tile height
    constexpr int SUBS = (TH / SH) * (kTileW / 8);
    const int n = p.todo[0] * SUBS;
    const int tiles = p.tiles_x * p.tiles_y;
    // Only as many workgroups as there are work items take part (the rest leave at once): with no tile on the list -- the
    // common case -- the launch costs one load per workgroup instead of two contended atomics (14 us for 512 workgroups).
    const int part = n < nworkers ? n : nworkers;
    if (me >= (part > 0 ? part : 1)) return;
    // work items differ by 10x (a staged sub-tile vs one that gathers from L2): after its first item (its own block id) a
    // workgroup draws tickets first come, first served
    __shared__ int next_item;
    int it = me;
    while (it < n) {
        const unsigned wid = (unsigned)p.todo[kTodoHdr + it / SUBS];
        const int sub = it % SUBS;
        const int b = wid / tiles, tile = wid - b * tiles;
        const int ty = tile / p.tiles_x, tx = tile - ty * p.tiles_x;
        process_tile<R, 1, true, 8, true, FT, STAGE, QOK>(p, b, ty * TH + (sub >> 1) * SH, tx * kTileW + (sub & 1) * 8, SH, wid, smem);
        __syncthreads();  // LDS (and next_item) are reused by the next sub-tile
        if (threadIdx.x == 0) next_item = part + atomicAdd(p.todo + 1, 1);
        __syncthreads();
        it = __builtin_amdgcn_readfirstlane(next_item);  // scalar: everything derived from it (b, map bases) stays in SGPRs
    }
    // the last workgroup to leave puts the counters back to zero for the next call: no memset node in front of every call.
    // Every participant has read todo[0] and drawn its last queue ticket before it gets here.
    if (threadIdx.x == 0 && (part <= 1 || atomicAdd(p.todo + 2, 1) == part - 1)) {
        p.todo[3] = p.todo[0];  // informational (tools/count_irregular.py, bench.py)
        p.todo[5] = p.todo[4];
        p.todo[4] = 0;
        p.todo[7] = p.todo[6];
        p.todo[6] = 0;
        p.todo[0] = 0;
        p.todo[1] = 0;
        p.todo[2] = 0;
    }
}

template <int R, int ROUNDS, typename FT, bool QOK = true>
__global__ __launch_bounds__(kThreads, 2) void local_corr_irregular_kernel(LcParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    second_launch_worker<R, ROUNDS, FT, kStageBytes, QOK>(p, smem, (int)blockIdx.x, (int)gridDim.x);
}

}  // namespace
