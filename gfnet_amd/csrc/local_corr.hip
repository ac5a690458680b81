// local_corr.hip -- fused local correlation for gfx950 (MI355X).
//
// Replaces utils/local_correlation.py:4-72 of the reference (called at model/network.py:553-554):
//   out[b,k,i,j] = sum_c f0[b,c,i,j]/sqrt(C) * grid_sample(f1[b,c], flow[b,:,i,j] + window[k])
// The reference materialises a (C,G,G,K) sampled tensor per batch element (26-59 MB) and makes
// three passes over it; here nothing but the (K,G,G) result is written.
//
// Fast path (one feature pixel per window tap, i.e. every call the reference makes):
//   * all K taps of a cell share one pair of bilinear fractions, so for each cell
//         D[y][x]   = sum_c f0[c] * f1[c][Y0+y][X0+x]        (y,x over the (2r+2)^2 patch)
//         out[ky,kx] = (w00 D[ky][kx] + w01 D[ky][kx+1] + w10 D[ky+1][kx] + w11 D[ky+1][kx+1])/sqrt(C)
//     which is 3x fewer FMAs and 4x fewer feature reads than sampling every tap;
//   * a workgroup (512 threads, 8 waves) owns a tile of 2*ROUNDS x 16 grid cells.  The bounding
//     box of the tile's patches is staged from f1 (NCHW, coalesced row reads, L2-resident) into
//     LDS as [pixel][16 channels + 4 pad] (80-byte slots), 16 channels at a time;
//   * D-stage: 16 lanes per cell, each lane owns patch positions p = s+16t.  A ds_read_b128 lane
//     group (the hardware's 16-lane b128 groups, MI355X_MICROARCH.md section LDS) reads 16
//     consecutive patch positions of ONE cell; with the 20-dword slot and a row pitch == patch
//     width (mod 16) these are 16 distinct 4-bank groups -> conflict-free 256 B/clk reads;
//     f0 is held in registers (16 per lane), accumulators in registers (<= 16 per round);
//   * epilogue: D goes through LDS (aliasing the stage), each wave combines 64 cells x taps and
//     stores 64-byte row segments of the (K,G,G) output.
//   * the reference adds the window offsets in normalised fp32 coordinates, tap by tap, so its
//     taps sit on whole-pixel steps only to ~3e-5 px (at W=280).  To stay bit-faithful the
//     epilogue uses, per cell and per tap row/column, the fraction of exactly that fp32 sequence
//     (a small LDS table); a cell for which some tap's floor() disagrees with (origin + tap
//     index) -- the centre within rounding of a pixel boundary, or a non-finite flow -- is redone
//     by the general per-tap routine at the end of the launch (about one cell in 10^4);
//   * tiles whose bounding box does not fit the stage (wild flow) are staged per 2x16 round, and
//     rounds that still do not fit use the general per-tap routine inside the same launch.
// General path (any C, radius, non-integer tap spacing: grid_based_correlation, pooled levels):
//   one thread per (cell, tap), per-tap bilinear gather exactly as grid_sample does it: the bilinear + zeros instantiation of
//   local_corr_mode_kernel (local_corr_modes.hip), whose per-tap routine (tap_dot on Taps<MODE>, local_corr_common.h,
//   sample_modes.h) is also what the tiled kernels call for flagged cells.  The feature0 gradient (gfn_local_corr_bwd_f0) is
//   gfn_local_corr_mode_bwd_f0 for bilinear + zeros.
//
// Block->tile mapping is XCD-aware (common.h): consecutive tiles of one image stay on one XCD so
// the 3-4x halo re-reads of f1 are served by that XCD's L2, not HBM.
#include <type_traits>
#include "local_corr_common.h"
#include "local_corr_tile.h"
#include "local_corr_lean.h"
#include "local_corr_mq.h"

namespace {

// shapes the lean tile path takes (it keeps at most 8 channels of the f0 block per wave in registers, addresses planes with
// 32-bit byte offsets, and reads fp16 quads at 4-byte alignment)
bool lean_shape(int C, int H, int W, int G, int r, int f16) {
    const long K = (long)(2 * r + 1) * (2 * r + 1);
    if (!(r >= 1 && r <= 7 && (C == 16 || C == 32 || C == 64) && !(f16 && (W & 1)) && (long)C * H * W < (1L << 30) && K * G * G < (1L << 30) &&
          (long)C * G * G < (1L << 30)))
        return false;
    // Large windows (r >= 5) stay on the round-1 kernel with quad staging: a lean tile kernel for them (f0 block staged chunk by chunk)
    // measured on par where the 4 x 16-cell tile's region fits the stage (r = 7 on 32 x 32 maps: 80.7 vs 79.5 us), slower where every
    // tile would be staged in halves (r = 6 at spacing 1.75: 113 vs 79 us) and under the raw soft-argmax flows scale 16 sees in the
    // bench (160 vs 110 + 44 us).
    return r <= 4;
}

// large windows on 64-channel maps: the matrix-core tile kernel of local_corr_mq.h is the first launch (byte offsets into the maps and
// the kOffRange marker share 31 bits)
bool mq_shape(int C, int H, int W, int G, int r, int f16) {
    const long K = (long)(2 * r + 1) * (2 * r + 1);
    return r >= 5 && r <= 7 && C == 64 && !(f16 && (W & 1)) && (long)C * H * W * (f16 ? 2 : 4) < 0x7FFFFFF0L &&
           K * G * G * 4 < 0x7FFFFFF0L && (long)C * G * G * 4 < 0x7FFFFFF0L;
}

// scratch layout of the lean path: header and tile list (ints), then the plan, 32-byte aligned
int *lean_plan_ptr(void *scratch, int B, int G) {
    const int64_t tiles_max = (int64_t)((G + 1) / 2) * ((G + 15) / 16) * B;  // what gfn_local_corr_scratch_bytes sized the list for
    return reinterpret_cast<int *>(((uintptr_t)scratch + 4 * (tiles_max + kTodoHdr) + 31) & ~(uintptr_t)31);
}

// ---- host: routing ----------------------------------------------------------------------------------------------------
// gfn_local_corr_fwd_dt's `variant`, decoded.  0: the tiled path (lean fp32 tile kernel for r <= 4, the matrix-core kernel for r >= 5
// on 64-channel maps); 1 (and 3, 5, 6, 7): general kernel; 2: the round-1 tile kernel for every radius; 4: the lean tile kernel with the
// round-2 fp32 FMA D-stage (bit-identical to variant 2; the fp32 cross-check / opt-out of the r >= 5 matrix-core kernel); + 8: `planned`.
struct LcVariant {
    bool tiled;    // 0, 2, 4: a tile kernel where the call allows one
    bool lean;     // 0, 4: the lean kernel where lean_shape() allows it
    bool mq;       // 0: the matrix-core kernel where mq_shape() allows it
    bool planned;  // + 8: gfn_refiner_input_plan_fwd_dt has already written this call's plan
};
LcVariant decode_variant(int variant) {
    const int v = variant & ~8;
    return {v == 0 || v == 2 || v == 4, v == 0 || v == 4, v == 0, (variant & 8) != 0};
}

enum class LcRoute {
    Refused,       // variant 8 on a call the lean path does not take
    General,       // local_corr_mode_kernel<FT, bilinear, zeros> (local_corr_modes.hip)
    Lean,          // (plan kernel) + local_corr_tile2_kernel (+ r <= 2: local_corr_irregular_kernel)
    Round1,        // local_corr_tile_kernel + local_corr_irregular_kernel, 16-byte quad staging at r >= 5 (QOK)
    Round1Narrow,  // the same with the narrow stage loads (!QOK): r >= 5 on fp16 maps of odd width
    Mq,            // local_corr_mq_kernel + local_corr_irregular_kernel
};

// how a forward call runs, from its shape and dtype (p as lc_params() fills it), its scratch and its variant
LcRoute lc_route(const LcParams &p, const void *scratch, int64_t scratch_bytes, LcVariant v) {
    const bool dense = !p.grid_based && p.win_h == p.H && p.win_w == p.W;  // one feature pixel per window tap
    const bool lean = v.lean && p.flow && dense && lean_shape(p.C, p.H, p.W, p.G, p.r, p.f16);
    if (v.planned && !lean) return LcRoute::Refused;
    // the tiled routes need the tile list in scratch; without it the general kernel still gives the right answer
    if (!v.tiled || !dense || p.C % kChunk || p.r < 1 || p.r > 7 || !scratch || scratch_bytes < gfn_local_corr_scratch_bytes(p.B, p.G) ||
        ((uintptr_t)scratch & 3))
        return LcRoute::General;
    if (lean) return LcRoute::Lean;
    // <= 80 KB (two workgroups per CU) for every shape GFNet uses; other C/r combinations still run, one workgroup per CU; absurdly
    // wide features go to the general kernel
    if (round1_lds(p.r, p.C) > kMaxLds) return LcRoute::General;
    // r >= 5 stages through a 32-bit buffer descriptor (local_corr_stage.h): maps of 2 GiB and more would wrap its byte count and
    // stage zeros; the general kernel (64-bit pointers) takes them
    if (p.r >= 5 && (long)p.C * p.H * p.W * (p.f16 ? 2 : 4) >= 0x7FFFFFF0L) return LcRoute::General;
    if (v.mq && p.flow && mq_shape(p.C, p.H, p.W, p.G, p.r, p.f16)) return LcRoute::Mq;
    // fp16 maps of odd width (35 x 35: scale 8 of a 280-pixel refinement pass) keep the narrow stage loads at r >= 5: an 8-byte quad
    // of such a row is not 4-byte aligned.  A kernel instantiation of its own, so that the staging form is a compile-time constant.
    return (p.r >= 5 && p.f16 && (p.W & 1)) ? LcRoute::Round1Narrow : LcRoute::Round1;
}

// the tile grid and the window parameters every tiled launch needs (what tap_general, the plan and the fraction tables read)
void tiled_window(LcParams &p) {
    p.tiles_x = (p.G + kTileW - 1) / kTileW;
    p.tiles_y = (p.G + 2 * round1_rounds(p.r) - 1) / (2 * round1_rounds(p.r));  // r <= 4: the lean kernel's 4 x 16-cell tiles too
    p.win_h = p.H; p.win_w = p.W; p.grid_based = 0;
    p.win_xhi = (float)(2.0 * p.r / p.W);
    p.win_yhi = (float)(2.0 * p.r / p.H);
    // exactly the fp32 operations linspace_at performs: (end - start) / (float)(steps - 1)
    const volatile float xlo = -p.win_xhi, ylo = -p.win_yhi, n1 = (float)(2 * p.r);
    p.win_xstep = (p.win_xhi - xlo) / n1;
    p.win_ystep = (p.win_yhi - ylo) / n1;
}

// f(std::integral_constant<int, R>, FT()) for radius r (R = r for r = 1 .. RMAX - 1, otherwise RMAX) and the map's dtype
template <int RMAX, typename F>
int with_radius(int r, bool f16, F &&f) {
    if (RMAX > 1 && r < RMAX) return with_radius<(RMAX > 1 ? RMAX - 1 : 1)>(r, f16, f);
    const std::integral_constant<int, RMAX> R;
    return f16 ? f(R, _Float16()) : f(R, float());
}

// ---- host: launchers ---------------------------------------------------------------------------------------------------------
// the second launch: the tiles the first launch (or the plan) listed, their number only known on the device.  One workgroup per
// CU at most: with nothing on the list (the common case) the launch is pure overhead.
template <int R, typename FT, bool QOK = true>
int launch_second(const LcParams &p, unsigned total, hipStream_t s) {
    constexpr int ROUNDS = round1_rounds(R);
    // per call and unconditional: the attribute is per device, a process may drive several
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(local_corr_irregular_kernel<R, ROUNDS, FT, QOK>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLds);
    const unsigned grid2 = total < 256 ? total : 256;
    hipLaunchKernelGGL((local_corr_irregular_kernel<R, ROUNDS, FT, QOK>), dim3(grid2), dim3(kThreads), round1_lds(R, p.C), s, p);
    return gfn::check_launch("local_corr_irregular_kernel");
}

template <int R, int NCH, typename FT>
void launch_tile2(const LcParams &p, unsigned total, size_t lds, hipStream_t s) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(local_corr_tile2_kernel<R, NCH, FT>), hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLds);
    hipLaunchKernelGGL((local_corr_tile2_kernel<R, NCH, FT>), dim3(total + lean_workers<R>()), dim3(kThreads), lds, s, p);
}

// the lean route (local_corr_lean.h): plan (unless the refiner-input launch wrote it), the tile kernel, and for r <= 2 the separate
// second launch (r >= 3: the tile kernel's first workgroups are the second launch)
template <int R, typename FT>
int launch_lean(const LcParams &p, unsigned total, hipStream_t s) {
    static_assert(Lean<R>::lds(64) <= kMaxLds, "the lean kernel's LDS holds every shape lean_shape() admits (C <= 64)");
    if (!p.planned) {
        hipLaunchKernelGGL((local_corr_plan_kernel<R>), dim3((total + 4 * kPlanPerWave - 1) / (4 * kPlanPerWave)), dim3(256), 0, s, p);
        if (int e = gfn::check_launch("local_corr_plan_kernel")) return e;
    }
    const size_t lds = Lean<R>::lds(p.C);
    switch (p.C) {  // the lean kernel is specialised on the number of 16-channel chunks
        case 16: launch_tile2<R, 1, FT>(p, total, lds, s); break;
        case 32: launch_tile2<R, 2, FT>(p, total, lds, s); break;
        default: launch_tile2<R, 4, FT>(p, total, lds, s); break;
    }
    if (int e = gfn::check_launch("local_corr_tile2_kernel")) return e;
    // (Round 5: marking the tile kernel hipExtAnyOrderLaunch behind a second launch issued first -- the two are independent, the plan
    // launch wrote the list -- does not make them run side by side on gfx950: 107.2 vs 108.5 us with three tiles listed, the flag is
    // documented as unsupported on GFX9.)
    return lean_workers<R>() > 0 ? GFN_OK : launch_second<R, FT>(p, total, s);
}

// the round-1 and matrix-core routes: the staged tile kernel (p.mq: the matrix-core kernel of local_corr_mq.h), then the second
// launch for the tiles it listed
template <int R, typename FT, bool QOK>
int launch_round1(const LcParams &p, unsigned total, hipStream_t s) {
    constexpr int ROUNDS = round1_rounds(R);
    if constexpr (R >= 5) {
        static_assert(ROUNDS == 1, "the matrix-core kernel's tiles are the round-1 kernel's 2 x 16 cells: they share the second launch");
        if (p.mq) {
            (void)hipFuncSetAttribute(reinterpret_cast<const void *>(local_corr_mq_kernel<R, 64, FT, QOK>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, kMqLds);
            hipLaunchKernelGGL((local_corr_mq_kernel<R, 64, FT, QOK>), dim3(total), dim3(kThreads), kMqLds, s, p);
            if (int e = gfn::check_launch("local_corr_mq_kernel")) return e;
            return launch_second<R, FT, QOK>(p, total, s);
        }
    }
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(local_corr_tile_kernel<R, ROUNDS, FT, QOK>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLds);
    hipLaunchKernelGGL((local_corr_tile_kernel<R, ROUNDS, FT, QOK>), dim3(total), dim3(kThreads), round1_lds(R, p.C), s, p);
    if (int e = gfn::check_launch("local_corr_tile_kernel")) return e;
    return launch_second<R, FT, QOK>(p, total, s);
}

// a tiled route of radius R (p.r)
template <int R, typename FT>
int launch_tiled(LcRoute route, const LcParams &p, unsigned total, hipStream_t s) {
    if constexpr (R <= 4) {  // lean_shape() never takes r >= 5: do not instantiate those kernels
        if (route == LcRoute::Lean) return launch_lean<R, FT>(p, total, s);
    }
    if constexpr (R >= 5 && sizeof(FT) == 2) {
        if (route == LcRoute::Round1Narrow) return launch_round1<R, FT, false>(p, total, s);
    }
    return launch_round1<R, FT, true>(p, total, s);
}

}  // namespace

// ints of scratch the tiled path wants: the list of tiles left to the irregular launch.
GFN_EXPORT int64_t gfn_local_corr_scratch_bytes(int B, int G) {
    // smallest tile is 2 x 16 cells -> at most B * ceil(G/2) * ceil(G/16) tiles, plus the counter
    const int64_t tiles = (int64_t)((G + 1) / 2) * ((G + 15) / 16);
    // header + tile list (ints), then the lean path's plan (16 bytes per tile, 16-byte aligned)
    return 4 * ((int64_t)B * tiles + kTodoHdr) + 32 + 4 * kPlanInts * (int64_t)B * tiles;
}

GFN_EXPORT int gfn_local_corr_fwd_ex(const float *f0, int64_t f0_bs, const float *f1, const float *f1_second,
                                     const float *flow, float *out, int64_t out_bs, int B, int C, int G, int H, int W,
                                     int r, int grid_based, int win_h, int win_w, int variant, void *scratch,
                                     int64_t scratch_bytes, gfn_stream_t stream) {
    return gfn_local_corr_fwd_dt(f0, f0_bs, f1, f1_second, GFN_F32, flow, out, out_bs, B, C, G, H, W, r, grid_based, win_h, win_w, variant, scratch,
                                 scratch_bytes, stream);
}

GFN_EXPORT int gfn_local_corr_fwd_dt(const float *f0, int64_t f0_bs, const void *f1, const void *f1_second, int f1_dtype,
                                     const float *flow, float *out, int64_t out_bs, int B, int C, int G, int H, int W,
                                     int r, int grid_based, int win_h, int win_w, int variant, void *scratch,
                                     int64_t scratch_bytes, gfn_stream_t stream) {
    if (f1_dtype != GFN_F32 && f1_dtype != GFN_F16) return gfn::fail(GFN_ERR_INVALID_ARG, "local_corr: feature dtype must be GFN_F32 or GFN_F16");
    if (int e = check_args("local_corr", !f0 || !f1 || !out, f1_second && (B & 1), B, C, G, H, W, r, win_h, win_w, f0_bs, out_bs, flow != nullptr,
                           GFN_SAMPLE_BILINEAR, GFN_PAD_ZEROS))
        return e;
    if (B == 0) return GFN_OK;
    hipStream_t s = (hipStream_t)stream;
    LcParams p = lc_params(f1, f1_second, f1_dtype == GFN_F16, flow, B, C, G, H, W, r, grid_based, win_h, win_w);
    p.f0 = f0; p.out = out; p.f0_bs = f0_bs; p.out_bs = out_bs;
    const LcVariant v = decode_variant(variant);
    const LcRoute route = lc_route(p, scratch, scratch_bytes, v);
    if (route == LcRoute::Refused) return gfn::fail(GFN_ERR_INVALID_ARG, "local_corr: variant 8 (plan present) on a call the lean path does not take");
    if (route == LcRoute::General) return gfn_lc_launch_taps(p, GFN_SAMPLE_BILINEAR, GFN_PAD_ZEROS, s);
    tiled_window(p);
    p.todo = reinterpret_cast<int *>(scratch);
    p.todo_ints = scratch_bytes / 4;
    p.planned = v.planned ? 1 : 0;
    p.mq = route == LcRoute::Mq ? 1 : 0;
    if (route == LcRoute::Lean) {  // scratch: the tile list, then the plan
        p.plan = lean_plan_ptr(scratch, B, G);
        p.todo_ints = (int64_t)((G + 1) / 2) * ((G + 15) / 16) * B + kTodoHdr;
    }
    const unsigned total = (unsigned)p.B * p.tiles_x * p.tiles_y;
    if ((size_t)p.todo_ints < (size_t)total + kTodoHdr) return gfn::fail(GFN_ERR_SCRATCH, "local_corr: scratch too small");
    return with_radius<7>(r, p.f16, [&](auto R, auto ft) { return launch_tiled<decltype(R)::value, decltype(ft)>(route, p, total, s); });
}

GFN_EXPORT int gfn_local_corr_fwd(const float *f0, int64_t f0_bs, const float *f1, const float *f1_second,
                                  const float *flow, float *out, int64_t out_bs, int B, int C, int G, int H, int W, int r,
                                  int grid_based, int win_h, int win_w, void *scratch, int64_t scratch_bytes,
                                  gfn_stream_t stream) {
    return gfn_local_corr_fwd_ex(f0, f0_bs, f1, f1_second, flow, out, out_bs, B, C, G, H, W, r, grid_based, win_h, win_w, 0,
                                 scratch, scratch_bytes, stream);
}

// ---- refiner input + plan in one launch ----------------------------------------------------------------------------------
GFN_EXPORT int gfn_local_corr_plans(int C, int H, int W, int G, int r, int f1_dtype) {
    return lean_shape(C, H, W, G, r, f1_dtype == GFN_F16) ? 1 : 0;
}

namespace {
template <int R, typename FT>
int launch_ri_plan(const gfn_ri::RiArgs &q, const LcParams &p, hipStream_t s, bool keep) {
    const unsigned q_blocks = (unsigned)(((long)q.G * q.G + 255) / 256);
    const unsigned tiles = (unsigned)(p.tiles_x * p.tiles_y);
    const unsigned p_blocks = (tiles + 4 * kPlanPerWave - 1) / (4 * kPlanPerWave);
    const int banded = gfn_ri::ri_bands(q.B, q.Bh, q_blocks) ? 1 : 0;  // symmetric batches: XCD-banded order of the refiner-input blocks
    const dim3 grid = banded ? dim3(gfn_ri::ri_banded_blocks(q.B, q_blocks) + p_blocks * (unsigned)q.B) : dim3(q_blocks + p_blocks, (unsigned)q.B);
    if (keep) hipLaunchKernelGGL((refiner_input_plan_kernel<R, FT, true>), grid, dim3(256), 0, s, q, p, q_blocks, p_blocks, banded);
    else hipLaunchKernelGGL((refiner_input_plan_kernel<R, FT, false>), grid, dim3(256), 0, s, q, p, q_blocks, p_blocks, banded);
    return gfn::check_launch("refiner_input_plan_kernel");
}
}  // namespace

GFN_EXPORT int gfn_refiner_input_plan_fwd_dt(const void *f0, const void *f1, int dtype, const float *flow, const float *disp_w,
                                             const float *disp_b, float *d, int64_t d_bs, int B, int C, int Hs, int Ws, int G, int disp_dim,
                                             float disp_scale, int symmetric, int r, void *scratch, int64_t scratch_bytes,
                                             gfn_stream_t stream) {
    gfn_ri::RiArgs q;
    bool keep;
    if (int e = gfn_ri::ri_args("refiner_input_plan", f0, f1, dtype, flow, disp_w, disp_b, d, d_bs, B, C, Hs, Ws, G, disp_dim, disp_scale, symmetric, q, keep))
        return e;
    if (!lean_shape(C, Hs, Ws, G, r, dtype == GFN_F16))
        return gfn::fail(GFN_ERR_INVALID_ARG, "refiner_input_plan: the local correlation of this shape takes no plan (ask gfn_local_corr_plans first)");
    if (!scratch || scratch_bytes < gfn_local_corr_scratch_bytes(B, G) || ((uintptr_t)scratch & 3))
        return gfn::fail(GFN_ERR_SCRATCH, "refiner_input_plan: scratch too small");
    if (B == 0) return GFN_OK;
    LcParams p = lc_params(nullptr, nullptr, dtype == GFN_F16, flow, B, C, G, Hs, Ws, r, 0, Hs, Ws);
    tiled_window(p);
    p.todo = reinterpret_cast<int *>(scratch);
    p.plan = lean_plan_ptr(scratch, B, G);
    return with_radius<4>(r, p.f16, [&](auto R, auto ft) { return launch_ri_plan<decltype(R)::value, decltype(ft)>(q, p, (hipStream_t)stream, keep); });  // lean_shape: r <= 4
}

GFN_EXPORT int gfn_local_corr_bwd_f0(const float *grad_out, int64_t grad_out_bs, const float *f1, const float *f1_second,
                                    const float *flow, float *grad_f0, int64_t grad_f0_bs, int B, int C, int G, int H, int W, int r,
                                    int grid_based, int win_h, int win_w, gfn_stream_t stream) {
    return gfn_local_corr_mode_bwd_f0(grad_out, grad_out_bs, f1, f1_second, flow, grad_f0, grad_f0_bs, B, C, G, H, W, r, grid_based, win_h, win_w,
                                      GFN_SAMPLE_BILINEAR, GFN_PAD_ZEROS, stream);
}

namespace {
__global__ __launch_bounds__(256) void avg_pool2_kernel(const float *in, float *out, int BC, int H, int W) {
    const int Ho = H / 2, Wo = W / 2;
    const long total = (long)BC * Ho * Wo;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int x = (int)(idx % Wo);
        const long t = idx / Wo;
        const int y = (int)(t % Ho);
        const long pl = t / Ho;
        const float *s = in + (pl * H + 2 * y) * W + 2 * x;
        out[idx] = (s[0] + s[1] + s[W] + s[W + 1]) / 4.f;
    }
}
}  // namespace

GFN_EXPORT int gfn_avg_pool2(const float *in, float *out, int BC, int H, int W, gfn_stream_t stream) {
    if (!in || !out || BC < 0 || H < 2 || W < 2) return gfn::fail(GFN_ERR_INVALID_ARG, "avg_pool2: bad argument");
    const long total = (long)BC * (H / 2) * (W / 2);
    if (total == 0) return GFN_OK;
    const unsigned grid = (unsigned)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
    hipLaunchKernelGGL(avg_pool2_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, in, out, BC, H, W);
    return gfn::check_launch("avg_pool2_kernel");
}
