// corr_softargmax_bwd.hip -- backward of the fused global correlation + soft-argmax (corr_softargmax.hip) for gfx950.
//
// The reference differentiates pos_embed(corr_volume(f0, f1)) (model/network.py:251-252, 415-440) through torch autograd, which
// keeps the volume and writes its gradient: 4 MiB each per direction at 32^2 x 32^2, 21 MiB at 48^2 x 48^2.  Per direction, with
// A-positions i, B-positions j, gamma_j the B-grid cell centre and G_i = dL/dflow_i:
//   s_ji = sum_c f0[c,i] f1[c,j] / sqrt(C),  P_ji = softmax_j(s_ji),  flow_i = sum_j P_ji gamma_j,  D_i = G_i . flow_i
//   dS_ji = P_ji (G_i . gamma_j - D_i),  dF0[c,i] = sum_j dS_ji f1[c,j] / sqrt(C),  dF1[c,j] = sum_i dS_ji f0[c,i] / sqrt(C)
// Two passes in the FlashAttention-2 manner, neither writes the volume and neither uses atomics (deterministic):
//   bwd_f0_kernel  one wave per 32 A-positions streams every B-position: online max / sum and the unnormalised
//                  sum_j e_ji (G_i . gamma_j - D_i) f1[:,j]  ->  dF0, and the row statistics (m_i, 1/(l_i sqrt C), G_i, D_i) into ws;
//   bwd_f1_kernel  one wave per 32 B-positions streams every A-position: recomputes s_ji, takes P_ji from the statistics, dF1.
// Every product is on the exact-fp32 matrix core (v_mfma_f32_32x32x2_f32: fp32 fmaf chains).  The correlation tile S is the forward's
// (corr_tile, acc_row, cell_centre and dir_image of corr_common.h: rows = streamed positions, columns = the wave's own); its weights W, still in the accumulator layout,
// are the B operand of the second product out[c][p] += sum_q Y[c][q] W[q][p] as they stand: lane (col, h) supplies W[q(r, h)][col]
// = acc[r] for k-step r, q(r, h) = (r & 3) + 8 (r >> 2) + 4 h.  Its A operand Y[c][q(r, h)] has the channel on the lane, the
// transpose of the coalesced tile load: the tile goes through LDS (one wave per workgroup, row stride 33: conflict-free both ways).
#include "corr_common.h"

namespace {

using namespace gfn;

constexpr int LDS_STRIDE = 33;

// out[cb][c][p] += sum_q Y[c][q] W[q][p] with Y staged in lds ([c][q], row stride LDS_STRIDE) and w[r] = W[q(r, h)][col]
template <int NCB>
__device__ __forceinline__ void weighted_sum(f32x16 (&out)[NCB], const float *lds, const float (&w)[16], int col, int h) {
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r)
            out[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(lds[(32 * cb + col) * LDS_STRIDE + acc_row(r, h)], w[r], out[cb], 0, 0, 0);
}

// KS = k-steps of 2 channels held in registers (as the forward); NCB = 32-channel blocks of the output; PF = prefetch the next tile
// (not at KS = 64: the second operand copy would push the allocation past the register file)
template <int KS, typename FT>
__global__ __launch_bounds__(64) void bwd_f0_kernel(const FT *__restrict__ f0, const FT *__restrict__ f1, const float *__restrict__ flow,
                                                    const float *__restrict__ gflow, float *__restrict__ g0, float *__restrict__ g1,
                                                    float4 *__restrict__ rec, float *__restrict__ dvec, int B, int Bh, int C, int H0,
                                                    int W0, int H1, int W1, float sqrt_c) {
    constexpr int NCB = (2 * KS + 31) / 32;
    constexpr bool PF = KS <= 32;
    __shared__ float lds[NCB * 32 * LDS_STRIDE];
    const int N0 = H0 * W0, N1 = H1 * W1;
    const int lane = threadIdx.x;
    const int itiles = (N0 + 31) >> 5;
    const int b = blockIdx.x / itiles, i0 = (blockIdx.x - b * itiles) << 5;
    const int col = lane & 31, h = lane >> 5;
    const int i = i0 + col, ic = min(i, N0 - 1);
    // symmetric batches are virtual (Bh = B/2): direction b >= Bh swaps the two arrays, and its dF0 is the gradient of f1[b - Bh]
    const FT *f0b = dir_image(f0, f1, b, Bh, (size_t)C * N0);
    const FT *f1b = dir_image(f1, f0, b, Bh, (size_t)C * N1);
    float *gout = (b < Bh ? g0 : g1) ? dir_image(g0, g1, b, Bh, (size_t)C * N0) : nullptr;
    const bool want = gout != nullptr;  // workgroup-uniform; without it only the statistics are made

    float xop[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        const int c = 2 * s + h;
        const float v = (float)f0b[(size_t)min(c, C - 1) * N0 + ic];
        xop[s] = c < C ? v : 0.f;
    }
    const float Gx = gflow[((size_t)b * 2 + 0) * N0 + ic], Gy = gflow[((size_t)b * 2 + 1) * N0 + ic];
    const float D = Gx * flow[((size_t)b * 2 + 0) * N0 + ic] + Gy * flow[((size_t)b * 2 + 1) * N0 + ic];
    const float inv_w1 = 1.0f / (float)W1;
    const float e_scale = 1.4426950408889634f / sqrt_c;  // exp(v / sqrt(C)) = exp2(v * log2(e) / sqrt(C))

    auto load_tile = [&](float (&a)[KS], int j0) {
        const int jl = min(j0 + col, N1 - 1);
#pragma unroll
        for (int s = 0; s < KS; ++s) a[s] = (float)f1b[(size_t)min(2 * s + h, C - 1) * N1 + jl];  // channels >= C meet a zero in xop
    };
    float m = -INFINITY, l = 0.f;
    f32x16 out[NCB];
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) out[cb] = f32x16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    float a_cur[KS], a_nxt[PF ? KS : 1];
    load_tile(a_cur, 0);
#pragma unroll
    for (int s = 0; s < KS; ++s) asm volatile("" : "+v"(a_cur[s]));  // land the first tile before the loop (see corr_softargmax.hip)
    for (int j0 = 0; j0 < N1; j0 += 32) {
        if constexpr (PF) {
            if (j0 + 32 < N1) load_tile(a_nxt, j0 + 32);
        }
        const f32x16 acc = corr_tile<KS>(a_cur, xop);
        if (want) {
#pragma unroll
            for (int s = 0; s < KS; ++s) lds[(2 * s + h) * LDS_STRIDE + col] = a_cur[s];
        }
        // the column's running maximum is shared by both half-waves (their rows j are summed by the same matrix product)
        float mt = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) mt = fmaxf(mt, j0 + acc_row(r, h) < N1 ? acc[r] : -INFINITY);
        mt = fmaxf(mt, other_half(mt));
        const float mn = fmaxf(m, mt);  // finite: row j0 of every tile is a position
        const float sc = __builtin_amdgcn_exp2f((m - mn) * e_scale);  // m = -inf on the first tile -> 0
        float w[16], lt = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int j = j0 + acc_row(r, h);
            const float e = j < N1 ? __builtin_amdgcn_exp2f((acc[r] - mn) * e_scale) : 0.f;
            float gx, gy;
            cell_centre(min(j, N1 - 1), H1, W1, inv_w1, gx, gy);
            lt += e;
            w[r] = e * (Gx * gx + Gy * gy - D);
        }
        l = fmaf(l, sc, lt);
        m = mn;
        if (want) {
            __syncthreads();  // the tile in lds (one wave per workgroup)
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb) out[cb] *= sc;
            weighted_sum<NCB>(out, lds, w, col, h);
            __syncthreads();  // before the next tile overwrites it
        }
        if constexpr (PF) {
#pragma unroll
            for (int s = 0; s < KS; ++s) a_cur[s] = a_nxt[s];
        } else if (j0 + 32 < N1) {
            load_tile(a_cur, j0 + 32);
        }
    }
    l += other_half(l);
    const float inv = 1.f / (l * sqrt_c);
    if (want && i < N0) {
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c = 32 * cb + acc_row(r, h);
                if (c < C) gout[(size_t)c * N0 + i] = out[cb][r] * inv;
            }
    }
    if (h == 0 && i < N0) {
        rec[(size_t)b * N0 + i] = make_float4(m, inv, Gx, Gy);
        dvec[(size_t)b * N0 + i] = D;
    }
}

// accumulate: symmetric batches, where bwd_f0_kernel has already written the other direction's share of the same image
template <int KS, typename FT>
__global__ __launch_bounds__(64) void bwd_f1_kernel(const FT *__restrict__ f0, const FT *__restrict__ f1, const float4 *__restrict__ rec,
                                                    const float *__restrict__ dvec, float *__restrict__ g0, float *__restrict__ g1, int B,
                                                    int Bh, int C, int H0, int W0, int H1, int W1, float sqrt_c) {
    constexpr int NCB = (2 * KS + 31) / 32;
    constexpr bool PF = KS <= 32;
    __shared__ float lds[NCB * 32 * LDS_STRIDE];
    const int N0 = H0 * W0, N1 = H1 * W1;
    const int lane = threadIdx.x;
    const int jtiles = (N1 + 31) >> 5;
    const int b = blockIdx.x / jtiles, j0 = (blockIdx.x - b * jtiles) << 5;
    const int col = lane & 31, h = lane >> 5;
    const int j = j0 + col, jc = min(j, N1 - 1);
    if (!(b < Bh ? g1 : g0)) return;  // whole workgroup
    float *gout = dir_image(g1, g0, b, Bh, (size_t)C * N1);
    const FT *f0b = dir_image(f0, f1, b, Bh, (size_t)C * N0);
    const FT *f1b = dir_image(f1, f0, b, Bh, (size_t)C * N1);

    float xop[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        const int c = 2 * s + h;
        const float v = (float)f1b[(size_t)min(c, C - 1) * N1 + jc];
        xop[s] = c < C ? v : 0.f;
    }
    float gx, gy;
    cell_centre(jc, H1, W1, 1.0f / (float)W1, gx, gy);
    const float e_scale = 1.4426950408889634f / sqrt_c;
    const float4 *recb = rec + (size_t)b * N0;
    const float *db = dvec + (size_t)b * N0;

    auto load_tile = [&](float (&a)[KS], int i0) {
        const int il = min(i0 + col, N0 - 1);
#pragma unroll
        for (int s = 0; s < KS; ++s) a[s] = (float)f0b[(size_t)min(2 * s + h, C - 1) * N0 + il];
    };
    f32x16 out[NCB];
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) out[cb] = f32x16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    float a_cur[KS], a_nxt[PF ? KS : 1];
    load_tile(a_cur, 0);
#pragma unroll
    for (int s = 0; s < KS; ++s) asm volatile("" : "+v"(a_cur[s]));  // land the first tile before the loop (see corr_softargmax.hip)
    for (int i0 = 0; i0 < N0; i0 += 32) {
        if constexpr (PF) {
            if (i0 + 32 < N0) load_tile(a_nxt, i0 + 32);
        }
        const f32x16 acc = corr_tile<KS>(a_cur, xop);  // acc[r] = s[j = j0 + col][i = i0 + q(r, h)] * sqrt(C)
#pragma unroll
        for (int s = 0; s < KS; ++s) lds[(2 * s + h) * LDS_STRIDE + col] = a_cur[s];
        float w[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = i0 + acc_row(r, h), il = min(i, N0 - 1);
            const float4 st = recb[il];  // (m_i, 1 / (l_i sqrt C), G_i)
            const float v = __builtin_amdgcn_exp2f((acc[r] - st.x) * e_scale) * st.y * (st.z * gx + st.w * gy - db[il]);
            w[r] = i < N0 ? v : 0.f;
        }
        __syncthreads();
        weighted_sum<NCB>(out, lds, w, col, h);
        __syncthreads();
        if constexpr (PF) {
#pragma unroll
            for (int s = 0; s < KS; ++s) a_cur[s] = a_nxt[s];
        } else if (i0 + 32 < N0) {
            load_tile(a_cur, i0 + 32);
        }
    }
    if (j < N1) {
        const bool accumulate = Bh != B;
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c = 32 * cb + acc_row(r, h);
                if (c < C) {
                    float *o = gout + (size_t)c * N1 + j;
                    *o = accumulate ? *o + out[cb][r] : out[cb][r];
                }
            }
    }
}

int64_t ws_bytes(int B, int H0, int W0) { return (int64_t)B * H0 * W0 * (int64_t)(sizeof(float4) + sizeof(float)); }

template <int KS, typename FT>
int launch(const FT *f0, const FT *f1, const float *flow, const float *gflow, float *g0, float *g1, int B, int Bh, int C, int H0, int W0,
           int H1, int W1, void *ws, hipStream_t stream) {
    const float sc = (float)sqrt((double)C);
    float4 *rec = static_cast<float4 *>(ws);
    float *dvec = reinterpret_cast<float *>(rec + (size_t)B * H0 * W0);
    const unsigned itiles = (unsigned)((H0 * W0 + 31) / 32), jtiles = (unsigned)((H1 * W1 + 31) / 32);
    hipLaunchKernelGGL((bwd_f0_kernel<KS, FT>), dim3((unsigned)B * itiles), dim3(64), 0, stream, f0, f1, flow, gflow, g0, g1, rec, dvec, B,
                       Bh, C, H0, W0, H1, W1, sc);
    if (int e = gfn::check_launch("corr_softargmax bwd_f0_kernel")) return e;
    if (!(Bh == B ? g1 != nullptr : (g0 || g1))) return GFN_OK;  // no B-side gradient is asked for
    hipLaunchKernelGGL((bwd_f1_kernel<KS, FT>), dim3((unsigned)B * jtiles), dim3(64), 0, stream, f0, f1, rec, dvec, g0, g1, B, Bh, C, H0,
                       W0, H1, W1, sc);
    return gfn::check_launch("corr_softargmax bwd_f1_kernel");
}

template <typename FT>
int dispatch(const void *f0, const void *f1, const float *flow, const float *gflow, float *g0, float *g1, int B, int Bh, int C, int H0,
             int W0, int H1, int W1, void *ws, hipStream_t stream) {
    const FT *a = static_cast<const FT *>(f0), *b = static_cast<const FT *>(f1);
    if (C <= 16) return launch<8, FT>(a, b, flow, gflow, g0, g1, B, Bh, C, H0, W0, H1, W1, ws, stream);
    if (C <= 32) return launch<16, FT>(a, b, flow, gflow, g0, g1, B, Bh, C, H0, W0, H1, W1, ws, stream);
    if (C <= 64) return launch<32, FT>(a, b, flow, gflow, g0, g1, B, Bh, C, H0, W0, H1, W1, ws, stream);
    return launch<64, FT>(a, b, flow, gflow, g0, g1, B, Bh, C, H0, W0, H1, W1, ws, stream);
}

}  // namespace

GFN_EXPORT int64_t gfn_corr_softargmax_bwd_ws_bytes(int B, int C, int H0, int W0, int H1, int W1) {
    (void)C; (void)H1; (void)W1;
    if (B <= 0 || H0 <= 0 || W0 <= 0) return 0;
    return ws_bytes(B, H0, W0);
}

GFN_EXPORT int gfn_corr_softargmax_bwd(const void *f0, const void *f1, int dtype, const float *flow, const float *grad_flow, float *grad_f0,
                                       float *grad_f1, int B, int C, int H0, int W0, int H1, int W1, int symmetric, void *ws,
                                       int64_t ws_bytes_, gfn_stream_t stream) {
    if (dtype != GFN_F32 && dtype != GFN_F16) return gfn::fail(GFN_ERR_INVALID_ARG, "corr_softargmax_bwd: feature dtype must be GFN_F32 or GFN_F16");
    if (!grad_flow) return gfn::fail(GFN_ERR_INVALID_ARG, "corr_softargmax_bwd: null grad_flow");
    if (int e = corr_check("corr_softargmax_bwd", f0, f1, flow, B, C, H0, W0, H1, W1, symmetric)) return e;
    if (B == 0 || (!grad_f0 && !grad_f1)) return GFN_OK;
    if (!ws || ws_bytes_ < ws_bytes(B, H0, W0) || ((uintptr_t)ws & 15))
        return gfn::fail(GFN_ERR_INVALID_ARG, "corr_softargmax_bwd: workspace missing, misaligned or smaller than gfn_corr_softargmax_bwd_ws_bytes");
    const int Bh = symmetric ? B / 2 : B;
    if (dtype == GFN_F16)
        return dispatch<_Float16>(f0, f1, flow, grad_flow, grad_f0, grad_f1, B, Bh, C, H0, W0, H1, W1, ws, (hipStream_t)stream);
    return dispatch<float>(f0, f1, flow, grad_flow, grad_f0, grad_f1, B, Bh, C, H0, W0, H1, W1, ws, (hipStream_t)stream);
}
