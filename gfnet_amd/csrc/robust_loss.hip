// The training objective on the homography ground truth: losses/robust_loss.py of the reference (get_gt_warp_homography :9-42,
// RobustLosses.regression_loss :65-90, RobustLosses.forward :92-128), one scale per call, all of that scale's iterations at once.
//
// Everything the loss reads is a pure function of the cell index, the 3x3 homography and the maps the model produced, so one pass
// does it: a thread takes VEC consecutive cells of one row (VEC = 4 / 2 / 1: the widest that divides w and the pointers' alignment,
// so no group straddles a row and none needs a tail), computes the ground-truth warp x2_n and the mask in registers (never stored),
// then for every iteration k reads flow_k (two planes) and cert_k once and accumulates
//     ce  += w_k * bce_with_logits(cert_k, prob)                      over every cell
//     rho += w_k * cs^a * ((epe_k / cs)^2 + 1)^(a/2)                  over masked cells
//     cnt += prob,   pck += [epe_last < pck_thr]                       over masked cells
// The four sums are reduced per wave (shuffles), per block (LDS, waves added in order) and written as one partial per block and
// quantity; rl_finish_kernel, a single workgroup, adds the partials in a fixed order in double and writes `stats`.  No floating-point
// atomics anywhere: identical calls give identical bits.  The backward recomputes x2_n, the mask and epe_k from the same inputs with the
// same expressions and writes the gradient maps, scaled by a grad_output that it reads from device memory.
#include <cmath>

#include "common.h"
#include "reduce.h"

namespace {

using gfn::wave_sum_lane0;

constexpr int kMaxItr = GFN_RL_MAX_ITR;
constexpr int kThreads = 256;
constexpr int kQuant = 4;          // ce, rho, count, pck
constexpr int kMaxSide = 32768;    // (2 * i + 1) * side of the nearest-exact index stays inside 32 bits
constexpr int64_t kMaxCells = (int64_t)1 << 30;

struct ItrMaps {
    const float *flow[kMaxItr];
    const float *cert[kMaxItr];
    float wk[kMaxItr];             // iteration_base ** (n_itr - k)
};

struct ItrGrads {
    float *gflow[kMaxItr];
    float *gcert[kMaxItr];
};

// what the ground-truth warp of a cell needs
struct Warp {
    const float *Hm;               // (B,3,3)
    const float *coords;           // (B,2,h,w) or null: the cell centres
    int h, w;
    float ext_a, ext_b;            // im_A.shape[2] - 1, im_B.shape[2] - 1 (the reference uses the height for both axes)
    float xs, xe, xstep, ys, ye, ystep;   // torch.linspace(-1 + 1/n, 1 - 1/n, n) of both axes
    const float *prev;             // (B,ph,pw) the previous scale's last end-point error, or null
    int ph, pw;
    float prev_thr;
};

template <int VEC>
__device__ __forceinline__ void loadv(const float *p, float (&v)[VEC]) {
    if constexpr (VEC == 4) {
        const float4 t = *reinterpret_cast<const float4 *>(p);
        v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
    } else if constexpr (VEC == 2) {
        const float2 t = *reinterpret_cast<const float2 *>(p);
        v[0] = t.x, v[1] = t.y;
    } else {
        v[0] = *p;
    }
}

template <int VEC>
__device__ __forceinline__ void storev(float *p, const float (&v)[VEC]) {
    if constexpr (VEC == 4) {
        *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else if constexpr (VEC == 2) {
        *reinterpret_cast<float2 *>(p) = make_float2(v[0], v[1]);
    } else {
        *p = v[0];
    }
}

// robust_loss.py:11-33 for one cell, fp32 in the reference's order: centre (or im_A_coords) -> pixel of A -> H -> dehomogenise
// (kornia's transform_points: by z, by 1 where |z| <= 1e-8) -> normalised in B.  (px, py) is x2, (nx, ny) x2_n.
__device__ __forceinline__ void gt_cell(const Warp &g, const float *Hb, size_t coord_off, size_t plane, int y, int x, float &cx, float &cy,
                                        float &px, float &py, float &nx, float &ny) {
    if (g.coords) {
        cx = g.coords[coord_off];
        cy = g.coords[coord_off + plane];
    } else {
        cx = gfn::linspace_step_at(g.xs, g.xe, g.xstep, g.w, x);
        cy = gfn::linspace_step_at(g.ys, g.ye, g.ystep, g.h, y);
    }
    const float ax = (cx + 1.0f) * g.ext_a * 0.5f, ay = (cy + 1.0f) * g.ext_a * 0.5f;
    const float X = Hb[0] * ax + Hb[1] * ay + Hb[2];
    const float Y = Hb[3] * ax + Hb[4] * ay + Hb[5];
    const float Z = Hb[6] * ax + Hb[7] * ay + Hb[8];
    const float zd = fabsf(Z) > 1e-8f ? Z : 1.0f;
    px = X / zd;
    py = Y / zd;
    nx = px / g.ext_b * 2.0f - 1.0f;
    ny = py / g.ext_b * 2.0f - 1.0f;
}

// the certainty target and regression mask of a cell (:31, :117-120): inside (-1, 1) on both axes, and the previous scale's error,
// read at the nearest-exact source cell min(floor((i + 0.5) * in / out), in - 1), below its threshold
__device__ __forceinline__ bool cell_mask(const Warp &g, int b, int y, int x, float nx, float ny) {
    bool m = nx < 1.0f && nx > -1.0f && ny < 1.0f && ny > -1.0f;
    if (g.prev) {
        const unsigned sy = min((unsigned)(2 * y + 1) * (unsigned)g.ph / (2u * (unsigned)g.h), (unsigned)g.ph - 1u);
        const unsigned sx = min((unsigned)(2 * x + 1) * (unsigned)g.pw / (2u * (unsigned)g.w), (unsigned)g.pw - 1u);
        m = m && g.prev[((size_t)b * g.ph + sy) * g.pw + sx] < g.prev_thr;
    }
    return m;
}

// group index -> (b, y, first x) and the cell / flow offsets; VEC cells of one row
template <int VEC>
__device__ __forceinline__ void group_cell(unsigned gi, int h, int w, int &b, int &y, int &x0, size_t &cell, size_t &fo) {
    const unsigned gpr = (unsigned)w / VEC;
    const unsigned row = gi / gpr;
    x0 = (int)(gi - row * gpr) * VEC;
    b = (int)(row / (unsigned)h);
    y = (int)(row - (unsigned)b * (unsigned)h);
    cell = ((size_t)b * h + y) * w + x0;
    fo = ((size_t)b * 2 * h + y) * w + x0;
}

template <int VEC>
__global__ __launch_bounds__(kThreads) void rl_fwd_kernel(ItrMaps it, Warp g, float *__restrict__ epe_last, float *__restrict__ part,
                                                          int n_itr, unsigned groups, float a_half, float cs, float cs_pow_a, float pck_thr) {
    __shared__ float red[kThreads / 64][kQuant];
    const unsigned gi = blockIdx.x * kThreads + threadIdx.x;
    float s_ce = 0.0f, s_rho = 0.0f, s_cnt = 0.0f, s_pck = 0.0f;
    if (gi < groups) {
        int b, y, x0;
        size_t cell, fo;
        group_cell<VEC>(gi, g.h, g.w, b, y, x0, cell, fo);
        const size_t plane = (size_t)g.h * g.w;
        const float *Hb = g.Hm + (size_t)b * 9;
        float nx[VEC], ny[VEC], t[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            float cx, cy, px, py;
            gt_cell(g, Hb, fo + v, plane, y, x0 + v, cx, cy, px, py, nx[v], ny[v]);
            t[v] = cell_mask(g, b, y, x0 + v, nx[v], ny[v]) ? 1.0f : 0.0f;
            s_cnt += t[v];
        }
        for (int k = 0; k < n_itr; ++k) {
            float fx[VEC], fy[VEC], cz[VEC], epe[VEC];
            loadv<VEC>(it.flow[k] + fo, fx);
            loadv<VEC>(it.flow[k] + fo + plane, fy);
            loadv<VEC>(it.cert[k] + cell, cz);
            const float wk = it.wk[k];
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                const float dx = fx[v] - nx[v], dy = fy[v] - ny[v];
                epe[v] = sqrtf(dx * dx + dy * dy);
                const float z = cz[v];
                s_ce += wk * (fmaxf(z, 0.0f) - z * t[v] + log1pf(expf(-fabsf(z))));
                if (t[v] != 0.0f) {
                    const float q = epe[v] / cs;
                    s_rho += wk * (cs_pow_a * powf(q * q + 1.0f, a_half));
                }
            }
            if (k == n_itr - 1) {
#pragma unroll
                for (int v = 0; v < VEC; ++v)
                    if (t[v] != 0.0f && epe[v] < pck_thr) s_pck += 1.0f;
                if (epe_last) storev<VEC>(epe_last + cell, epe);
            }
        }
    }
    float q[kQuant] = {wave_sum_lane0(s_ce), wave_sum_lane0(s_rho), wave_sum_lane0(s_cnt), wave_sum_lane0(s_pck)};
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < kQuant; ++i) red[wave][i] = q[i];
    }
    __syncthreads();
    if (threadIdx.x < kQuant) {
        float s = red[0][threadIdx.x];
#pragma unroll
        for (int wv = 1; wv < kThreads / 64; ++wv) s += red[wv][threadIdx.x];
        part[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = s;
    }
}

// second stage: one workgroup adds the nparts partials of each quantity in a fixed order (thread t takes t, t + 256, ...; then a
// tree over the threads), all in double, and writes the scale's statistics
__global__ __launch_bounds__(kThreads) void rl_finish_kernel(const float *__restrict__ part, unsigned nparts, double cells, double ce_weight,
                                                             float *__restrict__ stats) {
    __shared__ double red[kQuant][kThreads];
    double s[kQuant] = {0.0, 0.0, 0.0, 0.0};
    for (unsigned i = threadIdx.x; i < nparts; i += kThreads) {
#pragma unroll
        for (int qn = 0; qn < kQuant; ++qn) s[qn] += (double)part[(size_t)qn * nparts + i];
    }
#pragma unroll
    for (int qn = 0; qn < kQuant; ++qn) red[qn][threadIdx.x] = s[qn];
    __syncthreads();
    for (int half = kThreads / 2; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half) {
#pragma unroll
            for (int qn = 0; qn < kQuant; ++qn) red[qn][threadIdx.x] += red[qn][threadIdx.x + half];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double ce = red[0][0] / cells, rho = red[1][0], cnt = red[2][0], pck = red[3][0];
        // an empty mask: the reference's `ce_loss * 0.0` escape (:83-84); its pck_05 would be the mean of nothing
        const double reg = cnt > 0.0 ? rho / cnt : 0.0;
        stats[GFN_RL_STAT_LOSS] = (float)(ce_weight * ce + reg);
        stats[GFN_RL_STAT_CE] = (float)ce;
        stats[GFN_RL_STAT_REG] = (float)reg;
        stats[GFN_RL_STAT_COUNT] = (float)cnt;
        stats[GFN_RL_STAT_PCK] = (float)(cnt > 0.0 ? pck / cnt : 0.0);
        stats[GFN_RL_STAT_CELLS] = (float)cells;
        stats[GFN_RL_STAT_RHO_SUM] = (float)rho;
        stats[7] = 0.0f;
    }
}

template <int VEC>
__global__ __launch_bounds__(kThreads) void rl_bwd_kernel(ItrMaps it, ItrGrads gr, Warp g, const float *__restrict__ stats,
                                                          const float *__restrict__ grad_out, int n_itr, unsigned need, unsigned groups,
                                                          float a_half_m1, float cs, float reg_coef, float ce_coef) {
    const unsigned gi = blockIdx.x * kThreads + threadIdx.x;
    if (gi >= groups) return;
    int b, y, x0;
    size_t cell, fo;
    group_cell<VEC>(gi, g.h, g.w, b, y, x0, cell, fo);
    const size_t plane = (size_t)g.h * g.w;
    const float *Hb = g.Hm + (size_t)b * 9;
    const float go = *grad_out, cnt = stats[GFN_RL_STAT_COUNT];
    // reg_coef = a * cs^(a-2), ce_coef = ce_weight / (B*h*w); no masked cell, no regression gradient (:83-84)
    const float freg = cnt > 0.0f ? go * reg_coef / cnt : 0.0f, fce = go * ce_coef;
    float nx[VEC], ny[VEC], t[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
        float cx, cy, px, py;
        gt_cell(g, Hb, fo + v, plane, y, x0 + v, cx, cy, px, py, nx[v], ny[v]);
        t[v] = cell_mask(g, b, y, x0 + v, nx[v], ny[v]) ? 1.0f : 0.0f;
    }
    for (int k = 0; k < n_itr; ++k) {
        const float wk = it.wk[k];
        if (need & (1u << k)) {
            float fx[VEC], fy[VEC], gx[VEC], gy[VEC];
            loadv<VEC>(it.flow[k] + fo, fx);
            loadv<VEC>(it.flow[k] + fo + plane, fy);
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                const float dx = fx[v] - nx[v], dy = fy[v] - ny[v];
                const float q = sqrtf(dx * dx + dy * dy) / cs;
                // the norm's 1/epe cancels against rho's epe: nothing divides by epe, and epe == 0 gives 0
                const float coef = t[v] != 0.0f ? freg * wk * powf(q * q + 1.0f, a_half_m1) : 0.0f;
                gx[v] = coef * dx;
                gy[v] = coef * dy;
            }
            storev<VEC>(gr.gflow[k] + fo, gx);
            storev<VEC>(gr.gflow[k] + fo + plane, gy);
        }
        if (need & (1u << (kMaxItr + k))) {
            float cz[VEC], gc[VEC];
            loadv<VEC>(it.cert[k] + cell, cz);
#pragma unroll
            for (int v = 0; v < VEC; ++v) gc[v] = fce * wk * (1.0f / (1.0f + expf(-cz[v])) - t[v]);
            storev<VEC>(gr.gcert[k] + cell, gc);
        }
    }
}

__global__ __launch_bounds__(kThreads) void gt_warp_kernel(Warp g, float *__restrict__ out, float *__restrict__ prob,
                                                           float *__restrict__ x1n, unsigned cells, int normalized) {
    const unsigned gi = blockIdx.x * kThreads + threadIdx.x;
    if (gi >= cells) return;
    int b, y, x;
    size_t cell, fo;
    group_cell<1>(gi, g.h, g.w, b, y, x, cell, fo);
    float cx, cy, px, py, nx, ny;
    gt_cell(g, g.Hm + (size_t)b * 9, fo, (size_t)g.h * g.w, y, x, cx, cy, px, py, nx, ny);
    out[cell * 2] = normalized ? nx : px;
    out[cell * 2 + 1] = normalized ? ny : py;
    prob[cell] = cell_mask(g, b, y, x, nx, ny) ? 1.0f : 0.0f;
    if (x1n) {
        x1n[cell * 2] = cx;
        x1n[cell * 2 + 1] = cy;
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
bool aligned_to(const void *p, unsigned bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1u)) == 0; }

int check_grid(const char *what, int B, int h, int w) {
    if (B < 0 || h <= 0 || w <= 0) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: bad size (B=%d h=%d w=%d)", what, B, h, w);
    if (h > kMaxSide || w > kMaxSide) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: a grid side above %d", what, kMaxSide);
    if ((int64_t)B * h * w > kMaxCells) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: more than 2^30 cells (B*h*w)", what);
    return GFN_OK;
}

int check_extents(const char *what, double ext_a, double ext_b) {
    if (!(ext_a >= 0.0) || !(ext_b > 0.0))
        return gfn::fail(GFN_ERR_INVALID_ARG, "%s: image extents must be ext_a >= 0 and ext_b > 0 (heights of at least 1 and 2 pixels)", what);
    return GFN_OK;
}

// torch.linspace(-1 + 1/n, 1 - 1/n, n): the ends rounded to fp32 from the double expression, the step an fp32 division
void axis(int n, float &s, float &e, float &step) {
    s = (float)(-1.0 + 1.0 / n);
    e = (float)(1.0 - 1.0 / n);
    step = n > 1 ? (e - s) / (float)(n - 1) : 0.0f;
}

Warp make_warp(const float *Hm, const float *coords, int h, int w, double ext_a, double ext_b, const float *prev, int ph, int pw, double prev_thr) {
    Warp g;
    g.Hm = Hm, g.coords = coords, g.h = h, g.w = w, g.ext_a = (float)ext_a, g.ext_b = (float)ext_b;
    axis(w, g.xs, g.xe, g.xstep);
    axis(h, g.ys, g.ye, g.ystep);
    g.prev = prev, g.ph = ph, g.pw = pw, g.prev_thr = (float)prev_thr;
    return g;
}

// what the forward and the backward of a scale share; fills the per-iteration maps and weights
int check_scale(const char *what, const float *const *flows, const float *const *certs, int n_itr, const float *Hm, const float *prev_epe,
                int ph, int pw, const float *stats, int B, int h, int w, double ext_a, double ext_b, double cs, double iteration_base, ItrMaps &it) {
    if (!flows || !certs || !Hm || !stats) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: null pointer", what);
    if (n_itr < 1 || n_itr > kMaxItr) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: n_itr = %d outside 1..%d", what, n_itr, kMaxItr);
    for (int k = 0; k < kMaxItr; ++k) {
        it.flow[k] = k < n_itr ? flows[k] : nullptr;
        it.cert[k] = k < n_itr ? certs[k] : nullptr;
        it.wk[k] = k < n_itr ? (float)std::pow(iteration_base, (double)(n_itr - 1 - k)) : 0.0f;
        if (k < n_itr && (!it.flow[k] || !it.cert[k])) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: null flow or certainty of iteration %d", what, k + 1);
    }
    if (int rc = check_grid(what, B, h, w)) return rc;
    if (int rc = check_extents(what, ext_a, ext_b)) return rc;
    if (!(cs > 0.0) || !std::isfinite(cs)) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: cs = c * scale must be positive", what);
    if (prev_epe && (ph <= 0 || pw <= 0 || ph > kMaxSide || pw > kMaxSide))
        return gfn::fail(GFN_ERR_INVALID_ARG, "%s: prev_epe on a %d x %d grid (sides 1..%d)", what, ph, pw, kMaxSide);
    return GFN_OK;
}

// the widest vector every map of the call allows
int vec_width(int w, const ItrMaps &it, const ItrGrads *gr, const float *extra, int n_itr) {
    int vec = (w % 4 == 0) ? 4 : (w % 2 == 0) ? 2 : 1;
    auto fit = [&](const void *p) {
        while (vec > 1 && p && !aligned_to(p, 4u * vec)) vec >>= 1;
    };
    for (int k = 0; k < n_itr; ++k) {
        fit(it.flow[k]), fit(it.cert[k]);
        if (gr) fit(gr->gflow[k]), fit(gr->gcert[k]);
    }
    fit(extra);
    return vec;
}

int64_t ws_bytes_for(int B, int h, int w) {
    const int64_t blocks = ((int64_t)B * h * w + kThreads - 1) / kThreads;   // the scalar form: the most blocks any form launches
    return (blocks * kQuant * (int64_t)sizeof(float) + 15) / 16 * 16;
}

}  // namespace

GFN_EXPORT int64_t gfn_robust_loss_ws_bytes(int B, int h, int w, int n_itr) {
    if (B <= 0 || h <= 0 || w <= 0 || n_itr <= 0) return 0;
    return ws_bytes_for(B, h, w);
}

GFN_EXPORT int gfn_robust_loss_fwd(const float *const *flows, const float *const *certs, int n_itr, const float *Hm, const float *im_A_coords,
                                   const float *prev_epe, int ph, int pw, double prev_thresh, float *epe_last, float *stats, int B, int h, int w,
                                   double ext_a, double ext_b, double a, double cs, double ce_weight, double iteration_base, double pck_thresh,
                                   void *ws, int64_t ws_bytes, gfn_stream_t stream) {
    const char *what = "robust_loss_fwd";
    ItrMaps it;
    if (int rc = check_scale(what, flows, certs, n_itr, Hm, prev_epe, ph, pw, stats, B, h, w, ext_a, ext_b, cs, iteration_base, it)) return rc;
    if (B == 0) return GFN_OK;
    if (!ws || !aligned_to(ws, 16) || ws_bytes < ws_bytes_for(B, h, w))
        return gfn::fail(GFN_ERR_INVALID_ARG, "%s: workspace missing, not 16-byte aligned or too small (%lld bytes needed)", what,
                         (long long)ws_bytes_for(B, h, w));
    const Warp g = make_warp(Hm, im_A_coords, h, w, ext_a, ext_b, prev_epe, ph, pw, prev_thresh);
    const int vec = vec_width(w, it, nullptr, epe_last, n_itr);
    const unsigned groups = (unsigned)((int64_t)B * h * w / vec), blocks = (groups + kThreads - 1) / kThreads;
    float *part = static_cast<float *>(ws);
    const float a_half = (float)(a * 0.5), csf = (float)cs, cs_pow_a = (float)std::pow(cs, a), pck = (float)pck_thresh;
    hipStream_t s = (hipStream_t)stream;
#define GFN_RL(V) hipLaunchKernelGGL((rl_fwd_kernel<V>), dim3(blocks), dim3(kThreads), 0, s, it, g, epe_last, part, n_itr, groups, a_half, csf, cs_pow_a, pck)
    switch (vec) {
        case 4: GFN_RL(4); break;
        case 2: GFN_RL(2); break;
        default: GFN_RL(1); break;
    }
#undef GFN_RL
    if (int rc = gfn::check_launch("rl_fwd_kernel")) return rc;
    hipLaunchKernelGGL(rl_finish_kernel, dim3(1), dim3(kThreads), 0, s, (const float *)part, blocks, (double)B * h * w, ce_weight, stats);
    return gfn::check_launch("rl_finish_kernel");
}

GFN_EXPORT int gfn_robust_loss_bwd(const float *const *flows, const float *const *certs, int n_itr, const float *Hm, const float *im_A_coords,
                                   const float *prev_epe, int ph, int pw, double prev_thresh, const float *stats, const float *grad_out,
                                   float *const *g_flows, float *const *g_certs, int need, int B, int h, int w, double ext_a, double ext_b,
                                   double a, double cs, double ce_weight, double iteration_base, gfn_stream_t stream) {
    const char *what = "robust_loss_bwd";
    ItrMaps it;
    if (int rc = check_scale(what, flows, certs, n_itr, Hm, prev_epe, ph, pw, stats, B, h, w, ext_a, ext_b, cs, iteration_base, it)) return rc;
    if (!grad_out) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: null pointer", what);
    const int all = ((1 << n_itr) - 1) * ((1 << kMaxItr) + 1);
    if (need < 0 || (need & ~all)) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: need mask 0x%x names an iteration past n_itr = %d", what, need, n_itr);
    ItrGrads gr;
    for (int k = 0; k < kMaxItr; ++k) {
        const bool nf = need & (1 << k), nc = need & (1 << (kMaxItr + k));
        gr.gflow[k] = nf && g_flows ? g_flows[k] : nullptr;
        gr.gcert[k] = nc && g_certs ? g_certs[k] : nullptr;
        if ((nf && !gr.gflow[k]) || (nc && !gr.gcert[k]))
            return gfn::fail(GFN_ERR_INVALID_ARG, "%s: the need mask asks for a gradient whose pointer is null", what);
    }
    if (B == 0 || need == 0) return GFN_OK;
    const Warp g = make_warp(Hm, im_A_coords, h, w, ext_a, ext_b, prev_epe, ph, pw, prev_thresh);
    const int vec = vec_width(w, it, &gr, nullptr, n_itr);
    const unsigned groups = (unsigned)((int64_t)B * h * w / vec), blocks = (groups + kThreads - 1) / kThreads;
    const float a_half_m1 = (float)(a * 0.5 - 1.0), csf = (float)cs, reg_coef = (float)(a * std::pow(cs, a - 2.0)),
                ce_coef = (float)(ce_weight / ((double)B * h * w));
    hipStream_t s = (hipStream_t)stream;
#define GFN_RL(V) \
    hipLaunchKernelGGL((rl_bwd_kernel<V>), dim3(blocks), dim3(kThreads), 0, s, it, gr, g, stats, grad_out, n_itr, (unsigned)need, groups, a_half_m1, csf, reg_coef, ce_coef)
    switch (vec) {
        case 4: GFN_RL(4); break;
        case 2: GFN_RL(2); break;
        default: GFN_RL(1); break;
    }
#undef GFN_RL
    return gfn::check_launch("rl_bwd_kernel");
}

GFN_EXPORT int gfn_gt_warp_homography_fwd(const float *Hm, const float *im_A_coords, float *out, float *prob, float *x1_n, int B, int h, int w,
                                          double ext_a, double ext_b, int normalized, gfn_stream_t stream) {
    const char *what = "gt_warp_homography_fwd";
    if (!Hm || !out || !prob) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: null pointer", what);
    if (int rc = check_grid(what, B, h, w)) return rc;
    if (int rc = check_extents(what, ext_a, ext_b)) return rc;
    if (B == 0) return GFN_OK;
    const Warp g = make_warp(Hm, im_A_coords, h, w, ext_a, ext_b, nullptr, 0, 0, 0.0);
    const unsigned cells = (unsigned)((int64_t)B * h * w);
    hipLaunchKernelGGL(gt_warp_kernel, dim3((cells + kThreads - 1) / kThreads), dim3(kThreads), 0, (hipStream_t)stream, g, out, prob, x1_n, cells,
                       normalized);
    return gfn::check_launch("gt_warp_kernel");
}
