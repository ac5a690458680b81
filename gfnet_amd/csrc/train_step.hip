// What a training step does after backward(): trainer/train.py:29-43 of the reference (grad_scaler.unscale_, log_param_statistics :13-27,
// clip_grad_norm_, grad_scaler.step(AdamW), grad_scaler.update(), the scale floor :40-41, and the next step's zero_grad :30), as three
// launches over every parameter tensor at once and no host synchronisation.
//
// All of it is a streaming function of (p, g, exp_avg, exp_avg_sq) per element plus a handful of scalars.  The host hands over two device
// tables: one record per parameter tensor that has a gradient (gfn_ts_tensor) and one record per workgroup (gfn_ts_chunk: a run of at
// most GFN_TS_CHUNK elements of one tensor; a tensor's chunks are consecutive).
//   ts_norm_kernel    reads g and p: tests the raw g for inf / nan (as _amp_foreach_non_finite_check_and_unscale_ does before it
//                     multiplies), forms gu = g * inv_scale and accumulates gu^2 and p^2 in double per lane, so that no finite gradient
//                     overflows the sum.  64-lane shuffle tree, the four waves added in wave order from LDS, one (sum gu^2, sum p^2,
//                     nonfinite) partial per chunk in the workspace.
//   ts_finish_kernel  one workgroup.  Per tensor the chunk partials in chunk order; over the tensors thread t takes t, t + 256, ... and
//                     a fixed tree joins the threads; all in double.  Thread 0 then forms found_inf, the total gradient norm, the norm of
//                     the per-tensor parameter norms, clip_grad_norm_'s coefficient, advances the device step unless the step is skipped,
//                     applies _amp_update_scale_ and the floor, and writes the logged scalars.  Every thread then writes its tensors'
//                     AdamW coefficients, computed in double from the table's hyperparameters and rounded to fp32 where torch's
//                     _single_tensor_adam hands a Python float to an fp32 kernel.
//   ts_update_kernel  gu = (g * inv_scale) * clip_coef, then torch's single-tensor AdamW in fp32, in the operation order of ATen's CPU
//                     kernels, which is what the tests' oracle runs (addcmul as (value * a) * b, addcdiv as (value * a) / b; ATen's device
//                     kernels associate the other way, a difference of one rounding).  -ffp-contract=off: nothing is fused that torch
//                     does not fuse.  Writes nothing but zeros to g on a skipped step.
// Both streaming kernels take a full chunk on a path of its own, where every load is unconditional and issued before the first use; the
// last chunk of a tensor goes through guarded rounds.  The tensors' pointers are read from the table, so they are cast to the global
// address space by hand (global_load / global_store, not flat).
// No atomics: identical calls give identical bits.
#include <cmath>

#include "elem16.h"
#include "reduce.h"

namespace {

using gfn::f32x4;
using gfn::wave_sum_lane0;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kChunk = GFN_TS_CHUNK;
constexpr int kVecs = kChunk / (4 * kThreads);   // float4 per thread and array in a full chunk
constexpr int kScalarBatch = 8;                   // scalar path: loads in flight per thread and array
constexpr int kMaxTensors = 1 << 20;              // ts_finish_kernel loops: 4096 tensors per thread at the bound
constexpr int kMaxChunks = 1 << 23;               // grid x; 2^23 * 256 threads stays inside 32 bits
constexpr int kCtrlBytes = 64;
static_assert(kChunk % (4 * kThreads) == 0 && kVecs % 2 == 0, "a chunk is whole float4 rounds of the workgroup");

typedef gfn_ts_tensor TensorRec;
typedef gfn_ts_chunk ChunkRec;

struct State {          // GFN_TS_STATE_BYTES
    float scale;
    int tracker;
    long long step;
    float min_scale;
    int reserved[3];
};
static_assert(sizeof(State) == GFN_TS_STATE_BYTES, "state layout");
static_assert(sizeof(TensorRec) == 96 && sizeof(ChunkRec) == 16, "table layouts (gfnet_amd/trainer builds them with numpy)");

struct Ctrl {           // what the update kernel reads; the head of the workspace
    float inv_scale;
    float clip_coef;
    int skip;
    int pad[13];
};
static_assert(sizeof(Ctrl) == kCtrlBytes, "control block");

struct Coef {           // per tensor, fp32 as torch's kernels receive them
    float decay;        // 1 - lr * weight_decay
    float w1;           // 1 - beta1
    float beta2;
    float w2;           // 1 - beta2
    float bc2_sqrt;     // sqrt(1 - beta2^step)
    float neg_step;     // -(lr / (1 - beta1^step))
    float eps;
    float pad;
};

__device__ __forceinline__ bool nonfinite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }

// GradScaler.unscale_ multiplies by scale.double().reciprocal().float()
__device__ __forceinline__ float inverse_scale(float scale) { return (float)(1.0 / (double)scale); }

#define GFN_GLOBAL __attribute__((address_space(1)))
typedef GFN_GLOBAL float *gptr;
typedef const GFN_GLOBAL float *cgptr;
typedef GFN_GLOBAL f32x4 *gptr4;
typedef const GFN_GLOBAL f32x4 *cgptr4;

// per-lane accumulators of the norm pass
struct NormAcc {
    double sg = 0.0, sp = 0.0;
    bool bad = false;
    float inv;
    __device__ __forceinline__ void add(float gv, float pv) {
        bad = bad || nonfinite(gv);
        const double gu = (double)(gv * inv), pd = (double)pv;
        sg = fma(gu, gu, sg);
        sp = fma(pd, pd, sp);
    }
    __device__ __forceinline__ void add4(f32x4 gv, f32x4 pv) { add(gv.x, pv.x), add(gv.y, pv.y), add(gv.z, pv.z), add(gv.w, pv.w); }
};

// N unconditional loads per array, all issued before the first use
template <int N>
__device__ __forceinline__ void norm_vec_round(NormAcc &a, cgptr4 g4, cgptr4 p4, int i) {
    f32x4 gv[N], pv[N];
#pragma unroll
    for (int k = 0; k < N; ++k) gv[k] = g4[i + k * kThreads], pv[k] = p4[i + k * kThreads];
#pragma unroll
    for (int k = 0; k < N; ++k) a.add4(gv[k], pv[k]);
}

template <int N>
__device__ __forceinline__ void norm_scalar_round(NormAcc &a, cgptr g, cgptr p, int i) {
    float gv[N], pv[N];
#pragma unroll
    for (int k = 0; k < N; ++k) gv[k] = g[i + k * kThreads], pv[k] = p[i + k * kThreads];
#pragma unroll
    for (int k = 0; k < N; ++k) a.add(gv[k], pv[k]);
}

__global__ __launch_bounds__(kThreads) void ts_norm_kernel(const TensorRec *__restrict__ tensors, const ChunkRec *__restrict__ chunks,
                                                           const State *__restrict__ state, double *__restrict__ part) {
    __shared__ double red[kWaves][2];
    __shared__ int red_bad[kWaves];
    const ChunkRec c = chunks[blockIdx.x];
    const TensorRec &t = tensors[c.tensor];
    NormAcc a;
    a.inv = inverse_scale(state->scale);
    const cgptr g = (cgptr)(t.g + c.first), p = (cgptr)(t.p + c.first);
    const int tid = threadIdx.x, count = c.count;
    if (t.vec16) {
        const cgptr4 g4 = (cgptr4)g, p4 = (cgptr4)p;
        if (count == kChunk) {
            norm_vec_round<kVecs>(a, g4, p4, tid);
        } else {            // a tensor's last chunk: guarded rounds of two vectors, one vector, then a tail shorter than a vector
            const int nv = count >> 2;
            int i = tid;
            for (; i + kThreads < nv; i += 2 * kThreads) norm_vec_round<2>(a, g4, p4, i);
            if (i < nv) norm_vec_round<1>(a, g4, p4, i);
            const int e = nv * 4 + tid;
            if (e < count) a.add(g[e], p[e]);
        }
    } else {
        int base = 0;       // whole batches of the workgroup without a guard, then single elements
        for (; base + kScalarBatch * kThreads <= count; base += kScalarBatch * kThreads) norm_scalar_round<kScalarBatch>(a, g, p, base + tid);
        for (int i = base + tid; i < count; i += kThreads) a.add(g[i], p[i]);
    }
    const double sg = wave_sum_lane0(a.sg), sp = wave_sum_lane0(a.sp);
    const bool wave_bad = __ballot(a.bad) != 0ull;
    const int lane = tid & 63, wave = tid >> 6;
    if (lane == 0) red[wave][0] = sg, red[wave][1] = sp, red_bad[wave] = wave_bad;
    __syncthreads();
    if (tid == 0) {
        double x = red[0][0], y = red[0][1];
        int nb = red_bad[0];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) x += red[w][0], y += red[w][1], nb |= red_bad[w];
        double *o = part + (size_t)blockIdx.x * 3;
        o[0] = x, o[1] = y, o[2] = nb ? 1.0 : 0.0;
    }
}

__global__ __launch_bounds__(kThreads) void ts_finish_kernel(const TensorRec *__restrict__ tensors, int n_tensors, const double *__restrict__ part,
                                                             State *__restrict__ state, Ctrl *__restrict__ ctrl, Coef *__restrict__ coefs,
                                                             float *__restrict__ stats, double max_norm, float growth, float backoff,
                                                             int growth_interval) {
    __shared__ double red[3][kThreads];
    __shared__ long long s_step;
    __shared__ int s_skip;
    const int tid = threadIdx.x;
    double tg = 0.0, tp = 0.0, tb = 0.0;
    for (int t = tid; t < n_tensors; t += kThreads) {
        const double *q = part + (size_t)tensors[t].first_chunk * 3;
        const int nc = tensors[t].n_chunks;
        double sg = 0.0, sp = 0.0, sb = 0.0;
        for (int c = 0; c < nc; ++c) sg += q[3 * c], sp += q[3 * c + 1], sb += q[3 * c + 2];
        stats[GFN_TS_STATS + t] = sb > 0.0 ? 1.0f : 0.0f;
        tg += sg, tp += sp, tb += sb;
    }
    red[0][tid] = tg, red[1][tid] = tp, red[2][tid] = tb;
    __syncthreads();
    for (int half = kThreads / 2; half > 0; half >>= 1) {
        if (tid < half) {
#pragma unroll
            for (int qn = 0; qn < 3; ++qn) red[qn][tid] += red[qn][tid + half];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const bool found_inf = red[2][0] > 0.0;
        const double total = sqrt(red[0][0]);
        const float scale = state->scale;
        // clip_grad_norm_: max_norm / (total_norm + 1e-6), clamped to 1
        const double coef = max_norm / (total + 1e-6);
        ctrl->inv_scale = inverse_scale(scale);
        ctrl->clip_coef = (float)(coef < 1.0 ? coef : 1.0);
        ctrl->skip = found_inf;
        long long step = state->step;
        if (!found_inf && n_tensors > 0) state->step = ++step;
        s_step = step, s_skip = found_inf;
        // _amp_update_scale_, then the reference's floor (trainer/train.py:40-41)
        float ns = scale;
        int tracker = state->tracker;
        if (found_inf) {
            ns = scale * backoff;
            tracker = 0;
        } else if (++tracker == growth_interval) {
            const float grown = scale * growth;
            if (!nonfinite(grown)) ns = grown;
            tracker = 0;
        }
        if (ns < state->min_scale) ns = state->min_scale;
        state->scale = ns, state->tracker = tracker;
        stats[GFN_TS_STAT_GRAD_NORM] = (float)total;
        stats[GFN_TS_STAT_PARAM_NORM] = (float)sqrt(red[1][0]);
        stats[GFN_TS_STAT_GRAD_SCALE] = scale;
        stats[GFN_TS_STAT_FOUND_INF] = found_inf ? 1.0f : 0.0f;
        stats[GFN_TS_STAT_CLIP_COEF] = ctrl->clip_coef;
        stats[5] = stats[6] = stats[7] = 0.0f;
    }
    __syncthreads();
    if (s_skip) return;
    const double step = (double)s_step;
    for (int t = tid; t < n_tensors; t += kThreads) {
        const TensorRec &r = tensors[t];
        const double bc1 = 1.0 - pow(r.beta1, step), bc2 = 1.0 - pow(r.beta2, step);
        Coef c;
        c.decay = (float)(1.0 - r.lr * r.wd);
        c.w1 = (float)(1.0 - r.beta1);
        c.beta2 = (float)r.beta2;
        c.w2 = (float)(1.0 - r.beta2);
        c.bc2_sqrt = (float)sqrt(bc2);
        c.neg_step = (float)(-(r.lr / bc1));
        c.eps = (float)r.eps;
        c.pad = 0.0f;
        coefs[t] = c;
    }
}

// torch.optim.adam._single_tensor_adam (decoupled_weight_decay, amsgrad = maximize = capturable = False) for one element, each line in
// the association of ATen's CPU kernel for that op
struct Adam {
    Coef c;
    float inv, clip;
    bool lerp_small;
    __device__ __forceinline__ void one(float g, float &p, float &m, float &v) const {
        const float gu = g * inv * clip;                        // unscale_, then clip_grad_norm_'s mul_
        p = p * c.decay;                                        // param.mul_(1 - lr * weight_decay)
        const float diff = gu - m;                              // exp_avg.lerp_(grad, 1 - beta1): ATen's two forms of lerp
        m = lerp_small ? m + c.w1 * diff : gu - diff * (1.0f - c.w1);
        v = v * c.beta2;                                        // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
        v = v + c.w2 * gu * gu;
        const float denom = sqrtf(v) / c.bc2_sqrt + c.eps;      // (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps)
        p = p + c.neg_step * m / denom;                         // param.addcdiv_(exp_avg, denom, value=-step_size)
    }
    __device__ __forceinline__ void four(f32x4 g, f32x4 &p, f32x4 &m, f32x4 &v) const {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float pe = p[e], me = m[e], ve = v[e];
            one(g[e], pe, me, ve);
            p[e] = pe, m[e] = me, v[e] = ve;
        }
    }
};

// N vectors per array and thread: every load unconditional and issued before the first use, then the stores
template <int N>
__device__ __forceinline__ void update_vec_round(const Adam &a, gptr4 g4, gptr4 p4, gptr4 m4, gptr4 v4, int i, int zero_grads) {
    f32x4 g[N], p[N], m[N], v[N];
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const int j = i + k * kThreads;
        g[k] = g4[j], p[k] = p4[j], m[k] = m4[j], v[k] = v4[j];
    }
#pragma unroll
    for (int k = 0; k < N; ++k) a.four(g[k], p[k], m[k], v[k]);
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const int j = i + k * kThreads;
        p4[j] = p[k], m4[j] = m[k], v4[j] = v[k];
        if (zero_grads) g4[j] = (f32x4)(0.f);
    }
}

template <int N>
__device__ __forceinline__ void update_scalar_round(const Adam &a, gptr g, gptr p, gptr m, gptr v, int i, int zero_grads) {
    float ge[N], pe[N], me[N], ve[N];
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const int j = i + k * kThreads;
        ge[k] = g[j], pe[k] = p[j], me[k] = m[j], ve[k] = v[j];
    }
#pragma unroll
    for (int k = 0; k < N; ++k) a.one(ge[k], pe[k], me[k], ve[k]);
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const int j = i + k * kThreads;
        p[j] = pe[k], m[j] = me[k], v[j] = ve[k];
        if (zero_grads) g[j] = 0.f;
    }
}

__global__ __launch_bounds__(kThreads) void ts_update_kernel(const TensorRec *__restrict__ tensors, const ChunkRec *__restrict__ chunks,
                                                             const Ctrl *__restrict__ ctrl, const Coef *__restrict__ coefs, int zero_grads) {
    const int skip = ctrl->skip;
    if (skip && !zero_grads) return;
    const ChunkRec c = chunks[blockIdx.x];
    const TensorRec &t = tensors[c.tensor];
    const gptr g = (gptr)(t.g + c.first);
    const int tid = threadIdx.x, count = c.count;
    const int nv = t.vec16 ? count >> 2 : 0;
    const gptr4 g4 = (gptr4)g;
    if (skip) {             // only the gradients change: zero_grad
        for (int i = tid; i < nv; i += kThreads) g4[i] = (f32x4)(0.f);
        for (int i = nv * 4 + tid; i < count; i += kThreads) g[i] = 0.f;
        return;
    }
    Adam a;
    a.c = coefs[c.tensor];
    a.inv = ctrl->inv_scale, a.clip = ctrl->clip_coef;
    a.lerp_small = fabsf(a.c.w1) < 0.5f;
    const gptr p = (gptr)(t.p + c.first), m = (gptr)(t.exp_avg + c.first), v = (gptr)(t.exp_avg_sq + c.first);
    if (t.vec16) {
        const gptr4 p4 = (gptr4)p, m4 = (gptr4)m, v4 = (gptr4)v;
        if (count == kChunk) {
#pragma unroll
            for (int r = 0; r < kVecs / 2; ++r) update_vec_round<2>(a, g4, p4, m4, v4, tid + r * 2 * kThreads, zero_grads);
        } else {            // a tensor's last chunk: guarded rounds of two vectors, one vector, then a tail shorter than a vector
            int i = tid;
            for (; i + kThreads < nv; i += 2 * kThreads) update_vec_round<2>(a, g4, p4, m4, v4, i, zero_grads);
            if (i < nv) update_vec_round<1>(a, g4, p4, m4, v4, i, zero_grads);
            const int e = nv * 4 + tid;
            if (e < count) update_scalar_round<1>(a, g, p, m, v, e, zero_grads);
        }
    } else {
        int base = 0;       // whole batches of the workgroup without a guard, then single elements
        for (; base + kScalarBatch * kThreads <= count; base += kScalarBatch * kThreads)
            update_scalar_round<kScalarBatch>(a, g, p, m, v, base + tid, zero_grads);
        for (int i = base + tid; i < count; i += kThreads) update_scalar_round<1>(a, g, p, m, v, i, zero_grads);
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
int64_t ws_bytes_for(int64_t n_tensors, int64_t n_chunks) {
    return (kCtrlBytes + n_tensors * (int64_t)sizeof(Coef) + n_chunks * 3 * (int64_t)sizeof(double) + 15) / 16 * 16;
}

}  // namespace

GFN_EXPORT int64_t gfn_train_step_ws_bytes(int n_tensors, int n_chunks) {
    if (n_tensors < 0 || n_chunks < 0) return 0;
    return ws_bytes_for(n_tensors, n_chunks);
}

GFN_EXPORT int gfn_train_step(const gfn_ts_tensor *tensor_table, int n_tensors, const gfn_ts_chunk *chunk_table, int n_chunks, void *state,
                              double max_norm, double growth, double backoff, int growth_interval, int zero_grads, float *stats_out, void *ws,
                              int64_t ws_bytes, gfn_stream_t stream) {
    const char *what = "train_step";
    if (n_tensors < 0 || n_chunks < 0) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: negative table size (%d tensors, %d chunks)", what, n_tensors, n_chunks);
    if (n_tensors > kMaxTensors) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: %d tensors, at most %d (2^20) in one call", what, n_tensors, kMaxTensors);
    if (n_chunks > kMaxChunks) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: %d chunks, above the grid limit of %d (2^23)", what, n_chunks, kMaxChunks);
    if (n_tensors == 0 && n_chunks != 0) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: %d chunks of no tensor", what, n_chunks);
    if (!state || !stats_out) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: null state or stats_out", what);
    if ((n_tensors > 0 && !tensor_table) || (n_chunks > 0 && !chunk_table)) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: null table", what);
    if (!(max_norm >= 0.0) || !(growth >= 1.0) || !(backoff > 0.0 && backoff <= 1.0) || growth_interval < 1)
        return gfn::fail(GFN_ERR_INVALID_ARG, "%s: needs max_norm >= 0, growth >= 1, 0 < backoff <= 1, growth_interval >= 1", what);
    const int64_t need = ws_bytes_for(n_tensors, n_chunks);
    if (!ws || (reinterpret_cast<uintptr_t>(ws) & 15u) || ws_bytes < need)
        return gfn::fail(GFN_ERR_INVALID_ARG, "%s: workspace missing, not 16-byte aligned or too small (%lld bytes needed)", what, (long long)need);
    Ctrl *ctrl = static_cast<Ctrl *>(ws);
    Coef *coefs = reinterpret_cast<Coef *>(static_cast<char *>(ws) + kCtrlBytes);
    double *part = reinterpret_cast<double *>(static_cast<char *>(ws) + kCtrlBytes + (int64_t)n_tensors * sizeof(Coef));
    hipStream_t s = (hipStream_t)stream;
    if (n_chunks > 0) {
        hipLaunchKernelGGL(ts_norm_kernel, dim3(n_chunks), dim3(kThreads), 0, s, tensor_table, chunk_table, (const State *)state, part);
        if (int rc = gfn::check_launch("ts_norm_kernel")) return rc;
    }
    hipLaunchKernelGGL(ts_finish_kernel, dim3(1), dim3(kThreads), 0, s, tensor_table, n_tensors, (const double *)part, (State *)state, ctrl, coefs,
                       stats_out, max_norm, (float)growth, (float)backoff, growth_interval);
    if (int rc = gfn::check_launch("ts_finish_kernel")) return rc;
    if (n_chunks > 0) {
        hipLaunchKernelGGL(ts_update_kernel, dim3(n_chunks), dim3(kThreads), 0, s, tensor_table, chunk_table, (const Ctrl *)ctrl, (const Coef *)coefs,
                           zero_grads);
        return gfn::check_launch("ts_update_kernel");
    }
    return GFN_OK;
}
