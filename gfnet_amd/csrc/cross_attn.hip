// Cross-attention core of the cross-view decoder at head dim 8 (reference model/transformer/layers/attention.py:227-258, where
// flash_attn_func does this work): out = softmax(scale * Q K^T) V per (batch, head), forward and backward, for (B, N, H, 8)
// contiguous tensors in fp16 or fp32.  The N x N matrix is never written: the forward is an online softmax over key tiles, the
// backward recomputes P from the forward's lse: a pass by query tile for delta = sum_j P dP, one by key tile for dK and dV and one by
// query tile for dQ: no atomics, no scratch.
//
// One orientation serves all three kernels.  A head's rows are 8 values, the K of v_mfma_f32_32x32x8_f16, so a
// 32 x 32 tile of raw scores is ONE matrix instruction (fp32 inputs: four v_mfma_f32_32x32x2_f32, an fmaf chain bit for bit).
// The side a kernel keeps results for ("own": queries in the forward and in dQ, keys in dK/dV) is the B operand, so an own row
// sits on a lane (column = lane & 31) and the 32 rows of the side that streams past through LDS sit in the lane's 16 accumulator
// registers (rows acc_row(r, lane >> 5)): running maximum, running sum and the 8-wide fp32 results are per-lane registers, and
// the two lane halves of a row are merged once at the end.  What multiplies P or dS (V; K; dO and Q) is read from LDS as fp32
// rows: every lane of a half wants the same row, so the read is a broadcast.  P and dS are never rounded.
#include <hip/hip_fp16.h>

#include <cmath>
#include <initializer_list>

#include "common.h"

namespace {

using gfn::acc_row;
using gfn::f32x16;

constexpr int kThreads = 256;           // 4 waves: 4 own tiles of 32 rows per workgroup
constexpr int kOwn = 128;               // own rows per workgroup
constexpr int kChunk = 128;             // streamed rows staged per step (4 tiles); threads 0..127 stage one tensor, 128..255 another
constexpr int kRowImg = kChunk * 8 + kChunk;  // floats of a row image: 8 per row + 4 after every 4th row (see row_at)
constexpr float kLog2e = 1.4426950408889634f;
constexpr float kLn2 = 0.6931471805599453f;

typedef _Float16 h4 __attribute__((ext_vector_type(4)));

// one 8-value row as stored
template <typename T>
struct Row;
template <>
struct alignas(16) Row<_Float16> {
    _Float16 e[8];
};
template <>
struct alignas(16) Row<float> {
    float e[8];
};

template <typename T>
__device__ __forceinline__ Row<T> load_row(const T *p, bool ok) {
    Row<T> r;
    if (ok) {
        r = *reinterpret_cast<const Row<T> *>(p);
    } else {
#pragma unroll
        for (int d = 0; d < 8; ++d) r.e[d] = (T)0.0f;
    }
    return r;
}

// the MFMA operand fragment of lane half h for a row: fp16 -> values 4h..4h+3 (one 32x32x8 step); fp32 -> values h, h+2, h+4, h+6
// (the four 32x32x2 steps)
template <typename T>
struct Frag;
template <>
struct Frag<_Float16> {
    h4 v;
};
template <>
struct Frag<float> {
    float v[4];
};

__device__ __forceinline__ Frag<_Float16> frag_of(const Row<_Float16> &r, int h) {
    Frag<_Float16> f;
#pragma unroll
    for (int j = 0; j < 4; ++j) f.v[j] = h ? r.e[4 + j] : r.e[j];
    return f;
}
__device__ __forceinline__ Frag<float> frag_of(const Row<float> &r, int h) {
    Frag<float> f;
#pragma unroll
    for (int s = 0; s < 4; ++s) f.v[s] = h ? r.e[2 * s + 1] : r.e[2 * s];
    return f;
}

// D[i][j] = sum_k a[i][k] * b[k][j] over the 8 values: a's row on lane & 31 gives accumulator row i, b's row on lane & 31 column j
__device__ __forceinline__ f32x16 dot8(const Frag<_Float16> &a, const Frag<_Float16> &b) {
    f32x16 z = {};
    return __builtin_amdgcn_mfma_f32_32x32x8f16(a.v, b.v, z, 0, 0, 0);
}
__device__ __forceinline__ f32x16 dot8(const Frag<float> &a, const Frag<float> &b) {
    f32x16 acc = {};
#pragma unroll
    for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.v[s], b.v[s], acc, 0, 0, 0);
    return acc;
}

// LDS image of a staged chunk as the A operand.  fp16: the rows as stored, 16 bytes each: a wave's 64 fragment reads (8 bytes at
// [row][4h]) cover 512 contiguous bytes, conflict free.  fp32: transposed, [value][row]: a 32x32x2 step reads one float per lane
// from 32 consecutive addresses per half (row-major 32-byte rows would put rows r and r + 4 in one bank: 8-way).
template <typename T>
struct OpImg;
template <>
struct OpImg<_Float16> {
    alignas(16) _Float16 m[kChunk * 8];
    __device__ __forceinline__ void put(int row, const Row<_Float16> &r) { *reinterpret_cast<Row<_Float16> *>(&m[row * 8]) = r; }
    __device__ __forceinline__ Frag<_Float16> get(int tile, int lane) const {
        Frag<_Float16> f;
        f.v = *reinterpret_cast<const h4 *>(&m[(tile * 32 + (lane & 31)) * 8 + 4 * (lane >> 5)]);
        return f;
    }
};
template <>
struct OpImg<float> {
    alignas(16) float m[8 * kChunk];
    __device__ __forceinline__ void put(int row, const Row<float> &r) {
#pragma unroll
        for (int d = 0; d < 8; ++d) m[d * kChunk + row] = r.e[d];
    }
    __device__ __forceinline__ Frag<float> get(int tile, int lane) const {
        Frag<float> f;
#pragma unroll
        for (int s = 0; s < 4; ++s) f.v[s] = m[((lane >> 5) + 2 * s) * kChunk + tile * 32 + (lane & 31)];
        return f;
    }
};

// LDS image of a staged chunk as fp32 rows for broadcast reads.  The two halves of a wave read rows 4 apart (acc_row), which in
// plain 32-byte rows is 128 bytes = the same banks; 16 bytes of padding after every 4th row moves the second half 4 banks on, so
// each 16-byte read of the two halves touches 8 distinct banks.
__device__ __forceinline__ int row_at(int row) { return row * 8 + (row >> 2) * 4; }

template <typename T>
__device__ __forceinline__ void put_row(float *img, int row, const Row<T> &r) {
    float4 *p = reinterpret_cast<float4 *>(&img[row_at(row)]);
    p[0] = make_float4((float)r.e[0], (float)r.e[1], (float)r.e[2], (float)r.e[3]);
    p[1] = make_float4((float)r.e[4], (float)r.e[5], (float)r.e[6], (float)r.e[7]);
}

__device__ __forceinline__ void get_row(const float *img, int row, float out[8]) {
    const float4 *p = reinterpret_cast<const float4 *>(&img[row_at(row)]);
    const float4 a = p[0], b = p[1];
    out[0] = a.x, out[1] = a.y, out[2] = a.z, out[3] = a.w, out[4] = b.x, out[5] = b.y, out[6] = b.z, out[7] = b.w;
}

__device__ __forceinline__ float hw_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

__device__ __forceinline__ float other_half(float x) { return __shfl_xor(x, 32, 64); }

// lane half h stores values 4h..4h+3 of its row's 8 results (both halves hold all 8 after the merge); fp16: rounded to nearest
// even once, overflow to inf
__device__ __forceinline__ void store_half_row(_Float16 *p, const float v[8], int h) {
    h4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = (_Float16)(h ? v[4 + j] : v[j]);
    *reinterpret_cast<h4 *>(p + 4 * h) = o;
}
__device__ __forceinline__ void store_half_row(float *p, const float v[8], int h) {
    *reinterpret_cast<float4 *>(p + 4 * h) = h ? make_float4(v[4], v[5], v[6], v[7]) : make_float4(v[0], v[1], v[2], v[3]);
}

__device__ __forceinline__ int64_t row_offset(int b, int N, int n, int H, int hd) { return (((int64_t)b * N + n) * H + hd) * 8; }

// ---------------------------------------------------------------------------------------------------------------------------------
// forward: own = queries, streamed = keys (K as the A operand: S^T = K Q^T; V as fp32 rows)
template <typename T>
__global__ __launch_bounds__(kThreads) void cross_attn_fwd_kernel(const T *__restrict__ q, const T *__restrict__ k, const T *__restrict__ v,
                                                                  T *__restrict__ out, float *__restrict__ lse, int Nq, int Nk, int H,
                                                                  float scale) {
    __shared__ OpImg<T> kop;
    __shared__ alignas(16) float vrow[kRowImg];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5;
    const int hd = blockIdx.y, b = blockIdx.z;
    const int qi = (blockIdx.x * 4 + wave) * 32 + (lane & 31);
    const bool qok = qi < Nq;
    const Frag<T> qf = frag_of(load_row(q + row_offset(b, Nq, qok ? qi : 0, H, hd), qok), h);

    float m = -INFINITY, l = 0.f, o[8];
#pragma unroll
    for (int d = 0; d < 8; ++d) o[d] = 0.f;

    for (int k0 = 0; k0 < Nk; k0 += kChunk) {
        __syncthreads();  // the previous chunk has been consumed
        {
            const int row = tid & (kChunk - 1), key = k0 + row;
            const bool ok = key < Nk;
            if (tid < kChunk)
                kop.put(row, load_row(k + row_offset(b, Nk, ok ? key : 0, H, hd), ok));
            else
                put_row(vrow, row, load_row(v + row_offset(b, Nk, ok ? key : 0, H, hd), ok));
        }
        __syncthreads();
        const int left = Nk - k0, ntile = left >= kChunk ? kChunk / 32 : (left + 31) / 32;
#pragma unroll 1
        for (int t = 0; t < ntile; ++t) {
            const f32x16 s = dot8(kop.get(t, lane), qf);
            // scaled scores are rounded once, as the definition's `s * scale` is, and maximum and lse are kept in those units: the
            // backward forms the same rounded score, so where one key holds a row's weight score - lse is exactly 0 and P exactly 1
            float tv[16], mx = m;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                tv[r] = s[r] * scale;
                if (t * 32 + acc_row(r, h) < left) mx = fmaxf(mx, tv[r]);
            }
            // a lane half that has met no key yet (Nk < 5 leaves half 1 without any) keeps m = -inf, l = 0 and p = 0 throughout
            const float alpha = (m == -INFINITY) ? 0.f : hw_exp2((m - mx) * kLog2e);
            l *= alpha;
#pragma unroll
            for (int d = 0; d < 8; ++d) o[d] *= alpha;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = t * 32 + acc_row(r, h);
                // a key past the end weighs exactly zero: selected, not pushed below a sentinel
                const float e = hw_exp2((tv[r] - mx) * kLog2e);  // (evaluated for every row and selected: `ok ? exp2(..) : 0` is a branch per row)
                const float p = row < left ? e : 0.f;
                float vr[8];
                get_row(vrow, row, vr);
                l += p;
#pragma unroll
                for (int d = 0; d < 8; ++d) o[d] = fmaf(p, vr[d], o[d]);
            }
            m = mx;
        }
    }
    // merge the two lane halves of a query
    const float M = fmaxf(m, other_half(m));
    const float a = (m == -INFINITY) ? 0.f : hw_exp2((m - M) * kLog2e);
    l *= a;
    l += other_half(l);
#pragma unroll
    for (int d = 0; d < 8; ++d) {
        o[d] *= a;
        o[d] += other_half(o[d]);
        o[d] = o[d] / l;
    }
    if (qok) {
        store_half_row(out + row_offset(b, Nq, qi, H, hd), o, h);
        if (h == 0) lse[((int64_t)b * H + hd) * Nq + qi] = fmaf(log2f(l), kLn2, M);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The softmax backward needs, per query, delta = sum_j P dP (dP = dO V^T): dS = P (dP - delta).  It is formed as that sum, divided
// by sum_j P, in a pass of its own by query tile -- NOT as sum_d dO * O from the saved out, which is the same number in exact
// arithmetic: out carries half an ulp of its own rounding, dP - delta then carries that ulp times dO whatever P is, and for a row
// whose weight sits on one key with a large |k| * scale that is orders of magnitude above the row's true gradient and above what
// autograd of the plain definition gives (measured: 110 x the fp32 bound).  Dividing by sum_j P (1 up to the rounding of lse) keeps
// lse's rounding, which is common to a row's P, out of delta.  The key-tile pass needs every query's delta and the entry point has
// no scratch: the pass leaves delta in the first four bytes of the query's row of dq, which the dQ pass, launched last, reads
// before it overwrites the row.
template <typename T>
__device__ __forceinline__ float *delta_slot(T *dq_row) { return reinterpret_cast<float *>(dq_row); }

// delta: own = queries, streamed = keys (K and V as A operands: S^T = K Q^T, dP^T = V dO^T)
template <typename T>
__global__ __launch_bounds__(kThreads) void cross_attn_bwd_delta_kernel(const T *__restrict__ q, const T *__restrict__ k,
                                                                        const T *__restrict__ v, const float *__restrict__ lse,
                                                                        const T *__restrict__ dout, T *__restrict__ dq, int Nq, int Nk,
                                                                        int H, float scale) {
    __shared__ OpImg<T> kop, vop;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5;
    const int hd = blockIdx.y, b = blockIdx.z;
    const int qi = (blockIdx.x * 4 + wave) * 32 + (lane & 31);
    const bool qok = qi < Nq;
    const int64_t qoff = row_offset(b, Nq, qok ? qi : 0, H, hd);
    const Frag<T> qf = frag_of(load_row(q + qoff, qok), h);
    const Frag<T> dof = frag_of(load_row(dout + qoff, qok), h);
    const float lse_q = qok ? lse[((int64_t)b * H + hd) * Nq + qi] : 0.f;
    float acc = 0.f, psum = 0.f;
    for (int k0 = 0; k0 < Nk; k0 += kChunk) {
        __syncthreads();
        {
            const int row = tid & (kChunk - 1), key = k0 + row;
            const bool ok = key < Nk;
            const int64_t off = row_offset(b, Nk, ok ? key : 0, H, hd);
            if (tid < kChunk)
                kop.put(row, load_row(k + off, ok));
            else
                vop.put(row, load_row(v + off, ok));
        }
        __syncthreads();
        const int left = Nk - k0, ntile = left >= kChunk ? kChunk / 32 : (left + 31) / 32;
#pragma unroll 1
        for (int t = 0; t < ntile; ++t) {
            const f32x16 s = dot8(kop.get(t, lane), qf);
            const f32x16 dp = dot8(vop.get(t, lane), dof);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float e = hw_exp2((s[r] * scale - lse_q) * kLog2e);
                const float p = t * 32 + acc_row(r, h) < left ? e : 0.f;
                psum += p;
                acc = fmaf(p, dp[r], acc);
            }
        }
    }
    acc += other_half(acc);
    psum += other_half(psum);
    if (qok && h == 0) *delta_slot(dq + qoff) = acc / psum;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// dQ: own = queries, streamed = keys (K and V as A operands: S^T = K Q^T, dP^T = V dO^T; K as fp32 rows); launched last: its rows of dq
// hold delta until it stores them
template <typename T>
__global__ __launch_bounds__(kThreads) void cross_attn_bwd_dq_kernel(const T *__restrict__ q, const T *__restrict__ k,
                                                                     const T *__restrict__ v, const float *__restrict__ lse,
                                                                     const T *__restrict__ dout, T *dq, int Nq, int Nk, int H, float scale) {
    __shared__ OpImg<T> kop, vop;
    __shared__ alignas(16) float krow[kRowImg];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5;
    const int hd = blockIdx.y, b = blockIdx.z;
    const int qi = (blockIdx.x * 4 + wave) * 32 + (lane & 31);
    const bool qok = qi < Nq;
    const int64_t qoff = row_offset(b, Nq, qok ? qi : 0, H, hd);
    const Frag<T> qf = frag_of(load_row(q + qoff, qok), h);
    const Frag<T> dof = frag_of(load_row(dout + qoff, qok), h);
    const float delta = qok ? *delta_slot(dq + qoff) : 0.f;  // both lane halves of the row read it; the row is stored after the loop
    const float lse_q = qok ? lse[((int64_t)b * H + hd) * Nq + qi] : 0.f;

    float g[8];
#pragma unroll
    for (int d = 0; d < 8; ++d) g[d] = 0.f;

    for (int k0 = 0; k0 < Nk; k0 += kChunk) {
        __syncthreads();
        {
            const int row = tid & (kChunk - 1), key = k0 + row;
            const bool ok = key < Nk;
            if (tid < kChunk) {
                const Row<T> kr = load_row(k + row_offset(b, Nk, ok ? key : 0, H, hd), ok);
                kop.put(row, kr);
                put_row(krow, row, kr);
            } else {
                vop.put(row, load_row(v + row_offset(b, Nk, ok ? key : 0, H, hd), ok));
            }
        }
        __syncthreads();
        const int left = Nk - k0, ntile = left >= kChunk ? kChunk / 32 : (left + 31) / 32;
#pragma unroll 1
        for (int t = 0; t < ntile; ++t) {
            const f32x16 s = dot8(kop.get(t, lane), qf);
            const f32x16 dp = dot8(vop.get(t, lane), dof);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = t * 32 + acc_row(r, h);
                const float e = hw_exp2((s[r] * scale - lse_q) * kLog2e);  // (evaluated for every row and selected: `ok ? exp2(..) : 0` is a branch per row)
                const float p = row < left ? e : 0.f;
                const float ds = p * (dp[r] - delta);
                float kr[8];
                get_row(krow, row, kr);
#pragma unroll
                for (int d = 0; d < 8; ++d) g[d] = fmaf(ds, kr[d], g[d]);
            }
        }
    }
#pragma unroll
    for (int d = 0; d < 8; ++d) {
        g[d] += other_half(g[d]);
        g[d] *= scale;
    }
    if (qok) store_half_row(dq + qoff, g, h);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// dK, dV: own = keys, streamed = queries (Q and dO as A operands: S = Q K^T, dP = dO V^T; Q and dO as fp32 rows; lse and the delta
// pass's result per staged query)
template <typename T>
__global__ __launch_bounds__(kThreads) void cross_attn_bwd_dkv_kernel(const T *__restrict__ q, const T *__restrict__ k,
                                                                      const T *__restrict__ v, const float *__restrict__ lse,
                                                                      const T *__restrict__ dout, const T *__restrict__ dq,
                                                                      T *__restrict__ dk, T *__restrict__ dv, int Nq, int Nk, int H,
                                                                      float scale) {
    __shared__ OpImg<T> qop, doop;
    __shared__ alignas(16) float qrow[kRowImg];
    __shared__ alignas(16) float dorow[kRowImg];
    __shared__ float lses[kChunk], deltas[kChunk];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5;
    const int hd = blockIdx.y, b = blockIdx.z;
    const int ki = (blockIdx.x * 4 + wave) * 32 + (lane & 31);
    const bool kok = ki < Nk;
    const int64_t koff = row_offset(b, Nk, kok ? ki : 0, H, hd);
    const Frag<T> kf = frag_of(load_row(k + koff, kok), h);
    const Frag<T> vf = frag_of(load_row(v + koff, kok), h);

    float gk[8], gv[8];
#pragma unroll
    for (int d = 0; d < 8; ++d) gk[d] = gv[d] = 0.f;

    for (int q0 = 0; q0 < Nq; q0 += kChunk) {
        __syncthreads();
        {
            const int row = tid & (kChunk - 1), qi = q0 + row;
            const bool ok = qi < Nq;
            const int64_t off = row_offset(b, Nq, ok ? qi : 0, H, hd);
            if (tid < kChunk) {
                const Row<T> qr = load_row(q + off, ok);
                qop.put(row, qr);
                put_row(qrow, row, qr);
                lses[row] = ok ? lse[((int64_t)b * H + hd) * Nq + qi] : 0.f;
            } else {
                const Row<T> dor = load_row(dout + off, ok);
                doop.put(row, dor);
                put_row(dorow, row, dor);
                deltas[row] = ok ? *reinterpret_cast<const float *>(dq + off) : 0.f;
            }
        }
        __syncthreads();
        const int left = Nq - q0, ntile = left >= kChunk ? kChunk / 32 : (left + 31) / 32;
#pragma unroll 1
        for (int t = 0; t < ntile; ++t) {
            const f32x16 s = dot8(qop.get(t, lane), kf);
            const f32x16 dp = dot8(doop.get(t, lane), vf);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = t * 32 + acc_row(r, h);
                const float lq = lses[row], dl = deltas[row];
                const float e = hw_exp2((s[r] * scale - lq) * kLog2e);
                const float p = row < left ? e : 0.f;
                const float ds = p * (dp[r] - dl);
                float qr[8], dr[8];
                get_row(qrow, row, qr);
                get_row(dorow, row, dr);
#pragma unroll
                for (int d = 0; d < 8; ++d) {
                    gv[d] = fmaf(p, dr[d], gv[d]);
                    gk[d] = fmaf(ds, qr[d], gk[d]);
                }
            }
        }
    }
#pragma unroll
    for (int d = 0; d < 8; ++d) {
        gv[d] += other_half(gv[d]);
        gk[d] += other_half(gk[d]);
        gk[d] *= scale;
    }
    if (kok) {
        store_half_row(dk + koff, gk, h);
        store_half_row(dv + koff, gv, h);
    }
}

int check_args(const char *what, int dtype, int B, int Nq, int Nk, int H, int D, float scale, std::initializer_list<const void *> ptrs) {
    if (D != 8) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: head dim %d is not supported, only D = 8 (one v_mfma_f32_32x32x8_f16 per score tile)", what, D);
    if (dtype != GFN_F32 && dtype != GFN_F16) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: dtype must be GFN_F32 or GFN_F16, got %d", what, dtype);
    if (B < 0 || Nq < 0 || Nk < 1 || H < 1) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: bad size (B=%d Nq=%d Nk=%d H=%d)", what, B, Nq, Nk, H);
    if (B > 65535 || H > 65535) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: B and H are grid dimensions, at most 65535 (B=%d H=%d)", what, B, H);
    if (!std::isfinite(scale)) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: scale must be finite", what);
    if (B == 0 || Nq == 0) return GFN_OK;
    for (const void *p : ptrs) {
        if (!p) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: null pointer", what);
        if ((uintptr_t)p & 15) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: tensors must be 16-byte aligned (rows are read as one vector)", what);
    }
    return GFN_OK;
}

// delta pass -> dK, dV pass -> dQ pass, in that order: delta travels in dq (see cross_attn_bwd_delta_kernel)
template <typename T>
int launch_bwd(const void *q, const void *k, const void *v, const float *lse, const void *dout, void *dq, void *dk, void *dv, int B,
               int Nq, int Nk, int H, float scale, hipStream_t s) {
    const dim3 gq((Nq + kOwn - 1) / kOwn, H, B), gk((Nk + kOwn - 1) / kOwn, H, B);
    hipLaunchKernelGGL(cross_attn_bwd_delta_kernel<T>, gq, dim3(kThreads), 0, s, (const T *)q, (const T *)k, (const T *)v, lse,
                       (const T *)dout, (T *)dq, Nq, Nk, H, scale);
    if (int rc = gfn::check_launch("cross_attn_bwd_delta_kernel")) return rc;
    hipLaunchKernelGGL(cross_attn_bwd_dkv_kernel<T>, gk, dim3(kThreads), 0, s, (const T *)q, (const T *)k, (const T *)v, lse,
                       (const T *)dout, (const T *)dq, (T *)dk, (T *)dv, Nq, Nk, H, scale);
    if (int rc = gfn::check_launch("cross_attn_bwd_dkv_kernel")) return rc;
    hipLaunchKernelGGL(cross_attn_bwd_dq_kernel<T>, gq, dim3(kThreads), 0, s, (const T *)q, (const T *)k, (const T *)v, lse,
                       (const T *)dout, (T *)dq, Nq, Nk, H, scale);
    return gfn::check_launch("cross_attn_bwd_dq_kernel");
}

}  // namespace

GFN_EXPORT int gfn_cross_attn_fwd(const void *q, const void *k, const void *v, int dtype, int B, int Nq, int Nk, int H, int D, float scale,
                                  void *out, float *lse, gfn_stream_t stream) {
    const char *what = "gfn_cross_attn_fwd";
    if (int rc = check_args(what, dtype, B, Nq, Nk, H, D, scale, {q, k, v, out})) return rc;
    if (B == 0 || Nq == 0) return GFN_OK;
    if (!lse || ((uintptr_t)lse & 3)) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: lse missing or not 4-byte aligned", what);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((Nq + kOwn - 1) / kOwn, H, B);
    if (dtype == GFN_F16)
        hipLaunchKernelGGL(cross_attn_fwd_kernel<_Float16>, grid, dim3(kThreads), 0, s, (const _Float16 *)q, (const _Float16 *)k,
                           (const _Float16 *)v, (_Float16 *)out, lse, Nq, Nk, H, scale);
    else
        hipLaunchKernelGGL(cross_attn_fwd_kernel<float>, grid, dim3(kThreads), 0, s, (const float *)q, (const float *)k, (const float *)v,
                           (float *)out, lse, Nq, Nk, H, scale);
    return gfn::check_launch("cross_attn_fwd_kernel");
}

GFN_EXPORT int gfn_cross_attn_bwd(const void *q, const void *k, const void *v, const void *out, const float *lse, const void *dout, int dtype,
                                  int B, int Nq, int Nk, int H, int D, float scale, void *dq, void *dk, void *dv, gfn_stream_t stream) {
    const char *what = "gfn_cross_attn_bwd";
    if (int rc = check_args(what, dtype, B, Nq, Nk, H, D, scale, {q, k, v, out, dout, dq, dk, dv})) return rc;
    if (B == 0) return GFN_OK;
    hipStream_t s = (hipStream_t)stream;
    if (Nq == 0) {  // no query: dK = dV = 0
        if (!dk || !dv) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: null pointer", what);
        const size_t bytes = (size_t)B * Nk * H * 8 * (dtype == GFN_F16 ? 2 : 4);
        if (hipMemsetAsync(dk, 0, bytes, s) != hipSuccess || hipMemsetAsync(dv, 0, bytes, s) != hipSuccess)
            return gfn::fail(GFN_ERR_LAUNCH, "%s: hipMemsetAsync failed", what);
        return GFN_OK;
    }
    if (!lse || ((uintptr_t)lse & 3)) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: lse missing or not 4-byte aligned", what);
    return dtype == GFN_F16 ? launch_bwd<_Float16>(q, k, v, lse, dout, dq, dk, dv, B, Nq, Nk, H, scale, s)
                            : launch_bwd<float>(q, k, v, lse, dout, dq, dk, dv, B, Nq, Nk, H, scale, s);
}
