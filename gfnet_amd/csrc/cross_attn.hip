// Cross-attention core of the cross-view decoder at head dim 8 (reference model/transformer/layers/attention.py:227-258, where
// flash_attn_func does this work): out = softmax(scale * Q K^T) V per (batch, head), forward and backward, for (B, N, H, 8)
// contiguous tensors in fp16, bf16 or fp32.  The N x N matrix is never written: the forward is an online softmax over key tiles, the
// backward recomputes P from the forward's lse: a pass by query tile for delta = sum_j P dP, one by key tile for dK and dV and one by
// query tile for dQ: no atomics, no scratch.
//
// One orientation serves all three kernels.  A head's rows are 8 values, the K of v_mfma_f32_32x32x8_f16, so a
// 32 x 32 tile of raw scores is ONE matrix instruction (bf16 inputs: v_mfma_f32_32x32x8_bf16, the same shape; fp32 inputs: four v_mfma_f32_32x32x2_f32, an fmaf chain bit for bit).
// The side a kernel keeps results for ("own": queries in the forward and in dQ, keys in dK/dV) is the B operand, so an own row
// sits on a lane (column = lane & 31) and the 32 rows of the side that streams past through LDS sit in the lane's 16 accumulator
// registers (rows acc_row(r, lane >> 5)): running maximum, running sum and the 8-wide fp32 results are per-lane registers, and
// the two lane halves of a row are merged once at the end.  What multiplies P or dS (V; K; dO and Q) is read from LDS as fp32
// rows: every lane of a half wants the same row, so the read is a broadcast.  P and dS are never rounded.
#include <initializer_list>

#include "attn_common.h"

namespace {

using namespace gfn;
using namespace gfn::attn;

constexpr int kThreads = 256;           // 4 waves: 4 own tiles of 32 rows per workgroup
constexpr int kOwn = 128;               // own rows per workgroup
constexpr int kChunk = 128;             // streamed rows staged per step (4 tiles); threads 0..127 stage one tensor, 128..255 another
constexpr int kRowImg = kChunk * 8 + kChunk;  // floats of a row image: 8 per row + 4 after every 4th row (see row_at)

// one 8-value row as stored
template <typename T>
struct alignas(16) Row {
    T e[8];
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

// the MFMA operand fragment of lane half h for a row: fp16, bf16 -> values 4h..4h+3 (one 32x32x8 step); fp32 -> values h, h+2, h+4,
// h+6 (the four 32x32x2 steps)
template <typename T>
struct Frag {
    typename Elem16<T>::vec4 v;
};
template <>
struct Frag<float> {
    float v[4];
};

template <typename T>
__device__ __forceinline__ Frag<T> frag_of(const Row<T> &r, int h) {
    Frag<T> f;
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
// (fp16, bf16: one v_mfma_f32_32x32x8_f16 / _bf16, exact products in both)
template <typename T>
__device__ __forceinline__ f32x16 dot8(const Frag<T> &a, const Frag<T> &b) {
    f32x16 z = {};
    return mfma8(a.v, b.v, z);
}
__device__ __forceinline__ f32x16 dot8(const Frag<float> &a, const Frag<float> &b) {
    f32x16 acc = {};
#pragma unroll
    for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.v[s], b.v[s], acc, 0, 0, 0);
    return acc;
}

// LDS image of a staged chunk as the A operand.  fp16, bf16: the rows as stored, 16 bytes each: a wave's 64 fragment reads (8 bytes
// at [row][4h]) cover 512 contiguous bytes, conflict free.  fp32: transposed, [value][row]: a 32x32x2 step reads one float per lane
// from 32 consecutive addresses per half (row-major 32-byte rows would put rows r and r + 4 in one bank: 8-way).
template <typename T>
struct OpImg {
    alignas(16) T m[kChunk * 8];
    __device__ __forceinline__ void put(int row, const Row<T> &r) { *reinterpret_cast<Row<T> *>(&m[row * 8]) = r; }
    __device__ __forceinline__ Frag<T> get(int tile, int lane) const {
        Frag<T> f;
        f.v = *reinterpret_cast<const typename Elem16<T>::vec4 *>(&m[(tile * 32 + (lane & 31)) * 8 + 4 * (lane >> 5)]);
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

// lane half h stores values 4h..4h+3 of its row's 8 results (both halves hold all 8 after the merge).  fp16, bf16: rounded to nearest
// even once (v_cvt_f16_f32 / v_cvt_pk_bf16_f32) with no clamp: fp16 overflows to inf; bf16 has fp32's exponent range, so nothing
// overflows that was finite in fp32, and inf and NaN stay what they are
template <typename T>
__device__ __forceinline__ void store_half_row(T *p, const float v[8], int h) {
    typename Elem16<T>::vec4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = (T)(h ? v[4 + j] : v[j]);
    *reinterpret_cast<typename Elem16<T>::vec4 *>(p + 4 * h) = o;
}
__device__ __forceinline__ void store_half_row(float *p, const float v[8], int h) {
    *reinterpret_cast<float4 *>(p + 4 * h) = h ? make_float4(v[4], v[5], v[6], v[7]) : make_float4(v[0], v[1], v[2], v[3]);
}

__device__ __forceinline__ int64_t row_offset(int b, int N, int n, int H, int hd) { return (((int64_t)b * N + n) * H + hd) * 8; }

// where query i's lse sits, (B, H, Nq); the grid is (tiles of own rows, H, B) in every kernel
__device__ __forceinline__ int64_t lse_index(int Nq, int H, int i) { return ((int64_t)blockIdx.z * H + blockIdx.y) * Nq + i; }

// A lane's own row of the N its kernel keeps results for: lane half h, index i, whether it exists, and its offset (row 0's where it
// does not, so that the address is always one of the tensor's)
struct OwnRow {
    int lane, h, i;
    bool ok;
    int64_t off;
};
__device__ __forceinline__ OwnRow own_row(int N, int H) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = (blockIdx.x * 4 + wave) * 32 + (lane & 31);
    return {lane, lane >> 5, i, i < N, row_offset(blockIdx.z, N, i < N ? i : 0, H, blockIdx.y)};
}

// The loop every kernel runs over the N rows of the side that streams past, kChunk at a time: stage(first_half, row, n, offset, ok)
// once per thread puts row n of the tensors (slot `row` of the chunk; threads 0..127 are first_half and stage one tensor, 128..255
// the other; !ok: n is past the end, offset is row 0's and zeros are staged) into the kernel's own LDS images, then tile(t, left)
// runs for each 32-row tile t that has a row below left = the rows remaining from the chunk's start.  The tile loop stays rolled.
// (The kernels' tile lambdas take lane and h by value: captured by reference, every kernel's tile loop comes out a few address
// instructions longer, which measured 1 % at N = 1600.)
template <typename Stage, typename Tile>
__device__ __forceinline__ void stream_rows(int N, int H, Stage stage, Tile tile) {
    const int tid = threadIdx.x, hd = blockIdx.y, b = blockIdx.z;
    for (int n0 = 0; n0 < N; n0 += kChunk) {
        __syncthreads();  // the previous chunk has been consumed
        {
            const int row = tid & (kChunk - 1), n = n0 + row;
            const bool ok = n < N;
            if (tid < kChunk)  // (one call per half, each forming its offset: see the note at the forward's store)
                stage(true, row, n, row_offset(b, N, ok ? n : 0, H, hd), ok);
            else
                stage(false, row, n, row_offset(b, N, ok ? n : 0, H, hd), ok);
        }
        __syncthreads();
        const int left = N - n0, ntile = left >= kChunk ? kChunk / 32 : (left + 31) / 32;
#pragma unroll 1
        for (int t = 0; t < ntile; ++t) tile(t, left);
    }
}

// The backward's weight of one score, recomputed from the forward's lse.  The order is the forward's: the scaled score is rounded
// once, fl(s * scale), exactly as the forward rounded it before taking the maximum, and lse is in those units, so where one key
// holds a row's weight the difference is exactly 0 and P exactly 1; log2e multiplies afterwards (folding it into scale and lse is
// three roundings at the score's magnitude instead of a cancelling one: 2.4x the fp32 bound on dV).  A row past the end weighs
// exactly zero, and the exponential is evaluated for every row and then selected: `in_range ? exp2(..) : 0` is compiled as a branch
// per row, which cost 256 VGPRs and all but one wave per SIMD.
__device__ __forceinline__ float prob(float s, float scale, float lse, bool in_range) {
    const float e = hw_exp2((s * scale - lse) * kLog2e);
    return in_range ? e : 0.f;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// forward: own = queries, streamed = keys (K as the A operand: S^T = K Q^T; V as fp32 rows)
template <typename T>
__global__ __launch_bounds__(kThreads) void cross_attn_fwd_kernel(const T *__restrict__ q, const T *__restrict__ k, const T *__restrict__ v,
                                                                  T *__restrict__ out, float *__restrict__ lse, int Nq, int Nk, int H,
                                                                  float scale) {
    __shared__ OpImg<T> kop;
    __shared__ alignas(16) float vrow[kRowImg];
    const OwnRow own = own_row(Nq, H);
    const int lane = own.lane, h = own.h;
    const Frag<T> qf = frag_of(load_row(q + own.off, own.ok), h);

    float m = -INFINITY, l = 0.f, o[8];
#pragma unroll
    for (int d = 0; d < 8; ++d) o[d] = 0.f;

    stream_rows(
        Nk, H,
        [&](bool first, int row, int, int64_t off, bool ok) {
            if (first)
                kop.put(row, load_row(k + off, ok));
            else
                put_row(vrow, row, load_row(v + off, ok));
        },
        [&, lane, h](int t, int left) {
            const f32x16 s = dot8(kop.get(t, lane), qf);
            // scaled scores are rounded once, as the definition's `s * scale` is, and maximum and lse are kept in those units: the
            // backward forms the same rounded score (prob), so where one key holds a row's weight score - lse is exactly 0 and P exactly 1
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
                // a key past the end weighs exactly zero: selected, not pushed below a sentinel, and evaluated for every row first (see
                // prob, the backward's form of this weight)
                const float e = hw_exp2((tv[r] - mx) * kLog2e);
                const float p = row < left ? e : 0.f;
                float vr[8];
                get_row(vrow, row, vr);
                l += p;
#pragma unroll
                for (int d = 0; d < 8; ++d) o[d] = fmaf(p, vr[d], o[d]);
            }
            m = mx;
        });
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
    if (own.ok) {
        // The offset is formed again here, and stream_rows forms the staged row's once per thread half: with own.off held across the
        // loop, or with one offset shared by the two halves, the fp32 instantiation takes 114 to 125 VGPRs and loses a wave per SIMD.
        store_half_row(out + row_offset(blockIdx.z, Nq, own.i, H, blockIdx.y), o, h);
        if (h == 0) lse[lse_index(Nq, H, own.i)] = fmaf(log2f(l), kLn2, M);
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
// before it overwrites the row.  The slot is an fp32 value in a row of 8 T: a bf16 row is 16 bytes and 16-byte aligned exactly as an
// fp16 row is, so the parking carries over to bf16 unchanged (the narrowest row there is holds four floats).
template <typename T>
__device__ __forceinline__ float *delta_slot(T *dq_row) { return reinterpret_cast<float *>(dq_row); }

// delta: own = queries, streamed = keys (K and V as A operands: S^T = K Q^T, dP^T = V dO^T)
template <typename T>
__global__ __launch_bounds__(kThreads) void cross_attn_bwd_delta_kernel(const T *__restrict__ q, const T *__restrict__ k,
                                                                        const T *__restrict__ v, const float *__restrict__ lse,
                                                                        const T *__restrict__ dout, T *__restrict__ dq, int Nq, int Nk,
                                                                        int H, float scale) {
    __shared__ OpImg<T> kop, vop;
    const OwnRow own = own_row(Nq, H);
    const int lane = own.lane, h = own.h;
    const Frag<T> qf = frag_of(load_row(q + own.off, own.ok), h);
    const Frag<T> dof = frag_of(load_row(dout + own.off, own.ok), h);
    const float lse_q = own.ok ? lse[lse_index(Nq, H, own.i)] : 0.f;
    float acc = 0.f, psum = 0.f;
    stream_rows(
        Nk, H,
        [&](bool first, int row, int, int64_t off, bool ok) {
            if (first)
                kop.put(row, load_row(k + off, ok));
            else
                vop.put(row, load_row(v + off, ok));
        },
        [&, lane, h](int t, int left) {
            const f32x16 s = dot8(kop.get(t, lane), qf);
            const f32x16 dp = dot8(vop.get(t, lane), dof);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float p = prob(s[r], scale, lse_q, t * 32 + acc_row(r, h) < left);
                psum += p;
                acc = fmaf(p, dp[r], acc);
            }
        });
    acc += other_half(acc);
    psum += other_half(psum);
    if (own.ok && h == 0) *delta_slot(dq + own.off) = acc / psum;
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
    const OwnRow own = own_row(Nq, H);
    const int lane = own.lane, h = own.h;
    const Frag<T> qf = frag_of(load_row(q + own.off, own.ok), h);
    const Frag<T> dof = frag_of(load_row(dout + own.off, own.ok), h);
    const float delta = own.ok ? *delta_slot(dq + own.off) : 0.f;  // both lane halves of the row read it; the row is stored after the loop
    const float lse_q = own.ok ? lse[lse_index(Nq, H, own.i)] : 0.f;

    float g[8];
#pragma unroll
    for (int d = 0; d < 8; ++d) g[d] = 0.f;

    stream_rows(
        Nk, H,
        [&](bool first, int row, int, int64_t off, bool ok) {
            if (first) {
                const Row<T> kr = load_row(k + off, ok);
                kop.put(row, kr);
                put_row(krow, row, kr);
            } else {
                vop.put(row, load_row(v + off, ok));
            }
        },
        [&, lane, h](int t, int left) {
            const f32x16 s = dot8(kop.get(t, lane), qf);
            const f32x16 dp = dot8(vop.get(t, lane), dof);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = t * 32 + acc_row(r, h);
                const float ds = prob(s[r], scale, lse_q, row < left) * (dp[r] - delta);
                float kr[8];
                get_row(krow, row, kr);
#pragma unroll
                for (int d = 0; d < 8; ++d) g[d] = fmaf(ds, kr[d], g[d]);
            }
        });
#pragma unroll
    for (int d = 0; d < 8; ++d) {
        g[d] += other_half(g[d]);
        g[d] *= scale;
    }
    if (own.ok) store_half_row(dq + own.off, g, h);
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
    const OwnRow own = own_row(Nk, H);
    const int lane = own.lane, h = own.h;
    const Frag<T> kf = frag_of(load_row(k + own.off, own.ok), h);
    const Frag<T> vf = frag_of(load_row(v + own.off, own.ok), h);

    float gk[8], gv[8];
#pragma unroll
    for (int d = 0; d < 8; ++d) gk[d] = gv[d] = 0.f;

    stream_rows(
        Nq, H,
        [&](bool first, int row, int qi, int64_t off, bool ok) {
            if (first) {
                const Row<T> qr = load_row(q + off, ok);
                qop.put(row, qr);
                put_row(qrow, row, qr);
                lses[row] = ok ? lse[lse_index(Nq, H, qi)] : 0.f;
            } else {
                const Row<T> dor = load_row(dout + off, ok);
                doop.put(row, dor);
                put_row(dorow, row, dor);
                deltas[row] = ok ? *reinterpret_cast<const float *>(dq + off) : 0.f;
            }
        },
        [&, lane, h](int t, int left) {
            const f32x16 s = dot8(qop.get(t, lane), kf);
            const f32x16 dp = dot8(doop.get(t, lane), vf);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = t * 32 + acc_row(r, h);
                const float p = prob(s[r], scale, lses[row], row < left);
                const float ds = p * (dp[r] - deltas[row]);
                float qr[8], dr[8];
                get_row(qrow, row, qr);
                get_row(dorow, row, dr);
#pragma unroll
                for (int d = 0; d < 8; ++d) {
                    gv[d] = fmaf(p, dr[d], gv[d]);
                    gk[d] = fmaf(ds, qr[d], gk[d]);
                }
            }
        });
#pragma unroll
    for (int d = 0; d < 8; ++d) {
        gv[d] += other_half(gv[d]);
        gk[d] += other_half(gk[d]);
        gk[d] *= scale;
    }
    if (own.ok) {
        store_half_row(dk + own.off, gk, h);
        store_half_row(dv + own.off, gv, h);
    }
}

int check_args(const char *what, int dtype, int B, int Nq, int Nk, int H, int D, float scale, std::initializer_list<const void *> ptrs) {
    if (D != 8) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: head dim %d is not supported, only D = 8 (one v_mfma_f32_32x32x8_f16 per score tile)", what, D);
    if (dtype != GFN_F32 && dtype != GFN_F16 && dtype != GFN_BF16)
        return gfn::fail(GFN_ERR_INVALID_ARG, "%s: dtype must be GFN_F32, GFN_F16 or GFN_BF16, got %d", what, dtype);
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

template <typename T>
int launch_fwd(const void *q, const void *k, const void *v, void *out, float *lse, int B, int Nq, int Nk, int H, float scale, hipStream_t s) {
    hipLaunchKernelGGL(cross_attn_fwd_kernel<T>, dim3((Nq + kOwn - 1) / kOwn, H, B), dim3(kThreads), 0, s, (const T *)q, (const T *)k,
                       (const T *)v, (T *)out, lse, Nq, Nk, H, scale);
    return gfn::check_launch("cross_attn_fwd_kernel");
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
    if (dtype == GFN_F32) return launch_fwd<float>(q, k, v, out, lse, B, Nq, Nk, H, scale, s);
    return with_elem16(dtype, [&](auto e) { return launch_fwd<decltype(e)>(q, k, v, out, lse, B, Nq, Nk, H, scale, s); });
}

GFN_EXPORT int gfn_cross_attn_bwd(const void *q, const void *k, const void *v, const void *out, const float *lse, const void *dout, int dtype,
                                  int B, int Nq, int Nk, int H, int D, float scale, void *dq, void *dk, void *dv, gfn_stream_t stream) {
    const char *what = "gfn_cross_attn_bwd";
    if (int rc = check_args(what, dtype, B, Nq, Nk, H, D, scale, {q, k, v, out, dout, dq, dk, dv})) return rc;
    if (B == 0) return GFN_OK;
    hipStream_t s = (hipStream_t)stream;
    if (Nq == 0) {  // no query: dK = dV = 0
        if (!dk || !dv) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: null pointer", what);
        const size_t bytes = (size_t)B * Nk * H * 8 * (dtype == GFN_F32 ? 4 : 2);
        if (hipMemsetAsync(dk, 0, bytes, s) != hipSuccess || hipMemsetAsync(dv, 0, bytes, s) != hipSuccess)
            return gfn::fail(GFN_ERR_LAUNCH, "%s: hipMemsetAsync failed", what);
        return GFN_OK;
    }
    if (!lse || ((uintptr_t)lse & 3)) return gfn::fail(GFN_ERR_INVALID_ARG, "%s: lse missing or not 4-byte aligned", what);
    if (dtype == GFN_F32) return launch_bwd<float>(q, k, v, lse, dout, dq, dk, dv, B, Nq, Nk, H, scale, s);
    return with_elem16(dtype, [&](auto e) { return launch_bwd<decltype(e)>(q, k, v, lse, dout, dq, dk, dv, B, Nq, Nk, H, scale, s); });
}
