// kde.hip -- streaming Gaussian kernel density for gfx950.
//
// Replaces utils/kde.py:4-13 (called from GFNet.sample, model/network.py:408):
//   density[n] = sum_m exp(-|x_n - y_m|^2 / (2 std^2)),   y = x[::down]
// The reference materialises the N x M distance matrix through torch.cdist (1.6 GB in fp32 at
// N = M = 20 000, or an fp16 matrix that is 12 % off); here nothing but the N sums is written.
// The op is compute bound (N*M exponentials, 2*N*16 bytes of traffic): one thread per query,
// the reference points y_m are wave-uniform (scalar loads / SGPR operands), two points per step
// so that the subtract/multiply/fma chain packs into v_pk_*_f32, coordinates pre-scaled by
// sqrt(log2(e)/(2 std^2)) so that the exponential is a bare v_exp_f32 (2^x).
// Distances use the direct difference form (what cdist approximates with its |a|^2+|b|^2-2ab
// matrix product); fp32 accumulation.  When N is too small to fill the chip the M range is split
// over blockIdx.y and the partial sums are reduced by a second tiny kernel (deterministic, no
// float atomics).
#include "corr_common.h"  // split3; with it elem16.h, reduce.h and common.h: f32x16, acc_row
#include <cstdlib>

namespace {

using gfn::f32x2;
using gfn::other_half;

constexpr int kKdeThreads = 256;

// Pre-pass (D = 4): scale the coordinates once and lay the reference points out as pairs,
// ys[bt][m/2][d][2], so that the main loop reads (a_d, c_d) of two points as one SGPR pair and
// every arithmetic step is one packed v_pk_*_f32.  An odd tail is padded with a far-away point
// (its term is exp2(-inf) = 0).
__global__ __launch_bounds__(256) void kde4_prescale_kernel(const float *__restrict__ x, const float *__restrict__ y,
                                                            float *__restrict__ xs, float *__restrict__ ys, int N,
                                                            int M, long y_rs, long y_bs, float scale, int Bt, int round_fp16 = 0) {
    const int Mp = (M + 1) & ~1;
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long nx = (long)Bt * N * 4, ny = (long)Bt * Mp * 4;
    // round_fp16: the reference hands kde() fp16 coordinates (network.py:408, kde.py:6); rounding here saves the caller two
    // elementwise launches
    auto rnd = [&](float v) { return round_fp16 ? (float)(_Float16)v : v; };  // round to nearest even, like torch .half()
    if (idx < nx) xs[idx] = rnd(x[idx]) * scale;
    if (idx < ny) {
        const int bt = (int)(idx / ((long)Mp * 4));
        const long r = idx - (long)bt * Mp * 4;
        const int pair = (int)(r >> 3), d = (int)((r >> 1) & 3), which = (int)(r & 1);
        const int m = pair * 2 + which;
        ys[idx] = (m < M) ? rnd(y[(size_t)bt * y_bs + (size_t)m * y_rs + d]) * scale : 1e18f;
    }
}

// xs: (Bt, N, 4) pre-scaled queries; ys: (Bt, Mp/2, 4, 2) pre-scaled point pairs;
// part: (Bt, MS, N) partial sums (MS = gridDim.y) or the output itself when MS == 1.
__global__ __launch_bounds__(kKdeThreads) void kde4_kernel(const float *__restrict__ xs, const float *__restrict__ ys,
                                                           float *__restrict__ part, int N, int Mp) {
    const int bt = blockIdx.z;
    const int n = blockIdx.x * kKdeThreads + threadIdx.x;
    const int MS = gridDim.y, ms = blockIdx.y;
    const int npair = Mp >> 1;
    const int per = (npair + MS - 1) / MS;
    const int p0 = ms * per, p1 = min(npair, p0 + per);
    const float4 xv = (n < N) ? reinterpret_cast<const float4 *>(xs)[(size_t)bt * N + n] : make_float4(0, 0, 0, 0);
    const f32x2 x0 = {xv.x, xv.x}, x1 = {xv.y, xv.y}, x2 = {xv.z, xv.z}, x3 = {xv.w, xv.w};
    const f32x2 *yp = reinterpret_cast<const f32x2 *>(ys) + (size_t)bt * npair * 4;
    f32x2 acc = {0.f, 0.f};
#pragma unroll 4
    for (int p = p0; p < p1; ++p) {
        // wave-uniform address -> scalar loads; each operand below is an SGPR pair
        const f32x2 d0 = x0 - yp[(size_t)p * 4 + 0];
        const f32x2 d1 = x1 - yp[(size_t)p * 4 + 1];
        const f32x2 d2 = x2 - yp[(size_t)p * 4 + 2];
        const f32x2 d3 = x3 - yp[(size_t)p * 4 + 3];
        f32x2 sq = d0 * d0;
        sq = __builtin_elementwise_fma(d1, d1, sq);
        sq = __builtin_elementwise_fma(d2, d2, sq);
        sq = __builtin_elementwise_fma(d3, d3, sq);
        f32x2 e;
        e.x = __builtin_amdgcn_exp2f(-sq.x);
        e.y = __builtin_amdgcn_exp2f(-sq.y);
        acc += e;
    }
    if (n < N) part[((size_t)bt * MS + ms) * N + n] = acc.x + acc.y;
}

// ---- spatially culled variant -------------------------------------------------------------------
// With std = 0.1 on coordinates in [-1,1] a term is below 2^-32 once the points are 6.7 std apart,
// and the matches lie on a 2-D manifold of the 4-D space, so most of the N x M pairs contribute
// nothing.  The caller sorts queries and reference points along a Morton curve of the A-image
// coordinates (gfn_kde_morton_keys + a sort); every 64 consecutive points then form a compact block.
// Each wave owns one block of 64 queries, keeps its bounding box, and skips every reference block
// whose box is farther than the cut-off (kde4_mfma_kernel below).  Truncation error < M * 2^-32
// absolute (densities are >= 1 from the self term).
constexpr float kKdeCutoffLog2 = 32.f;

// 16-bit position of a point along a Hilbert curve over the A-image coordinates (8 bits per axis; the B-image position follows
// it for inliers).  A Z-order (Morton) key was used first: runs of 64 consecutive points that straddle a quadrant boundary
// of the Z curve have huge bounding boxes and are never culled; the Hilbert curve is continuous, its runs stay compact.
__device__ __forceinline__ unsigned curve_key16(float4 v) {
    unsigned x = (unsigned)fminf(fmaxf((v.x + 1.f) * 128.f, 0.f), 255.f);
    unsigned y = (unsigned)fminf(fmaxf((v.y + 1.f) * 128.f, 0.f), 255.f);
    unsigned d = 0;
#pragma unroll
    for (unsigned s = 128; s > 0; s >>= 1) {
        const unsigned rx = (x & s) ? 1u : 0u, ry = (y & s) ? 1u : 0u;
        d += s * s * ((3u * rx) ^ ry);
        if (!ry) {  // rotate the quadrant
            if (rx) { x = 255u - x; y = 255u - y; }
            const unsigned t = x; x = y; y = t;
        }
    }
    return d;
}

__global__ __launch_bounds__(256) void kde4_morton_kernel(const float *__restrict__ x, int *__restrict__ keys, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    keys[i] = (int)curve_key16(reinterpret_cast<const float4 *>(x)[i]);
}

// Stable sort of one row of points by its 16-bit curve key, one 1024-thread workgroup per row: two least-significant-digit
// passes of 8 bits.  Every wave owns one contiguous sixteenth of the row.  Per pass: (A) each wave counts the digits of its
// segment (LDS atomics on its own row of a [wave][digit] table); (B) one exclusive scan turns the table into the first
// output position of every (digit, wave) -- digits major, waves minor, which is exactly the stable order; (C) each wave walks
// its segment again IN ORDER, 64 elements at a time: an element's position is its (digit, wave) cursor + the number of
// lower lanes with the same digit (eight ballots), and the first lane of every digit group advances the cursor.  Step (C)
// needs no workgroup barrier (a wave's LDS operations are ordered), so a pass has three barriers in total -- the first
// version re-synchronised the workgroup four times per 1024 elements and took 0.13 ms; this one takes ~0.03 ms.  The
// result is the permutation a stable library sort gives (torch.sort of the 32 x 20000 keys: 0.53 ms in 76 launches).
constexpr int kSortThreads = 1024;
constexpr int kSortWaves = kSortThreads / 64;

__device__ __forceinline__ unsigned morton16(float4 v) { return curve_key16(v); }  // historical name: the sort key

__global__ __launch_bounds__(kSortThreads) void kde4_morton_sort_kernel(const float *__restrict__ x, float *__restrict__ xsorted,
                                                                        int *__restrict__ perm, unsigned *__restrict__ tmp, int N) {
    __shared__ unsigned cur[kSortWaves][256];  // (A) counts, (B)/(C) next output position of (wave, digit)
    __shared__ unsigned tot[256];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float4 *xr = reinterpret_cast<const float4 *>(x) + (size_t)row * N;
    unsigned *t0 = tmp + (size_t)row * N;  // pass-0 output: index (24 bits; N <= 65535*16) | high digit of the key << 24
    const int per_wave = ((N + kSortWaves - 1) / kSortWaves + 63) & ~63;
    const int w0 = wave * per_wave, w1 = min(N, w0 + per_wave);
    for (int pass = 0; pass < 2; ++pass) {
        for (int e = tid; e < kSortWaves * 256; e += kSortThreads) (&cur[0][0])[e] = 0;
        __syncthreads();
        // ---- (A) digit counts of this wave's segment
        constexpr int UF = 4;  // loads in flight per lane: a wave's walk is otherwise one exposed L2 / DRAM round trip per 64 elements
        for (int n0 = w0 + lane; n0 < w1; n0 += 64 * UF) {
            float4 pv[UF];
            unsigned tv[UF];
#pragma unroll
            for (int q = 0; q < UF; ++q) {
                const int n = min(n0 + 64 * q, N - 1);
                if (pass == 0) pv[q] = xr[n];
                else tv[q] = t0[n];
            }
#pragma unroll
            for (int q = 0; q < UF; ++q) {
                if (n0 + 64 * q < w1) atomicAdd(&cur[wave][pass == 0 ? morton16(pv[q]) & 255u : tv[q] >> 24], 1u);
            }
        }
        __syncthreads();
        // ---- (B) exclusive scan, digits major / waves minor
        if (tid < 256) {
            unsigned s = 0;
#pragma unroll
            for (int w = 0; w < kSortWaves; ++w) s += cur[w][tid];
            tot[tid] = s;
        }
        __syncthreads();
        if (wave == 0) {  // 256 totals, four per lane
            unsigned c[4], s = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) { c[q] = tot[lane * 4 + q]; s += c[q]; }
            unsigned incl = s;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned v = __shfl_up(incl, o);
                if (lane >= o) incl += v;
            }
            unsigned run = incl - s;
#pragma unroll
            for (int q = 0; q < 4; ++q) { tot[lane * 4 + q] = run; run += c[q]; }
        }
        __syncthreads();
        if (tid < 256) {
            unsigned run = tot[tid];
#pragma unroll
            for (int w = 0; w < kSortWaves; ++w) {
                const unsigned c = cur[w][tid];
                cur[w][tid] = run;
                run += c;
            }
        }
        __syncthreads();
        // ---- (C) ordered scatter of this wave's segment
        for (int nb = w0; nb < w1; nb += 64 * UF) {
            float4 pv[UF];
            unsigned tv[UF];
#pragma unroll
            for (int q = 0; q < UF; ++q) {
                const int n = min(nb + 64 * q + lane, N - 1);
                if (pass == 0) pv[q] = xr[n];
                else tv[q] = t0[n];
            }
#pragma unroll
            for (int q = 0; q < UF; ++q) {
                const int n = nb + 64 * q + lane;
                const bool live = n < w1;
                const unsigned key = pass == 0 ? morton16(pv[q]) : 0u, packed = pass == 0 ? 0u : tv[q];
                const int src = pass == 0 ? n : (int)(packed & 0xFFFFFFu);
                const unsigned digit = live ? (pass == 0 ? key & 255u : packed >> 24) : 0u;
                unsigned long long peers = __ballot(live);  // lanes of this wave with the same digit
#pragma unroll
                for (int bit = 0; bit < 8; ++bit) {
                    const unsigned long long m = __ballot((digit >> bit) & 1u);
                    peers &= ((digit >> bit) & 1u) ? m : ~m;
                }
                const unsigned below = (unsigned)__popcll(peers & ((1ull << lane) - 1ull));
                if (live) {
                    const unsigned pos = cur[wave][digit] + below;
                    if (pass == 0) {
                        t0[pos] = (unsigned)src | ((key >> 8) << 24);
                    } else {
                        perm[(size_t)row * N + pos] = src;
                        reinterpret_cast<float4 *>(xsorted)[(size_t)row * N + pos] = xr[src];
                    }
                }
                // all lanes have read the cursor (the reads above precede this write in the wave's LDS order)
                if (live && below == 0) cur[wave][digit] += (unsigned)__popcll(peers);
            }
        }
        __syncthreads();  // pass 1 reads what other waves wrote to t0
    }
}

// ys: pre-scaled point pairs (Bt, Mp/2, 4, 2) as written by kde4_prescale_kernel; box: (Bt, nblk, 8) =
// min[4], max[4] of each block of 64 reference points (32 pairs).  One wave per block.
// box32 (optional): (Bt, 2*nblk, 8) the same for the two 32-point halves of every block (the matrix-core kernel culls per
// 32 x 32 tile).
__global__ __launch_bounds__(256) void kde4_bbox_kernel(const float *__restrict__ ys, float *__restrict__ box, float *__restrict__ box32,
                                                        int M, int Mp, int Bt) {
    const int lane = threadIdx.x & 63;
    const int nblk = (Mp + 63) >> 6;
    const long wid = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wid >= (long)Bt * nblk) return;
    const int bt = (int)(wid / nblk), blk = (int)(wid - (long)bt * nblk);
    const int m = blk * 64 + lane;
    float lo[4], hi[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const float v = (m < M) ? ys[((size_t)bt * (Mp >> 1) + (m >> 1)) * 8 + d * 2 + (m & 1)] : 0.f;
        lo[d] = (m < M) ? v : 3e38f;
        hi[d] = (m < M) ? v : -3e38f;
    }
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) {
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            lo[d] = fminf(lo[d], __shfl_xor(lo[d], o));
            hi[d] = fmaxf(hi[d], __shfl_xor(hi[d], o));
        }
    }
    if (box32) {
        const int l = lane & 31;
        float *b32 = box32 + (wid * 2 + (lane >> 5)) * 8;
        if (l < 4) b32[l] = lo[l];
        else if (l < 8) b32[l] = hi[l - 4];
    }
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        lo[d] = fminf(lo[d], other_half(lo[d]));
        hi[d] = fmaxf(hi[d], other_half(hi[d]));
    }
    if (lane < 4) box[wid * 8 + lane] = lo[lane];
    else if (lane < 8) box[wid * 8 + lane] = hi[lane - 4];
}

// ---- matrix-core culled kernel -------------------------------------------------------------------
// The exponent |x-y|^2 = |x|^2 + |y|^2 - 2 x.y of a 32 x 32 tile of (query, point) pairs is one pair of
// v_mfma_f32_32x32x16_bf16: every fp32 coordinate is split into three bf16 pieces (8+8+8 mantissa bits,
// exact), the products that matter (h.h, h.l, l.h, h.ll, ll.h, l.l per axis: 24 slots) and the squared
// norms (3 + 3 slots against ones) fill K = 32, so D comes out as the exponent itself (error ~1e-5 from the
// fp32 accumulation of +-300 magnitudes, i.e. 1e-5 relative on a term).  What is left on the VALU per pair
// is v_exp_f32 and half a packed add -- 2.4x fewer vector cycles than the difference form (kde4_kernel).
using gfn::bf16x8;
using gfn::f32x16;
using gfn::split3;  // (h, l, ll here are its h, m, l)

// Operand images: op[(bt*T + tile)*4 + g][row 0..31] = 8 bf16, g = MFMA (0/1) * 2 + k half; one thread per point.
//   MFMA 0  k 0-7 : A xh  nxh 1 nxl 1   B yh  1 nyh 1 nyl      k 8-15: A xh xl    B yl yh
//   MFMA 1  k 0-7 : A xh  xll           B yll yh               k 8-15: A xl  nxll 1 0 0   B yl  1 nyll 0 0
// with y = -2 * (scaled point), nx = |x|^2, ny = |point|^2 (scaled).  The large terms (h.h products, leading pieces of
// the norms) sit in ONE accumulation so that no intermediate sum is large (a +-400 intermediate cost 4e-5 relative on a
// term; this order 1e-5).  Padding points get ny = 1e30 (term 0).
__global__ __launch_bounds__(256) void kde4_operands_kernel(const float *__restrict__ xs, const float *__restrict__ ys,
                                                            bf16x8 *__restrict__ aop, bf16x8 *__restrict__ bop,
                                                            unsigned long long *__restrict__ colacc, int N, int M, int Mp,
                                                            int NT, int MT, int Bt) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long na = (long)Bt * NT * 32, nb = (long)Bt * MT * 32;
    // colacc (symmetric call): the column accumulators start at 0 -- the launch has na >= Bt * N threads, which saves a memset
    if (colacc && idx < (long)Bt * N) colacc[idx] = 0ull;
    const __bf16 one = (__bf16)1.f, zero = (__bf16)0.f;
    if (idx < na) {
        const int bt = (int)(idx / ((long)NT * 32)), n = (int)(idx - (long)bt * NT * 32);
        __bf16 h[4], l[4], ll[4], nh = zero, nl = zero, nll = zero;
        float nx = 0.f;
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const float v = n < N ? xs[((size_t)bt * N + n) * 4 + d] : 0.f;
            split3(v, h[d], l[d], ll[d]);
            nx = fmaf(v, v, nx);
        }
        split3(nx, nh, nl, nll);
        bf16x8 *dst = aop + ((size_t)bt * NT + (n >> 5)) * 4 * 32 + (n & 31);
        dst[0] = bf16x8{h[0], h[1], h[2], h[3], nh, one, nl, one};
        dst[32] = bf16x8{h[0], h[1], h[2], h[3], l[0], l[1], l[2], l[3]};
        dst[64] = bf16x8{h[0], h[1], h[2], h[3], ll[0], ll[1], ll[2], ll[3]};
        dst[96] = bf16x8{l[0], l[1], l[2], l[3], nll, one, zero, zero};
    }
    if (idx < nb) {
        const int bt = (int)(idx / ((long)MT * 32)), m = (int)(idx - (long)bt * MT * 32);
        __bf16 h[4], l[4], ll[4], nh, nl, nll;
        float ny = 0.f;
        const bool real = m < M;
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const float v = real ? ys[((size_t)bt * (Mp >> 1) + (m >> 1)) * 8 + d * 2 + (m & 1)] : 0.f;
            split3(-2.f * v, h[d], l[d], ll[d]);
            ny = fmaf(v, v, ny);
        }
        split3(real ? ny : 1e30f, nh, nl, nll);
        bf16x8 *dst = bop + ((size_t)bt * MT + (m >> 5)) * 4 * 32 + (m & 31);
        dst[0] = bf16x8{h[0], h[1], h[2], h[3], one, nh, one, nl};
        dst[32] = bf16x8{l[0], l[1], l[2], l[3], h[0], h[1], h[2], h[3]};
        dst[64] = bf16x8{ll[0], ll[1], ll[2], ll[3], h[0], h[1], h[2], h[3]};
        dst[96] = bf16x8{l[0], l[1], l[2], l[3], one, nll, zero, zero};
    }
}

// One wave = 64 queries (two 32-row tiles); reference blocks of 64 points (two 32-column tiles) culled by their
// bounding boxes.  Lane (col = lane&31, kh = lane>>5) accumulates its column of every tile;
// the 32 columns are summed across lanes once at the end.
//   * the cull runs 64 blocks at a time: lane L tests block base+L against the wave's query box, one ballot gives the
//     survivor mask, and the wave then walks the set bits (the per-block test cost 20 vector instructions and one exposed
//     L2 round trip for each of the 313 blocks of a 20000-point row; now 5 of each);
//   * the operands of the next surviving block are requested before the current block's MFMAs issue;
//   * both column tiles' MFMAs are issued before the first exponential, so the matrix pipe works under the v_exp stream;
//   * this file is compiled with -amdgpu-mfma-vgpr-form: the products land in VGPRs, not in AGPRs that cost one
//     v_accvgpr_read per exponential (build.py).
// What bounds the kernel is v_exp_f32 (quarter rate: 16 cycles per wave instruction) on the surviving pairs.
//
// SYM (queries == points, the call GFNet.sample makes): exp(-|x_i - x_j|^2) is symmetric, so a wave only visits the
// blocks p >= its own block q.  A tile with p > q feeds the row sums of its 64 queries as before AND, summed down the
// lane's column, the densities of the 64 points of block p -- half the exponentials.  The column sums of all waves meet
// in one accumulator per point; to keep the result independent of the order in which waves arrive they are added as
// 2^-40 fixed-point integers (integer addition is associative; densities < 2^23 fit 64 bits), and kde_combine_kernel
// adds the two halves.  The diagonal block p == q holds both (i,j) and (j,i) and feeds row sums only.
//
// Dispatch order: in the symmetric kernel the wave of query block q visits p >= q only, so a workgroup's work falls from about twice
// the mean at the first 256 queries of a row to nothing at the last.  A (x, ms, bt) grid is handed out x fastest and bt slowest:
// the heaviest workgroups of the last rows start when the chip is already draining (2.5 rounds of workgroups at 32 x 20000) and
// the launch ends on them.  The grid is therefore one-dimensional and kde_wg() maps the linear id with x OUTERMOST: every row's
// heavy workgroups go out first, the nearly empty ones fill the tail.  (The hardware promises no order; the map is a bijection
// and waves are independent, so only the time depends on it.)
struct KdeWg { int x, ms, bt; };
__device__ __forceinline__ KdeWg kde_wg(unsigned id, int MS, int Bt) {
    const unsigned r = id / (unsigned)Bt;
    // the divisions run on the vector unit; their (uniform) results belong in scalar registers: the kernel has no VGPR to spare
    return KdeWg{__builtin_amdgcn_readfirstlane((int)(r / (unsigned)MS)), __builtin_amdgcn_readfirstlane((int)(r % (unsigned)MS)),
                 __builtin_amdgcn_readfirstlane((int)(id % (unsigned)Bt))};
}
// Column sums (SYM): a block's column value leaves as one 64-bit atomic per lane at the end of the block, and the wait for the next
// block's operands (vmcnt(0)) then also covers that atomic's round trip.  Parking the values in a per-wave LDS ring of 8 blocks
// and issuing them back to back behind a later block's operand prefetch, so that they retire under its MFMAs and exponentials, was
// built and measured level on top of the map (profiles/kde_dispatch.md); it is not kept.
constexpr float kKdeFixScale = 1099511627776.f;  // 2^40
template <bool SYM>
__global__ __launch_bounds__(kKdeThreads, 4) void kde4_mfma_kernel(const float *__restrict__ xs, const bf16x8 *__restrict__ aop,
                                                                const bf16x8 *__restrict__ bop, const float *__restrict__ box,
                                                                float *__restrict__ part, unsigned long long *__restrict__ colacc,
                                                                int N, int Mp, int NT, int MT, int MS, int Bt) {
    const KdeWg wg = kde_wg(blockIdx.x, MS, Bt);
    const int bt = wg.bt, ms = wg.ms;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // scalar, and q0, qblk, b0 with it
    const int q0 = wg.x * kKdeThreads + wave * 64;
    if (q0 >= N) return;
    const int n = q0 + lane;
    const int nblk = (Mp + 63) >> 6;
    const int per = (nblk + MS - 1) / MS;
    const int qblk = q0 >> 6;
    const int b0 = SYM ? max(ms * per, qblk) : ms * per, b1 = min(nblk, ms * per + per);
    const float4 xv = (n < N) ? reinterpret_cast<const float4 *>(xs)[(size_t)bt * N + n] : make_float4(0, 0, 0, 0);
    float qlo[4] = {xv.x, xv.y, xv.z, xv.w}, qhi[4] = {xv.x, xv.y, xv.z, xv.w};
    if (n >= N) {
#pragma unroll
        for (int d = 0; d < 4; ++d) { qlo[d] = 3e38f; qhi[d] = -3e38f; }
    }
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) {  // lanes 0-31 / 32-63: the two row tiles
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            qlo[d] = fminf(qlo[d], __shfl_xor(qlo[d], o));
            qhi[d] = fmaxf(qhi[d], __shfl_xor(qhi[d], o));
        }
    }
    float ql0[4], qh0[4], ql1[4], qh1[4];  // wave-uniform boxes of row tile 0 / 1 (scalar registers)
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        ql0[d] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(qlo[d]), 0));
        qh0[d] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(qhi[d]), 0));
        ql1[d] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(qlo[d]), 32));
        qh1[d] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(qhi[d]), 32));
    }
    const int col = lane & 31, kh = lane >> 5;
    unsigned long long *cacc = SYM ? colacc + (size_t)bt * N : nullptr;
    const bf16x8 *ap = aop + ((size_t)bt * NT + (q0 >> 5)) * 128 + kh * 32 + col;
    const bf16x8 a00 = ap[0], a01 = ap[64], a10 = ap[128], a11 = ap[192];  // [row tile][MFMA]
    const bf16x8 *bp = bop + (size_t)bt * MT * 128 + kh * 32 + col;
    const float4 *bx = reinterpret_cast<const float4 *>(box + (size_t)bt * nblk * 16);  // 32-point tile boxes: [tile][lo4, hi4]
    f32x2 acc0[8], acc1[8];  // [r/2] = rows r, r+1 of the lane's column (packed adds)
#pragma unroll
    for (int r = 0; r < 8; ++r) acc0[r] = f32x2{0.f, 0.f}, acc1[r] = f32x2{0.f, 0.f};
    const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    auto near = [&](const float (&ql)[4], const float (&qh)[4], const float4 lo, const float4 hi) {
        const float g0 = fmaxf(fmaxf(ql[0] - hi.x, lo.x - qh[0]), 0.f), g1 = fmaxf(fmaxf(ql[1] - hi.y, lo.y - qh[1]), 0.f);
        const float g2 = fmaxf(fmaxf(ql[2] - hi.z, lo.z - qh[2]), 0.f), g3 = fmaxf(fmaxf(ql[3] - hi.w, lo.w - qh[3]), 0.f);
        return !(fmaf(g3, g3, fmaf(g2, g2, fmaf(g1, g1, g0 * g0))) > kKdeCutoffLog2);
    };
    for (int base = b0; base < b1; base += 64) {
        // lane L tests the four 32 x 32 tiles of (this wave's two row tiles) x (block base+L's two column tiles)
        bool k00 = false, k01 = false, k10 = false, k11 = false;  // [row tile][column tile]
        if (base + lane < b1) {
            const float4 *t = bx + (size_t)(base + lane) * 4;
            const float4 lo0 = t[0], hi0 = t[1], lo1 = t[2], hi1 = t[3];
            k00 = near(ql0, qh0, lo0, hi0); k01 = near(ql0, qh0, lo1, hi1);
            k10 = near(ql1, qh1, lo0, hi0); k11 = near(ql1, qh1, lo1, hi1);
        }
        const unsigned long long m00 = __ballot(k00), m01 = __ballot(k01), m10 = __ballot(k10), m11 = __ballot(k11);
        unsigned long long mask = m00 | m01 | m10 | m11;
        if (!mask) continue;
        bf16x8 c0, c1, c2, c3;  // [column tile][MFMA] of the current block
        int cur = base + __builtin_ctzll(mask), nxt = 0;
        {
            const bf16x8 *b = bp + (size_t)cur * 256;
            mask &= mask - 1;
            c0 = b[0], c1 = b[64], c2 = b[128], c3 = b[192];
        }
        // land the first block here: otherwise every MFMA of the loop is made to wait for the prefetch as well
        asm volatile("" : "+v"(c0), "+v"(c1), "+v"(c2), "+v"(c3));
        while (true) {
            const bool more = mask != 0;
            bf16x8 n0 = c0, n1 = c1, n2 = c2, n3 = c3;
            if (more) {
                nxt = base + __builtin_ctzll(mask);
                const bf16x8 *b = bp + (size_t)nxt * 256;
                mask &= mask - 1;
                n0 = b[0], n1 = b[64], n2 = b[128], n3 = b[192];
            }
            const int bit = cur - base;
            const bool s00 = (m00 >> bit) & 1, s01 = (m01 >> bit) & 1, s10 = (m10 >> bit) & 1, s11 = (m11 >> bit) & 1;  // scalar
            // column tile 0 then column tile 1, each: MFMAs, then its exponentials -- the products of the two tiles share
            // registers (4 waves per SIMD instead of 3); other waves' exponentials run under this wave's MFMAs
            float cs0 = 0.f, cs1 = 0.f;  // SYM: this lane's column of the two column tiles (one register each: the pair sums are folded
                                         // per column tile -- as f32x2 they were 4 more live registers and the kernel spilled 5 at 128)
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) {
                const bool sa = ct ? s01 : s00, sb = ct ? s11 : s10;
                const bf16x8 ca = ct ? c2 : c0, cb = ct ? c3 : c1;
                f32x16 e0 = zero16, e1 = zero16;
                if (sa) {
                    e0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a00, ca, zero16, 0, 0, 0);
                    e0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a01, cb, e0, 0, 0, 0);
                }
                if (sb) {
                    e1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a10, ca, zero16, 0, 0, 0);
                    e1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a11, cb, e1, 0, 0, 0);
                }
                f32x2 cs = f32x2{0.f, 0.f};
                if (sa) {
#pragma unroll
                    for (int r = 0; r < 8; ++r) {
                        const f32x2 x = f32x2{__builtin_amdgcn_exp2f(-e0[2 * r]), __builtin_amdgcn_exp2f(-e0[2 * r + 1])};
                        acc0[r] += x;
                        if (SYM) cs += x;
                    }
                }
                if (sb) {
#pragma unroll
                    for (int r = 0; r < 8; ++r) {
                        const f32x2 x = f32x2{__builtin_amdgcn_exp2f(-e1[2 * r]), __builtin_amdgcn_exp2f(-e1[2 * r + 1])};
                        acc1[r] += x;
                        if (SYM) cs += x;
                    }
                }
                if (ct) cs1 = cs.x + cs.y; else cs0 = cs.x + cs.y;
            }
            if (SYM && cur != qblk) {  // wave-uniform
                // rows 4kh.. of both row tiles are in this lane, the other half of the rows in lane ^ 32
                float s0 = cs0, s1 = cs1;
                s0 += other_half(s0);
                s1 += other_half(s1);
                const float sv = kh ? s1 : s0;  // lanes 0-31: column tile 0, lanes 32-63: column tile 1
                const int pt = cur * 64 + lane;
                if (pt < N) atomicAdd(cacc + pt, (unsigned long long)(sv * kKdeFixScale));
            }
            if (!more) break;
            c0 = n0, c1 = n1, c2 = n2, c3 = n3;
            cur = nxt;
        }
    }
    // sum the 32 columns (lanes with the same kh), then lanes col == 0 hold rows (r&3) + 8(r>>2) + 4kh of each row tile
    float *dst = part + ((size_t)bt * MS + ms) * N;
    // the butterfly's five permute indices are worked out HERE, from a lane id the compiler cannot trace back: with __shfl_xor it
    // computed them in front of the main loop and carried them across it in scratch (5 spilled registers at the 128 cap)
    int lane_late = lane;
    asm volatile("" : "+v"(lane_late));
    auto xor_lane = [&](float v, int o) {
        return __int_as_float(__builtin_amdgcn_ds_bpermute((lane_late ^ o) << 2, __float_as_int(v)));
    };
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        float v0 = acc0[r >> 1][r & 1], v1 = acc1[r >> 1][r & 1];
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) {
            v0 += xor_lane(v0, o);
            v1 += xor_lane(v1, o);
        }
        const int row = gfn::acc_row(r, kh);
        if (col == 0 && q0 + row < N) dst[q0 + row] = v0;
        if (col == 0 && q0 + 32 + row < N) dst[q0 + 32 + row] = v1;
    }
}

// any point dimension D (the reference never uses anything but 4)
__global__ __launch_bounds__(kKdeThreads) void kde_generic_kernel(const float *__restrict__ x,
                                                                  const float *__restrict__ y, float *__restrict__ part,
                                                                  int N, int M, int D, long y_rs, long y_bs,
                                                                  float scale) {
    const int bt = blockIdx.z;
    const int n = blockIdx.x * kKdeThreads + threadIdx.x;
    const int MS = gridDim.y, ms = blockIdx.y;
    const int per = (M + MS - 1) / MS;
    const int m0 = ms * per, m1 = min(M, m0 + per);
    if (n >= N) return;
    const float *xn = x + ((size_t)bt * N + n) * D;
    const float *yb = y + (size_t)bt * y_bs;
    float acc = 0.f;
    for (int m = m0; m < m1; ++m) {
        float s = 0.f;
        for (int d = 0; d < D; ++d) {
            const float t = (xn[d] - yb[(size_t)m * y_rs + d]) * scale;
            s = fmaf(t, t, s);
        }
        acc += __builtin_amdgcn_exp2f(-s);
    }
    part[((size_t)bt * MS + ms) * N + n] = acc;
}

__global__ __launch_bounds__(256) void kde_reduce_kernel(const float *__restrict__ part, float *__restrict__ out, int N,
                                                         int MS, int Bt) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)Bt * N) return;
    const int bt = (int)(idx / N), n = (int)(idx - (long)bt * N);
    float s = 0.f;
    for (int k = 0; k < MS; ++k) s += part[((size_t)bt * MS + k) * N + n];  // fixed order: reproducible
    out[idx] = s;
}

// symmetric kernel: density = row sums (split-M partials, fixed order) + column sums (fixed point)
__global__ __launch_bounds__(256) void kde_combine_kernel(const float *__restrict__ part, const unsigned long long *__restrict__ colacc,
                                                          const int *__restrict__ perm, float *__restrict__ out, int N, int MS, int Bt) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)Bt * N) return;
    const int bt = (int)(idx / N), n = (int)(idx - (long)bt * N);
    float s = 0.f;
    for (int k = 0; k < MS; ++k) s += part[((size_t)bt * MS + k) * N + n];
    if (colacc) s += (float)((double)colacc[idx] * (1.0 / 1099511627776.0));
    out[perm ? (size_t)bt * N + perm[idx] : (size_t)idx] = s;  // perm: back to the caller's order (sorted position -> original index)
}

// GFNet.sample's elementwise steps (model/network.py:391-393, 409-410)
__global__ __launch_bounds__(256) void threshold_kernel(const float *__restrict__ c, float *__restrict__ out, long n, float thr) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = c[i] > thr ? 1.f : c[i];
}

__global__ __launch_bounds__(256) void balance_kernel(const float *__restrict__ density, float *__restrict__ p, long n,
                                                      float min_density, float floor_p, int round_fp16) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        float d = density[i];
        if (round_fp16) d = (float)(_Float16)d;  // kde(half=True) returns fp16 (kde.py:13)
        p[i] = d < min_density ? floor_p : 1.f / (d + 1.f);
    }
}

}  // namespace

GFN_EXPORT int gfn_threshold_certainty(const float *certainty, float *out, int64_t n, float thresh, gfn_stream_t stream) {
    if (!certainty || !out || n < 0) return gfn::fail(GFN_ERR_INVALID_ARG, "threshold_certainty: bad argument");
    if (n == 0) return GFN_OK;
    hipLaunchKernelGGL(threshold_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, certainty, out,
                       (long)n, thresh);
    return gfn::check_launch("threshold_kernel");
}

GFN_EXPORT int gfn_balance_weights(const float *density, float *p, int64_t n, float min_density, float floor_p, int round_fp16,
                                   gfn_stream_t stream) {
    if (!density || !p || n < 0) return gfn::fail(GFN_ERR_INVALID_ARG, "balance_weights: bad argument");
    if (n == 0) return GFN_OK;
    hipLaunchKernelGGL(balance_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, density, p,
                       (long)n, min_density, floor_p, round_fp16);
    return gfn::check_launch("balance_kernel");
}

GFN_EXPORT int gfn_kde_morton_keys(const float *x, int *keys, int64_t n, gfn_stream_t stream) {
    if (!x || !keys || n < 0 || ((uintptr_t)x & 15)) return gfn::fail(GFN_ERR_INVALID_ARG, "kde_morton_keys: bad argument");
    if (n == 0) return GFN_OK;
    hipLaunchKernelGGL(kde4_morton_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, keys, (long)n);
    return gfn::check_launch("kde4_morton_kernel");
}

GFN_EXPORT int gfn_kde_morton_sort(const float *x, float *x_sorted, int *perm, int *scratch, int Bt, int N, gfn_stream_t stream) {
    if (!x || !x_sorted || !perm || !scratch || Bt < 0 || N < 0 || (((uintptr_t)x | (uintptr_t)x_sorted) & 15))
        return gfn::fail(GFN_ERR_INVALID_ARG, "kde_morton_sort: bad argument");
    if (N > 65535 * 16) return gfn::fail(GFN_ERR_INVALID_ARG, "kde_morton_sort: row too long");
    if (Bt == 0 || N == 0) return GFN_OK;
    hipLaunchKernelGGL(kde4_morton_sort_kernel, dim3(Bt), dim3(kSortThreads), 0, (hipStream_t)stream, x, x_sorted, perm,
                       reinterpret_cast<unsigned *>(scratch), N);
    return gfn::check_launch("kde4_morton_sort_kernel");
}

// Scratch floats for gfn_kde_density_sorted: pre-scaled copies, block boxes, split-M partials.
GFN_EXPORT int64_t gfn_kde_sorted_scratch_floats(int Bt, int N, int M) {
    const int Mp = (M + 1) & ~1;
    const int64_t nblk = (Mp + 63) / 64, ntile = (N + 63) / 64 * 2;
    return (int64_t)Bt * N * 4 + (int64_t)Bt * Mp * 4 + Bt * nblk * 24 + (int64_t)Bt * 32 * N + 64 +
           (Bt * ntile * 32 + Bt * nblk * 64) * 16 + 8 +  // + the matrix-core operand images (64 B per query / point)
           (int64_t)Bt * N * 2 + 4;                        // + the fixed-point column sums of the symmetric kernel
}

// Density of spatially sorted 4-D points (see kde4_mfma_kernel): x (Bt,N,4), y (Bt,M,4), both in
// the order of their gfn_kde_morton_keys; out (Bt,N) in the order of x.
GFN_EXPORT int gfn_kde_density_sorted(const float *x, const float *y, float *out, const int *perm, int Bt, int N, int M, double std,
                                      int round_fp16, float *scratch, int64_t scratch_floats, gfn_stream_t stream) {
    if (!x || !y || !out || !scratch) return gfn::fail(GFN_ERR_INVALID_ARG, "kde_sorted: null pointer");
    if (Bt < 0 || N < 0 || M <= 0 || !(std > 0) || Bt > 65535) return gfn::fail(GFN_ERR_INVALID_ARG, "kde_sorted: bad argument");
    // the expanded exponent carries scale^2 (|x|^2 + |y|^2) = 0.72 * 8 (E / std)^2 in fp32 for coordinates within +-E: below 2048
    // (one ulp = 2^-13, 8.5e-5 on a term) up to E = 16 std.  Coordinates are image coordinates, E = 1: refuse what cannot hold 1e-4.
    if (std < GFN_KDE_SORTED_MIN_STD)
        return gfn::fail(GFN_ERR_INVALID_ARG, "kde_sorted: std=%g below %g, the expanded exponent loses the 1e-4 parity: use gfn_kde_density",
                         std, GFN_KDE_SORTED_MIN_STD);
    if (scratch_floats < gfn_kde_sorted_scratch_floats(Bt, N, M) || ((uintptr_t)scratch & 15) || ((uintptr_t)x & 15))
        return gfn::fail(GFN_ERR_SCRATCH, "kde_sorted: scratch too small or misaligned");
    if (Bt == 0 || N == 0) return GFN_OK;
    hipStream_t s = (hipStream_t)stream;
    const float scale = (float)sqrt(1.4426950408889634 / (2.0 * std * std));
    const int Mp = (M + 1) & ~1, nblk = (Mp + 63) / 64;
    float *xs = scratch, *ys = xs + (int64_t)Bt * N * 4, *box = ys + (int64_t)Bt * Mp * 4;
    float *box32 = box + (((int64_t)Bt * nblk * 8 + 3) & ~3);  // per 32-point tile
    float *part = box32 + (int64_t)Bt * nblk * 16;
    const long tot = (long)Bt * 4 * (N > Mp ? N : Mp);
    hipLaunchKernelGGL(kde4_prescale_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, x, y, xs, ys, N, M, 4L,
                       (long)M * 4, scale, Bt, round_fp16);
    hipLaunchKernelGGL(kde4_bbox_kernel, dim3((unsigned)(((long)Bt * nblk + 3) / 4)), dim3(256), 0, s, ys, box, box32, M, Mp, Bt);
    int MS = 1;
    {   // same rule as the dense kernel: enough workgroups for the chip, at least 8 blocks of points per split
        const long blocks = (long)Bt * ((N + kKdeThreads - 1) / kKdeThreads);
        while (blocks * MS < 2048 && nblk / (MS * 2) >= 8 && MS < 32) MS *= 2;
    }
    float *dst = (MS > 1 || perm) ? part : out;  // perm: results leave through the combine kernel, in the caller's order
    const bool sym = x == y && N == M;
    const int NT = (N + 63) / 64 * 2, MT = nblk * 2;
    float *opbase = part + (((int64_t)Bt * 32 * N + 3) & ~(int64_t)3);
    bf16x8 *aop = reinterpret_cast<bf16x8 *>(opbase), *bop = aop + (int64_t)Bt * NT * 128;
    const long npts = (long)Bt * 32 * (NT > MT ? NT : MT);
    // the symmetric kernel's fixed-point column sums; kde4_operands_kernel clears them
    unsigned long long *colacc = sym ? reinterpret_cast<unsigned long long *>(bop + (int64_t)Bt * MT * 128) : nullptr;
    hipLaunchKernelGGL(kde4_operands_kernel, dim3((unsigned)((npts + 255) / 256)), dim3(256), 0, s, xs, ys, aop, bop, colacc, N, M, Mp,
                       NT, MT, Bt);
    // one-dimensional grid, unpacked by kde_wg()
    const long nwg = (long)((N + kKdeThreads - 1) / kKdeThreads) * MS * Bt;
    if (nwg > 0x7fffffffL) return gfn::fail(GFN_ERR_INVALID_ARG, "kde_sorted: Bt * N too large for one launch");
    if (sym) {
        hipLaunchKernelGGL(kde4_mfma_kernel<true>, dim3((unsigned)nwg), dim3(kKdeThreads), 0, s, xs, aop, bop, box32, part, colacc, N, Mp,
                           NT, MT, MS, Bt);
        if (int e = gfn::check_launch("kde4_mfma_kernel")) return e;
        const long total = (long)Bt * N;
        hipLaunchKernelGGL(kde_combine_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, part, colacc, perm, out, N, MS, Bt);
        return gfn::check_launch("kde_combine_kernel");
    }
    hipLaunchKernelGGL(kde4_mfma_kernel<false>, dim3((unsigned)nwg), dim3(kKdeThreads), 0, s, xs, aop, bop, box32, dst, nullptr, N, Mp,
                       NT, MT, MS, Bt);
    if (int e = gfn::check_launch("kde4_mfma_kernel")) return e;
    if (MS > 1 || perm) {
        const long total = (long)Bt * N;
        hipLaunchKernelGGL(kde_combine_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, part, nullptr, perm, out, N, MS, Bt);
        return gfn::check_launch("kde_combine_kernel");
    }
    return GFN_OK;
}

GFN_EXPORT int gfn_kde_msplit(int Bt, int N, int M) {
    // enough blocks to fill 256 CUs x 8, but keep >= 512 reference points per split
    const long blocks = (long)Bt * ((N + kKdeThreads - 1) / kKdeThreads);
    int ms = 1;
    while (blocks * ms < 2048 && M / (ms * 2) >= 512) ms *= 2;
    return ms;
}

// Scratch floats gfn_kde_density wants for (Bt, N, M, D): the pre-scaled copies (D == 4) plus the
// split-M partial sums.  With less scratch the call still works (single pass / generic kernel).
GFN_EXPORT int64_t gfn_kde_scratch_floats(int Bt, int N, int M, int D) {
    const int MS = gfn_kde_msplit(Bt, N, M);
    int64_t n = MS > 1 ? (int64_t)Bt * MS * N : 0;
    if (D == 4) n += (int64_t)Bt * N * 4 + (int64_t)Bt * ((M + 1) & ~1) * 4;
    return n;
}

GFN_EXPORT int gfn_kde_density(const float *x, const float *y, float *out, int Bt, int N, int M, int D,
                               int64_t y_row_stride, int64_t y_batch_stride, double std, float *scratch,
                               int64_t scratch_floats, gfn_stream_t stream) {
    if (!x || !y || !out) return gfn::fail(GFN_ERR_INVALID_ARG, "kde: null pointer");
    if (Bt < 0 || N < 0 || M < 0 || D <= 0 || y_row_stride < D || !(std > 0))
        return gfn::fail(GFN_ERR_INVALID_ARG, "kde: bad argument Bt=%d N=%d M=%d D=%d std=%g", Bt, N, M, D, std);
    if (Bt > 65535) return gfn::fail(GFN_ERR_INVALID_ARG, "kde: batch > 65535");
    if (Bt == 0 || N == 0) return GFN_OK;
    hipStream_t s = (hipStream_t)stream;
    if (M == 0) {
        hipError_t e = hipMemsetAsync(out, 0, sizeof(float) * (size_t)Bt * N, s);
        return e == hipSuccess ? GFN_OK : gfn::fail(GFN_ERR_LAUNCH, "kde: memset failed");
    }
    if (!scratch) scratch_floats = 0;
    // exp(-d^2/(2 std^2)) = 2^(-(d*scale)^2),  scale = sqrt(log2(e) / (2 std^2))
    const float scale = (float)sqrt(1.4426950408889634 / (2.0 * std * std));
    const int Mp = (M + 1) & ~1;
    const int64_t pre = (int64_t)Bt * N * 4 + (int64_t)Bt * Mp * 4;
    const bool fast = D == 4 && scratch_floats >= pre && ((uintptr_t)scratch % 16) == 0;
    int64_t left = scratch_floats - (fast ? pre : 0);
    float *pscratch = scratch + (fast ? pre : 0);
    int MS = gfn_kde_msplit(Bt, N, M);
    if (MS > 1 && left < (int64_t)Bt * MS * N) MS = 1;  // no room for partials: single pass
    float *part = MS > 1 ? pscratch : out;
    const dim3 grid((N + kKdeThreads - 1) / kKdeThreads, MS, Bt);
    if (fast) {
        float *xs = scratch, *ys = scratch + (int64_t)Bt * N * 4;
        const long tot = (long)Bt * 4 * (N > Mp ? N : Mp);
        hipLaunchKernelGGL(kde4_prescale_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, x, y, xs, ys, N, M,
                           (long)y_row_stride, (long)y_batch_stride, scale, Bt);
        hipLaunchKernelGGL(kde4_kernel, grid, dim3(kKdeThreads), 0, s, xs, ys, part, N, Mp);
    } else {
        hipLaunchKernelGGL(kde_generic_kernel, grid, dim3(kKdeThreads), 0, s, x, y, part, N, M, D, (long)y_row_stride,
                           (long)y_batch_stride, scale);
    }
    if (int e = gfn::check_launch("kde_kernel")) return e;
    if (MS > 1) {
        const long total = (long)Bt * N;
        hipLaunchKernelGGL(kde_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, part, out, N, MS, Bt);
        return gfn::check_launch("kde_reduce_kernel");
    }
    return GFN_OK;
}
