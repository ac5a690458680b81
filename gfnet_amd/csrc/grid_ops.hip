// grid_ops.hip -- the small gather / elementwise kernels around the correlation on the hot path
// (gfx950).  All are HBM/L2-bound one-pass kernels with coalesced stores along the grid row.
//
//   gfn_refiner_input_fwd  ConvRefiner.forward prefix, model/network.py:533-555: the two
//                          grid_samples, the displacement embedding (1x1 conv of 2 channels) --
//                          written straight into the channel slices of the concat buffer `d`
//                          (the local-correlation kernel fills the last slice), so the
//                          reference's torch.cat copy of up to 417 channels disappears.
//   gfn_grid_sample_fwd    F.grid_sample(bilinear, zeros, align_corners=False): gfn_grid_sample_mode_fwd (grid_modes.hip)
//   gfn_interp_bilinear_fwd F.interpolate(mode='bilinear', align_corners=False), network.py:238-249,271-281
//   gfn_interp_bilinear_bwd its adjoint as a gather (training: the backbone's ViT-map resize under deterministic algorithms)
//   gfn_flow_update_fwd    displacement scaling / eval-time zeroing / accumulation, network.py:262-268
//   gfn_flow_update_resize_fwd  a scale's last flow update and the resize to the next grid through one LDS tile,
//                          network.py:262-268 + 271-281
//   gfn_match_post_fwd     certainty attenuation, sigmoid, out-of-range masking, clamp, warp
//                          assembly, network.py:332-338 + 358-384
#include "common.h"
#include "refiner_input.h"

namespace {

using namespace gfn_ri;

template <typename FT, bool KEEP>
__global__ __launch_bounds__(256) void refiner_input_kernel(RiArgs q, unsigned q_blocks, int banded) {
    if (banded) {  // 1-D grid, XCD-banded order (refiner_input.h)
        int b;
        unsigned x;
        if (ri_banded(blockIdx.x, q_blocks, q.Bh, b, x)) refiner_input_cell<FT, KEEP>(q, b, x * 256u + threadIdx.x);
        return;
    }
    refiner_input_cell<FT, KEEP>(q, ri_direction(q.B, q.Bh, blockIdx.y), blockIdx.x * 256u + threadIdx.x);
}

// ATen upsample_bilinear2d, align_corners=False: src = max(0, (dst+0.5)*in/out - 0.5).  One axis of one output: the two
// source indices and their weights.  Every bilinear resize below goes through interp_tap + bilerp, so they all round alike.
struct Tap {
    int i0, i1;
    float l, h;
};
__device__ __forceinline__ Tap interp_tap(int n_in, int n_out, int o) {
    const float s = (float)n_in / (float)n_out;
    float f = ((float)o + 0.5f) * s - 0.5f;
    f = f < 0.f ? 0.f : f;
    Tap t;
    t.i0 = (int)f;
    t.i1 = t.i0 + (t.i0 < n_in - 1 ? 1 : 0);
    t.l = f - (float)t.i0;
    t.h = 1.f - t.l;
    return t;
}
__device__ __forceinline__ float bilerp(const Tap &ty, const Tap &tx, float v00, float v01, float v10, float v11) {
    return ty.h * (tx.h * v00 + tx.l * v01) + ty.l * (tx.h * v10 + tx.l * v11);
}
__device__ __forceinline__ float interp_at(const float *pl, int H, int W, int Ho, int Wo, int y, int x) {
    const Tap ty = interp_tap(H, Ho, y), tx = interp_tap(W, Wo, x);
    return bilerp(ty, tx, pl[(size_t)ty.i0 * W + tx.i0], pl[(size_t)ty.i0 * W + tx.i1], pl[(size_t)ty.i1 * W + tx.i0],
                  pl[(size_t)ty.i1 * W + tx.i1]);
}

// ---- image resize + normalise ----------------------------------------------------
// ATen upsample_bicubic2d, align_corners=False: src = (dst+0.5)*in/out - 0.5 (not clamped), taps floor(src)-1 .. +2 with
// clamped indices, cubic convolution coefficients with A = -0.75, rows first then columns.  (sample_modes.h has the same
// polynomials in ATen's grid_sampler argument order, cubic_conv2((1 - t) + 1) for cubic2(2 - t): other bits, kept apart.)
__device__ __forceinline__ float cubic1(float x) { return ((-0.75f + 2.f) * x - (-0.75f + 3.f)) * x * x + 1.f; }
__device__ __forceinline__ float cubic2(float x) { return ((-0.75f * x - 5.f * -0.75f) * x + 8.f * -0.75f) * x - 4.f * -0.75f; }
__device__ __forceinline__ void cubic_coeffs(float t, float c[4]) {
    c[0] = cubic2(t + 1.f);
    c[1] = cubic1(t);
    c[2] = cubic1(1.f - t);
    c[3] = cubic2(2.f - t);
}

struct NormParams {
    float mean[3], std[3];
};

// in (B, >=3, H, W) with batch stride in_bs; out (B, 3, Ho, Wo) = (resize(in[:, :3]) - mean) / std.  One thread per output
// pixel (the three channels share indices and coefficients).  mode 0 bilinear, 1 bicubic.
__global__ __launch_bounds__(256) void resize_normalize_kernel(const float *__restrict__ in, long in_bs, float *__restrict__ out,
                                                               int B, int H, int W, int Ho, int Wo, int mode, NormParams np) {
    const long total = (long)B * Ho * Wo;
    const float sy = (float)H / (float)Ho, sx = (float)W / (float)Wo;
    const bool same = H == Ho && W == Wo;  // transforms.Resize returns the image untouched
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int x = (int)(idx % Wo);
        const long t = idx / Wo;
        const int y = (int)(t % Ho), b = (int)(t / Ho);
        const float *src = in + (size_t)b * in_bs;
        float v[3];
        if (same) {
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = src[((size_t)c * H + y) * W + x];
        } else if (mode == 0) {
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = interp_at(src + (size_t)c * H * W, H, W, Ho, Wo, y, x);
        } else {
            const float fy = ((float)y + 0.5f) * sy - 0.5f, fx = ((float)x + 0.5f) * sx - 0.5f;
            const float flx = floorf(fx), fly = floorf(fy);
            const int ix = (int)flx, iy = (int)fly;
            float cx[4], cy[4];
            cubic_coeffs(fx - flx, cx);
            cubic_coeffs(fy - fly, cy);
            int xs[4], ys[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                xs[i] = min(max(ix - 1 + i, 0), W - 1);
                ys[i] = min(max(iy - 1 + i, 0), H - 1);
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float *pl = src + (size_t)c * H * W;
                float rows[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float *r = pl + (size_t)ys[i] * W;
                    rows[i] = r[xs[0]] * cx[0] + r[xs[1]] * cx[1] + r[xs[2]] * cx[2] + r[xs[3]] * cx[3];
                }
                v[c] = rows[0] * cy[0] + rows[1] * cy[1] + rows[2] * cy[2] + rows[3] * cy[3];
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) out[(((size_t)b * 3 + c) * Ho + y) * Wo + x] = (v[c] - np.mean[c]) / np.std[c];
    }
}

// Four consecutive outputs of one row per thread (one 16-byte store per plane when the row pitch allows), 32-bit index
// arithmetic inside a plane: the one-output-per-thread form with 64-bit div/mod ran at 1 TB/s.  A thread serves up to
// kResizePlanes planes (a direction's two flow planes and its certainty, in the loop's calls) with ONE set of taps: the row's
// tap and the four column taps do not depend on the plane.
constexpr int kResizePlanes = 3;

__device__ __forceinline__ void interp_quad(const float *(&pl)[kResizePlanes], float *(&oplane)[kResizePlanes], int np,
                                            int H, int W, int Ho, int Wo, unsigned q, int Wq) {
    const int y = (int)(q / (unsigned)Wq), x0 = ((int)q - y * Wq) * 4;
    const Tap ty = interp_tap(H, Ho, y);
    const int r0 = ty.i0 * W, r1 = ty.i1 * W;
    Tap tx[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) tx[k] = interp_tap(W, Wo, min(x0 + k, Wo - 1));  // past a ragged row end: the last column again, not stored
    const bool quad = x0 + 3 < Wo && (Wo & 3) == 0;
    const int o = y * Wo + x0;
#pragma unroll
    for (int p = 0; p < kResizePlanes; ++p) {
        if (p >= np) break;
        const float *__restrict__ s = pl[p];
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            v[k] = bilerp(ty, tx[k], s[r0 + tx[k].i0], s[r0 + tx[k].i1], s[r1 + tx[k].i0], s[r1 + tx[k].i1]);
        float *d = oplane[p] + o;
        if (quad && (((uintptr_t)oplane[p] & 15) == 0)) {
            *reinterpret_cast<float4 *>(d) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (x0 + k < Wo) d[k] = v[k];
        }
    }
}

__global__ __launch_bounds__(256) void interp_bilinear_kernel(const float *__restrict__ in, float *__restrict__ out, int BC,
                                                              int H, int W, int Ho, int Wo) {
    const int Wq = (Wo + 3) >> 2;
    const unsigned q = blockIdx.x * 256u + threadIdx.x;
    if (q >= (unsigned)(Wq * Ho)) return;
    for (int g = blockIdx.y * kResizePlanes; g < BC; g += gridDim.y * kResizePlanes) {  // block-uniform
        const float *pl[kResizePlanes];
        float *op[kResizePlanes];
#pragma unroll
        for (int p = 0; p < kResizePlanes; ++p) {
            const int i = min(g + p, BC - 1);
            pl[p] = in + (size_t)i * H * W;
            op[p] = out + (size_t)i * Ho * Wo;
        }
        interp_quad(pl, op, min(kResizePlanes, BC - g), H, W, Ho, Wo, q, Wq);
    }
}

// two tensors of the same spatial size in one launch (flow + certainty between scales: half the launches of the loop)
__global__ __launch_bounds__(256) void interp_bilinear_pair_kernel(const float *__restrict__ in_a, float *__restrict__ out_a, int BCa,
                                                                   const float *__restrict__ in_b, float *__restrict__ out_b, int BCb,
                                                                   int H, int W, int Ho, int Wo) {
    const int Wq = (Wo + 3) >> 2, BC = BCa + BCb;
    const unsigned q = blockIdx.x * 256u + threadIdx.x;
    if (q >= (unsigned)(Wq * Ho)) return;
    for (int g = blockIdx.y * kResizePlanes; g < BC; g += gridDim.y * kResizePlanes) {  // block-uniform
        const float *pl[kResizePlanes];
        float *op[kResizePlanes];
#pragma unroll
        for (int p = 0; p < kResizePlanes; ++p) {
            const int i = min(g + p, BC - 1);
            const bool second = i >= BCa;
            pl[p] = second ? in_b + (size_t)(i - BCa) * H * W : in_a + (size_t)i * H * W;
            op[p] = second ? out_b + (size_t)(i - BCa) * Ho * Wo : out_a + (size_t)i * Ho * Wo;
        }
        interp_quad(pl, op, min(kResizePlanes, BC - g), H, W, Ho, Wo, q, Wq);
    }
}

// The resize's adjoint as a gather: an input pixel p of one axis is a tap of the outputs o whose source coordinate
// (o + 1/2) n_in / n_out - 1/2 lies in (p - 1, p + 1).  That interval in closed form, widened by one output on each side against
// the rounding of interp_tap's fp32 arithmetic (as dx_candidates does in refiner_input_bwd.hip); pixels 0 and 1 start at output 0,
// where the source coordinate is clamped.  Whether a candidate really has the pixel as a tap, and with which weight, is decided by
// interp_tap itself.
__device__ __forceinline__ void interp_bwd_candidates(int p, int n_in, int n_out, int &first, int &last) {
    const float r = (float)n_out / (float)n_in;
    first = p <= 1 ? 0 : max(0, (int)floorf(((float)p - 0.5f) * r - 0.5f) - 1);
    last = min(n_out - 1, (int)ceilf(((float)p + 1.5f) * r - 0.5f) + 1);
}
// the weight of input index p in one axis' tap; at the clamped far border both taps are the same pixel and both weights count
__device__ __forceinline__ bool interp_bwd_weight(const Tap &t, int p, double &w) {
    w = (t.i0 == p ? (double)t.h : 0.0) + (t.i1 == p ? (double)t.l : 0.0);
    return (t.i0 == p) | (t.i1 == p);
}

// One thread per input pixel and up to kResizePlanes planes: the outputs that read the pixel, in ascending (row, column) order,
// summed in double (a row's columns first, then the row's weight) and rounded to fp32 once.  No atomics; grad_in is overwritten.
__global__ __launch_bounds__(256) void interp_bilinear_bwd_kernel(const float *__restrict__ gout, float *__restrict__ gin, int BC, int H,
                                                                  int W, int Ho, int Wo) {
    const unsigned pix = blockIdx.x * 256u + threadIdx.x;
    if (pix >= (unsigned)(H * W)) return;
    const int py = (int)(pix / (unsigned)W), px = (int)pix - py * W;
    int y0, y1, x0, x1;
    interp_bwd_candidates(py, H, Ho, y0, y1);
    interp_bwd_candidates(px, W, Wo, x0, x1);
    for (int g = blockIdx.y * kResizePlanes; g < BC; g += gridDim.y * kResizePlanes) {  // block-uniform
        const int np = min(kResizePlanes, BC - g);
        const float *__restrict__ src = gout + (size_t)g * Ho * Wo;
        const size_t oplane = (size_t)Ho * Wo;
        double acc[kResizePlanes];
#pragma unroll
        for (int p = 0; p < kResizePlanes; ++p) acc[p] = 0.0;
        for (int y = y0; y <= y1; ++y) {
            double wy;
            if (!interp_bwd_weight(interp_tap(H, Ho, y), py, wy)) continue;
            double row[kResizePlanes];
#pragma unroll
            for (int p = 0; p < kResizePlanes; ++p) row[p] = 0.0;
            for (int x = x0; x <= x1; ++x) {
                double wx;
                if (!interp_bwd_weight(interp_tap(W, Wo, x), px, wx)) continue;
#pragma unroll
                for (int p = 0; p < kResizePlanes; ++p)
                    if (p < np) row[p] += wx * (double)src[(size_t)p * oplane + (size_t)y * Wo + x];
            }
#pragma unroll
            for (int p = 0; p < kResizePlanes; ++p) acc[p] += wy * row[p];
        }
#pragma unroll
        for (int p = 0; p < kResizePlanes; ++p)
            if (p < np) gin[(size_t)(g + p) * H * W + pix] = (float)acc[p];
    }
}

// One cell of network.py:262-268, the only copy of these expressions: the displacement from the refiner's increment, the
// eval-time zeroing against the previous displacement (`pp`, planes GG apart; NULL on a single-iteration scale), the carry of
// the displacement (when `store_prev`) and the accumulation.  f / c come in as the cell's flow and certainty and leave updated.
__device__ __forceinline__ void flow_update_cell(float &fx, float &fy, float &c, float dlx, float dly, float dc, float *pp, int GG,
                                                 bool store_prev, float scale, float div_x, float div_y, int zero_small, int first) {
    float dx = scale * (dlx / div_x), dy = scale * (dly / div_y);  // network.py:262-263
    if (zero_small) {  // network.py:256,264-265
        const float px = first ? 1e-7f : pp[0], py = first ? 1e-7f : pp[GG];
        if (fabsf(dx - px) / fabsf(px) < 1e-6f) dx = 0.f;
        if (fabsf(dy - py) / fabsf(py) < 1e-6f) dy = 0.f;
    }
    if (pp && store_prev) {
        pp[0] = dx;
        pp[GG] = dy;
    }
    fx = fx + dx;
    fy = fy + dy;
    c = c + dc;
}

// dflow: (B, >=2, G, G) displacement increment with batch stride dflow_bs, dcert: (B, >=1, G, G) certainty increment with
// dcert_bs (the refiner's two outputs; one (B,3,G,G) tensor or two).  flow_in/cert_in -> flow_out/cert_out (may alias).
// flow_in / cert_in may be the same buffers as flow_out / cert_out (gfn_flow_update_fwd updates in place): no __restrict__ on them.
// Cells of a direction on blockIdx.x, directions on blockIdx.y: no division, 32-bit offsets inside a direction.
// MODE 0: the whole step.  MODE 1: only the carry of the displacement into disp_prev (behind the fused kernel below, which must
// not store it while neighbouring workgroups still read it).
template <int MODE>
__global__ __launch_bounds__(256) void flow_update_kernel(const float *flow_in, const float *cert_in,
                                                          float *flow_out, float *cert_out, const float *__restrict__ dflow,
                                                          long dflow_bs, const float *__restrict__ dcert, long dcert_bs,
                                                          float *__restrict__ disp_prev, int B, int G, float scale, float div_x,
                                                          float div_y, int zero_small, int first) {
    const int GG = G * G;
    const int r = (int)(blockIdx.x * 256u + threadIdx.x);
    if (r >= GG) return;
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        const float *dl = dflow + (size_t)b * dflow_bs + r;
        float *pp = disp_prev ? disp_prev + (size_t)b * 2 * GG + r : nullptr;  // NULL: single-iteration scale, nothing to carry
        if (MODE == 1) {
            float fx = 0.f, fy = 0.f, c = 0.f;
            flow_update_cell(fx, fy, c, dl[0], dl[GG], 0.f, pp, GG, true, scale, div_x, div_y, zero_small, first);
            continue;
        }
        const size_t o = (size_t)b * 2 * GG + r, oc = (size_t)b * GG + r;
        float fx = flow_in[o], fy = flow_in[o + GG], c = cert_in[oc];
        flow_update_cell(fx, fy, c, dl[0], dl[GG], dcert[(size_t)b * dcert_bs + r], pp, GG, true, scale, div_x, div_y, zero_small, first);
        flow_out[o] = fx;
        flow_out[o + GG] = fy;
        cert_out[oc] = c;
    }
}

// The last update of a scale and the resize of its result to the next grid (R = G_next / G, 1 or 2) in one launch.  A workgroup
// owns 16 x 16 cells of one direction (blockIdx = tile column, tile row, direction): it updates them and the ring of cells
// around them that lie inside the map into LDS -- every source cell of the tile's outputs once; interp_tap clamps at the
// border, so no output needs a cell outside the map --, writes its own cells to flow_out / cert_out, and after one barrier
// each thread interpolates four consecutive outputs of a row for the three planes from LDS with one set of taps.
// LDS: three planes of 18 rows of 18 floats.  A half wave reads 4 output rows x 8 quads = source rows j..j+2 at even columns:
// with an 18-float pitch those are banks {0..14}, {18..32}, {36..50} (mod 32), one 2-way conflict per read; a 19-float pitch
// gives five.  Ring cells are another workgroup's own cells, so nothing here may store disp_prev where it is also read
// (STORE_PREV false: the caller stores it with flow_update_kernel<1> afterwards), and the outputs must not alias the inputs.
constexpr int kTile = 16, kPitch = kTile + 2;

template <int R, bool STORE_PREV>
__global__ __launch_bounds__(256) void flow_update_resize_kernel(const float *__restrict__ flow_in, const float *__restrict__ cert_in,
                                                                 float *__restrict__ flow_out, float *__restrict__ cert_out,
                                                                 const float *__restrict__ dflow, long dflow_bs,
                                                                 const float *__restrict__ dcert, long dcert_bs, float *disp_prev, int G,
                                                                 float scale, float div_x, float div_y, int zero_small, int first,
                                                                 float *__restrict__ flow_next, float *__restrict__ cert_next) {
    __shared__ float tile[3][kPitch][kPitch];
    const int b = blockIdx.z, ty0 = blockIdx.y * kTile, tx0 = blockIdx.x * kTile, GG = G * G, Go = G * R;
    const float *fin = flow_in + (size_t)b * 2 * GG, *cin = cert_in + (size_t)b * GG;
    const float *dl = dflow + (size_t)b * dflow_bs, *dc = dcert + (size_t)b * dcert_bs;
    float *fout = flow_out + (size_t)b * 2 * GG, *cout = cert_out + (size_t)b * GG;
    float *prev = disp_prev ? disp_prev + (size_t)b * 2 * GG : nullptr;
    for (int i = threadIdx.x; i < kPitch * kPitch; i += 256) {
        const int ly = i / kPitch, lx = i - ly * kPitch, y = ty0 - 1 + ly, x = tx0 - 1 + lx;
        if (y < 0 || y >= G || x < 0 || x >= G) continue;
        const bool own = ly >= 1 && ly <= kTile && lx >= 1 && lx <= kTile;
        const int r = y * G + x;
        float fx = fin[r], fy = fin[r + GG], c = cin[r];
        flow_update_cell(fx, fy, c, dl[r], dl[r + GG], dc[r], prev ? prev + r : nullptr, GG, STORE_PREV && own, scale, div_x, div_y,
                         zero_small, first);
        tile[0][ly][lx] = fx;
        tile[1][ly][lx] = fy;
        tile[2][ly][lx] = c;
        if (own) {
            fout[r] = fx;
            fout[r + GG] = fy;
            cout[r] = c;
        }
    }
    __syncthreads();
    // the tile's outputs: 16 R rows of 4 R quads
    if (threadIdx.x >= kTile * R * 4 * R) return;
    const int oy = ty0 * R + (int)threadIdx.x / (4 * R), ox = tx0 * R + ((int)threadIdx.x % (4 * R)) * 4;
    if (oy >= Go || ox >= Go) return;
    const Tap ty = interp_tap(G, Go, oy);
    const int r0 = ty.i0 - (ty0 - 1), r1 = ty.i1 - (ty0 - 1);
    Tap tx[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        tx[k] = interp_tap(G, Go, min(ox + k, Go - 1));  // past a ragged row end: the last column again, not stored
        tx[k].i0 -= tx0 - 1;
        tx[k].i1 -= tx0 - 1;
    }
    const bool quad = ox + 3 < Go && (Go & 3) == 0;
    const int o = oy * Go + ox;
#pragma unroll
    for (int p = 0; p < 3; ++p) {
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            v[k] = bilerp(ty, tx[k], tile[p][r0][tx[k].i0], tile[p][r0][tx[k].i1], tile[p][r1][tx[k].i0], tile[p][r1][tx[k].i1]);
        float *plane = p < 2 ? flow_next + ((size_t)b * 2 + p) * Go * Go : cert_next + (size_t)b * Go * Go;
        if (quad && (((uintptr_t)plane & 15) == 0)) {
            *reinterpret_cast<float4 *>(plane + o) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (ox + k < Go) plane[o + k] = v[k];
        }
    }
}

__global__ __launch_bounds__(256) void match_post_kernel(const float *__restrict__ flow, const float *__restrict__ cert,
                                                         const float *__restrict__ cert16, float *__restrict__ warp,
                                                         float *__restrict__ cert_out, int Bimg, int G, int Gc,
                                                         int symmetric) {
    const int Gw = symmetric ? 2 * G : G;
    const long total = (long)Bimg * G * Gw;
    const float lo = (float)(-1 + 1.0 / G), hi = (float)(1 - 1.0 / G);
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int jw = (int)(idx % Gw);
        long t = idx / Gw;
        const int i = (int)(t % G);
        const int b = (int)(t / G);
        const bool second = jw >= G;  // the B->A half of a symmetric warp
        const int j = second ? jw - G : jw;
        const int fb = second ? Bimg + b : b;
        const size_t cell = (size_t)i * G + j, GG = (size_t)G * G;
        float fx = flow[((size_t)fb * 2 + 0) * GG + cell], fy = flow[((size_t)fb * 2 + 1) * GG + cell];
        float c = cert[(size_t)fb * GG + cell];
        if (cert16) {  // network.py:332-338
            const float low = interp_at(cert16 + (size_t)fb * Gc * Gc, Gc, Gc, G, G, i, j);
            c = c - 0.5f * low * (low < 0.f ? 1.f : 0.f);
        }
        c = 1.f / (1.f + expf(-c));                          // :361
        if (fabsf(fx) > 1.f || fabsf(fy) > 1.f) c = 0.f;     // :368-370
        fx = fx < -1.f ? -1.f : (fx > 1.f ? 1.f : fx);       // :371, torch.clamp: a NaN component stays NaN (fminf / fmaxf drop it)
        fy = fy < -1.f ? -1.f : (fy > 1.f ? 1.f : fy);
        const float gx = gfn::linspace_at(lo, hi, G, j), gy = gfn::linspace_at(lo, hi, G, i);  // :362-367
        const float4 w = second ? make_float4(fx, fy, gx, gy) : make_float4(gx, gy, fx, fy);   // :373-378
        reinterpret_cast<float4 *>(warp)[idx] = w;
        cert_out[idx] = c;
    }
}

inline unsigned grid_for(long total, int cap = 16384) {
    long g = (total + 255) / 256;
    return (unsigned)(g < 1 ? 1 : (g > cap ? cap : g));
}

// in-plane offsets are 32-bit in the resize and flow-update kernels
constexpr int kMaxGrid = 46340;  // floor(sqrt(2^31))

inline dim3 flow_update_grid(int B, int G) { return dim3((unsigned)(((long)G * G + 255) / 256), (unsigned)(B < 65535 ? B : 65535)); }

}  // namespace

GFN_EXPORT int gfn_refiner_input_fwd(const float *f0, const float *f1, const float *flow, const float *disp_w,
                                     const float *disp_b, float *d, int64_t d_bs, int B, int C, int Hs, int Ws, int G,
                                     int disp_dim, float disp_scale, int symmetric, gfn_stream_t stream) {
    return gfn_refiner_input_fwd_dt(f0, f1, GFN_F32, flow, disp_w, disp_b, d, d_bs, B, C, Hs, Ws, G, disp_dim, disp_scale, symmetric, stream);
}

GFN_EXPORT int gfn_refiner_input_fwd_dt(const void *f0, const void *f1, int dtype, const float *flow, const float *disp_w,
                                        const float *disp_b, float *d, int64_t d_bs, int B, int C, int Hs, int Ws, int G,
                                        int disp_dim, float disp_scale, int symmetric, gfn_stream_t stream) {
    RiArgs q;
    bool keep;
    if (int e = ri_args("refiner_input", f0, f1, dtype, flow, disp_w, disp_b, d, d_bs, B, C, Hs, Ws, G, disp_dim, disp_scale, symmetric, q, keep)) return e;
    if (B == 0) return GFN_OK;
    const unsigned q_blocks = (unsigned)(((long)G * G + 255) / 256);
    const int banded = gfn_ri::ri_bands(q.B, q.Bh, q_blocks) ? 1 : 0;
    const dim3 grid = banded ? dim3(gfn_ri::ri_banded_blocks(B, q_blocks)) : dim3(q_blocks, (unsigned)B);
    if (dtype == GFN_F16) {
        if (keep) hipLaunchKernelGGL((refiner_input_kernel<_Float16, true>), grid, dim3(256), 0, (hipStream_t)stream, q, q_blocks, banded);
        else hipLaunchKernelGGL((refiner_input_kernel<_Float16, false>), grid, dim3(256), 0, (hipStream_t)stream, q, q_blocks, banded);
    } else {
        if (keep) hipLaunchKernelGGL((refiner_input_kernel<float, true>), grid, dim3(256), 0, (hipStream_t)stream, q, q_blocks, banded);
        else hipLaunchKernelGGL((refiner_input_kernel<float, false>), grid, dim3(256), 0, (hipStream_t)stream, q, q_blocks, banded);
    }
    return gfn::check_launch("refiner_input_kernel");
}

GFN_EXPORT int gfn_grid_sample_fwd(const float *in, const float *grid, float *out, int64_t out_bs, int B, int C, int H,
                                   int W, int Ho, int Wo, gfn_stream_t stream) {
    return gfn_grid_sample_mode_fwd(in, GFN_F32, grid, out, out_bs, B, C, H, W, Ho, Wo, GFN_SAMPLE_BILINEAR, GFN_PAD_ZEROS, stream);
}

GFN_EXPORT int gfn_interp_bilinear_fwd(const float *in, float *out, int BC, int H, int W, int Ho, int Wo,
                                       gfn_stream_t stream) {
    if (!in || !out || BC < 0 || H <= 0 || W <= 0 || Ho <= 0 || Wo <= 0)
        return gfn::fail(GFN_ERR_INVALID_ARG, "interp_bilinear: bad argument");
    if (BC == 0) return GFN_OK;
    if ((long)H * W >= (1L << 31) || (long)Ho * Wo >= (1L << 31)) return gfn::fail(GFN_ERR_INVALID_ARG, "interp_bilinear: plane too large");
    const unsigned gx = (unsigned)(((long)Ho * ((Wo + 3) / 4) + 255) / 256);
    const int groups = (BC + kResizePlanes - 1) / kResizePlanes;
    hipLaunchKernelGGL(interp_bilinear_kernel, dim3(gx, (unsigned)(groups < 65535 ? groups : 65535)), dim3(256), 0, (hipStream_t)stream, in,
                       out, BC, H, W, Ho, Wo);
    return gfn::check_launch("interp_bilinear_kernel");
}

GFN_EXPORT int gfn_interp_bilinear_bwd(const float *grad_out, float *grad_in, int BC, int H, int W, int Ho, int Wo, gfn_stream_t stream) {
    if (!grad_out || !grad_in || BC < 0 || H <= 0 || W <= 0 || Ho <= 0 || Wo <= 0)
        return gfn::fail(GFN_ERR_INVALID_ARG, "interp_bilinear_bwd: bad argument");
    if (BC == 0) return GFN_OK;
    if ((long)H * W >= (1L << 31) || (long)Ho * Wo >= (1L << 31))
        return gfn::fail(GFN_ERR_INVALID_ARG, "interp_bilinear_bwd: plane too large");
    const unsigned gx = (unsigned)(((long)H * W + 255) / 256);
    const int groups = (BC + kResizePlanes - 1) / kResizePlanes;
    hipLaunchKernelGGL(interp_bilinear_bwd_kernel, dim3(gx, (unsigned)(groups < 65535 ? groups : 65535)), dim3(256), 0, (hipStream_t)stream,
                       grad_out, grad_in, BC, H, W, Ho, Wo);
    return gfn::check_launch("interp_bilinear_bwd_kernel");
}

GFN_EXPORT int gfn_interp_bilinear_pair_fwd(const float *in_a, float *out_a, int BCa, const float *in_b, float *out_b, int BCb, int H,
                                            int W, int Ho, int Wo, gfn_stream_t stream) {
    if (!in_a || !out_a || !in_b || !out_b || BCa < 0 || BCb < 0 || H <= 0 || W <= 0 || Ho <= 0 || Wo <= 0)
        return gfn::fail(GFN_ERR_INVALID_ARG, "interp_bilinear_pair: bad argument");
    if (BCa + BCb == 0) return GFN_OK;
    if ((long)H * W >= (1L << 31) || (long)Ho * Wo >= (1L << 31)) return gfn::fail(GFN_ERR_INVALID_ARG, "interp_bilinear_pair: plane too large");
    const unsigned gx = (unsigned)(((long)Ho * ((Wo + 3) / 4) + 255) / 256);
    if ((long)BCa + BCb >= (1L << 31)) return gfn::fail(GFN_ERR_INVALID_ARG, "interp_bilinear_pair: too many planes");
    const int groups = (BCa + BCb + kResizePlanes - 1) / kResizePlanes;
    hipLaunchKernelGGL(interp_bilinear_pair_kernel, dim3(gx, (unsigned)(groups < 65535 ? groups : 65535)), dim3(256), 0,
                       (hipStream_t)stream, in_a, out_a, BCa, in_b, out_b, BCb, H, W, Ho, Wo);
    return gfn::check_launch("interp_bilinear_pair_kernel");
}

GFN_EXPORT int gfn_resize_normalize_fwd(const float *in, int64_t in_bs, float *out, int B, int H, int W, int Ho, int Wo, int mode,
                                        const float *mean3, const float *std3, gfn_stream_t stream) {
    if (!in || !out || !mean3 || !std3 || B < 0 || H <= 0 || W <= 0 || Ho <= 0 || Wo <= 0 || in_bs < 3L * H * W)
        return gfn::fail(GFN_ERR_INVALID_ARG, "resize_normalize: bad argument");
    if (mode != 0 && mode != 1) return gfn::fail(GFN_ERR_INVALID_ARG, "resize_normalize: mode must be 0 (bilinear) or 1 (bicubic)");
    NormParams np;
    for (int c = 0; c < 3; ++c) {
        if (!(std3[c] != 0.f)) return gfn::fail(GFN_ERR_INVALID_ARG, "resize_normalize: zero std");
        np.mean[c] = mean3[c];
        np.std[c] = std3[c];
    }
    if (B == 0) return GFN_OK;
    hipLaunchKernelGGL(resize_normalize_kernel, dim3(grid_for((long)B * Ho * Wo)), dim3(256), 0, (hipStream_t)stream, in, (long)in_bs,
                       out, B, H, W, Ho, Wo, mode, np);
    return gfn::check_launch("resize_normalize_kernel");
}

GFN_EXPORT int gfn_flow_update_fwd(float *flow, float *certainty, const float *delta, int64_t delta_bs, float *disp_prev,
                                   int B, int G, int scale, int W0, int H0, int zero_small, int first_iteration,
                                   gfn_stream_t stream) {
    if (!flow || !certainty || !delta || !disp_prev || B < 0 || G <= 0 || W0 <= 0 || H0 <= 0 || delta_bs < 3L * G * G)
        return gfn::fail(GFN_ERR_INVALID_ARG, "flow_update: bad argument");
    if (G > kMaxGrid) return gfn::fail(GFN_ERR_INVALID_ARG, "flow_update: grid too large");
    if (B == 0) return GFN_OK;
    hipLaunchKernelGGL(flow_update_kernel<0>, flow_update_grid(B, G), dim3(256), 0, (hipStream_t)stream, flow, certainty, flow,
                       certainty, delta, (long)delta_bs, delta + 2L * G * G, (long)delta_bs, disp_prev, B, G, (float)scale,
                       (float)(4 * W0), (float)(4 * H0), zero_small, first_iteration);
    return gfn::check_launch("flow_update_kernel");
}

GFN_EXPORT int gfn_flow_update_out_fwd(const float *flow_in, const float *cert_in, float *flow_out, float *cert_out,
                                       const float *dflow, int64_t dflow_bs, const float *dcert, int64_t dcert_bs, float *disp_prev,
                                       int B, int G, int scale, int W0, int H0, int zero_small, int first_iteration,
                                       gfn_stream_t stream) {
    if (!flow_in || !cert_in || !flow_out || !cert_out || !dflow || !dcert || B < 0 || G <= 0 || W0 <= 0 || H0 <= 0 ||
        dflow_bs < 2L * G * G || dcert_bs < (long)G * G || (!disp_prev && !first_iteration))
        return gfn::fail(GFN_ERR_INVALID_ARG, "flow_update_out: bad argument");
    if (G > kMaxGrid) return gfn::fail(GFN_ERR_INVALID_ARG, "flow_update_out: grid too large");
    if (B == 0) return GFN_OK;
    hipLaunchKernelGGL(flow_update_kernel<0>, flow_update_grid(B, G), dim3(256), 0, (hipStream_t)stream, flow_in, cert_in, flow_out,
                       cert_out, dflow, (long)dflow_bs, dcert, (long)dcert_bs, disp_prev, B, G, (float)scale, (float)(4 * W0),
                       (float)(4 * H0), zero_small, first_iteration);
    return gfn::check_launch("flow_update_kernel");
}

GFN_EXPORT int gfn_flow_update_resize_fwd(const float *flow_in, const float *cert_in, float *flow_out, float *cert_out,
                                          const float *dflow, int64_t dflow_bs, const float *dcert, int64_t dcert_bs, float *disp_prev,
                                          int B, int G, int scale, int W0, int H0, int zero_small, int first_iteration,
                                          float *flow_next, float *cert_next, int G_next, gfn_stream_t stream) {
    if (!flow_in || !cert_in || !flow_out || !cert_out || !dflow || !dcert || !flow_next || !cert_next || B < 0 || G <= 0 || W0 <= 0 ||
        H0 <= 0 || dflow_bs < 2L * G * G || dcert_bs < (long)G * G || (!disp_prev && !first_iteration))
        return gfn::fail(GFN_ERR_INVALID_ARG, "flow_update_resize: bad argument");
    if (G_next != G && (G > kMaxGrid || G_next != 2 * G))
        return gfn::fail(GFN_ERR_INVALID_ARG, "flow_update_resize: G_next must be G or 2 G (use flow_update_out + interp_bilinear_pair)");
    if (G_next > kMaxGrid) return gfn::fail(GFN_ERR_INVALID_ARG, "flow_update_resize: grid too large");
    if (flow_in == flow_out || cert_in == cert_out)
        return gfn::fail(GFN_ERR_INVALID_ARG, "flow_update_resize: outputs must not alias the inputs");
    if (B > 65535) return gfn::fail(GFN_ERR_INVALID_ARG, "flow_update_resize: more than 65535 directions");
    if (B == 0) return GFN_OK;
    // disp_prev is read only by the zeroing test of a later iteration; there a ring cell would read what its owner stores
    const bool deferred = disp_prev && zero_small && !first_iteration;
    const unsigned tiles = (unsigned)((G + kTile - 1) / kTile);
    const dim3 grid(tiles, tiles, (unsigned)B);
    const float s = (float)scale, dx = (float)(4 * W0), dy = (float)(4 * H0);
#define GFN_FUR_LAUNCH(R, SP)                                                                                                        \
    hipLaunchKernelGGL((flow_update_resize_kernel<R, SP>), grid, dim3(256), 0, (hipStream_t)stream, flow_in, cert_in, flow_out,      \
                       cert_out, dflow, (long)dflow_bs, dcert, (long)dcert_bs, disp_prev, G, s, dx, dy, zero_small, first_iteration, \
                       flow_next, cert_next)
    if (G_next == G) {
        if (deferred) GFN_FUR_LAUNCH(1, false);
        else GFN_FUR_LAUNCH(1, true);
    } else {
        if (deferred) GFN_FUR_LAUNCH(2, false);
        else GFN_FUR_LAUNCH(2, true);
    }
#undef GFN_FUR_LAUNCH
    if (int e = gfn::check_launch("flow_update_resize_kernel")) return e;
    if (deferred) {
        hipLaunchKernelGGL(flow_update_kernel<1>, flow_update_grid(B, G), dim3(256), 0, (hipStream_t)stream, nullptr, nullptr, nullptr,
                           nullptr, dflow, (long)dflow_bs, dcert, (long)dcert_bs, disp_prev, B, G, s, dx, dy, zero_small, first_iteration);
        return gfn::check_launch("flow_update_kernel");
    }
    return GFN_OK;
}

GFN_EXPORT int gfn_match_post_fwd(const float *flow, const float *certainty, const float *cert16_or_null, float *warp,
                                  float *cert_out, int B_images, int G, int Gc, int symmetric, gfn_stream_t stream) {
    if (!flow || !certainty || !warp || !cert_out || B_images < 0 || G <= 0 || (cert16_or_null && Gc <= 0))
        return gfn::fail(GFN_ERR_INVALID_ARG, "match_post: bad argument");
    if (B_images == 0) return GFN_OK;
    const long total = (long)B_images * G * (symmetric ? 2 * G : G);
    hipLaunchKernelGGL(match_post_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, flow, certainty,
                       cert16_or_null, warp, cert_out, B_images, G, Gc, symmetric);
    return gfn::check_launch("match_post_kernel");
}
