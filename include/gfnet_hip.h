/*
 * gfnet_hip.h -- C ABI of libgfnet_hip.so: the MI355X (gfx950) kernels behind GFNet's
 * dense-correlation -> flow -> balanced-sampling -> homography-solve path.
 *
 * The reference (KN-Zhang/GFNet) has no FFI layer: its boundary is a set of Python functions.
 * Each entry point below replaces the arithmetic of one of them; the Python mirror that keeps the
 * reference's signatures lives in gfnet_amd/ (see INTEGRATION.md for the binding a maintainer of
 * the reference would add).  Paths cited are relative to the reference repository.
 *
 * Conventions (all entry points):
 *   - plain pointers and sizes only; every tensor pointer is a DEVICE pointer to fp32 data,
 *     NCHW-contiguous unless a stride argument says otherwise; the caller owns every buffer,
 *     the library never allocates or frees device memory (scratch is passed in explicitly);
 *   - work is enqueued on `stream` (a hipStream_t passed as void*; NULL = the default stream) and
 *     the call returns without synchronising; it is safe to capture into a hipGraph;
 *   - return value: GFN_OK (0) or a negative GFN_ERR_* code; gfn_last_error() gives the text
 *     (thread-local).  Nothing is launched when an argument error is returned;
 *   - no global mutable state; single host thread per stream is assumed, as in the reference;
 *   - sampled maps are finite feature maps: a sampling corner outside the image reads pixel 0 of its plane with weight 0, so
 *     a non-finite value there would turn the zero it stands for into NaN.
 */
#ifndef GFNET_HIP_H
#define GFNET_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GFN_OK 0
#define GFN_ERR_INVALID_ARG (-1) /* bad size / null pointer / unsupported combination */
#define GFN_ERR_LAUNCH (-2)      /* hipLaunchKernel / runtime error, see gfn_last_error() */
#define GFN_ERR_SCRATCH (-3)     /* scratch buffer too small */

#define GFN_ABI_VERSION 1

/* storage type of the feature pyramids (BASELINE config 5 keeps them in fp16; reference: model/network.py:171-173 runs the
 * backbone under autocast, utils/utils.py:306-320).  Arithmetic and every other tensor stay fp32. */
#define GFN_F32 0
#define GFN_F16 1
/* bf16 tensors: taken by gfn_conv_block_bf16_fwd and the gfn_conv_block_train_bf16_* entry points (maps), by gfn_cross_attn_fwd / gfn_cross_attn_bwd (q, k, v,
 * out and the gradients), by gfn_self_attn_fwd (qkv, out); the gfn_decoder_*_bf16_* entry points and
 * gfn_ls_add_layernorm_bf16_fwd are the bf16 class by name and take no dtype.  Every other entry point refuses it */
#define GFN_BF16 2

typedef void *gfn_stream_t; /* hipStream_t */

/* Library / device introspection.  gfn_device_arch() copies the gcnArchName of the current
 * device ("gfx950...") into buf. */
int gfn_abi_version(void);
const char *gfn_last_error(void);
int gfn_device_arch(char *buf, int buflen);

/* ---------------------------------------------------------------------------------------------
 * local_correlation -- utils/local_correlation.py:4-72 (called from model/network.py:553-554).
 *
 *   out[b, k, i, j] = sum_c f0[b,c,i,j] / sqrt(C) * bilinear(f1[b,c], p(b,i,j) + offset(k))
 *
 * k = ky*(2r+1)+kx (x fastest); zeros padding, align_corners=False; p = flow[b,:,i,j] in
 * normalised [-1,1] coordinates, or the identity grid when flow == NULL (then G == win_h ==
 * win_w is required, as in the reference).  The window offsets are
 * linspace(-2r/win_h, 2r/win_h, 2r+1) x linspace(-2r/win_w, 2r/win_w, 2r+1) normalised units
 * (grid_based != 0: +-2r/G on both axes, local_correlation.py:34-40).  For num_level == 1 the
 * reference has win_h == H, win_w == W (one feature pixel per tap); on pooled levels
 * (local_correlation.py:61-71) the caller passes the pooled f1 with the original win_h/win_w.
 *
 *   f0   (B,C,G,G)  batch stride f0_bs floats (>= C*G*G; lets f0 live inside a concat buffer)
 *   f1   (B,C,H,W)  contiguous; or, for a symmetric batch (model/network.py:213-222 concatenates
 *                   (A,B) against (B,A)), f1 = the B-image maps (B/2,C,H,W) used by directions
 *                   b < B/2 and f1_second = the A-image maps used by b >= B/2 -- no concatenated
 *                   copy is needed.  f1_second == NULL: plain batch.
 *   flow (B,2,G,G)  contiguous, or NULL
 *   out  (B,K,G,G)  batch stride out_bs floats (>= K*G*G), K = (2r+1)^2
 *
 * Fast path (LDS-tiled, shared bilinear fractions): C % 16 == 0, 1 <= r <= 7, !grid_based,
 * win_h == H, win_w == W, and `scratch` (device memory, gfn_local_corr_scratch_bytes(B, G) bytes,
 * 4-byte aligned; holds the list of tiles whose search windows do not fit the LDS stage and are
 * finished by a second, gather-based launch.  Its first 16 bytes are counters that must be ZERO on entry: zero
 * them once after allocation -- every successful call leaves them zero again (the second launch resets them, so
 * no memset precedes a call); after a call that returned an error, zero them again before reuse).  Anything else -- including scratch == NULL -- runs
 * the general per-tap kernel.  Flow values are unrestricted (out-of-image taps read zeros).
 */
int64_t gfn_local_corr_scratch_bytes(int B, int G);
int gfn_local_corr_fwd(const float *f0, int64_t f0_bs, const float *f1, const float *f1_second, const float *flow,
                       float *out, int64_t out_bs, int B, int C, int G, int H, int W, int r, int grid_based, int win_h,
                       int win_w, void *scratch, int64_t scratch_bytes, gfn_stream_t stream);

/* Variant selector for experiments/tests: 0 = auto (as above: the lean tile path of csrc/local_corr_lean.h for r <= 4; for r >= 5 on
 * 64-channel maps the matrix-core tile kernel of csrc/local_corr_mq.h -- split-bf16 products with fp32 accumulation, NOT bit-identical to
 * the fp32 FMA kernels: each product is exact to 2^-17 relative, so a value is within 2^-17 * sum_c |f0_c * f1_c| / sqrt(C) of the fp32
 * result (a few 1e-6, i.e. inside 1e-4 * max(1, |ref|), on unit-scale features; the bound follows the operands' magnitude, not the
 * result's; variant 4 is the opt-out, gfnet_amd.ops.LOCAL_CORR_FP32 in Python) -- and the round-1 tile kernel above for other channel counts), 1 = force the general per-tap kernel, 2 = the
 * round-1 fp32 tile kernel for every radius (the cross-check of the other paths), 4 = fp32 FMA arithmetic whatever the radius: the lean
 * tile path for r <= 4, the round-1 kernel for r >= 5 (bit-identical to 2); + 8: the plan of this call is already in scratch
 * (gfn_refiner_input_plan_fwd_dt; only with 0).  Same arguments otherwise.
 * Scratch header (ints): [0] tiles left to the second launch, [1..2] its queue counters, [3] last call's [0], [4] cells redone
 * per tap, [5] last call's [4], [6] tiles staged as two halves (sampled), [7] last call's [6]; [0..2], [4], [6] are zero
 * between calls.  [4]..[7] are informational and approximate: the r >= 3 kernels publish and reset them from inside the launch
 * while other workgroups may still be adding, so a handful of flagged cells can be attributed to the next call. */
int gfn_local_corr_fwd_ex(const float *f0, int64_t f0_bs, const float *f1, const float *f1_second, const float *flow,
                          float *out, int64_t out_bs, int B, int C, int G, int H, int W, int r, int grid_based, int win_h,
                          int win_w, int variant, void *scratch, int64_t scratch_bytes, gfn_stream_t stream);

/* The same with the feature map f1 (and f1_second) stored as f1_dtype = GFN_F32 or GFN_F16 (read directly, widened in
 * registers; f0, flow and out stay fp32). */
int gfn_local_corr_fwd_dt(const float *f0, int64_t f0_bs, const void *f1, const void *f1_second, int f1_dtype, const float *flow,
                          float *out, int64_t out_bs, int B, int C, int G, int H, int W, int r, int grid_based, int win_h,
                          int win_w, int variant, void *scratch, int64_t scratch_bytes, gfn_stream_t stream);

/* Backward of gfn_local_corr_fwd with respect to f0 -- the only gradient the reference lets through
 * (utils/local_correlation.py:54-60: sampling coordinates and feature1 are used under no_grad):
 *   grad_f0[b,c,i,j] = (sum_k grad_out[b,k,i,j] * bilinear(f1[b,c], tap k of cell (i,j))) / sqrt(C).
 * Same arguments as the forward; grad_out (B,K,G,G) with batch stride grad_out_bs, grad_f0 (B,C,G,G) with grad_f0_bs.
 * This is gfn_local_corr_mode_bwd_f0 with GFN_SAMPLE_BILINEAR and GFN_PAD_ZEROS. */
int gfn_local_corr_bwd_f0(const float *grad_out, int64_t grad_out_bs, const float *f1, const float *f1_second, const float *flow,
                          float *grad_f0, int64_t grad_f0_bs, int B, int C, int G, int H, int W, int r, int grid_based, int win_h,
                          int win_w, gfn_stream_t stream);

/* F.avg_pool2d(x, 2, 2) between correlation levels (utils/local_correlation.py:71).
 * in (BC,H,W) -> out (BC,H/2,W/2). */
int gfn_avg_pool2(const float *in, float *out, int BC, int H, int W, gfn_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Global correlation + soft-argmax -- model/network.py:415-428 (GFNet.corr_volume) and :430-440
 * (GFNet.pos_embed), called at :251-252.
 *   V[b,j,i]     = sum_c f0[b,c,i] * f1[b,c,j] / sqrt(C)        vol: (B,H1,W1,H0,W0)
 *   flow[b,:,i]  = sum_j softmax_j(V[b,j,i]) * (x_j, y_j)        flow: (B,2,H0,W0)
 * gfn_corr_softargmax_fwd is the fused form (the volume is never written); with symmetric != 0
 * f0/f1 hold B/2 images each and directions b >= B/2 swap their roles (the reference's
 * cat((A,B)) vs cat((B,A)) batch, model/network.py:213-222, without the copies);
 * gfn_corr_volume_fwd writes the volume (and the flow too when flow_or_null != NULL);
 * gfn_pos_embed_fwd is pos_embed on a caller-supplied volume.  f0 (B,C,H0,W0), f1 (B,C,H1,W1),
 * C <= 128.
 */
int gfn_corr_softargmax_fwd(const float *f0, const float *f1, float *flow, int B, int C, int H0, int W0, int H1, int W1,
                            int symmetric, gfn_stream_t stream);
/* The same with the feature maps stored as dtype = GFN_F32 or GFN_F16 (widened on load; products and sums fp32). */
int gfn_corr_softargmax_fwd_dt(const void *f0, const void *f1, int dtype, float *flow, int B, int C, int H0, int W0, int H1, int W1,
                               int symmetric, gfn_stream_t stream);
/* The same with a caller-owned workspace (round 6).  On 33..64-channel maps whose rows are 32..64 positions wide (GFNet's stride-16
 * features, model/network.py:251-252) the products of all three flow calls run on the bf16 matrix core instruction with both operands
 * split three ways (x = h + m + l exactly; six of the nine piece products kept, the dropped ones <= 2^-23 of |a||b|: measured closer
 * to a float64 evaluation than fp32 fma chains).  gfn_corr_softargmax_fwd and _dt split the operands inside the kernel, every wave
 * again; here, with ws_bytes >= gfn_corr_softargmax_ws_bytes(B, C, H1, W1), the B-positions' operand is split ONCE into ws (16-byte
 * aligned device memory, contents undefined afterwards).  ws == NULL or too small: same results as the in-kernel split, slower.
 * gfn_corr_softargmax_ws_bytes returns 0 for shapes that take no workspace. */
int64_t gfn_corr_softargmax_ws_bytes(int B, int C, int H1, int W1);
int gfn_corr_softargmax_fwd_ws(const void *f0, const void *f1, int dtype, float *flow, int B, int C, int H0, int W0, int H1, int W1,
                               int symmetric, void *ws, int64_t ws_bytes, gfn_stream_t stream);
/* Backward of gfn_corr_softargmax_fwd_ws (training: the reference differentiates pos_embed(corr_volume(f0, f1)),
 * model/network.py:251-252, 415-440, through torch autograd).  flow = the forward's output, grad_flow = dL/dflow, both (B,2,H0,W0)
 * fp32.  grad_f0 (B',C,H0,W0) / grad_f1 (B',C,H1,W1) fp32 (B' = B, or B/2 with symmetric != 0) are OVERWRITTEN with the gradients
 * with respect to the caller's f0 / f1 (fp32 or fp16 as dtype; fp16 maps give the gradient of their widened fp32 copy); either may
 * be NULL, and its share is then not computed.  Symmetric batches are indexed as in the forward and each image's gradient is the sum
 * over both directions it takes part in.  Same limits as the forward (C <= 128; symmetric: even batch, equal map sizes).  ws:
 * >= gfn_corr_softargmax_bwd_ws_bytes(...) bytes of 16-byte aligned device memory (per-position softmax statistics; contents
 * undefined afterwards).  Never writes the volume or its gradient; no atomics, so two calls give the same bits. */
int64_t gfn_corr_softargmax_bwd_ws_bytes(int B, int C, int H0, int W0, int H1, int W1);
int gfn_corr_softargmax_bwd(const void *f0, const void *f1, int dtype, const float *flow, const float *grad_flow, float *grad_f0,
                            float *grad_f1, int B, int C, int H0, int W0, int H1, int W1, int symmetric, void *ws, int64_t ws_bytes,
                            gfn_stream_t stream);
int gfn_corr_volume_fwd(const float *f0, const float *f1, float *vol, float *flow_or_null, int B, int C, int H0, int W0,
                        int H1, int W1, gfn_stream_t stream);
int gfn_pos_embed_fwd(const float *vol, float *flow, int B, int H0, int W0, int H1, int W1, gfn_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * ConvRefiner.forward prefix -- model/network.py:533-555.  Writes, into the concat buffer
 * d (B, 2C+disp_dim[+K], G, G) with batch stride d_bs:
 *   d[:, 0:C]          = grid_sample(f0, cell centres)                    (:539-547)
 *   d[:, C:2C]         = grid_sample(f1, flow)                            (:537)
 *   d[:, 2C:2C+disp]   = disp_w @ (disp_scale * (flow - centres)) + disp_b (:548-549),
 *                        disp_scale = 40/32 * scale_factor, disp_w (disp_dim,2), disp_b (disp_dim)
 * The local-correlation slice d[:, 2C+disp:] is filled by gfn_local_corr_fwd with
 * f0 = d (batch stride d_bs) and out = d + (2C+disp)*G*G (batch stride d_bs).
 * symmetric bit 0 (1): f0/f1 hold B/2 images each; direction b < B/2 queries f0[b] against f1[b],
 * direction b >= B/2 queries f1[b-B/2] against f0[b-B/2].
 * symmetric bit 1 (2, GFN_RI_KEEP_GRID_FEATURE): d[:, 0:C] is left as it is -- grid_sample(f0, cell centres) depends on f0
 * and G only, so the second refiner iteration at a scale (num_itr = 2, model/network.py:257-268: same features, new flow)
 * passes the d of the first one and has only x_hat and the displacement embedding rewritten.
 */
#define GFN_RI_KEEP_GRID_FEATURE 2
int gfn_refiner_input_fwd(const float *f0, const float *f1, const float *flow, const float *disp_w, const float *disp_b,
                          float *d, int64_t d_bs, int B, int C, int Hs, int Ws, int G, int disp_dim, float disp_scale,
                          int symmetric, gfn_stream_t stream);
/* The same with the two feature maps stored as dtype = GFN_F32 or GFN_F16 (gathered directly, widened in registers; d is fp32). */
int gfn_refiner_input_fwd_dt(const void *f0, const void *f1, int dtype, const float *flow, const float *disp_w, const float *disp_b,
                             float *d, int64_t d_bs, int B, int C, int Hs, int Ws, int G, int disp_dim, float disp_scale,
                             int symmetric, gfn_stream_t stream);
/* gfn_refiner_input_fwd_dt that, in the same launch, also plans the tiles of the local correlation that follows it in
 * ConvRefiner.forward (model/network.py:537-555; both only read the flow): call gfn_local_corr_fwd_dt next with the same B, C,
 * G, Hs, Ws, r, flow, dtype and scratch and variant = 8 ("plan present"), which then skips its own plan launch.  Only for shapes
 * with gfn_local_corr_plans(...) != 0 (the lean tile path: 1 <= r <= 4, C in {16, 32, 64}, ...); scratch as for
 * gfn_local_corr_fwd (gfn_local_corr_scratch_bytes(B, G) bytes, counters zero). */
int gfn_local_corr_plans(int C, int H, int W, int G, int r, int f1_dtype);
int gfn_refiner_input_plan_fwd_dt(const void *f0, const void *f1, int dtype, const float *flow, const float *disp_w, const float *disp_b,
                                  float *d, int64_t d_bs, int B, int C, int Hs, int Ws, int G, int disp_dim, float disp_scale,
                                  int symmetric, int r, void *scratch, int64_t scratch_bytes, gfn_stream_t stream);

/* Backward of gfn_refiner_input_fwd_dt (+ the local correlation that fills d's last K planes) on a plain batch, bilinear sampling
 * with zeros padding (training: the reference differentiates model/network.py:537-555 through torch autograd).  grad_d = dL/dd,
 * (B, 2C+disp_dim+K, G, G) with batch stride d_bs; f1 (B,C,Hs,Ws) as the forward read it (dtype = GFN_F32 or GFN_F16), flow and
 * disp_w the forward's.  gf0 (B,C,G,G) contiguous or NULL: the gradient the local correlation sends to its feature0 = d[:, 0:C]
 * (gfn_local_corr_bwd_f0 on grad_d's last K planes); NULL when there is no correlation slice.  Outputs, all fp32 and OVERWRITTEN,
 * each may be NULL and is then not computed:
 *   dx      (B,C,Hs,Ws)  adjoint of sampling f0 at the cell centres, applied to grad_d[:, 0:C] + gf0: a gather, no atomics
 *   dy      (B,C,Hs,Ws)  adjoint of sampling f1 along the flow: a scatter with fp32 atomic adds; the call clears dy on `stream`
 *                        first.  On this entry point its last bits can differ from run to run (the order the adds arrive in);
 *                        gfn_refiner_input_bwd_det below gives the same sum bit for bit on every run
 *   dflow   (B,2,G,G)    derivative of x_hat with respect to the sampling coordinate (ATen's grid_sampler rule: corners outside
 *                        the image count as zeros; cells 10^6 pixels outside or non-finite get none) plus
 *                        disp_scale * disp_w^T grad_emb.  The local correlation adds nothing: the reference samples its window
 *                        under no_grad (utils/local_correlation.py:54-60)
 *   ddisp_w (disp_dim,2) disp_scale * sum grad_emb * (flow - centres), ddisp_b (disp_dim) sum grad_emb: per-workgroup partial sums
 *                        in `scratch` and a second-stage sum, both in a fixed order (no atomics)
 * scratch: >= gfn_refiner_input_bwd_scratch_bytes(B, G, disp_dim) bytes of 4-byte aligned device memory when ddisp_w or ddisp_b is
 * wanted (contents undefined afterwards), unused otherwise.  Same size limits as the forward (C * Hs * Ws < 2^31). */
int64_t gfn_refiner_input_bwd_scratch_bytes(int B, int G, int disp_dim);
int gfn_refiner_input_bwd(const float *grad_d, int64_t d_bs, const void *f1, int dtype, const float *flow, const float *disp_w,
                          const float *gf0, float *dx, float *dy, float *dflow, float *ddisp_w, float *ddisp_b, int B, int C, int Hs,
                          int Ws, int G, int disp_dim, int K, float disp_scale, void *scratch, int64_t scratch_bytes,
                          gfn_stream_t stream);
/* gfn_refiner_input_bwd with a bit-reproducible dy: the same arguments, limits and launches, and dx, dflow, ddisp_w, ddisp_b are
 * the plain call's bits.  dy[b] is the order-independent sum of the plain call's terms t = weight * g (fp32 products, g =
 * grad_d[b, C + c, cell], one term per live cell, channel and corner inside the map) in 64-bit fixed point:
 *   M_b = the largest finite |g| over grad_d[b, C:2C], M_b < 2^E_b (frexp), k_b = 62 - E_b - ceil(log2(G * G));
 *   every finite term adds llrint((double)t * 2^k_b) to its element's 64-bit integer accumulator (integer addition commutes; the
 *   weights lie in [0, 1] and at most G * G terms reach one element, so |sum| < 2^62 for every accepted input);
 *   dy = (float)ldexp((double)acc, -k_b): within G * G * 2^-k_b / 2 of the exact sum of the terms, then one fp32 rounding.
 * An element that received a non-finite term (g inf or NaN) is NaN -- exactly the elements the plain call makes non-finite -- and
 * M_b ignores non-finite values, so every other element is unaffected.  M_b = 0 or no finite value: the finite terms are zeros.
 * k_b is per sample: a sample's dy does not depend on its batch peers.
 * ws: >= gfn_refiner_input_bwd_det_ws_bytes(B, C, Hs, Ws) bytes of 8-byte aligned device memory when dy is wanted (an accumulator
 * and a flag bit per element, a word per sample; cleared by the call on `stream`, contents undefined afterwards); too small,
 * misaligned or NULL: GFN_ERR_SCRATCH.  dy == NULL needs no workspace and is the plain call. */
int64_t gfn_refiner_input_bwd_det_ws_bytes(int B, int C, int Hs, int Ws);
int gfn_refiner_input_bwd_det(const float *grad_d, int64_t d_bs, const void *f1, int dtype, const float *flow, const float *disp_w,
                              const float *gf0, float *dx, float *dy, float *dflow, float *ddisp_w, float *ddisp_b, int B, int C,
                              int Hs, int Ws, int G, int disp_dim, int K, float disp_scale, void *scratch, int64_t scratch_bytes,
                              void *ws, int64_t ws_bytes, gfn_stream_t stream);

/* F.grid_sample(in, grid, mode='bilinear', padding_mode='zeros', align_corners=False):
 * in (B,C,H,W), grid (B,Ho,Wo,2) -> out (B,C,Ho,Wo) with batch stride out_bs.  This is gfn_grid_sample_mode_fwd with GFN_F32,
 * GFN_SAMPLE_BILINEAR and GFN_PAD_ZEROS; like it, it refuses H * W >= 2^31 (pixel offsets are 32-bit). */
int gfn_grid_sample_fwd(const float *in, const float *grid, float *out, int64_t out_bs, int B, int C, int H, int W,
                        int Ho, int Wo, gfn_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Sampling modes -- the `sample_mode` / `padding_mode` the reference passes straight to F.grid_sample
 * (utils/local_correlation.py:4-16, 55-58, 66-68; ConvRefiner(sample_mode=...), model/network.py:464, 502, 537, 547, 553-554).
 * ATen grid_sampler_2d semantics with align_corners=False: nearest rounds the padded coordinate half to even; bilinear weighs
 * the four corners of the padded coordinate; bicubic takes the 4 x 4 taps around the UN-padded coordinate, pads each tap on
 * its own and uses cubic convolution with A = -0.75 (rows along x first, then along y).  Taps outside the image read 0;
 * coordinates 10^6 pixels or more outside the image, and non-finite ones, read 0 in every mode.
 * These entry points are the general per-tap route for every combination (bilinear + zeros included); the LDS-tiled and
 * matrix-core paths above serve bilinear + zeros only and are not reached from here.
 */
#define GFN_SAMPLE_BILINEAR 0
#define GFN_SAMPLE_NEAREST 1
#define GFN_SAMPLE_BICUBIC 2
#define GFN_PAD_ZEROS 0
#define GFN_PAD_BORDER 1
#define GFN_PAD_REFLECTION 2

/* gfn_local_corr_fwd_dt's arguments without variant and scratch, plus the two codes:
 *   out[b, k, i, j] = sum_c f0[b,c,i,j] / sqrt(C) * sample(f1[b,c], p(b,i,j) + offset(k))
 * Any C and r, fp32 / fp16 f1, f1_second, grid_based and flow == NULL as there.  With GFN_SAMPLE_BILINEAR + GFN_PAD_ZEROS this
 * is the general kernel of gfn_local_corr_fwd_dt (what that runs with scratch == NULL). */
int gfn_local_corr_mode_fwd(const float *f0, int64_t f0_bs, const void *f1, const void *f1_second, int f1_dtype, const float *flow,
                            float *out, int64_t out_bs, int B, int C, int G, int H, int W, int r, int grid_based, int win_h, int win_w,
                            int sample_mode, int padding_mode, gfn_stream_t stream);
/* Its gradient with respect to f0 (fp32 f1; feature1 and the coordinates under no_grad); gfn_local_corr_bwd_f0 is this call with
 * GFN_SAMPLE_BILINEAR + GFN_PAD_ZEROS. */
int gfn_local_corr_mode_bwd_f0(const float *grad_out, int64_t grad_out_bs, const float *f1, const float *f1_second, const float *flow,
                               float *grad_f0, int64_t grad_f0_bs, int B, int C, int G, int H, int W, int r, int grid_based, int win_h,
                               int win_w, int sample_mode, int padding_mode, gfn_stream_t stream);
/* F.grid_sample(in, grid, mode, padding_mode, align_corners=False): in (B,C,H,W) stored as in_dtype = GFN_F32 or GFN_F16,
 * grid (B,Ho,Wo,2) fp32 -> out (B,C,Ho,Wo) fp32 with batch stride out_bs. */
int gfn_grid_sample_mode_fwd(const void *in, int in_dtype, const float *grid, float *out, int64_t out_bs, int B, int C, int H, int W,
                             int Ho, int Wo, int sample_mode, int padding_mode, gfn_stream_t stream);
/* gfn_refiner_input_fwd_dt (same arguments and `symmetric` bits, GFN_RI_KEEP_GRID_FEATURE included) with both grid_samples in
 * `sample_mode`; padding is always zeros, as in the reference's ConvRefiner.  Fill the local-correlation slice with
 * gfn_local_corr_mode_fwd (f0 = d, out = d + (2C+disp)*G*G, batch strides d_bs). */
int gfn_refiner_input_mode_fwd_dt(const void *f0, const void *f1, int dtype, const float *flow, const float *disp_w, const float *disp_b,
                                  float *d, int64_t d_bs, int B, int C, int Hs, int Ws, int G, int disp_dim, float disp_scale,
                                  int symmetric, int sample_mode, gfn_stream_t stream);

/* F.interpolate(x, size=(Ho,Wo), mode='bilinear', align_corners=False) -- model/network.py:238-249,
 * 271-281, 333-335.  in (BC,H,W) -> out (BC,Ho,Wo). */
int gfn_interp_bilinear_fwd(const float *in, float *out, int BC, int H, int W, int Ho, int Wo, gfn_stream_t stream);
/* Its adjoint: grad_out (BC,Ho,Wo) -> grad_in (BC,H,W), OVERWRITTEN.  A gather: one thread per input pixel visits the outputs
 * whose two source taps can include it (membership and weights from the forward's own tap set-up; at the clamped border both taps
 * of an output can be the same pixel and both weights count) and adds them in ascending (row, column) order, in double, rounded to
 * fp32 once.  No atomics: the same bits on every run.  Any ratio; same size limits as the forward. */
int gfn_interp_bilinear_bwd(const float *grad_out, float *grad_in, int BC, int H, int W, int Ho, int Wo, gfn_stream_t stream);
/* The same for two tensors of one spatial size in a single launch -- the flow (B,2,H,W) and certainty (B,1,H,W) pair the
 * scale loop resizes together at model/network.py:238-249 and 271-281. */
int gfn_interp_bilinear_pair_fwd(const float *in_a, float *out_a, int BCa, const float *in_b, float *out_b, int BCb, int H, int W,
                                 int Ho, int Wo, gfn_stream_t stream);

/* Flow/certainty accumulation of one refiner iteration -- model/network.py:262-268, in place:
 *   disp = scale * (delta[:,0]/(4*W0), delta[:,1]/(4*H0)); eval mode (zero_small): components with
 *   |disp - disp_prev| / |disp_prev| < 1e-6 are zeroed (disp_prev = 1e-7 when first_iteration);
 *   flow += disp; certainty += delta[:,2]; disp_prev <- disp.
 * flow (B,2,G,G), certainty (B,1,G,G), delta (B,>=3,G,G) with batch stride delta_bs, disp_prev (B,2,G,G). */
int gfn_flow_update_fwd(float *flow, float *certainty, const float *delta, int64_t delta_bs, float *disp_prev, int B, int G,
                        int scale, int W0, int H0, int zero_small, int first_iteration, gfn_stream_t stream);
/* The same step out of place and with the refiner's two outputs as they come (network.py:259-268 keeps every iteration's
 * flow and certainty): flow_out = flow_in + disp(dflow), cert_out = cert_in + dcert; dflow (B,>=2,G,G) with batch stride
 * dflow_bs, dcert (B,>=1,G,G) with dcert_bs.  Outputs may alias the inputs.  disp_prev may be NULL when first_iteration is
 * set and no further iteration follows at this scale (the displacement is then not stored). */
int gfn_flow_update_out_fwd(const float *flow_in, const float *cert_in, float *flow_out, float *cert_out, const float *dflow,
                            int64_t dflow_bs, const float *dcert, int64_t dcert_bs, float *disp_prev, int B, int G, int scale,
                            int W0, int H0, int zero_small, int first_iteration, gfn_stream_t stream);
/* gfn_flow_update_out_fwd followed by gfn_interp_bilinear_pair_fwd of its two results to the next grid, in one launch --
 * model/network.py:262-268 and 271-281: the last update of a scale and the resize that seeds the next one.  A workgroup
 * updates 16 x 16 cells plus a one-cell halo into LDS, writes its cells to flow_out / cert_out (and disp_prev) and
 * interpolates flow_next (B,2,G_next,G_next) / cert_next (B,1,G_next,G_next) from LDS; all five results are bit for bit
 * those of the two calls.  G_next must be G or 2 * G (anything else: GFN_ERR_INVALID_ARG, use the two calls).  Outputs must
 * NOT alias the inputs here (neighbouring workgroups read each other's input cells).  When disp_prev is read and written
 * (zero_small, not first_iteration) it is stored by a second small launch for the same reason. */
int gfn_flow_update_resize_fwd(const float *flow_in, const float *cert_in, float *flow_out, float *cert_out, const float *dflow,
                               int64_t dflow_bs, const float *dcert, int64_t dcert_bs, float *disp_prev, int B, int G, int scale,
                               int W0, int H0, int zero_small, int first_iteration, float *flow_next, float *cert_next, int G_next,
                               gfn_stream_t stream);

/* match() post-processing -- model/network.py:332-338 + 358-384.
 *   flow (nb,2,G,G), certainty (nb,1,G,G) finest-scale logits, nb = 2*B_images when symmetric;
 *   cert16_or_null (nb,1,Gc,Gc): scale-16 certainty for the attenuation term, or NULL;
 *   warp (B_images, G, Gw, 4), cert_out (B_images, G, Gw), Gw = 2G (symmetric) or G.
 *   A NaN flow component stays NaN in the warp and does not touch the certainty, as torch.clamp and `> 1` do (:368-371). */
int gfn_match_post_fwd(const float *flow, const float *certainty, const float *cert16_or_null, float *warp, float *cert_out,
                       int B_images, int G, int Gc, int symmetric, gfn_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Gaussian KDE -- utils/kde.py:4-13 (called from GFNet.sample, model/network.py:408).
 *   out[bt,n] = sum_m exp(-|x[bt,n] - y[bt,m]|^2 / (2 std^2))
 * x (Bt,N,D) contiguous; y: Bt blocks of M rows, row stride y_row_stride floats (= down*D for
 * x[::down]), batch stride y_batch_stride floats; out (Bt,N).  scratch: optional device buffer of
 * gfn_kde_scratch_floats(...) floats (pre-scaled copies + split-M partial sums); with less the
 * call falls back to a slower single-pass kernel but stays correct.
 */
int gfn_kde_msplit(int Bt, int N, int M);
int64_t gfn_kde_scratch_floats(int Bt, int N, int M, int D);
int gfn_kde_density(const float *x, const float *y, float *out, int Bt, int N, int M, int D, int64_t y_row_stride,
                    int64_t y_batch_stride, double std, float *scratch, int64_t scratch_floats, gfn_stream_t stream);

/* Spatially culled KDE for 4-D matches (same sum as gfn_kde_density up to terms below 2^-32): the
 * caller orders x and y by gfn_kde_morton_keys (any stable sort of the int keys) and passes the
 * sorted arrays; out is in the order of the sorted x (or the original one, see perm).  scratch: gfn_kde_sorted_scratch_floats().
 * Blocks of 64 reference points farther than 6.7 std from a wave's 64 queries are skipped.
 * Supported domain: the exponent is formed on the matrix core as |x|^2 + |y|^2 - 2 x.y with fp32 accumulators, so its error
 * grows with (|coordinate| / std)^2 and not with the distance.  The 1e-4 relative parity with float64 holds for
 * |coordinate| <= 16 std (measured 6e-5 at that edge; 2e-4 at 30 std, 3e-3 at 100 std: DESIGN.md).  The extent is data and
 * is not checked; std is: gfn_kde_density_sorted refuses std < GFN_KDE_SORTED_MIN_STD = 1/16, the edge for image coordinates
 * in [-1, 1].  gfn_kde_density (difference form) has no such limit. */
#define GFN_KDE_SORTED_MIN_STD 0.0625
int gfn_kde_morton_keys(const float *x, int *keys, int64_t n, gfn_stream_t stream);
/* The order itself: rows of x (Bt,N,4) stably sorted by their Morton key, one launch.  x_sorted (Bt,N,4),
 * perm (Bt,N): x_sorted[b][i] = x[b][perm[b][i]]; scratch: Bt*N ints. */
int gfn_kde_morton_sort(const float *x, float *x_sorted, int *perm, int *scratch, int Bt, int N, gfn_stream_t stream);
int64_t gfn_kde_sorted_scratch_floats(int Bt, int N, int M);
/* perm (Bt,N) from gfn_kde_morton_sort of x, or NULL: with it the densities are written in the caller's original order
 * (out[b][perm[b][i]] = density of x_sorted[b][i]); without it, in the sorted order. */
int gfn_kde_density_sorted(const float *x, const float *y, float *out, const int *perm, int Bt, int N, int M, double std,
                           int round_fp16, float *scratch, int64_t scratch_floats, gfn_stream_t stream);
/* round_fp16: coordinates rounded to fp16 before use, as GFNet.sample hands them to kde() (network.py:408, kde.py:6). */

/* GFNet.sample's elementwise steps (model/network.py:385-414):
 *   gfn_threshold_certainty: out = certainty > thresh ? 1 : certainty            (:391-393)
 *   gfn_balance_weights:     p = density < min_density ? floor_p : 1/(density+1)  (:409-410; 10, 1e-7)
 * (the two torch.multinomial draws stay with torch's generator, as in the reference). */
int gfn_threshold_certainty(const float *certainty, float *out, int64_t n, float thresh, gfn_stream_t stream);
int gfn_balance_weights(const float *density, float *p, int64_t n, float min_density, float floor_p, int round_fp16,
                        gfn_stream_t stream);  /* round_fp16: density rounded to fp16 first (kde(half=True) returns fp16, kde.py:13) */

/* Weighted sampling without replacement -- the two torch.multinomial(p, num_samples, replacement=False) draws of
 * GFNet.sample (model/network.py:400-402, 411-413).  Exponential race like torch's implementation (key = w / Exp(1),
 * the num_samples largest keys win) with a counter-based generator: same distribution, its own random stream, the same
 * result for the same seed.  weights (Bt,N) with row stride row_stride (non-negative; zero-weight entries are drawn only
 * when fewer than K positive ones exist), out (Bt,K) int64 indices in increasing order, scratch: Bt*(N + 2048) ints.
 * After the call, scratch[:Bt*N] holds the keys as bit patterns and the next Bt*2048 ints hold the first-pass histogram
 * (per row, the counts of the keys' top 11 bits).
 * one_above: weights above it count as 1 -- the certainty threshold of model/network.py:391-393 applied on the fly
 * (+INFINITY: off). */
int gfn_sample_without_replacement(const float *weights, int64_t row_stride, int64_t *out, int *scratch, int Bt, int N, int K,
                                   uint64_t seed, float one_above, gfn_stream_t stream);
/* The gathers that follow a draw (model/network.py:403-404, 414): out_matches[b][i] = matches[b][idx[b][i]] (rows of four
 * floats, 16-byte aligned), out_certainty[b][i] = certainty[b][idx[b][i]], thresholded like above.  matches (Bt,N,4),
 * certainty (Bt,N), idx (Bt,K) int64. */
int gfn_gather_matches(const float *matches, const float *certainty, const int64_t *idx, float *out_matches, float *out_certainty,
                       int Bt, int N, int K, float one_above, gfn_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Homography solve -- estimation.py:60-77 (cv2.findHomography(..., cv2.RANSAC, confidence=0.99999,
 * ransacReprojThreshold=3) in the reference; OpenCV's published pipeline restated, see
 * oracle/homography_oracle.c) and estimation.py:26-45 (convert_coordinates).
 *
 * gfn_convert_matches: matches (n,4) normalised warp rows -> pts (n,4) pixel (x,y,u,v), float32,
 *   (w-1)*(x+1)/2 per coordinate.
 * gfn_homography_ransac: pts (Bt,N,4) pixels -> H (Bt,9) row-major double (H[8] = 1),
 *   ninl (Bt) inlier count of the chosen hypothesis, best_t (Bt) its index or -1,
 *   mask (Bt,N) bytes or NULL.  Failure (fewer than 4 inliers / degenerate) gives diag(0,0,1),
 *   the reference's convention (estimation.py:74-76).  stage: 0 = RANSAC -> DLT on inliers ->
 *   lm_iters LM steps; 1 = RANSAC only; 2 = RANSAC + DLT.  scratch: gfn_homography_scratch_bytes().
 * gfn_homography_dlt: one-shot weighted normalised DLT ("grid-DLT"): weight (Bt,N) float or NULL;
 *   ok (Bt) = 1 on success.
 */
int gfn_convert_matches(const float *matches, float *pts, int64_t n, float wA, float hA, float wB, float hB,
                        gfn_stream_t stream);
int64_t gfn_homography_scratch_bytes(int Bt, int iters);
int gfn_homography_ransac(const float *pts, int Bt, int N, double thresh, int iters, uint64_t seed, int lm_iters, int stage,
                          double *H, int *ninl, int *best_t, unsigned char *mask, void *scratch, int64_t scratch_bytes,
                          gfn_stream_t stream);
/* The same with OpenCV's termination rule (cv::RANSACPointSetRegistrator::run): 0 < confidence < 1 -- whenever a hypothesis
 * beats the best inlier count so far the iteration bound becomes log(1 - confidence) / log(1 - w^4), w = its inlier ratio
 * (estimation.py:66-72 passes 0.99999); confidence <= 0 scores all `iters` hypotheses like gfn_homography_ransac.  In both
 * modes a 4-point subset with collinear points or inconsistent orientation is re-drawn (checkSubset).  iters_used (Bt) or
 * NULL: the bound each pair stopped at. */
int gfn_homography_ransac_ex(const float *pts, int Bt, int N, double thresh, int iters, double confidence, uint64_t seed, int lm_iters,
                             int stage, double *H, int *ninl, int *best_t, unsigned char *mask, int *iters_used, void *scratch,
                             int64_t scratch_bytes, gfn_stream_t stream);
int gfn_homography_dlt(const float *pts, const float *weight, int Bt, int N, double *H, int *ok, gfn_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Image resize + normalise in front of the backbone -- GFNet.match's
 * get_tuple_transform_ops(resize, mode, normalize=True), model/network.py:293-346 with utils/utils.py:18-27,
 * 87-116: torchvision Resize on a float tensor with antialias=None (= F.interpolate(mode,
 * align_corners=False), no antialiasing) followed by Normalize on the first three channels.
 *   in (B, >=3, H, W) floats in [0,1], batch stride in_bs floats; out (B,3,Ho,Wo) = (resize(in[:, :3]) - mean) / std;
 *   mode 0 = bilinear (the reference's mode=2: path inputs and the upsample pass), 1 = bicubic (PIL / tensor
 *   inputs); mean3 / std3: three host floats each (ImageNet statistics in the reference).
 */
int gfn_resize_normalize_fwd(const float *in, int64_t in_bs, float *out, int B, int H, int W, int Ho, int Wo, int mode,
                             const float *mean3, const float *std3, gfn_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Refiner conv stack -- ConvRefiner.create_block / forward, model/network.py:471-487
 * and :560-563: nine blocks of depthwise 5x5 conv -> BatchNorm2d(eval) -> ReLU -> 1x1 conv, then a
 * final 1x1 conv to 3 channels.  Depthwise, norm and accumulation always fp32; the 1x1 products fp32
 * (default) or fp16.
 *
 * gfn_conv_block_pack: lays one block's parameters out for the kernels (device to device):
 *   dw_w (C,25) depthwise taps, dw_b (C) or NULL, bn_alpha/bn_beta (C) the eval-mode BatchNorm as
 *   y = x*alpha + beta (alpha = weight/sqrt(running_var+eps), beta = bias - running_mean*alpha),
 *   pw_w (M,C) and pw_b (M) the 1x1 conv; packed: gfn_conv_block_packed_floats(C, M) floats.
 * gfn_conv_block_fwd: y = pw(relu(bn(dw(x)))) for x (B,C,G,G) -> y (B,M,G,G), zero padding 2; y must
 *   not alias x.  variant bit 0 (1): two-pass form (depthwise kernel -> t_scratch (B*C*G*G floats) ->
 *   GEMM kernel) instead of the fused kernel; also taken when G % 4 != 0; bit-identical results.
 *   variant bit 1 (2): the 1x1 conv takes fp16 operands (W and relu output rounded to nearest fp16,
 *   v_mfma_f32_32x32x16_f16, fp32 accumulation) -- the reference's autocast numerics class for its
 *   amp=True refiners (model/network.py:560-562) -- instead of fp32 throughout.  t_scratch may be NULL
 *   when the fused kernel applies.
 * gfn_pointwise_conv_fwd: y[b] = W . t[b] + bias for a few output channels (M <= 16; the final C -> 3
 *   conv, network.py:505,563): w (M,K), t (B,K,N), y (B,M,N).
 */
int64_t gfn_conv_block_packed_floats(int C, int M);
int gfn_conv_block_pack(const float *dw_w, const float *dw_b, const float *bn_alpha, const float *bn_beta, const float *pw_w,
                        const float *pw_b, float *packed, int C, int M, gfn_stream_t stream);
int gfn_conv_block_fwd(const float *x, const float *packed, float *y, float *t_scratch, int B, int C, int M, int G, int variant,
                       gfn_stream_t stream);
int gfn_pointwise_conv_fwd(const float *w, const float *bias, const float *t, float *y, int B, int M, int K, int N,
                           gfn_stream_t stream);

/* gfn_conv_block_half_fwd: the same block with fp16 maps in HBM -- the reference's amp=True refiners, where every map
 *   between two blocks is a float16 tensor (torch.autocast around block1 + hidden_blocks, model/network.py:560-562).
 *   Arithmetic = the autocast class: the depthwise 5x5 runs on the matrix core too (v_mfma_f32_16x16x32_f16: the input halo --
 *   also a first block's fp32 concat -- and the folded taps rounded to fp16, fp32 accumulation), BatchNorm + ReLU fp32, ReLU output
 *   and 1x1 weights fp16, fp32 accumulation.  A map of dtype GFN_F16 is (B, ceil(C/2), G, G) of half2: channels 2p and 2p+1 of
 *   a cell side by side, the odd channel past C zero (the kernel writes it so).  x_dtype / y_dtype: GFN_F32 (B, C, G, G) floats or GFN_F16; at least one of them GFN_F16 (a
 *   stack's first block reads the fp32 concat, its last one writes fp32).  G must be a multiple of 4.
 *   Locality of a non-finite input: gfn_conv_block_fwd multiplies a cell only by the taps that reach it, so an inf / NaN at cell
 *   (i, j) of one channel makes y non-finite (over all M) at most at |drow| <= 2, |dcol| <= 2.  Here the depthwise is a banded
 *   matrix product: a 16-cell window of a halo row is multiplied by the band's zero entries too (0 * inf = NaN), and the two
 *   channels of a pair share the window.  y may be non-finite at |drow| <= 2, |dcol| <= 11 of the cell, whichever channel of
 *   the pair held it -- the zero odd channel past M of a half map included (0 * inf) --; every other value of y has the bits
 *   of the call without it.  In both entry points a NaN that reaches the ReLU ends there (fmaxf(NaN, 0) = 0: such a cell
 *   contributes 0 to the 1x1 conv, where torch's relu would hand the NaN on); +inf passes it. */
int gfn_conv_block_half_fwd(const void *x, int x_dtype, const float *packed, void *y, int y_dtype, int B, int C, int M, int G,
                            gfn_stream_t stream);

/* gfn_conv_block_bf16_fwd: the same block with bf16 maps in HBM -- the refiners under torch.autocast(dtype=torch.bfloat16)
 *   (model/network.py:560-562 under amp_dtype=torch.bfloat16), the class a model trained with gfn_conv_block_train_bf16_* is
 *   evaluated in.  gfn_conv_block_half_fwd's kernel on the bf16 instructions, the same tile shapes and routes.
 *   Arithmetic class: depthwise 5x5 on v_mfma_f32_16x16x32_bf16 (the input halo -- also a first block's fp32 concat -- and the
 *   folded taps rounded to bf16, fp32 accumulation), BatchNorm + ReLU fp32, ReLU output and 1x1 weights bf16 on
 *   v_mfma_f32_32x32x16_bf16, fp32 accumulation and bias; a bf16 output is rounded once, to nearest even.  bf16 has fp32's exponent
 *   range: nothing that is finite in fp32 becomes inf here (an fp16 map ends at 65504).
 *   packed: from gfn_conv_block_pack_bf16 -- the arguments, layout and gfn_conv_block_packed_floats size of gfn_conv_block_pack, with
 *   the two 16-bit sections (1x1 weights, banded depthwise taps) rounded to bf16 instead of fp16; every fp32 section is the same.
 *   A block packed for one class must not be handed to the other entry point (the sizes agree: nothing can check it).
 *   A map of dtype GFN_BF16 is (B, ceil(C/2), G, G) of bf16 pairs: the half map's layout, the odd channel past C zero (the kernel
 *   writes it so).  x_dtype / y_dtype: GFN_F32 or GFN_BF16, at least one of them GFN_BF16; GFN_F16 is refused with a message.
 *   G % 4 == 0, x != y, and the size limits of gfn_conv_block_half_fwd.
 *   Locality of a non-finite input: gfn_conv_block_half_fwd's envelope -- y may differ from the call without the value at
 *   |drow| <= 2, |dcol| <= 11 of its cell, in every output channel, whichever channel of the pair held it (the zero odd channel
 *   past M of a bf16 map included); every other value of y keeps its bits.  A NaN that reaches the ReLU ends there, +inf passes. */
int gfn_conv_block_pack_bf16(const float *dw_w, const float *dw_b, const float *bn_alpha, const float *bn_beta, const float *pw_w,
                             const float *pw_b, float *packed, int C, int M, gfn_stream_t stream);
int gfn_conv_block_bf16_fwd(const void *x, int x_dtype, const float *packed, void *y, int y_dtype, int B, int C, int M, int G,
                            gfn_stream_t stream);

/* gfn_conv_block_route: the launch decision of gfn_conv_block_fwd (entry = GFN_CBR_ENTRY_FWD, a = variant, b ignored),
 *   gfn_conv_block_half_fwd (entry = GFN_CBR_ENTRY_HALF, a = x_dtype, b = y_dtype) or gfn_conv_block_bf16_fwd (entry =
 *   GFN_CBR_ENTRY_BF16, a = x_dtype, b = y_dtype: field for field the answer of GFN_CBR_ENTRY_HALF for the same shape with GFN_F16
 *   where this one has GFN_BF16) for a shape, answered on the host: no device,
 *   no stream (csrc/conv_block_fused.h conv_route, the struct the launchers themselves switch on).  Fills route[GFN_CBR_*]
 *   (route_len >= GFN_CBR_FIELDS ints) and returns GFN_CBR_FIELDS; returns 0, route untouched, where the entry point would refuse
 *   the shape (gfn_last_error says why).  FUSED: 1 = dwpw_fused_kernel, then TW, MT, NS, NB, KW are its template parameters, NGRP
 *   slab groups of 32*MT*NS output channels, TILES_X x TILES_Y cell tiles of TW x (128*NB/TW) cells per map, NWORK = B * tiles *
 *   NGRP work items, TPB of them per workgroup; 0 = the two-pass form: dw5x5_kernel<VEC>, then pw_gemm_kernel<GEMM_MT> over NBLK
 *   row blocks.  F16: 16-bit 1x1 operands; HIN / HOUT: 16-bit map in / out (fp16 or bf16, as the entry says); MM: matrix-core
 *   depthwise.  Fields of the other form: 0. */
#define GFN_CBR_ENTRY_FWD 0
#define GFN_CBR_ENTRY_HALF 1
#define GFN_CBR_ENTRY_BF16 2
#define GFN_CBR_FUSED 0
#define GFN_CBR_TW 1
#define GFN_CBR_MT 2
#define GFN_CBR_NS 3
#define GFN_CBR_NB 4
#define GFN_CBR_KW 5
#define GFN_CBR_F16 6
#define GFN_CBR_HIN 7
#define GFN_CBR_HOUT 8
#define GFN_CBR_MM 9
#define GFN_CBR_NGRP 10
#define GFN_CBR_NWORK 11
#define GFN_CBR_TPB 12
#define GFN_CBR_VEC 13
#define GFN_CBR_NBLK 14
#define GFN_CBR_GEMM_MT 15
#define GFN_CBR_TILES_X 16
#define GFN_CBR_TILES_Y 17
#define GFN_CBR_FIELDS 18
int gfn_conv_block_route(int entry, int a, int b, int B, int C, int M, int G, int *route, int route_len);

/* One conv block in TRAINING mode (model.train(); ConvRefiner.create_block / forward, model/network.py:471-487, 560-563, which
 * torch autograd differentiates in the reference): Conv2d(C,C,5,pad 2,groups=C[,bias]) -> BatchNorm2d on the batch's own
 * statistics -> ReLU -> Conv2d(C,M,1), fp32 throughout on contiguous maps; csrc/conv_stack_train.hip.  Every reduction is
 * two-stage in a fixed order (no floating-point atomics): identical calls give identical bits.
 *
 * gfn_conv_block_train_fwd: x (B,C,G,G) -> u = dw5x5(x) + dw_b (B,C,G,G; kept for the backward), mean and invstd (C) of u over
 *   the batch (biased variance; per-tile shifted sums merged with Chan's formula in double), y = pw(relu(bn(u))) (B,M,G,G) with
 *   the 1x1 products on the exact-fp32 matrix core.  dw_w (C,25), dw_b (C) or NULL, bn_w / bn_b (C) BatchNorm's weight and bias,
 *   pw_w (M,C), pw_b (M).  running_mean / running_var (C) are updated in place as torch does: (1 - momentum) * old + momentum *
 *   batch value, the variance unbiased (n / (n - 1)); B*G*G >= 2.  x, u and y must be three different maps.
 * gfn_conv_block_train_bwd: gy = dL/dy (B,M,G,G), and x, u, mean, invstd, dw_w, bn_w, bn_b, pw_w as the forward had them ->
 *   gx (B,C,G,G), d_dw_w (C,25), d_dw_b (C), d_bn_w, d_bn_b (C), d_pw_w (M,C), d_pw_b (M), all OVERWRITTEN.  `need` is a sum of
 *   GFN_CBT_NEED_*: only what it names is computed and only those pointers are touched (d_dw_b may be NULL with GFN_CBT_NEED_DW:
 *   a block without depthwise bias); need = 0 launches nothing.  The ReLU mask is recomputed from u with the forward's expression.
 * ws: gfn_conv_block_train_ws_bytes(B, C, M, G, backward = 0 / 1) bytes of 16-byte aligned device memory, contents undefined
 *   before and after (the backward keeps its gz map there).  Limits: B <= 65535, C*G*G and M*G*G <= 2^29 - 1. */
#define GFN_CBT_NEED_X 1  /* gx */
#define GFN_CBT_NEED_DW 2 /* d_dw_w, d_dw_b */
#define GFN_CBT_NEED_BN 4 /* d_bn_w, d_bn_b */
#define GFN_CBT_NEED_PW 8 /* d_pw_w, d_pw_b */
#define GFN_CBT_NEED_ALL 15
int64_t gfn_conv_block_train_ws_bytes(int B, int C, int M, int G, int backward);
int gfn_conv_block_train_fwd(const float *x, const float *dw_w, const float *dw_b, const float *bn_w, const float *bn_b,
                             float *running_mean, float *running_var, const float *pw_w, const float *pw_b, float *u, float *mean,
                             float *invstd, float *y, int B, int C, int M, int G, double momentum, double eps, void *ws,
                             int64_t ws_bytes, gfn_stream_t stream);
int gfn_conv_block_train_bwd(const float *gy, const float *x, const float *u, const float *mean, const float *invstd,
                             const float *dw_w, const float *bn_w, const float *bn_b, const float *pw_w, float *gx, float *d_dw_w,
                             float *d_dw_b, float *d_bn_w, float *d_bn_b, float *d_pw_w, float *d_pw_b, int B, int C, int M, int G,
                             int need, void *ws, int64_t ws_bytes, gfn_stream_t stream);

/* The same block in the reference's autocast training class (every ConvRefiner has amp=True, model/network.py:90-152, and
 * trainer/train.py:29-43 scales the loss): fp16 maps in HBM; csrc/conv_stack_train_half.hip.  The entry points above are fp32
 * throughout and unchanged.
 *
 * Maps -- x, u, y, gy, gx -- are plain contiguous (B,C,G,G) fp16 (torch.float16; NOT the half2 channel-pair layout of
 *   gfn_conv_block_half_fwd), any C and any G.  x_dtype = GFN_F32 makes x the fp32 concat of a stack's first block: it is rounded
 *   to fp16 on load, and gx is then fp32, unrounded.  Parameters, their gradients, mean and invstd are fp32; depthwise taps and 1x1
 *   weights are rounded to fp16 where they are operands.  Every sum is fp32 (statistics merged in double); u is rounded once and
 *   statistics, normalisation and backward read that rounded u; t = relu(bn(u)) is rounded as the 1x1 operand; the backward's gz
 *   map is rounded before BatchNorm's backward reads it.  The three 1x1 products run on v_mfma_f32_32x32x16_f16.  Rounding is to
 *   nearest even and overflows to inf (never clamps to 65504), so a loss scale that is too large shows in the gradients.
 * Arguments, `need`, limits, the running-buffer update and bit-for-bit reproducibility are those of the fp32 entry points;
 *   ws: gfn_conv_block_train_half_ws_bytes bytes, 16-byte aligned. */
int64_t gfn_conv_block_train_half_ws_bytes(int B, int C, int M, int G, int backward);
int gfn_conv_block_train_half_fwd(const void *x, int x_dtype, const float *dw_w, const float *dw_b, const float *bn_w,
                                  const float *bn_b, float *running_mean, float *running_var, const float *pw_w, const float *pw_b,
                                  void *u, float *mean, float *invstd, void *y, int B, int C, int M, int G, double momentum,
                                  double eps, void *ws, int64_t ws_bytes, gfn_stream_t stream);
int gfn_conv_block_train_half_bwd(const void *gy, const void *x, int x_dtype, const void *u, const float *mean, const float *invstd,
                                  const float *dw_w, const float *bn_w, const float *bn_b, const float *pw_w, void *gx,
                                  float *d_dw_w, float *d_dw_b, float *d_bn_w, float *d_bn_b, float *d_pw_w, float *d_pw_b, int B,
                                  int C, int M, int G, int need, void *ws, int64_t ws_bytes, gfn_stream_t stream);

/* The same block in the bf16 autocast class (a ConvRefiner built with amp=True, amp_dtype=torch.bfloat16): bf16 maps in HBM;
 * csrc/conv_stack_train_bf16.hip, the same kernels as the fp16 class over another element (csrc/conv_train_16bit.h).  bf16 keeps
 * fp32's exponent range, so nothing overflows at 65504 and a step in this class needs no loss scale.
 *
 * Maps -- x, u, y, gy, gx -- are plain contiguous (B,C,G,G) bf16 (torch.bfloat16), any C and any G.  x_dtype = GFN_F32 makes x the
 *   fp32 concat of a stack's first block: it is rounded to bf16 on load, and gx is then fp32, unrounded; x_dtype = GFN_BF16 a bf16
 *   map; GFN_F16 is refused.  Parameters, their gradients, mean and invstd are fp32; depthwise taps and 1x1 weights are rounded to
 *   bf16 where they are operands.  Every sum is fp32 (statistics merged in double); u is rounded once and statistics, normalisation
 *   and backward read that rounded u; t = relu(bn(u)) is rounded as the 1x1 operand; the backward's gz map is rounded before
 *   BatchNorm's backward reads it.  The three 1x1 products run on v_mfma_f32_32x32x16_bf16.  Rounding is to nearest even with no
 *   clamp; inf and NaN propagate.
 * Arguments, `need`, limits, the running-buffer update and bit-for-bit reproducibility are those of the fp32 entry points;
 *   ws: gfn_conv_block_train_bf16_ws_bytes bytes, 16-byte aligned. */
int64_t gfn_conv_block_train_bf16_ws_bytes(int B, int C, int M, int G, int backward);
int gfn_conv_block_train_bf16_fwd(const void *x, int x_dtype, const float *dw_w, const float *dw_b, const float *bn_w,
                                  const float *bn_b, float *running_mean, float *running_var, const float *pw_w, const float *pw_b,
                                  void *u, float *mean, float *invstd, void *y, int B, int C, int M, int G, double momentum,
                                  double eps, void *ws, int64_t ws_bytes, gfn_stream_t stream);
int gfn_conv_block_train_bf16_bwd(const void *gy, const void *x, int x_dtype, const void *u, const float *mean, const float *invstd,
                                  const float *dw_w, const float *bn_w, const float *bn_b, const float *pw_w, void *gx,
                                  float *d_dw_w, float *d_dw_b, float *d_bn_w, float *d_bn_b, float *d_pw_w, float *d_pw_b, int B,
                                  int C, int M, int G, int need, void *ws, int64_t ws_bytes, gfn_stream_t stream);

/* The training objective on a homography ground truth (losses/robust_loss.py: get_gt_warp_homography :9-42,
 * RobustLosses.regression_loss :65-90 and the per-scale body of RobustLosses.forward :92-128); csrc/robust_loss.hip.  One call
 * is one scale with all of its iterations; fp32 contiguous maps on an h x w grid, batch B.
 *
 * The ground-truth warp of a cell (never stored by the loss): its centre x1_n = linspace(-1 + 1/n, 1 - 1/n, n) per axis (x from
 *   w, y from h), or im_A_coords (B,2,h,w) when given; pixels x1 = (x1_n + 1) * ext_a * 0.5 with ext_a = im_A.shape[2] - 1 on BOTH
 *   axes (:25); x2 = H (B,3,3) applied to (x1, 1), divided by z (by 1 where |z| <= 1e-8; kornia's transform_points :26);
 *   x2_n = x2 / ext_b * 2 - 1 with ext_b = im_B.shape[2] - 1 > 0 (:28-29); prob = 1 where both coordinates of x2_n lie strictly
 *   inside (-1, 1), else 0 (:31-33).  With prev_epe (B,ph,pw), the previous scale's last end-point error, prob is further
 *   multiplied by [prev_epe at the nearest-exact source cell min(floor((i + 0.5) * in / out), in - 1) < prev_thresh] (:117-120).
 * gfn_gt_warp_homography_fwd: out (B,h,w,2) = x2_n (normalized != 0) or x2, prob (B,h,w), x1_n (B,h,w,2) unless NULL.
 * gfn_robust_loss_fwd: flows / certs are HOST arrays of n_itr (1..8) device pointers, flow_k (B,2,h,w) and cert_k (B,1,h,w) of
 *   iteration k = 1..n_itr in order.  With w_k = iteration_base ** (n_itr - k), epe_k = ||flow_k - x2_n||:
 *     ce  = sum_k w_k * mean over all B*h*w cells of binary_cross_entropy_with_logits(cert_k, prob)                  (:77-78)
 *     reg = (sum over cells with prob = 1 of sum_k w_k * cs^a * ((epe_k / cs)^2 + 1)^(a/2)) / count, 0 when count = 0  (:81-84)
 *   stats (8 floats, GFN_RL_STAT_*): loss = ce_weight * ce + reg, ce, reg, count, pck = the fraction of masked cells whose last
 *   iteration has epe < pck_thresh (0 when count = 0; :73-74), the number of cells, the unnormalised regression sum, 0.
 *   epe_last (B,h,w), unless NULL, receives the last iteration's epe of every cell: the next scale's prev_epe (:115, :127).
 *   Two launches: the streaming pass leaves one partial per block and quantity in ws (reduced per wave, then per block, in a fixed
 *   order), a single workgroup adds them in a fixed order in double.  No floating-point atomics: identical calls, identical bits.
 * gfn_robust_loss_bwd: the same inputs, stats as the forward left them and grad_out, a DEVICE scalar (dL/dloss) ->
 *     g_flows[k] (B,2,h,w) = grad_out * w_k / count * a * cs^(a-2) * ((epe_k / cs)^2 + 1)^(a/2 - 1) * (flow_k - x2_n), 0 off the mask
 *     g_certs[k] (B,1,h,w) = grad_out * ce_weight * w_k * (sigmoid(cert_k) - prob) / (B*h*w)
 *   OVERWRITTEN, for the iterations `need` names: bit k-1 asks for g_flows[k-1], bit 8+k-1 for g_certs[k-1]; other entries of the
 *   two host arrays (or the arrays themselves) may be NULL.  need = 0 launches nothing.  H, prev_epe and the mask carry no gradient.
 * Maps are read and written with 16- or 8-byte vector accesses when w is a multiple of 4 or 2 and every map pointer is so aligned.
 * ws: gfn_robust_loss_ws_bytes(B, h, w, n_itr) bytes, 16-byte aligned, contents undefined before and after.
 * Limits: h, w, ph, pw <= 32768, B*h*w <= 2^30, cs > 0; B = 0 is valid and launches nothing. */
#define GFN_RL_STAT_LOSS 0
#define GFN_RL_STAT_CE 1
#define GFN_RL_STAT_REG 2
#define GFN_RL_STAT_COUNT 3
#define GFN_RL_STAT_PCK 4
#define GFN_RL_STAT_CELLS 5
#define GFN_RL_STAT_RHO_SUM 6
#define GFN_RL_STATS 8
#define GFN_RL_MAX_ITR 8 /* the most iterations a scale may have: the length of the host pointer arrays, the stride of `need`'s halves */
int64_t gfn_robust_loss_ws_bytes(int B, int h, int w, int n_itr);
int gfn_robust_loss_fwd(const float *const *flows, const float *const *certs, int n_itr, const float *H, const float *im_A_coords,
                        const float *prev_epe, int ph, int pw, double prev_thresh, float *epe_last, float *stats, int B, int h, int w,
                        double ext_a, double ext_b, double a, double cs, double ce_weight, double iteration_base, double pck_thresh,
                        void *ws, int64_t ws_bytes, gfn_stream_t stream);
int gfn_robust_loss_bwd(const float *const *flows, const float *const *certs, int n_itr, const float *H, const float *im_A_coords,
                        const float *prev_epe, int ph, int pw, double prev_thresh, const float *stats, const float *grad_out,
                        float *const *g_flows, float *const *g_certs, int need, int B, int h, int w, double ext_a, double ext_b,
                        double a, double cs, double ce_weight, double iteration_base, gfn_stream_t stream);
int gfn_gt_warp_homography_fwd(const float *H, const float *im_A_coords, float *out, float *prob, float *x1_n, int B, int h, int w,
                               double ext_a, double ext_b, int normalized, gfn_stream_t stream);

/* What a training step does after backward() (trainer/train.py:29-43: grad_scaler.unscale_, log_param_statistics :13-27,
 * clip_grad_norm_, grad_scaler.step(optimizer) with torch.optim.AdamW, grad_scaler.update(), the floor of the scale at :40-41, and the
 * optimizer.zero_grad() of the next step :30); csrc/train_step.hip.  One call is one step over every parameter tensor: three launches
 * (ts_norm_kernel, ts_finish_kernel, ts_update_kernel), no host synchronisation, no atomics -- identical calls, identical bits.
 *
 * tensor_table: DEVICE array of n_tensors gfn_ts_tensor records, one per parameter that has a gradient.  p, g, exp_avg, exp_avg_sq are
 *   fp32, contiguous, numel elements each; lr .. eps are the parameter group's AdamW hyperparameters (amsgrad = maximize = False);
 *   first_chunk / n_chunks name the tensor's run of chunk records; vec16 != 0 allows 16-byte accesses and may be set only when all
 *   four pointers are 16-byte aligned (otherwise every access is a single float: gradients that are views at odd element offsets).
 * chunk_table: DEVICE array of n_chunks gfn_ts_chunk records, one per workgroup: elements first .. first + count - 1 of tensor
 *   `tensor`, 1 <= count <= GFN_TS_CHUNK, first a multiple of GFN_TS_CHUNK; no chunk spans two tensors, the chunks of a tensor are
 *   consecutive and ascending and cover it exactly once; a tensor of no elements has no chunk.
 * state: GFN_TS_STATE_BYTES on the DEVICE, read and written: float scale, int32 tracker (clean steps since the scale last changed),
 *   int64 step (AdamW's step count; it lives on the device because a skipped step must not advance it and the host does not look),
 *   float min_scale (read only), 12 bytes reserved.
 * The step: found_inf = any raw g is inf or nan; gu = g * (1 / scale); grad_norm = sqrt(sum gu^2) over all tensors and param_norm =
 *   sqrt(sum p^2) (the norm of the per-tensor norms, :18), accumulated in double, so that finite gradients never overflow them;
 *   clip_coef = min(1, max_norm / (grad_norm + 1e-6)).  Unless found_inf: step += 1 and per element, in fp32 and in the operation order
 *   of torch.optim.adam._single_tensor_adam with each op associated as ATen's CPU kernel does (addcmul_ as (value * a) * b, addcdiv_
 *   as (value * a) / b; ATen's device kernels associate the other way, one rounding apart), gu *= clip_coef, p *= 1 - lr * wd, m = lerp(m, gu, 1 - beta1), v = v * beta2 +
 *   (1 - beta2) * gu * gu, p += -(lr / (1 - beta1^step)) * m / (sqrt(v) / sqrt(1 - beta2^step) + eps); with found_inf none of p, m, v,
 *   step is written.  Then the scale (torch's _amp_update_scale_): found_inf -> scale *= backoff, tracker = 0; else tracker += 1 and at
 *   growth_interval scale *= growth (kept when that overflows), tracker = 0; then scale = max(scale, min_scale).
 *   zero_grads != 0 stores 0 to every g after reading it, on skipped steps too; otherwise g is left as it came in, still scaled.
 * stats_out: GFN_TS_STATS + n_tensors floats on the device: GFN_TS_STAT_* (grad_scale is the scale this step used), then one 0 / 1
 *   flag per tensor: its raw gradient held an inf or nan.
 * ws: gfn_train_step_ws_bytes(n_tensors, n_chunks) bytes, 16-byte aligned, contents undefined before and after.
 * Limits: n_tensors <= 2^20 (the single workgroup of ts_finish_kernel loops over them), n_chunks <= 2^23 (the grid).  n_tensors = 0
 *   is valid (the tables may be NULL): only the scale rule runs, with found_inf = 0, and the step count stays. */
#define GFN_TS_CHUNK 4096
#define GFN_TS_STATE_BYTES 32
#define GFN_TS_STAT_GRAD_NORM 0
#define GFN_TS_STAT_PARAM_NORM 1
#define GFN_TS_STAT_GRAD_SCALE 2
#define GFN_TS_STAT_FOUND_INF 3
#define GFN_TS_STAT_CLIP_COEF 4
#define GFN_TS_STATS 8
typedef struct gfn_ts_tensor {
    float *p, *g, *exp_avg, *exp_avg_sq;
    int64_t numel;
    double lr, wd, beta1, beta2, eps;
    int32_t first_chunk, n_chunks, vec16, reserved;
} gfn_ts_tensor; /* 96 bytes */
typedef struct gfn_ts_chunk {
    int32_t tensor, count;
    int64_t first;
} gfn_ts_chunk; /* 16 bytes */
int64_t gfn_train_step_ws_bytes(int n_tensors, int n_chunks);
int gfn_train_step(const gfn_ts_tensor *tensor_table, int n_tensors, const gfn_ts_chunk *chunk_table, int n_chunks, void *state,
                   double max_norm, double growth, double backoff, int growth_interval, int zero_grads, float *stats_out, void *ws,
                   int64_t ws_bytes, gfn_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Training pairs (the batch a training step consumes) -- datasets/generate_random_H_large_size.py:6-85 (random_four_points, randomH)
 * as datasets/homography_dataset_large_size.py:148-228 calls it per sample on host workers, with kornia's get_perspective_transform,
 * transform_points and warp_perspective; csrc/pair_synth.hip.  The crop, the 640 x 640 warp and the centre crop of an image are ONE
 * projective map from output pixels to source pixels, so a batch is one parameter launch and one warp launch and the intermediates
 * are never made.  The reference solves its 8 x 8 systems (entries up to 640^2) and inverts in fp32; here every solve, inverse and
 * pixel coordinate is double.  3 x 3 matrices are inverted as adjugate / determinant: exact for the identity and integer translations.
 *
 * gfn_perspective_from_points: kornia.geometry.transform.get_perspective_transform (generate_random_H_large_size.py:30, 71) for n
 *   four-point problems.  src, dst (n,4,2) float (x, y) -> H (n,3,3) double with H[8] = 1 and dst ~ H src.  The 8 x 8 system is
 *   kornia's (rows [x y 1 0 0 0 -xu -yu | u], [0 0 0 x y 1 -xv -yv | v]), solved for H - identity -- the right-hand side is then
 *   dst - src, which is exact, so src == dst gives the identity bit for bit -- by Gaussian elimination with partial pivoting, a row
 *   per lane (csrc/ge_solve8.h).  ok (n): 1, or 0 with H = identity when three of the source points lie on a line (or coincide),
 *   a pivot vanishes or a component is not finite.
 * gfn_random_h_params: randomH's geometry for B samples from their random draws.  draws (B,18) int32: crop_x, crop_y (:50-51), then
 *   the corner draws of image 1 and of image 2, each tl x,y; tr x,y; br x,y; bl x,y (:7-22; for bi = False the caller writes the
 *   target points of :23 into image 2's eight).  crop_size = the side of the crop (:53-54), deform_area (:57); out_h, out_w = the
 *   centre-cropped size crop_size - 2 * (deform_area / 2) (:34), checked; final_h, final_w = the size the images are resized to
 *   afterwards (:73-74).  Per sample: H_1t, H_2t (:23-30), H_1t2t = H_2t H_1t^-1, the corner flow and H_s2t (:62-71) and, when
 *   the final size differs from the output size, diag(final_h / out_h, final_h / out_h, 1) H_s2t diag(final_w / out_w, final_w /
 *   out_w, 1)^-1 -- :77-79 as written, the height ratio on both axes on the left, the width ratio on both on the right.  Writes
 *   H_s2t32 (B,3,3) float (what the reference hands to the loss), H_s2t64 (B,3,3) double, M_A and M_B (B,3,3) double: output pixel
 *   -> source-image pixel of the two images, translate(crop_x, crop_y) H_it^-1 translate(deform_area / 2, deform_area / 2), and
 *   ok (B): 1 when all three solves succeeded.  Any of the five outputs may be NULL.
 * gfn_warp_perspective_fwd: kornia's warp_perspective(align_corners=True, mode="bilinear", padding_mode="zeros") (:33, :83;
 *   homography_dataset_large_size.py:207) with the Normalize of :184-185 optionally fused.  out (B,C,Ho,Wo) float, batch stride
 *   out_bs: pixel (u, v) of sample b reads its source at (x, y) = (X / Z, Y / Z), (X, Y, Z) = M_b (u, v, 1), evaluated in double
 *   (invert != 0: M_b is first inverted, i.e. M holds kornia's source -> destination matrices); bilinear in PIXEL coordinates, a
 *   neighbour outside the source counting as 0; floor and fractions from the double, the blend in fp32 in the order
 *   (1-fy) * ((1-fx) * v00 + fx * v01) + fy * ((1-fx) * v10 + fx * v11); then (v - mean[c]) / std[c] when mean and std (C floats
 *   each, DEVICE memory) are given (both or neither).  A non-finite coordinate reads 0.  Sources are given per sample, so a batch
 *   may hold images of different sizes and views of larger buffers: src_planes, a DEVICE array of B pointers to channel 0 of each
 *   sample, and src_dims, DEVICE (B,3) int32 rows (H, W, channel stride in floats); rows are W floats apart, H * W < 2^31.
 *   No atomics: identical calls give identical bits.  B <= 65535; B, Ho or Wo = 0 is valid and launches nothing. */
int gfn_perspective_from_points(const float *src, const float *dst, double *H, int *ok, int n, gfn_stream_t stream);
int gfn_random_h_params(const int *draws, int B, int crop_size, int deform_area, int out_h, int out_w, int final_h, int final_w,
                        float *H_s2t32, double *H_s2t64, double *M_A, double *M_B, int *ok, gfn_stream_t stream);
int gfn_warp_perspective_fwd(const float *const *src_planes, const int *src_dims, const double *M, int invert, float *out,
                             int64_t out_bs, int B, int C, int Ho, int Wo, const float *mean, const float *std, gfn_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Photometric augmentation (decoded uint8 pixels -> the float images the pair synthesis consumes) -- the `initial_transforms` of
 * train.py:74-79 and :88-93: Resize(640), ColorJitter, RandomGrayscale, RandomGaussianBlur (datasets/homography_dataset_large_size.py:
 * 17-28), ToTensor, which the reference runs per image on host workers on PIL images; csrc/photometric.hip.  What executes there is
 * Pillow, and every stage here maps uint8 to uint8 with Pillow's arithmetic: pinned against Pillow 12.2.0, NOT against torchvision.
 * A batch holds images of different sizes: `src` / `dst` are DEVICE arrays of N pointers, dims DEVICE (N,3) int32 rows (H, W, row
 * stride in bytes) of (H,W,3) interleaved uint8 images.  max_h / max_w: the largest height and width in the batch (they size the
 * grid).  N <= 65535; N = 0 or an empty largest image is valid and launches nothing.  Pointer tables and sums are 8-byte aligned,
 * int tables 4-byte.  Identical calls give identical bits: the only atomics are the integer sums of gfn_photo_stats.
 *
 * gfn_photo_resize_u8: Image.resize(BILINEAR) (train.py:75 Resize(640), which antialiases on PIL images), both passes in one launch:
 *   a pass is clip8((sum_k w_k x_k + 2^21) >> 22) over the taps [min, min + count) of an output index, horizontal first into uint8.
 *   recs: DEVICE (N, GFN_PHOTO_RESIZE_REC) int32 rows (Hout, Wout, x offset, x taps, y offset, y taps); an axis table starts at
 *   coef[offset] with Xout (min, count) pairs, then Xout rows of `taps` 22-bit fixed-point weights, computed by the host in double
 *   as Resample.c does.  dst images are dense (Hout,Wout,3).  Hout = 0: the image is skipped.  max_out_h / max_out_w: largest output.
 * gfn_photo_stats: sums[i] += sum of L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16 over image i as it stands when contrast's turn
 *   comes in its chain (ImageEnhance.Contrast's mean, torchvision's adjust_contrast), for every image whose record enables contrast;
 *   sums (N) int64, zero on entry.
 * gfn_photo_jitter_blur: per image its record's chain, then ToTensor.  params: DEVICE (N, GFN_PHOTO_REC) int32 rows: order[4] (the
 *   GFN_PHOTO_* ops in ColorJitter's drawn order), the brightness, contrast and saturation factors (float bits), the hue byte
 *   trunc(hue_factor * 255) & 255, the grey flag (RandomGrayscale), the box radius R of the blur (float bits; 0 = no blur, < 2), the
 *   mask of enabled ops (bit GFN_PHOTO_*), one unused.  Brightness / contrast / saturation: ImageEnhance's blend a + f (b - a) in
 *   float against black / the constant int(mean(L) + 0.5) from `sums` / L; hue: Pillow's RGB -> HSV -> RGB with H shifted; grey:
 *   convert("L") into all channels; blur: ImageFilter.GaussianBlur's three box passes along rows, then three along columns, indices
 *   clamped to the image.  dst: out_u8 != 0 (H,W,3) uint8, else planar (3,H,W) float = u8 / 255 (ToTensor), dense. */
#define GFN_PHOTO_BRIGHTNESS 0
#define GFN_PHOTO_CONTRAST 1
#define GFN_PHOTO_SATURATION 2
#define GFN_PHOTO_HUE 3
#define GFN_PHOTO_REC 12
#define GFN_PHOTO_RESIZE_REC 6
int gfn_photo_resize_u8(const void *const *src, const int *src_dims, void *const *dst, const int *recs, const int *coef, int N,
                        int max_out_h, int max_out_w, gfn_stream_t stream);
int gfn_photo_stats(const void *const *src, const int *dims, const int *params, int64_t *sums, int N, int max_h, int max_w,
                    gfn_stream_t stream);
int gfn_photo_jitter_blur(const void *const *src, const int *dims, const int *params, const int64_t *sums, void *const *dst, int out_u8,
                          int N, int max_h, int max_w, gfn_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Cross-attention core of the cross-view decoder -- model/transformer/layers/attention.py:227-258 (CrossFlashAttention2.forward:
 * the flash_attn_func call at :252, which all shipped configs select with attention_type "FLASH2" and which raises at :230-231
 * where flash_attn is absent); csrc/cross_attn.hip.  Per batch b and head h, with s[i][j] = scale * sum_d q[b,i,h,d] * k[b,j,h,d]:
 *   out[b,i,h,:] = sum_j softmax_j(s[i][j]) * v[b,j,h,:]        lse[b,h,i] = max_j s[i][j] + log sum_j exp(s[i][j] - max)
 * q, out, dout, dq (B,Nq,H,D) and k, v, dk, dv (B,Nk,H,D), contiguous (what q_proj(x).reshape(B,N,H,D) gives and flash_attn_func
 * takes: no transposes), stored as dtype = GFN_F32, GFN_F16 or GFN_BF16, 16-byte aligned; lse (B,H,Nq) fp32.  D must be 8 (dim 64
 * over 8 heads: the K of v_mfma_f32_32x32x8_f16 and of v_mfma_f32_32x32x8_bf16); any other D returns GFN_ERR_INVALID_ARG.  H, Nq, Nk >= 1 are arbitrary (tails, Nk = 1),
 * scale any finite value (0 gives the mean of v); B, H <= 65535.  No scratch, no allocation, the N x N matrix is never written.
 * Arithmetic: the raw scores on the matrix core with fp32 accumulation (fp16 inputs: exact products; fp32 inputs: the fp32-input
 * instruction, an fmaf chain bit for bit), online softmax and P V in fp32 (P is never rounded), fp16 results rounded to nearest
 * once, overflow to inf.  A key past Nk in a tail tile weighs exactly zero.
 * GFN_BF16 is the fp16 path on the bf16 instruction: exact products, everything between them fp32, results rounded to bf16 to
 * nearest even once; bf16 has fp32's exponent range, so nothing finite in fp32 overflows and nothing is clamped.
 * gfn_cross_attn_fwd writes out and lse. */
int gfn_cross_attn_fwd(const void *q, const void *k, const void *v, int dtype, int B, int Nq, int Nk, int H, int D, float scale,
                       void *out, float *lse, gfn_stream_t stream);
/* Its backward (the reference differentiates attention.py:252 through flash-attn's autograd function): lse as the forward left it,
 * dout = dL/dout -> dq, dk, dv, all OVERWRITTEN.  P is recomputed from lse.  Three launches: delta = sum_j P dP / sum_j P by query
 * tile, dk and dv by key tile, dq by query tile.  delta is formed as that sum and not as sum_d dout * out: the saved out carries its
 * own rounding, which for a row whose weight sits on one key of large norm would exceed the row's whole gradient; `out` is therefore
 * checked like the other pointers but not read.  Between the launches delta lives in the first four bytes of each row of dq (the
 * caller's buffer, overwritten by the last launch; a bf16 row is 16 bytes as an fp16 row is): no scratch.  No atomics, so identical calls give identical bits.  Sums are
 * fp32, fp16 results are rounded once and overflow to inf (never clamped), so a loss scale that is too large shows. */
int gfn_cross_attn_bwd(const void *q, const void *k, const void *v, const void *out, const float *lse, const void *dout, int dtype,
                       int B, int Nq, int Nk, int H, int D, float scale, void *dq, void *dk, void *dv, gfn_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * One layer of the FPN pyramid in inference -- model/FPN.py:95-128 (Conv2d: conv, BatchNorm, leaky ReLU), :43-52 (the decoder's
 * Sequential(conv, BatchNorm, Swish) heads), :59-66 (cat(interpolate(intra), convN1) into innerN, plus convN1) and
 * model/network.py:66, 182 (merge_layer and its residual); csrc/fpn_conv.hip.  fp32, NCHW, contiguous:
 *   out = act(conv(cat(x0', x1), weight) * scale[c] + shift[c]) + residual          zero padding K/2, out (B, Cout, Ho, Wo) with
 *   Ho = (H + stride - 1) / stride, Wo likewise.
 * x0 (B, C0, H, W); with up0 != 0 x0 is (B, C0, H/2, W/2) and x0' its 2x bilinear upsample, exactly F.interpolate(scale_factor=2,
 * mode="bilinear", align_corners=False) (H and W even), computed on the way in and never written.  x1 (B, C1, H, W) or NULL with
 * C1 = 0.  weight (Cout, C0 + C1, K, K) as torch stores it; scale, shift (Cout): BatchNorm's running statistics, its affine and
 * the conv bias, folded by the caller.  residual (B, Cout, Ho, Wo) or NULL; it may alias x0 or x1, out may alias nothing.
 * K in {1, 3, 5, 7}, stride in {1, 2}, act 0 (none), 1 (leaky ReLU with `slope`) or 2 (x * sigmoid(x)); C0 >= 1, 1 <= Cout <= 256,
 * any H, W >= 1, B <= 65535; every map of ONE image below 2^31 bytes (the batch may exceed 4 GB: batch offsets are 64-bit).
 * Anything else returns GFN_ERR_INVALID_ARG before a launch; B = 0 returns GFN_OK.  fp32 operands and fmaf accumulation in a fixed
 * order, no atomics: identical calls give identical bits.  Cout a multiple of 8 takes the LDS-tiled kernel, others a plain one. */
int gfn_conv2d_bn_act_fwd(const float *x0, int C0, int up0, const float *x1, int C1, const float *weight, const float *scale,
                          const float *shift, const float *residual, float *out, int B, int H, int W, int Cout, int K, int stride,
                          int act, float slope, gfn_stream_t stream);

/* The same layer in an fp16 CLASS, inference only; csrc/fpn_conv_half.hip: fp16 maps in memory as stored, the convolution an
 * implicit GEMM on the matrix core (v_mfma_f32_16x16x32_f16 below 32 output channels, v_mfma_f32_32x32x16_f16 from there).
 * x0, x1, residual, out: fp16, NCHW, contiguous, shapes and meaning (up0, x1, residual, K, stride, act, slope) as above; scale,
 * shift (Cout) fp32.  residual may alias x0 or x1, out aliases nothing.
 * weight: the (Cout, Cin, K, K) weight rounded ONCE to fp16 to nearest even and PACKED by the caller (ops.conv2d_pack_half) as
 *   packed[co][cg][u][c] = weight[co][8 cg + c][u / K][u % K]     fp16, (CoutP, CG, UP, 8), 16-byte aligned
 * in k-index order k = (cg UP + u) 8 + c: CG = ceil(Cin / 8) groups of eight input channels, u = ky K + kx the tap, UP = K K rounded
 * up to a multiple of 4 (4, 12, 28, 52), CoutP = Cout rounded up to a multiple of 16 where Cout < 32 and of 32 otherwise.  Whatever
 * lies past Cin, past K K or past Cout is ZERO.  Eight consecutive k -- one tap's eight channels -- are a lane's fragment of a
 * matrix instruction, one aligned 16-byte read.
 * Limits: those of gfn_conv2d_bn_act_fwd (per-image maps below 2^31 bytes, counted in fp16), and Cout a MULTIPLE OF 8: this class
 * has no general kernel.  Anything else returns GFN_ERR_INVALID_ARG before a launch; B = 0 returns GFN_OK.  Batch offsets are
 * 64-bit.  No atomics and a fixed order of sums: identical calls give identical bits.
 * The class's arithmetic: products fp16 x fp16, exact in fp32; sums fp32 on the matrix core.  With up0 the coarse fp16 values are
 * interpolated in fp32 in ATen's order of operations (as the fp32 entry does) and the result is rounded once to fp16 as the
 * operand.  Scale, shift, activation and the residual add are fp32; ONE rounding to nearest even at the store; a value past 65504
 * is stored as +-inf (nothing is clamped), as in the refiners' "amp" class.
 * Not here: bf16 (nothing downstream reads bf16 maps as stored), training, Cout that is no multiple of 8. */
int gfn_conv2d_bn_act_half_fwd(const void *x0, int C0, int up0, const void *x1, int C1, const void *weight, const float *scale,
                               const float *shift, const void *residual, void *out, int B, int H, int W, int Cout, int K, int stride,
                               int act, float slope, gfn_stream_t stream);

/* The same layer in TRAINING mode (model.train(): the reference trains the whole FPN, trainer/train.py:108, through torch autograd);
 * csrc/fpn_conv_train.hip.  fp32, NCHW, contiguous, x = cat(x0, x1) with x0 (B, C0, H, W) and x1 (B, C1, H, W) or NULL with C1 = 0 (no
 * up0 in these three: x0 is read as it is; the gfn_conv2d_up_bn_act_train_* entry points below take the coarse map):
 *   u    = conv(x, weight)                      zero padding K/2; the conv bias is NOT in u
 *   mean, invstd (Cout) of u over B*Ho*Wo       biased variance, eps inside the root
 *   out  = act(bn_w * (u - mean) * invstd + bn_b) + residual             (evaluated as u * alpha + beta', alpha = bn_w * invstd)
 *   running_mean <- (1 - m) running_mean + m (mean + conv_bias)          running_var <- (1 - m) running_var + m var * n / (n - 1)
 * gfn_conv2d_bn_act_train_fwd writes u (B, Cout, Ho, Wo; the ONE map kept for the backward), mean, invstd and out, and updates the
 *   running buffers in place.  conv_bias (Cout) may be NULL; residual (B, Cout, Ho, Wo) may be NULL and may alias x0 or x1; u and out
 *   alias nothing.  The gradient of residual is gy itself and is left to the caller.  The gradient of a conv bias in front of
 *   batch statistics is analytically zero (the bias cancels in u - mean): there is no pointer for it, the caller returns exact zeros
 *   (torch returns rounding noise around 1e-7 there).
 * gfn_conv2d_bn_act_train_bwd: gy = dL/dout and x0, x1, weight, bn_w, bn_b, u, mean, invstd as the forward had them -> gx0 (B, C0, H,
 *   W), gx1 (B, C1, H, W), d_weight (Cout, C0 + C1, K, K), d_bn_w, d_bn_b (Cout), all OVERWRITTEN.  `need` is a sum of GFN_CBT_NEED_X
 *   (gx0 and gx1), GFN_CBT_NEED_W (d_weight) and GFN_CBT_NEED_BN (d_bn_w, d_bn_b): only what it names is computed and only those
 *   pointers are touched; need = 0 launches nothing.  The activation's derivative is recomputed from u, mean and invstd with the
 *   forward's expression.
 * Limits: those of gfn_conv2d_bn_act_fwd, and C0 + C1 <= 65535 and B*Ho*Wo >= 2 (one value per channel has no variance; torch
 *   refuses it too).  Anything else returns GFN_ERR_INVALID_ARG before a launch; B = 0 returns GFN_OK.
 * Arithmetic: operands and products fp32.  Every reduction is two-stage in a fixed order -- the statistics (per 4096 values of a
 *   plane the mean and the squares about it, merged with Chan's formula in double), d_bn_w / d_bn_b (fp32 partials, summed in
 *   double) and the weight gradient (fp32 runs of 32 products, P partial gradients summed in double) -- and there are no
 *   floating-point atomics: identical calls give identical bits.
 * ws: gfn_conv2d_bn_act_train_ws_bytes(...) bytes of 16-byte aligned device memory, contents undefined before and after.  In floats,
 *   each term rounded up to 4:  forward  2 Cout B ceil(Ho Wo / 4096) + 2 max(Cout, C0, C1);  backward  that + 2 Cout + B Cout Ho Wo (the
 *   gu map) + Cout Cin K K (the repacked weight) + P Cout Cin K K with P = min(512, 2^22 / (Cout Cin K K), B ceil(Ho / 8)
 *   ceil(Wo / 32)), at least 1: the partial weight gradients never take more than 16 MiB. */
#define GFN_CBT_NEED_W 2 /* d_weight of gfn_conv2d_bn_act_train_bwd */
int64_t gfn_conv2d_bn_act_train_ws_bytes(int C0, int C1, int B, int H, int W, int Cout, int K, int stride, int backward);
int gfn_conv2d_bn_act_train_fwd(const float *x0, int C0, const float *x1, int C1, const float *weight, const float *conv_bias,
                                const float *bn_w, const float *bn_b, float *running_mean, float *running_var, const float *residual,
                                float *u, float *mean, float *invstd, float *out, int B, int H, int W, int Cout, int K, int stride,
                                int act, float slope, double momentum, double eps, void *ws, int64_t ws_bytes, gfn_stream_t stream);
int gfn_conv2d_bn_act_train_bwd(const float *gy, const float *x0, int C0, const float *x1, int C1, const float *weight, const float *bn_w,
                                const float *bn_b, const float *u, const float *mean, const float *invstd, float *gx0, float *gx1,
                                float *d_weight, float *d_bn_w, float *d_bn_b, int B, int H, int W, int Cout, int K, int stride, int act,
                                float slope, int need, void *ws, int64_t ws_bytes, gfn_stream_t stream);

/* The training layer with the decoder's 2x upsample inside it (model/FPN.py:59, skip + innerN(cat(interpolate(intra), skip))): the three
 * entry points above with `int up0` after C0; up0 = 0 is the entry point above, launch for launch.  With up0 != 0:
 *   x0 is (B, C0, H/2, W/2) and stands for x0', exactly F.interpolate(x0, scale_factor=2, mode="bilinear", align_corners=False), in
 *   both directions; x1, residual, u, out and gy are at (H, W); gx0 is (B, C0, H/2, W/2), the gradient of x0 itself.  x0' is never
 *   written: the convolution interpolates while it stages its halo tile (gfn_conv2d_bn_act_fwd's up0), the weight gradient stages the
 *   coarse footprint of its tile in LDS and interpolates from there with the same operations in the same order, so both directions
 *   read the same x0' bit for bit.
 *   gx0: the gradient of x0' is written at (H, W) into the workspace by the stride-1 input-gradient launch, and ft_up2_adjoint_kernel
 *   applies the transposed upsample as a gather: per coarse value the rows 2c-1 .. 2c+2 and the columns likewise, weights 1/4, 3/4,
 *   3/4, 1/4 each way, the border weights folded onto the first and last row and column as the forward's clamps fold them; 16 taps in
 *   a fixed order, no atomics.  With a need mask without GFN_CBT_NEED_X neither is launched.
 * Limits: those above, and with up0 H and W even and stride 1; the 2^31-byte bound on x0 is that of its doubled image.  Anything else
 *   returns GFN_ERR_INVALID_ARG before a launch; gfn_conv2d_up_bn_act_train_ws_bytes returns 0 for it.
 * ws: with up0 the backward size grows by B C0 H W floats (rounded up to 4), the gradient of x0'; the forward size is unchanged. */
int64_t gfn_conv2d_up_bn_act_train_ws_bytes(int C0, int up0, int C1, int B, int H, int W, int Cout, int K, int stride, int backward);
int gfn_conv2d_up_bn_act_train_fwd(const float *x0, int C0, int up0, const float *x1, int C1, const float *weight, const float *conv_bias,
                                   const float *bn_w, const float *bn_b, float *running_mean, float *running_var, const float *residual,
                                   float *u, float *mean, float *invstd, float *out, int B, int H, int W, int Cout, int K, int stride,
                                   int act, float slope, double momentum, double eps, void *ws, int64_t ws_bytes, gfn_stream_t stream);
int gfn_conv2d_up_bn_act_train_bwd(const float *gy, const float *x0, int C0, int up0, const float *x1, int C1, const float *weight,
                                   const float *bn_w, const float *bn_b, const float *u, const float *mean, const float *invstd, float *gx0,
                                   float *gx1, float *d_weight, float *d_bn_w, float *d_bn_b, int B, int H, int W, int Cout, int K, int stride,
                                   int act, float slope, int need, void *ws, int64_t ws_bytes, gfn_stream_t stream);

/* The FPN layer in the reference's TF32 CLASS, inference and training; csrc/fpn_conv_tf32.hip.  The reference runs its FPN
 * (model/FPN.py) outside autocast in fp32 tensors with cuDNN's TF32 convolutions: train.py:151 sets torch.backends.cudnn.allow_tf32,
 * which is also torch's default for convolutions.  It keeps fp32 maps, rounds the operands of each product and sums in fp32.  gfx950
 * has no TF32 matrix instruction; this class is SPLIT-bf16 on the bf16 one, said once here:
 *   the split of an fp32 value v:  hi = bf16(v) to nearest even (v_cvt_pk_bf16_f32), lo = bf16(v - hi), and lo = 0 where hi is not
 *     finite, so that an inf stays an inf as on the fp32 path and does not become inf - inf;
 *   a product a b of the convolution is a_hi b_hi + a_hi b_lo + a_lo b_hi: each of the three is exact in fp32, they are summed into
 *     an fp32 accumulator by v_mfma_f32_16x16x32_bf16 (Cout < 32) or v_mfma_f32_32x32x16_bf16 (Cout >= 32); a_lo b_lo is dropped;
 *   with up0 the interpolated value is computed in fp32 exactly as on the fp32 path and then split;
 *   scale, shift, activation and residual are fp32 and every map is fp32, in and out.  A fixed order of sums and no atomics:
 *     identical calls give identical bits.
 * Against exact arithmetic the class errs by at most 3 * 2^-16 * sum |a| |b| per output before fp32 accumulation (2^-8 per
 * rounding; measured 1.8 * 2^-16) -- the figure beside TF32's 2^-10.
 * gfn_conv2d_bn_act_tf32_fwd: gfn_conv2d_bn_act_fwd's arguments, meaning, limits and refusals; weight is the
 *   plain fp32 (Cout, C0 + C1, K, K) weight, split and packed on the device by one small launch into ws:
 *   gfn_conv2d_bn_act_tf32_ws_bytes(C0, C1, Cout, K) bytes, 16-byte aligned (0 for sizes the entry refuses).  Cout must be a MULTIPLE OF
 *   8, as in the fp16 class; anything else returns GFN_ERR_INVALID_ARG before a launch.
 * gfn_conv2d_bn_act_train_tf32_{ws_bytes,fwd,bwd}: gfn_conv2d_up_bn_act_train_*'s arguments (up0 and the need mask included), meaning,
 *   limits, refusals and saved tensors (u, mean, invstd, all fp32) for both existing pairs.  In the class: the forward convolution u,
 *   the stride-1 input gradient (the same convolution of gu with the transposed and flipped weight), and the weight gradient under
 *   stride 1 without up0 -- a GEMM over the pixels on v_mfma_f32_16x16x32_bf16 with gu and the shifted x both split, per-workgroup
 *   partials added in order in double as on the fp32 path.  On today's fp32 kernels, whose exact products lie inside the class's
 *   bound: the stride-2 input gradient (ft_gather_s2_kernel), the weight gradient under stride 2 and under up0 (ft_wgrad_kernel), and
 *   any convolution launch whose output-channel count -- for an input gradient C0 or C1 of the layer -- is not a multiple of 8.  The BatchNorm passes are the fp32 entries' own.  ws grows by the largest packed weight of the launches. */
int64_t gfn_conv2d_bn_act_tf32_ws_bytes(int C0, int C1, int Cout, int K);
int gfn_conv2d_bn_act_tf32_fwd(const float *x0, int C0, int up0, const float *x1, int C1, const float *weight, const float *scale,
                               const float *shift, const float *residual, float *out, int B, int H, int W, int Cout, int K, int stride,
                               int act, float slope, void *ws, int64_t ws_bytes, gfn_stream_t stream);
int64_t gfn_conv2d_bn_act_train_tf32_ws_bytes(int C0, int up0, int C1, int B, int H, int W, int Cout, int K, int stride, int backward);
int gfn_conv2d_bn_act_train_tf32_fwd(const float *x0, int C0, int up0, const float *x1, int C1, const float *weight, const float *conv_bias,
                                     const float *bn_w, const float *bn_b, float *running_mean, float *running_var, const float *residual,
                                     float *u, float *mean, float *invstd, float *out, int B, int H, int W, int Cout, int K, int stride,
                                     int act, float slope, double momentum, double eps, void *ws, int64_t ws_bytes, gfn_stream_t stream);
int gfn_conv2d_bn_act_train_tf32_bwd(const float *gy, const float *x0, int C0, int up0, const float *x1, int C1, const float *weight,
                                     const float *bn_w, const float *bn_b, const float *u, const float *mean, const float *invstd, float *gx0,
                                     float *gx1, float *d_weight, float *d_bn_w, float *d_bn_b, int B, int H, int W, int Cout, int K,
                                     int stride, int act, float slope, int need, void *ws, int64_t ws_bytes, gfn_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Self-attention forward of the DINOv2 ViT at head dim 64 -- model/transformer/layers/attention.py:77-101 (Attention.forward:
 * the F.scaled_dot_product_attention call at :96, which MemEffAttention falls back to without xformers, :106-110);
 * csrc/self_attn.hip.  Per batch b and head h, with s[i][j] = scale * sum_d q[b,i,h,d] * k[b,j,h,d]:
 *   out[b,i,h,:] = sum_j softmax_j(s[i][j]) * v[b,j,h,:]
 * qkv is the PACKED projection (B,N,3,H,D) contiguous -- what self.qkv(x).reshape(B,N,3,H,C/H) gives: q = qkv[:,:,0], k = [:,:,1],
 * v = [:,:,2], no permutes and no copies -- and out (B,N,H,D) contiguous, so out.reshape(B,N,C) feeds proj; both 16-byte aligned.
 * dtype must be GFN_F16 or GFN_BF16 (qkv and out in that type) and D must be 64; N, H >= 1 are arbitrary (tails on both axes), scale any finite value (0 gives the mean of
 * v); B * H * ceil(N / 128) is the grid, at most 2^31 - 1.  Anything else returns GFN_ERR_INVALID_ARG before a launch; B = 0 returns
 * GFN_OK.  No scratch, no allocation, nothing N x N is written.  Forward only: the reference freezes the ViT.
 * Arithmetic: the raw scores on the matrix core (exact products, fp32 accumulation), online softmax in fp32 from a running maximum
 * that starts at -inf, a key past N in a tail tile weighs exactly zero (selected by its index); the weights are rounded to fp16
 * once for P V on the matrix core (fp32 accumulation; the row sum takes the unrounded weights), results rounded to fp16 once,
 * overflow to inf.  No atomics: identical calls give identical bits.
 * GFN_BF16 is the same kernel on v_mfma_f32_32x32x16_bf16: exact products, everything between them fp32 as above, the weights
 * rounded to bf16 to nearest even once, results divided once and rounded to bf16 to nearest even once.  One limit of its own: the
 * fp32 accumulator of P V holds sum_j p_j v_j with weights relative to the running maximum (each at most 1) until the one division,
 * so it can reach N * max|v|.  In fp16 that cannot leave fp32's range; in bf16 it can.  Results are finite where N * max|v| is
 * below fp32's largest value (3.4e38); nothing is clamped, past that the result is inf or NaN. */
int gfn_self_attn_fwd(const void *qkv, int dtype, int B, int N, int H, int D, float scale, void *out, gfn_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * The seam of a ViT block in one pass -- model/transformer/layers/block.py:83-106 with layer_scale.py (x + ls(f(norm(x))) and the
 * norm that follows); csrc/layernorm.hip.  x, y, x_out, h_out (rows, C) contiguous, gamma, weight, bias (C), all stored as dtype =
 * GFN_F32 or GFN_F16 and 16-byte aligned:
 *   x_out = x + gamma * y          h_out = (x_out - mean) / sqrt(var + eps) * weight + bias     (mean, biased var over a row)
 * y == NULL: plain LayerNorm of x (gamma and x_out may then be NULL and are not touched).  h_out == NULL: only the residual
 * update (weight and bias may then be NULL).  Both NULL is an error.  x_out may alias x; h_out may alias nothing.  C a multiple of
 * 8 from 8 to 8192 (the row is held in registers), rows >= 0 arbitrary; anything else returns GFN_ERR_INVALID_ARG before a launch.
 * Arithmetic: fp32; x_out = fma(gamma, y, x) rounded to the storage type once; mean and variance two-pass (sum of squared
 * distances from the mean) over x_out AS STORED, i.e. after that rounding, which is what a following norm reads in the reference.
 * GFN_BF16 is refused here: bf16 tensors go to gfn_ls_add_layernorm_bf16_fwd below. */
int gfn_ls_add_layernorm_fwd(const void *x, const void *y, const void *gamma, const void *weight, const void *bias, float eps,
                             int dtype, int64_t rows, int C, void *x_out, void *h_out, gfn_stream_t stream);
/* The same seam with every tensor stored as bf16 (GFN_BF16; the class is in the name, so there is no dtype argument): the same
 * kernel, argument rules and refusals.  16-byte accesses of eight values, widened exactly; x_out and h_out rounded to bf16 to nearest
 * even once each; the statistics are the same two fp32 passes over x_out as stored in bf16. */
int gfn_ls_add_layernorm_bf16_fwd(const void *x, const void *y, const void *gamma, const void *weight, const void *bias, float eps,
                                  int64_t rows, int C, void *x_out, void *h_out, gfn_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * A block of the cross-view decoder around its attention core, inference in the fp16 autocast class; csrc/decoder_block.hip.
 * Width C = 64 (8 heads of 8) and hidden width 256 only.  X is the residual stream of both views, cat(x, y): (2B, N, 64) fp32
 * contiguous.  Parameters are passed as the module stores them (fp32, a Linear weight (out, in)) and rounded to fp16 once while a
 * workgroup stages them; every pointer 16-byte aligned.  Every product runs on the matrix core (v_mfma_f32_32x32x8_f16: exact
 * products, fp32 accumulation); LayerNorm is fp32, two-pass (mean, then the squared distances from it) over the row as read, biased
 * variance.  Persistent workgroups over 32-token tiles; no scratch, no allocation, no atomics: identical calls give identical bits,
 * and a row's result depends on that row alone (a non-finite row stays in its row).  Forward only.
 *
 * gfn_decoder_qkv_fwd -- what precedes gfn_cross_attn_fwd: model/transformer/layers/block.py:327 (norm1; the other view's tokens
 * are not normalised, pre_norm_query) and attention.py:236-238 (the three bias-free projections), with the torch.cat((y, x)) of
 * crossview_decoder_light.py:53-54 folded into where k and v are written.  For batch entry b and token n:
 *   q[b,n]              = fp16(wq . fp16(LayerNorm(X[b,n]) * norm_weight + norm_bias))
 *   k[(b + B) mod 2B,n] = fp16(wk . fp16(X[b,n]))          v likewise with wv
 * q, k, v (2B, N, 8, 8) fp16 contiguous, as gfn_cross_attn_fwd takes them; results rounded once, overflow to inf.  B2 = 2B must be
 * even, N >= 1, B2 * N < 2^31 - 32; anything else returns GFN_ERR_INVALID_ARG before a launch.  B2 = 0 returns GFN_OK. */
int gfn_decoder_qkv_fwd(const float *x, const float *norm_weight, const float *norm_bias, float eps, const float *wq, const float *wk,
                        const float *wv, int B2, int N, int C, void *q, void *k, void *v, gfn_stream_t stream);
/* gfn_decoder_post_fwd -- what follows it: attention.py:255 (the output projection), the rest of block.py:327-328 with
 * layer_scale.py (both LayerScales and residual adds, norm2) and mlp.py (fc1, the exact erf GELU, fc2).  Per row, with a the
 * attention output (rows, 64) fp16:
 *   x1    = x  + gamma1 * (wproj . a + bproj)
 *   x_out = x1 + gamma2 * (w2 . fp16(GELU(w1 . fp16(LayerNorm(x1) * norm_weight + norm_bias) + b1)) + b2)
 * x, x_out (rows, 64) fp32; x_out may be x.  w1 (hidden, C), w2 (C, hidden).  Operands are rounded to fp16 where the reference's
 * autocast rounds the input of a Linear; the proj, fc1 and fc2 results, which the reference rounds to fp16, stay fp32 in registers.
 * C must be 64, hidden 256, 0 <= rows < 2^31 - 32; anything else returns GFN_ERR_INVALID_ARG before a launch.  rows = 0 returns
 * GFN_OK. */
int gfn_decoder_post_fwd(const float *x, const void *attn, const float *wproj, const float *bproj, const float *gamma1,
                         const float *norm_weight, const float *norm_bias, float eps, const float *w1, const float *b1, const float *w2,
                         const float *b2, const float *gamma2, int64_t rows, int C, int hidden, float *x_out, gfn_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Training of those blocks: the backward of the two launches above, which are themselves the training forward (the fp16 autocast
 * class is the reference's training class, model/network.py:171).  Both differentiate the forward AS THE KERNELS COMPUTE IT, every
 * fp16 rounding taken as the identity (autocast's backward).  Products run on v_mfma_f32_32x32x8_f16 with operands rounded to fp16
 * once; a parameter gradient is a sum over tokens of an outer product, taken on the matrix core with the tokens as its K dimension.
 * No atomics: every workgroup leaves fp32 partial sums in ws and a later launch adds them in a fixed order, so identical calls
 * give identical bits in every output; the grids depend on rows alone, not on the device.  Nothing (rows, hidden) is written.
 * gX and g_attn of a row depend on that row alone: a non-finite row of the incoming gradient stays in its row there (and reaches
 * the parameter gradients).  Same sizes as the forward entries, refused the same way.
 * ws: gfn_decoder_bwd_ws_bytes(rows) bytes (one size serves both entries), 16-byte aligned, contents undefined before and after. */
int64_t gfn_decoder_bwd_ws_bytes(int64_t rows);
/* gfn_decoder_qkv_bwd -- backward of gfn_decoder_qkv_fwd (block.py:327, attention.py:236-238, crossview_decoder_light.py:53-54).
 * gq, gk, gv (2B, N, 8, 8) fp16 as gfn_cross_attn_bwd writes them; row r's k and v were written at row (r + rows / 2) mod rows, so
 * its gk and gv are read from there (gk', gv').  With n = fp16(LayerNorm(X) * norm_weight + norm_bias):
 *   gx = LayerNorm^T(wq^T gq) + wk^T gk' + wv^T gv'       (2B, N, 64) fp32
 *   g_wq = sum gq (x) n   g_wk = sum gk' (x) fp16(X)   g_wv = sum gv' (x) fp16(X)   g_norm_weight, g_norm_bias: norm1's   all fp32 */
int gfn_decoder_qkv_bwd(const float *x, const float *norm_weight, const float *norm_bias, float eps, const float *wq, const float *wk,
                        const float *wv, const void *gq, const void *gk, const void *gv, int B2, int N, int C, float *gx, float *g_wq,
                        float *g_wk, float *g_wv, float *g_norm_weight, float *g_norm_bias, void *ws, int64_t ws_bytes,
                        gfn_stream_t stream);
/* gfn_decoder_post_bwd -- backward of gfn_decoder_post_fwd (attention.py:255, block.py:327-328, layer_scale.py, mlp.py).  x and attn
 * are the forward's inputs: x1, norm2's output n, u = w1 n + b1 and GELU(u) are recomputed, not saved.  Per row, with g = gx_out:
 *   gu = (w2^T (gamma2 g)) GELU'(u)      g1 = g + LayerNorm^T(w1^T gu)      gx = g1      g_attn = fp16(wproj^T (gamma1 g1))
 * g_attn (rows, 64) fp16, rounded once, overflow to inf: the dout of gfn_cross_attn_bwd.  The parameter gradients, fp32, of the
 * parameters' shapes: g_w2 = gamma2_c sum g (x) fp16(GELU(u)), g_b2 = gamma2_c sum g, g_gamma2 = sum g (w2 fp16(GELU(u)) + b2)
 * (formed from the same sums, without dividing by gamma2), g_w1 = sum gu (x) n, g_b1 = sum gu, g_norm_weight and g_norm_bias
 * (norm2's), and g_wproj, g_bproj, g_gamma1 from g1 and attn as the fc2 three are from g and GELU(u). */
int gfn_decoder_post_bwd(const float *x, const void *attn, const float *wproj, const float *bproj, const float *gamma1,
                         const float *norm_weight, const float *norm_bias, float eps, const float *w1, const float *b1, const float *w2,
                         const float *b2, const float *gamma2, const float *gx_out, int64_t rows, int C, int hidden, float *gx,
                         void *g_attn, float *g_wproj, float *g_bproj, float *g_gamma1, float *g_norm_weight, float *g_norm_bias,
                         float *g_w1, float *g_b1, float *g_w2, float *g_b2, float *g_gamma2, void *ws, int64_t ws_bytes,
                         gfn_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * The same four entry points in the bf16 autocast class (model/network.py:171 with amp_dtype = torch.bfloat16); the same kernels of
 * csrc/decoder_block.hip instantiated for the other element.  Argument for argument their fp16 siblings, with bf16 wherever those
 * have fp16: q, k, v, attn, gq, gk, gv and g_attn are bf16 tensors, parameters and operands are rounded to bf16 once (to nearest
 * even, NaN kept, no clamp: bf16 has fp32's exponent range, so there is no overflow to inf to speak of), every product runs on
 * v_mfma_f32_32x32x8_bf16 with fp32 accumulation.  Everything the fp16 class keeps in fp32 stays fp32: X, LayerNorm, GELU, all
 * parameters and their gradients, the partial sums.  Same sizes, same refusals, same grids, same determinism; the workspace is
 * gfn_decoder_bwd_ws_bytes(rows), which serves both classes (the partials are fp32).
 * gfn_decoder_qkv_bf16_fwd -- block.py:327, attention.py:236-238, crossview_decoder_light.py:53-54, as gfn_decoder_qkv_fwd. */
int gfn_decoder_qkv_bf16_fwd(const float *x, const float *norm_weight, const float *norm_bias, float eps, const float *wq, const float *wk,
                             const float *wv, int B2, int N, int C, void *q, void *k, void *v, gfn_stream_t stream);
/* gfn_decoder_post_bf16_fwd -- attention.py:255, block.py:327-328, layer_scale.py, mlp.py, as gfn_decoder_post_fwd. */
int gfn_decoder_post_bf16_fwd(const float *x, const void *attn, const float *wproj, const float *bproj, const float *gamma1,
                              const float *norm_weight, const float *norm_bias, float eps, const float *w1, const float *b1,
                              const float *w2, const float *b2, const float *gamma2, int64_t rows, int C, int hidden, float *x_out,
                              gfn_stream_t stream);
/* gfn_decoder_qkv_bf16_bwd -- backward of gfn_decoder_qkv_bf16_fwd (block.py:327, attention.py:236-238,
 * crossview_decoder_light.py:53-54), as gfn_decoder_qkv_bwd; gq, gk, gv bf16 as gfn_cross_attn_bwd writes them with GFN_BF16. */
int gfn_decoder_qkv_bf16_bwd(const float *x, const float *norm_weight, const float *norm_bias, float eps, const float *wq, const float *wk,
                             const float *wv, const void *gq, const void *gk, const void *gv, int B2, int N, int C, float *gx,
                             float *g_wq, float *g_wk, float *g_wv, float *g_norm_weight, float *g_norm_bias, void *ws, int64_t ws_bytes,
                             gfn_stream_t stream);
/* gfn_decoder_post_bf16_bwd -- backward of gfn_decoder_post_bf16_fwd (attention.py:255, block.py:327-328, layer_scale.py, mlp.py), as
 * gfn_decoder_post_bwd; g_attn (rows, 64) bf16, rounded once: the dout of gfn_cross_attn_bwd with GFN_BF16. */
int gfn_decoder_post_bf16_bwd(const float *x, const void *attn, const float *wproj, const float *bproj, const float *gamma1,
                              const float *norm_weight, const float *norm_bias, float eps, const float *w1, const float *b1,
                              const float *w2, const float *b2, const float *gamma2, const float *gx_out, int64_t rows, int C,
                              int hidden, float *gx, void *g_attn, float *g_wproj, float *g_bproj, float *g_gamma1,
                              float *g_norm_weight, float *g_norm_bias, float *g_w1, float *g_b1, float *g_w2, float *g_b2,
                              float *g_gamma2, void *ws, int64_t ws_bytes, gfn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GFNET_HIP_H */
