/*
 * leastereo_hip.h — C ABI of libleastereo_hip.so, the MI355X (gfx950) kernels
 * behind LEAStereo's inference hot path.
 *
 * The reference (devmentality/LEAStereo) is pure PyTorch and has no FFI; each
 * entry point below replaces the aten op sequence at the cited reference line,
 * and is what a ctypes/cffi binding of that path binds.
 *
 * Conventions
 *   - All tensors are caller-owned device buffers, NCDHW (or NCHW) contiguous
 *     in W, H, D order; channel stride is always D*H*W.  A per-batch stride
 *     (in elements) lets an operand be a channel slice of a larger tensor, which
 *     is how torch.cat (skip_model_3d.py:74,150,155) becomes free.
 *   - `stream` is a hipStream_t (NULL = legacy default stream).  No call
 *     allocates, synchronises or touches the host after argument checks, so every
 *     call is hipGraph-capturable.
 *   - Return 0 on success; LEA_E_INVALID / LEA_E_UNSUPPORTED on bad arguments
 *     (nothing launched); otherwise a hipError_t from the launch.
 *     lea_last_error() describes the last failure on the calling thread.
 *   - dtype: LEA_F32 (the reference's arithmetic) for the entries below that take
 *     one; the bf16 path (configs 3/4) has its own *_bf16 entries at the end.
 */
#ifndef LEASTEREO_HIP_H
#define LEASTEREO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LEA_ABI_VERSION 14

#define LEA_F32 0
#define LEA_BF16 1

#define LEA_OK 0
#define LEA_E_INVALID 1001
#define LEA_E_UNSUPPORTED 1002

/* conv epilogue flags */
#define LEA_RELU 1u     /* ReLU after the BN affine (operations_3d.py:45-46)          */
#define LEA_RESIDUAL 2u /* y = act(...) + residual: the cell's `sum(new_states)`
                           (skip_model_3d.py:69); residual may alias y               */
#define LEA_PAIR_SUM 4u /* two ConvBRs summed, a cell step of two conv terms
                           (skip_model_3d.py:57-69): y = act(BN_a(conv_a(x))) +
                           act(BN_b(conv_b(x2))) -- input channels [0, cin - cin2) are
                           conv_a's, [cin - cin2, cin) conv_b's (the weights packed as one
                           conv over the concatenation), scale/shift hold 2 * cout values
                           (a's, then b's); exclusive with LEA_RESIDUAL.  Where an engine
                           supports it (lea_conv3d_bnrelu_wino: cout <= 32, W % 4 == 0;
                           lea_conv3d_bnrelu_bf16: the D-streaming 3x3x3 layers), else
                           LEA_E_UNSUPPORTED                                           */

int lea_abi_version(void);
const char* lea_last_error(void);

/* Cost volume.  Replaces retrain/LEAStereo.py:34-48 (zero-init + 2*D3 strided copies).
 *   cost[b, c,   i, h, w] = left [b, c, h, w]     for w >= i
 *   cost[b, C+c, i, h, w] = right[b, c, h, w - i] for w >= i,   0 for w < i
 * left/right: [B, C, H, W]; cost: [B, 2C, D3, H, W].  D3 = int(maxdisp / 3). */
int lea_build_cost_volume(const void* left, const void* right, void* cost,
                          int B, int C, int H, int W, int D3, int dtype, void* stream);

/* Packed-weight size (in floats) for a ConvBR of the given shape; k in {1, 3}. */
size_t lea_conv3d_packed_floats(int cout, int cin, int k);

/* Re-lay an OIDHW fp32 weight ([cout, cin, k, k, k], device) into the kernel's
 * packed layout (device).  Done once per load_state_dict. */
int lea_conv3d_pack_weights(const float* w, float* packed, int cout, int cin, int k,
                            void* stream);

/* ConvBR3d.  Replaces models/operations_3d.py:41-47 (Conv3d no bias, stride 1,
 * pad k/2 -> BatchNorm3d eval -> ReLU) with BN folded on the host into
 *   scale = gamma / sqrt(var + eps),  shift = beta - mean * scale
 * (both NULL = bn=False).  Input channels [0, cin-cin2) come from x and
 * [cin-cin2, cin) from x2 (cin2 = 0: single source), i.e. the conv reads
 * torch.cat((x, x2), 1) without it existing (skip_model_3d.py:150,155).
 * x: [B, cin-cin2, D, H, W], x2: [B, cin2, D, H, W], y/residual: [B, cout, D, H, W],
 * each at its own batch stride. */
int lea_conv3d_bnrelu(const void* x, int64_t x_bstride,
                      const void* x2, int64_t x2_bstride, int cin2,
                      const float* w_packed, const float* scale, const float* shift,
                      const void* residual, int64_t r_bstride,
                      void* y, int64_t y_bstride,
                      int B, int cin, int cout, int D, int H, int W, int k,
                      unsigned flags, int dtype, void* stream);

/* Two 1x1x1 ConvBR3d of the same input in one pass over it (a matching cell's `preprocess`
 * and the next cell's `pre_preprocess` read the same tensor, skip_model_3d.py:52-53,75):
 * w_packed is lea_conv3d_pack_weights (k = 1) of the two weights stacked along cout, head A's
 * [cout_a, cin] first.  Head A writes y_a [B, cout_a, D, H, W], head B y_b [B, cout_b, D, H, W],
 * each with its own batch stride, folded BN (both NULL = none) and flags (LEA_RELU only:
 * neither head takes a residual; LEA_RESIDUAL is LEA_E_INVALID).  x / x2 / cin2 as for
 * lea_conv3d_bnrelu.  Each head is bit-identical to its own lea_conv3d_bnrelu (k = 1) launch. */
int lea_conv1x1_heads(const void* x, int64_t x_bstride, const void* x2, int64_t x2_bstride,
                      int cin2, const float* w_packed,
                      const float* scale_a, const float* shift_a, void* y_a, int64_t ya_bstride,
                      int cout_a, unsigned flags_a,
                      const float* scale_b, const float* shift_b, void* y_b, int64_t yb_bstride,
                      int cout_b, unsigned flags_b,
                      int B, int cin, int D, int H, int W, int dtype, void* stream);
/* Kernel instantiation lea_conv1x1_heads launches (cout = cout_a + cout_b). */
const char* lea_conv1x1_heads_kernel_name(int B, int cout, int D, int H, int W);

/* ConvBR3d of a trilinearly resampled input: conv(interp(x, [D, H, W],
 * align_corners=True)) with the interpolation done while staging, so the
 * resampled volume never reaches HBM.  Replaces the F.interpolate + ConvBR pairs
 * of Cell.forward (skip_model_3d.py:44-53) and the head's Upsample + last_3
 * (:162-173).  x: [B, cin, Di, Hi, Wi]; y/residual: [B, cout, D, H, W]. */
int lea_conv3d_bnrelu_resampled(const void* x, int64_t x_bstride, int Di, int Hi, int Wi,
                                const float* w_packed, const float* scale, const float* shift,
                                const void* residual, int64_t r_bstride,
                                void* y, int64_t y_bstride,
                                int B, int cin, int cout, int D, int H, int W, int k,
                                unsigned flags, int dtype, void* stream);

/* Matching-net stem0 on the cost volume without materialising it: the ConvBR3d
 * (3x3x3) of cost = [B, 2C, D3, H, W] as built by lea_build_cost_volume
 * (retrain/LEAStereo.py:34-48 then skip_model_3d.py:141), reading the feature maps
 * left/right [B, C, H, W] (batch stride f_bstride) directly.  Bit-identical to
 * lea_build_cost_volume + lea_conv3d_bnrelu; saves the 2*4*B*C*D3*H*W-byte volume's
 * write and read.  C must be a multiple of 4.  y: [B, cout, D3, H, W]. */
int lea_conv3d_bnrelu_costvolume(const void* left, const void* right, int64_t f_bstride,
                                 const float* w_packed, const float* scale, const float* shift,
                                 void* y, int64_t y_bstride, int B, int C, int cout, int D3,
                                 int H, int W, unsigned flags, int dtype, void* stream);
const char* lea_conv3d_costvolume_kernel_name(int B, int cout, int D3, int H, int W);

/* Name of the kernel instantiation a conv of this output shape launches
 * (matches the demangled name rocprofv3 reports), for a single source of at most 128 input
 * channels; NULL if unsupported.  Every *_kernel_name query answers NULL, with lea_last_error
 * set, for a plan without an instantiation (a tile override can ask for one): the launch
 * returns LEA_E_UNSUPPORTED. */
const char* lea_conv3d_kernel_name(int B, int cout, int D, int H, int W, int k, int resampled);
/* The same for the whole argument list of lea_conv3d_bnrelu / lea_conv3d_bnrelu_resampled
 * (cin2 of the cin input channels in the second source): a resampled 1x1 of more than 128
 * input channels or of two sources runs on the register-staged engine. */
const char* lea_conv3d_launch_kernel_name(int B, int cin, int cin2, int cout, int D, int H, int W, int k,
                                          int resampled);

/* ---- 2D feature net (retrain/new_model_2d.py; models/operations_2d.py:31-47) ----
 * 1x1 Conv2d and bilinear (align_corners) resizes of the feature net use the 3D
 * entry points with D = Di = 1 (a bilinear resize is the trilinear one on a
 * single plane, bit for bit).  The 3x3 convs have their own packing and entry. */

/* Packed-weight size (floats) / packing of a Conv2d 3x3 weight [cout, cin, 3, 3]. */
size_t lea_conv2d_packed_floats(int cout, int cin);
int lea_conv2d_pack_weights(const float* w, float* packed, int cout, int cin, void* stream);

/* ConvBR2d 3x3, stride 1, pad 1 (folded BN as in lea_conv3d_bnrelu, LEA_RELU,
 * LEA_RESIDUAL -- the 2D cell's sum, including its skip_connect terms).
 * x: [B, cin, H, W], y/residual: [B, cout, H, W], each at its own batch stride. */
int lea_conv2d_bnrelu(const void* x, int64_t x_bstride, const float* w_packed,
                      const float* scale, const float* shift, const void* residual,
                      int64_t r_bstride, void* y, int64_t y_bstride, int B, int cin, int cout,
                      int H, int W, unsigned flags, int dtype, void* stream);

/* Kernel instantiation lea_conv2d_bnrelu launches for this shape. */
const char* lea_conv2d_kernel_name(int B, int cout, int H, int W);

/* Two ConvBR2d 3x3 s1 p1 of the same input in one launch (a feature-net cell's two ops
 * on s0, retrain/new_model_2d.py:41-75 -- the reference runs them as two convs): weights
 * and folded BN of both stacked along cout (w_packed: lea_conv2d_pack_weights of the
 * [cout, cin, 3, 3] stack), couts [0, c1) written to y with the residual (flags as for
 * lea_conv2d_bnrelu), couts [c1, cout) to y2 without it.  cin <= 16, cout <= 32 and
 * c1 % 8 == 0 (the few-channel tile; LEA_E_UNSUPPORTED beyond it); fp32. */
int lea_conv2d_bnrelu_pair(const void* x, int64_t x_bstride, const float* w_packed,
                           const float* scale, const float* shift, const void* residual,
                           int64_t r_bstride, void* y, int64_t y_bstride, void* y2,
                           int64_t y2_bstride, int B, int cin, int cout, int c1, int H, int W,
                           unsigned flags, void* stream);

/* Feature-net stem1: Conv2d 3x3, stride 3, pad 1 -> BN -> ReLU (new_model_2d.py:94).
 * w: the raw [cout, cin, 3, 3] weight (no packing).  x: [B, cin, Hi, Wi];
 * y: [B, cout, (Hi-1)/3+1, (Wi-1)/3+1]. */
int lea_conv2d_s3_bnrelu(const void* x, int64_t x_bstride, const float* w, const float* scale,
                         const float* shift, void* y, int64_t y_bstride, int B, int cin, int cout,
                         int Hi, int Wi, unsigned flags, int dtype, void* stream);

/* Feature-net stems 0 + 1 fused (retrain/new_model_2d.py:93-94): ConvBR2d 3x3 s1 p1
 * (cin -> c0) then ConvBR2d 3x3 s3 p1 (c0 -> c1), both with folded BN and ReLU, without
 * writing stem0's full-resolution output (stride 3 tiles it: each stem0 pixel feeds one
 * stem1 pixel).  w0: [c0, cin, 3, 3], w1: [c1, c0, 3, 3] raw f32.  x: [B, cin, Hi, Wi] f32;
 * y: [B, c1, Ho, Wo] f32 (dtype LEA_F32) or c8 [B, c1/8, 1, Ho, Wo, 8] bf16 (LEA_BF16),
 * Ho = (Hi - 1) / 3 + 1.  Instantiated for 3 -> 16 -> 32 (the searched feature net).
 * Image b is read at x + b * x_bstride (elements, any sign): two separately allocated
 * images (the left / right pair) run as one B = 2 launch with x_bstride = right - left. */
int lea_feature_stem_bnrelu(const float* x, int64_t x_bstride, const float* w0, const float* scale0,
                            const float* shift0, const float* w1, const float* scale1,
                            const float* shift1, void* y, int64_t y_bstride, int B, int cin, int c0,
                            int c1, int Hi, int Wi, int dtype, void* stream);


/* Trilinear resample.  Replaces F.interpolate(mode='trilinear') at
 * skip_model_3d.py:48,50 and nn.Upsample at :162-164 (align_corners=1), with
 * PyTorch's source-index rule, then an optional epilogue
 *   y = act(scale[c] * interp(x) + shift[c])      (scale/shift NULL: identity)
 * with act = ReLU under LEA_RELU.  With the epilogue it completes an up-sampling
 * ConvBR1x1 whose conv ran at the input resolution (the conv and the
 * interpolation commute). */
int lea_resample3d_trilinear(const void* x, int64_t x_bstride, void* y, int64_t y_bstride,
                             int B, int C, int Di, int Hi, int Wi, int Do, int Ho, int Wo,
                             int align_corners, const float* scale, const float* shift,
                             unsigned flags, int dtype, void* stream);

/* Head conv of an upsampled tensor, from per-tap partial sums.  Replaces
 * last_3(Upsample(y)) (skip_model_3d.py:161-173, 3x3x3 conv after a trilinear
 * align_corners=True resize): with q[b][co*27 + tap] = sum_ci W[co][ci][tap]*y[ci]
 * computed at the low resolution (lea_conv3d_bnrelu, k=1, 27*cout outputs),
 *   y_out[b][co](v) = act(scale[co] * sum_tap interp(q[b][co*27+tap])(v + off(tap)) + shift[co])
 * over the [Do, Ho, Wo] output, taps outside it contributing 0 (zero padding).
 * q: [B, 27*cout, Di, Hi, Wi]; y_out: [B, cout, Do, Ho, Wo].  workspace: device
 * scratch of lea_tapsum_workspace_bytes(B, cout, Hi, Wi, Do) bytes, 16-B aligned
 * (the d-interpolated partial sums; the caller owns it, as every buffer here). */
size_t lea_tapsum_workspace_bytes(int B, int cout, int Hi, int Wi, int Do);
int lea_tapsum_upsample(const void* q, int64_t q_bstride, void* y, int64_t y_bstride,
                        int B, int cout, int Di, int Hi, int Wi, int Do, int Ho, int Wo,
                        const float* scale, const float* shift, unsigned flags,
                        void* workspace, int dtype, void* stream);

/* Disparity regression.  Replaces models/build_model_2d.py:52-57 + :33-42:
 *   U = trilinear(cost, [maxdisp, 3*H3, 3*W3], align_corners=False)
 *   disp[b, h, w] = sum_d d * softmax(-U, dim=d)
 * fused, U never materialised.  cost: [B, 1, D3, H3, W3]; disp: [B, 3H3, 3W3] fp32.
 * dtype LEA_BF16 (the bf16 path; cost still f32) uses the hardware exp. */
int lea_disparity_regression(const void* cost, float* disp, int B, int D3, int H3, int W3,
                             int maxdisp, int dtype, void* stream);

/* Disparity regression with per-pixel confidence (ABI 14).  lea_disparity_regression's
 * fused head (build_model_2d.py:52-57) that also writes what the distribution it forms
 * says about each pixel -- what the reference's unused DispEntropy (build_model_2d.py:11-24;
 * as written: softmax instead of softmin, then a softmin over the image height) set out
 * to give.  Per pixel, with U[od], od in [0, maxdisp), the up-sampled cost as above,
 * p = softmax(-U) and v[k], k in [0, D3), the bilinearly (H, W) interpolated cost planes:
 *   disp       = sum_od od p[od]: lea_disparity_regression's output, bit for bit under its
 *                default form at the configured depths D3 in {4, 8, 16, 32, 64, 88}
 *   entropy    = -sum_od p ln p, nats, in [0, ln maxdisp] (p == 0 contributes 0)
 *   winner     k* = the first index of min_k v[k], od* = 3 k* + 1 (od = 3k + 1 lies on
 *                plane k; defined on the planes because U[0] == U[1] and U[maxdisp-2],
 *                U[maxdisp-1] tie up to rounding: an argmin over od flips at the ends)
 *   peak       = sum_{|od - od*| <= radius} p[od], in (0, 1]: the mass around the mode
 *   disp_local = sum_{|od - od*| <= radius} od p[od] / peak: the soft-argmin of the
 *                winner's window, which does not average two modes
 * the window clipped to [0, maxdisp); radius in 1..16 (4 = the nine samples of planes
 * k* - 1 .. k* + 1).  cost: [B, 1, D3, H3, W3] f32; every output [B, 3H3, 3W3] f32.
 * entropy, peak, disp_local: NULL = not wanted (never written); at least one non-NULL.
 * maxdisp must be 3 * D3 (else LEA_E_UNSUPPORTED; lea_disparity_regression takes the
 * rest).  No output may overlap another or cost (LEA_E_INVALID).  dtype as for
 * lea_disparity_regression.  One launch; lea_disparity_set_register_form does not
 * affect it. */
int lea_disparity_regression_stats(const void* cost, float* disp, float* entropy, float* peak,
                                   float* disp_local, int B, int D3, int H3, int W3, int maxdisp,
                                   int radius, int dtype, void* stream);

/* Left-right check (additive: the ABI number stays 14; a library without these symbols
 * fails to load).  The matching cost already scores every (left pixel, disparity) pair, so
 * the right view's distribution is the up-sampled cost read along its diagonals -- right
 * pixel xr at disparity od is left pixel xr + od -- one more head-sized launch on the cost
 * the forward has produced, not a second forward on the mirrored pair.
 *
 * Right-view disparity.  U[od, y, x] as for lea_disparity_regression: the trilinear
 * align_corners=False up-sampling of cost[b, 0] to [MD, Ho, Wo]; MD = maxdisp = 3 D3 is
 * required, Ho = 3 H3, Wo = 3 W3.  For a right-image pixel (y, xr):
 *   candidate od is in view iff xr + od <= Wo - 1 (at least od = 0 always is)
 *   n = min(MD, Wo - xr)
 *   p_R[od] = softmax over od < n of (-U[od, y, xr + od])
 *   disp_right[b, y, xr] = sum_{od < n} od p_R[od]
 * The last column is therefore exactly 0; MD > Wo is legal.
 * cost: [B, 1, D3, H3, W3] f32; disp_right: [B, 3H3, 3W3] f32.  Any D3 >= 1.
 * maxdisp != 3 D3: LEA_E_UNSUPPORTED.  A null pointer, a non-positive size or an output
 * that overlaps the cost: LEA_E_INVALID.  dtype as for lea_disparity_regression (LEA_BF16:
 * the hardware exponential; anything else unknown: LEA_E_UNSUPPORTED).  One launch, no
 * allocation, no synchronisation. */
int lea_disparity_regression_right(const void* cost, float* disp_right, int B, int D3, int H3,
                                   int W3, int maxdisp, int dtype, void* stream);

/* The check and the scanline fill, per left pixel (y, x) with dL = disp_left[b, y, x] and
 * threshold > 0:
 *   xi = floor(x - dL + 0.5), in f32 without contraction
 *   state (uint8) = 2 (out of view)   if xi < 0 or xi > W - 1
 *                   1 (inconsistent)  otherwise, if dL is not finite or
 *                                     !(|dL - disp_right[b, y, xi]| <= threshold)
 *                   0 (consistent)    otherwise
 *   disp_filled   = dL bit for bit where state == 0; elsewhere the dL of the nearest
 *                   state-0 pixel to the left on the same row and of the nearest one to the
 *                   right, the smaller of the two (the background is the smaller
 *                   disparity); the one that exists if only one does; dL unchanged if the
 *                   row has none.
 * disp_left, disp_right, disp_filled: [B, H, W] f32; state: [B, H, W] bytes.  state or
 * disp_filled may be NULL (not wanted, never written); both NULL: LEA_E_INVALID.  Any
 * W >= 1.  threshold not > 0 or not finite: LEA_E_INVALID.  No output may overlap an input
 * or the other output (LEA_E_INVALID).  One launch. */
int lea_disparity_lr_check(const float* disp_left, const float* disp_right, uint8_t* state,
                           float* disp_filled, int B, int H, int W, float threshold, void* stream);

/* Edge-aware training loss (additive: the ABI number stays 14).  The reference's objective
 * is train.py:107-118 combined_loss = smooth-L1 over the valid pixels + edge_loss_w *
 * gradient_aware_loss2 (edge_detection.py:68-74), whose target is smoothed by two 5x5
 * median passes on the host (edge_detection.py:7-11).  Three entries keep all of it on the
 * device: the median, the forward sums and the gradient.  None synchronises the host,
 * allocates or reads anything back; batch strides are in elements.
 *
 * 5x5 median, once or twice over.  y[b] = med(x[b]) for iterations = 1, med(med(x[b])) for
 * iterations = 2, med being the exact 5x5 median (the 13th of the 25 window values) with
 * the border replicated, as OpenCV's medianBlur documents (BORDER_REPLICATE).  The second
 * pass replicates the first pass's outputs at the border.  One launch either way.
 * x, y: [B, H, W] f32, batch strides >= H*W; H, W >= 1 (sizes below 5 are legal).
 * x must hold no NaN (the result is then unspecified); +-inf is an ordinary value.
 * A null pointer, iterations outside {1, 2}, a batch stride below H*W, a non-positive size
 * or a y that overlaps x: LEA_E_INVALID, before any launch. */
int lea_median5x5_f32(const float* x, int64_t x_bstride, float* y, int64_t y_bstride, int B,
                      int H, int W, int iterations, void* stream);

/* Forward sums.  pred, target, tsmooth (the twice-median target): [B, H, W] f32, H, W >= 3.
 *   m = (target < maxdisp) & (target > 0.001),  d = pred - target
 *   sums[0] = number of pixels in m
 *   sums[1] = sum over m of smooth_l1(d), beta = 1: 0.5 d^2 if |d| < 1, else |d| - 0.5
 *   sums[2] = sum over m of |d|                               (the train loop's EPE)
 *   sums[3] = sum over the batch and the (H-2) x (W-2) positions of the valid 3x3
 *             cross-correlation of |Sx pred| exp(-|Sx tsmooth|) + |Sy pred| exp(-|Sy tsmooth|),
 *             Sx = [[-1,0,1],[-2,0,2],[-1,0,1]], Sy = [[1,2,1],[0,0,0],[-1,-2,-1]]; the
 *             mask does not apply to it.
 * The losses are sums[1] / sums[0] and sums[3] / (B (H-2)(W-2)); the weight between them
 * is the caller's.  Terms in f32, summed in float64 in a fixed order: the same inputs give
 * the same bits.  sums: 4 doubles on the device; workspace:
 * lea_edge_loss_workspace_bytes(B, H, W) bytes on the device, both 8-byte aligned.  One
 * pass over the maps and a one-workgroup reduction of its partials, in this call. */
size_t lea_edge_loss_workspace_bytes(int B, int H, int W);
int lea_edge_loss_f32(const float* pred, int64_t pred_bstride, const float* target,
                      int64_t target_bstride, const float* tsmooth, int64_t tsmooth_bstride,
                      int B, int H, int W, float maxdisp, double* sums, void* workspace,
                      void* stream);

/* Gradient with respect to pred of g_d * sums[1] / sums[0] + g_e * sums[3] / (B (H-2)(W-2)):
 *   dpred = g_d m clamp(d, -1, 1) / n  +  g_e / (B (H-2)(W-2)) * sum over the positions that
 *           cover the pixel of sign(Sx pred) exp(-|Sx tsmooth|) Sx[ky][kx]
 *                            + sign(Sy pred) exp(-|Sy tsmooth|) Sy[ky][kx]
 * with sign(0) = 0.  n = sums[0] (as lea_edge_loss_f32 left it) and scales = {g_d, g_e}
 * (2 floats) are read on the device.  n = 0: the direct part is 0.  One launch, no atomics,
 * every pixel of dpred written.  dpred may overlap none of the inputs. */
int lea_edge_loss_grad_f32(const float* pred, int64_t pred_bstride, const float* target,
                           int64_t target_bstride, const float* tsmooth, int64_t tsmooth_bstride,
                           const double* sums, const float* scales, float* dpred,
                           int64_t dpred_bstride, int B, int H, int W, float maxdisp,
                           void* stream);

/* Photometric consistency (additive: the ABI number stays 14).  The right image is warped
 * to the left view with a disparity map and compared with the left image by an SSIM + L1
 * error: a label-free quality measure and the self-supervised training signal.  Three
 * entries: the workspace query, the forward sums (with two optional maps) and the gradient
 * with respect to the disparity.  None synchronises the host, allocates or reads anything
 * back; batch strides are in elements.
 *
 * Inputs.  left, right: [B, C, H, W] f32, 1 <= C <= 4, H, W >= 3, the (C, H, W) block
 * contiguous, any batch stride >= C*H*W.  disp: [B, H, W] f32, batch stride >= H*W.
 * exclude: NULL or [B, H, W] bytes, batch stride >= H*W; non-zero = the pixel takes no part
 * (the state of lea_disparity_lr_check can be passed as it is).  0 <= alpha <= 1, c1, c2 > 0.
 *
 * Warp, per pixel (y, x) and channel c, R = right[b, c]:
 *   xs      = float(x) - disp[b, y, x]            one f32 subtraction
 *   in_view = isfinite(disp) && xs >= 0 && xs <= W - 1
 *   x0      = min(floor(xs), W - 2),  t = xs - x0  (exact; 0 <= t <= 1)
 *   w_c     = R[y, x0] + t (R[y, x0 + 1] - R[y, x0]),  correctly rounded to f32
 *   dw_c / ddisp = -(R[y, x0 + 1] - R[y, x0])      at an integer xs: the cell to its right
 *   out of view: w_c = 0 and the derivative is 0.
 * Masks: v(p) = in_view(p) && !exclude(p); vs(p) = p is an interior position
 * (1 <= y <= H - 2, 1 <= x <= W - 2) and v holds on all nine pixels of its 3x3 window.
 * Terms, in f32:
 *   l1(p)    = mean_c |L_c - w_c|
 *   dssim(p) = mean_c clamp((1 - SSIM_c(p)) / 2, 0, 1)
 *   SSIM     = (2 mu_x mu_y + c1)(2 s_xy + c2) / ((mu_x^2 + mu_y^2 + c1)(s_x^2 + s_y^2 + c2))
 *              over the 3x3 window, x = left, y = warped; mu = box sum / 9,
 *              s_x^2 = E[x^2] - mu_x^2, s_xy = E[xy] - mu_x mu_y (evaluated in the centred
 *              form sum (x - mu)^2 / 9, the same function with less cancellation).
 * Sums, float64, in a fixed order (per-workgroup partials in the workspace, reduced by one
 * workgroup in the same call; the same inputs give the same bits):
 *   sums[0] = #v   sums[1] = sum_v l1   sums[2] = #vs   sums[3] = sum_vs dssim
 * The loss is (1 - alpha) sums[1] / sums[0] + alpha sums[3] / sums[2], a term whose count is
 * 0 being 0.
 * Optional outputs (NULL = not written): warped [B, C, H, W] contiguous; err [B, H, W]
 * contiguous = (1 - alpha) l1 + alpha dssim where vs holds, l1 where only v holds, -1
 * elsewhere.  alpha is used for err only.
 * sums: 4 doubles on the device; workspace: lea_photometric_workspace_bytes(B, H, W) bytes
 * on the device; both 8-byte aligned.
 * LEA_E_INVALID, before any launch: a null left, right, disp, sums or workspace; B < 1;
 * C outside 1..4; H or W < 3; a batch stride below the map size; alpha outside [0, 1]; c1 or
 * c2 not positive; sums, workspace, warped or err overlapping an input or one another;
 * sums or workspace misaligned. */
size_t lea_photometric_workspace_bytes(int B, int H, int W);
int lea_photometric_f32(const float* left, int64_t left_bstride, const float* right,
                        int64_t right_bstride, const float* disp, int64_t disp_bstride,
                        const uint8_t* exclude, int64_t exclude_bstride, int B, int C, int H,
                        int W, float alpha, float c1, float c2, double* sums, void* workspace,
                        float* warped, float* err, void* stream);

/* ddisp [B, H, W] = the gradient with respect to disp of
 * g_l sums[1] / sums[0] + g_s sums[3] / sums[2]; scales = {g_l, g_s} (2 floats) and the
 * counts sums[0], sums[2] (as lea_photometric_f32 left them) are read on the device; a term
 * whose count is 0 has gradient 0.  The L1 part uses sign(w_c - L_c) with sign(0) = 0; the
 * SSIM part uses the unclamped derivative (the clamp only bites where rounding pushed SSIM
 * past +-1, and the true derivative there is 0), in the gather form: with n1, n2, d1, d2 the
 * four SSIM factors of window p and S = n1 n2 / (d1 d2),
 *   dS_p / dw_q = (a_p + b_p w_q + c_p L_q) / 9
 *   a = 2 mu_x (n2 - n1) / (d1 d2) - 2 S mu_y (1/d1 - 1/d2),  b = -2 S / d2,  c = 2 n1 / (d1 d2)
 * summed over the <= 9 windows with vs that hold q.  Every pixel is written (0 where v
 * fails), one launch, no atomics.  ddisp: batch stride >= H*W; it may overlap none of the
 * inputs, sums or scales.  Argument checks as for lea_photometric_f32. */
int lea_photometric_grad_f32(const float* left, int64_t left_bstride, const float* right,
                             int64_t right_bstride, const float* disp, int64_t disp_bstride,
                             const uint8_t* exclude, int64_t exclude_bstride, int B, int C,
                             int H, int W, float c1, float c2, const double* sums,
                             const float* scales, float* ddisp, int64_t ddisp_bstride,
                             void* stream);

/* Confidence-weighted edge-preserving disparity refinement (additive: the ABI number stays
 * 14): the weighted-least-squares smoothing of OpenCV's ximgproc disparity WLS filter, solved
 * with the fast global smoother (Min et al., "Fast global image smoothing based on weighted
 * least squares", 2014).  Confident pixels keep their disparity; excluded, non-finite and
 * zero-confidence ones are filled from confident neighbours on the same side of an edge of
 * the guide image.  Neither entry synchronises the host, allocates or reads anything back.
 *
 * Inputs.  guide: [B, C, H, W] f32, 1 <= C <= 4, the (C, H, W) block contiguous, batch
 * stride guide_bstride >= C*H*W in elements.  disp: [B, H, W] f32.  conf: [B, H, W] f32 or
 * NULL (= 1 everywhere).  exclude: [B, H, W] bytes or NULL; non-zero = no evidence (the
 * state of lea_disparity_lr_check can be passed as it is).  Any H, W >= 1.
 * lambda > 0, sigma > 0, 1 <= iterations (T) <= 8 (the result is unspecified for a lambda
 * above 1e30, where lambda_t w overflows the reciprocal).
 *
 * Evidence.  c0 = conf, but 0 where exclude != 0, disp is not finite, or conf is not finite
 * or <= 0; f0 = disp where c0 > 0, else 0 (a NaN under a zero weight never enters the
 * arithmetic).  num = c0 * f0, den = c0.
 * Edge weights, once per call, with the accurate expf:
 *   wh[y, x] = exp(-(max_c |G[c, y, x+1] - G[c, y, x]|) / sigma)   for x < W - 1
 *   wv[y, x] = the same along y                                     for y < H - 1
 * Schedule.  For t = 1 .. T: lambda_t = 1.5 lambda 4^(T-t) / (4^T - 1), formed in double on
 * the host and cast to f32; iteration t is a horizontal pass (every row), then a vertical
 * pass (every column), both with lambda_t.
 * One pass solves, for every line of n pixels with neighbour weights w_i (between i and
 * i + 1), the system (I + lambda_t L) u = r:
 *   a_i = -lambda_t w_(i-1) (0 at i = 0),  c_i = -lambda_t w_i (0 at i = n - 1),
 *   b_i = 1 - a_i - c_i,    a_i u_(i-1) + b_i u_i + c_i u_(i+1) = r_i
 * for the two right-hand sides num and den, which share the matrix; the pass overwrites
 * both.  A line of one pixel is the identity.  The systems are strictly diagonally dominant,
 * so they are eliminated without pivoting, in f32 (a Thomas sweep per line: the same inputs
 * give the same bits, call after call).
 * Outputs.  refined [B, H, W] = num / den where den > 1e-30f; elsewhere disp bit for bit, or
 * 0 if disp is not finite (den underflows only deep inside a region without evidence at a
 * small lambda).  support [B, H, W] (NULL = not written) = den: how much confident evidence
 * reached the pixel.
 * workspace: lea_disparity_refine_workspace_bytes(B, H, W) bytes on the device (0 for a
 * non-positive size), 4-byte aligned.  2 + 4 T launches on the stream; capturable.
 * LEA_E_INVALID, before any launch: a null guide, disp, workspace or refined; B, H or W < 1
 * (or B above 32767, H or W above 2^21, B*H*W above 2^31 - 1); C outside 1..4; iterations outside 1..8;
 * lambda or sigma not a finite number > 0; a guide batch stride below C*H*W; a misaligned
 * workspace; refined or support overlapping an input, the workspace or one another; the
 * workspace overlapping an input. */
size_t lea_disparity_refine_workspace_bytes(int B, int H, int W);
int lea_disparity_refine_f32(const float* guide, int64_t guide_bstride, const float* disp,
                             const float* conf, const uint8_t* exclude, int B, int C, int H,
                             int W, float lambda, float sigma, int iterations, void* workspace,
                             float* refined, float* support, void* stream);

/* Speckle filter (additive: the ABI number stays 14): the connected components of a
 * disparity map and the removal of the small ones, OpenCV's filterSpeckles (the
 * speckleWindowSize / speckleRange of StereoBM / StereoSGBM), on the device.  It belongs
 * between the left-right check and the refinement: the refinement spreads a confident
 * speckle, and fills an excluded one from its neighbours.  Neither entry synchronises the
 * host, allocates or reads anything back.
 *
 * Inputs.  disp: [B, H, W] f32.  exclude: [B, H, W] bytes or NULL (the state of
 * lea_disparity_lr_check can be passed as it is).  max_diff: finite, >= 0.  max_size: >= 0.
 * fill: any float, NaN allowed.
 * Connectivity.  A pixel is a wall if its disp is not finite or its exclude is non-zero; a
 * wall belongs to no component.  Two 4-neighbours of the same image are connected if neither
 * is a wall and fabsf(a - b) <= max_diff in f32 (the subtraction is exactly rounded; -0.0 and
 * 0.0 are connected at max_diff = 0).  The components are the connected components of that
 * graph: the edges are pairwise, so the values may drift along a component.  Images of a
 * batch never connect.
 * Outputs, each [B, H, W], each optional through NULL (never written), at least one required:
 *   labels   (int32) the smallest linear index y*W + x of the pixel's component; -1 for a wall
 *   size     (int32) the number of pixels of the pixel's component; 0 for a wall
 *   state    (uint8) exclude where that is non-zero; elsewhere 3 (LEA_LR_SPECKLE, beside the
 *            0 / 1 / 2 of lea_disparity_lr_check) where 0 < size <= max_size and 0 otherwise;
 *            a pixel whose disp is not finite and whose exclude is 0 gets 3 too: it carries
 *            no evidence.  max_size = 0 removes no component.
 *   filtered (f32) fill where state != 0, disp bit for bit elsewhere
 * The labels are canonical and the sizes integer sums, so all four are the same bits call
 * after call, whatever the scheduling.
 * workspace: lea_disparity_speckle_workspace_bytes(B, H, W) bytes on the device (0 for a
 * non-positive size), 4-byte aligned; its contents need not be initialised.  Four launches on
 * the stream (three when the image is one tile); capturable.
 * LEA_E_INVALID, before any launch: a null disp or workspace; every output null; B, H or
 * W < 1 (or B above 65535, H above 1048560, H*W not below 2^31); max_diff negative or not finite;
 * max_size negative; a misaligned workspace; an output overlapping an input, the workspace or
 * another output; the workspace overlapping an input. */
#define LEA_LR_SPECKLE 3
size_t lea_disparity_speckle_workspace_bytes(int B, int H, int W);
int lea_disparity_speckle_f32(const float* disp, const uint8_t* exclude, int B, int H, int W,
                              float max_diff, int max_size, float fill, void* workspace,
                              int32_t* labels, int32_t* size, uint8_t* state, float* filtered,
                              void* stream);

/* Point cloud (additive: the ABI number stays 14): the reprojection of a disparity map to 3-D
 * through a 4 x 4 matrix (OpenCV's reprojectImageTo3D), the validity of every pixel, and the
 * valid points compacted in row-major pixel order with their colours, pixel indices and
 * normals, on the device.  It is the last stage of the chain: after the left-right check, the
 * speckle filter and the refinement.  Neither entry synchronises the host, allocates or reads
 * anything back: the number of points stays on the device.
 *
 * Inputs.  disp: [B, H, W] f32.  exclude: [B, H, W] bytes or NULL (the state of
 * lea_disparity_lr_check / lea_disparity_speckle_f32 can be passed as it is; any non-zero byte
 * excludes).  image: uint8 [B, H, W, pix_stride] or NULL, pix_stride 3 or 4, the first three
 * channels are the colour (what lea_standardize_crop_u8 takes).  Q: f32 [16] per image on the
 * device, row-major, image b's at Q + b * q_bstride (floats; 0 = one matrix for all, else
 * >= 16).  min_disp, max_disp: not NaN, infinities allowed.  normal_max_diff: >= 0, +inf
 * allowed.  capacity: rows per image of the compact outputs.
 * Point.  With d = disp[y, x] and every product and sum rounded on its own, in this order:
 *   h_r = ((Q[r][0] * x + Q[r][1] * y) + Q[r][2] * d) + Q[r][3],  r = 0 .. 3
 *   P = (h_0 / h_3, h_1 / h_3, h_2 / h_3)      (IEEE divisions)
 * The pixel is valid when exclude is 0 (or NULL), d is finite, min_disp < d <= max_disp, and
 * the three coordinates of P are finite (they are not where h_3 = 0).
 * Normal of a valid pixel p.  Along an axis a neighbour q is usable when it is inside the
 * image, valid, and fabsf(d_q - d_p) <= normal_max_diff (the speckle filter's connectivity).
 * dx = P(x + 1) - P(x - 1) with both usable, one-sided against P(p) with one, absent with
 * none; dy the same along y.  c = dx x dy, n = c / |c| (sqrtf of the sum of squares), negated
 * when n . P > 0: towards a camera at the origin.  (0, 0, 0) when dx or dy is absent or |c|
 * is 0 or not finite.
 * Outputs, each optional through NULL (never written), at least one required:
 *   points  [B, H, W, 3] f32   the organised cloud; a quiet NaN in all three where not valid
 *   valid   [B, H, W] u8       1 / 0
 *   count   [B] int32          the number of valid pixels, also where it exceeds capacity
 *   xyz     [B, capacity, 3] f32   row k of image b: the point of its k-th valid pixel in
 *                                  row-major order, the bits of points at that pixel
 *   rgb     [B, capacity, 3] u8    its colour (needs image)
 *   index   [B, capacity] int32    its y * W + x
 *   normals [B, capacity, 3] f32   its normal
 * Rows at and beyond min(count[b], capacity) are not written; with count[b] > capacity the
 * first capacity points are kept.  A row is a function of the validity map alone (ballots and
 * an exclusive scan, no atomics), so every output is the same bits call after call.
 * workspace: lea_disparity_pointcloud_workspace_bytes(B, H, W) bytes on the device (0 for a
 * non-positive size), 4-byte aligned; its contents need not be initialised.  Three launches
 * on the stream (two without a compact output, one with points / valid alone); capturable,
 * and a replay reads Q anew.
 * LEA_E_INVALID, before any launch: a null disp, Q or workspace; every output null; rgb
 * without image; pix_stride not 3 or 4 with an image; B, H or W < 1 (or B above 65535,
 * B*H*W above 2^31 - 1); a Q stride that is neither 0 nor >= 16; capacity negative, or 0 with
 * a compact output; min_disp, max_disp or normal_max_diff NaN, normal_max_diff negative; a
 * misaligned workspace; an output overlapping an input, the workspace or another output; the
 * workspace overlapping an input. */
size_t lea_disparity_pointcloud_workspace_bytes(int B, int H, int W);
int lea_disparity_pointcloud_f32(const float* disp, const uint8_t* exclude, const void* image,
                                 int pix_stride, const float* Q, int64_t q_bstride, int B, int H,
                                 int W, float min_disp, float max_disp, float normal_max_diff,
                                 int capacity, void* workspace, float* points, uint8_t* valid,
                                 int32_t* count, float* xyz, uint8_t* rgb, int32_t* index,
                                 float* normals, void* stream);

/* Rectification (additive: the ABI number stays 14): the first stage of the chain.  One launch
 * undistorts and rectifies both raw views of a batch, bilinear, uint8 in and out, from a
 * calibration block in device memory or from given maps.  It takes no workspace, uses no
 * atomics, makes no host copy and does not synchronise; capturable, the same bits call after
 * call, and a replay reads calib (or maps_in) anew.
 *
 * Inputs.  left, right: uint8 [B, H, W, pix_stride], pix_stride 3 or 4, as decoded; every
 * channel is interpolated, alpha included.  Exactly one of calib and maps_in.  fill: the
 * border value, 0 .. 255.
 *   calib    f32 [Bc, 2, 24] on the device, Bc 1 or B; view 0 is left.  The 24 floats of a view:
 *            M[9] row-major, M = R_k^T K_new,k^-1 (a rectified pixel (u, v, 1) to a ray of the
 *            raw camera); fx, fy, cx, cy of the raw camera; model (1.0f = fisheye, equidistant;
 *            anything else = the pinhole rational model); k[8]; two pad floats.
 *   maps_in  f32 [Bm, 2, 2, Ho, Wo] on the device, Bm 1 or B: view, then x / y.
 * Map stage (calib), every operation a separately rounded float32 operation in this order:
 *   X = (M0 u + M1 v) + M2, Y = (M3 u + M4 v) + M5, Wc = (M6 u + M7 v) + M8; unless Wc > 0 both
 *   coordinates are NaN.  x = X / Wc, y = Y / Wc, xx = x x, yy = y y, r2 = xx + yy.
 *   Pinhole, k = k1 k2 p1 p2 k3 k4 k5 k6:
 *     rad = (1 + r2 (k1 + r2 (k2 + r2 k3))) / (1 + r2 (k4 + r2 (k5 + r2 k6)))
 *     xd = x rad + ((2 p1) (x y) + p2 (r2 + 2 xx)),  yd = y rad + (p1 (r2 + 2 yy) + (2 p2) (x y))
 *   Fisheye, k = k1 .. k4: r = sqrtf(r2), t = atanf(r), t2 = t t,
 *     td = t (1 + t2 (k1 + t2 (k2 + t2 (k3 + t2 k4)))), (xd, yd) = (x, y) td / r (factor 1 where
 *     r <= 1e-8f).
 *   sx = fx xd + cx, sy = fy yd + cy.
 * Pixel stage, the same for computed and given maps, exact: a pixel is valid when
 * 0 <= sx <= W - 1 and 0 <= sy <= H - 1 (NaN fails); an invalid pixel is fill in every channel.
 * A valid one: x0 = floorf(sx), ax = sx - x0, likewise y; the tap x0 + 1 is clamped to W - 1
 * (its weight is 0 there); top = a + ax (b - a), bot = c + ax (d - c), v = top + ay (bot - top),
 * each operation rounded on its own; the output is rintf(v) (half to even).
 * Outputs.  out_left, out_right: uint8 [B, Ho, Wo, pix_stride].  valid: uint8 [B, 2, Ho, Wo]
 * (1 / 0) or NULL.  maps_out: f32 [B, 2, 2, Ho, Wo] or NULL, the source coordinates the launch
 * used.  Any 48 floats of calib and any values of maps_in are memory-safe (NaN, infinities,
 * 1e30): no value is converted to an integer before the validity test has bounded it.
 * LEA_E_INVALID, before the launch: a null image or output image; pix_stride not 3 or 4; B, H,
 * W, Ho or Wo < 1 (or B above 32767, a size above 65535); both or neither of calib and maps_in;
 * Bc or Bm neither 1 nor B; fill outside 0 .. 255; calib, maps_in or maps_out not 4-byte
 * aligned; an output overlapping an input or another output. */
int lea_rectify_pair_u8(const void* left, const void* right, int pix_stride, int B, int H, int W,
                        const float* calib, int Bc, const float* maps_in, int Bm, int Ho, int Wo,
                        int fill, void* out_left, void* out_right, uint8_t* valid, float* maps_out,
                        void* stream);

/* View synthesis (additive: the ABI number stays 14): an image pushed forward through its own
 * disparity map into another view on the baseline, as a 1-D mesh render per scanline: neighbouring
 * source pixels of one surface span a segment, each target pixel takes the nearest surface that
 * covers it, and what nothing covers is a hole that the scanline rule of lea_disparity_lr_check
 * can fill.  One launch, no workspace, no float atomics, no host copy, no synchronisation;
 * capturable, the same bits call after call, and a replay reads scales anew.
 *
 * Inputs.  image: [B, C, H, W] f32, 1 <= C <= 4, batch stride image_bstride >= C*H*W (elements).
 * disp: [B, H, W] f32, batch stride disp_bstride >= H*W; negative disparities are legal and
 * "nearer" always means the larger d.  exclude: [B, H, W] bytes or NULL (the state of
 * lea_disparity_lr_check / lea_disparity_speckle_f32 can be passed as it is; any non-zero byte
 * excludes).  scales: B floats on the device.  max_diff: finite, >= 0.  1 <= max_stretch <= 64.
 * fill: 0 or 1.  W <= LEA_FORWARD_WARP_MAX_W; B*H <= 2^31 - 1.
 * Per item b and row y, with s = scales[b] and every operation a separately rounded float32
 * operation:
 *   t_x = x - (s * d_x);  ok(x): d_x finite, exclude 0 and t_x finite (a non-finite s makes the
 *   whole item holes).
 *   Point x, for every ok(x): covers u = rintf(t_x) when 0 <= u <= W - 1; z = d_x, a = 0.
 *   Segment x, 0 <= x < W - 1: exists when ok(x), ok(x + 1), |d_{x+1} - d_x| <= max_diff and
 *   0 < den = t_{x+1} - t_x <= max_stretch (fold-overs, degenerate spans and surfaces stretched
 *   further are discontinuities).  It covers every integer u with t_x <= u <= t_{x+1} and
 *   0 <= u <= W - 1;  a = (u - t_x) / den,  z = ((1 - a) * d_x) + (a * d_{x+1}).
 *   Winner at u: the candidate of the largest z (as numbers, -0 = +0); among equal z the larger
 *   source column; for one column the segment over the point.
 *   Hit: state 0; warped_c = ((1 - a) * I_c[x]) + (a * I_c[x+1]), I_c[x] for a point; zview = z;
 *   source = float(x) + a.  The lerp is exact at a = 0 and a = 1, so s = 0 returns image and
 *   disp bit for bit (but for the sign of a zero: (1 * -0) + (0 * v) is +0).
 *   Hole (no candidate): state 1, source -1.  fill = 0: warped = fill_value, zview = NaN.
 *   fill = 1: colour and zview of the nearest hit to the left on the row or of the nearest to
 *   the right, the one of the smaller zview (the background), the left one on a tie, the one that
 *   exists if only one does; a row without a hit as fill = 0.  state stays 1.
 * Outputs, each optional through NULL (never written), at least one required: warped
 * [B, C, H, W] f32, zview [B, H, W] f32, state [B, H, W] u8, source [B, H, W] f32, contiguous.
 * Any contents of disp and scales are memory-safe (NaN, infinities, 1e30, denormals): no value is
 * converted to an integer before a float comparison has bounded it, and a segment covers at most
 * max_stretch + 1 targets.
 * LEA_E_INVALID, before the launch: a null image, disp or scales; every output null; B, H or
 * W < 1 or beyond the limits above; C outside 1 .. 4; a batch stride below its block; max_diff
 * negative or not finite; max_stretch outside 1 .. 64 or NaN; fill neither 0 nor 1; an output
 * overlapping an input, scales or another output. */
#define LEA_FORWARD_WARP_MAX_W 4096
int lea_forward_warp_f32(const float* image, int64_t image_bstride, const float* disp,
                         int64_t disp_bstride, const uint8_t* exclude, const float* scales, int B,
                         int C, int H, int W, float max_diff, float max_stretch, int fill,
                         float fill_value, float* warped, float* zview, uint8_t* state,
                         float* source, void* stream);

/* Surface model (additive: the ABI number stays 14): point clouds rasterised into a regular
 * ground grid that keeps, per cell, the highest surface seen there (a digital surface model)
 * and the colour or the row of that surface (an orthophoto).  The grid is a persistent
 * accumulator: any number of lea_dsm_splat_f32 calls add clouds to it, lea_dsm_resolve_f32 reads
 * it out without changing it, lea_dsm_clear empties it.  No entry synchronises the host,
 * allocates or reads anything back; all three are capturable.
 *
 * The key.  A surface is keys: uint64 [B, GH, GW]; 0 is an empty cell.  A hit of height z with a
 * 32-bit payload has the key (ord(z) << 32) | payload, where ord maps the bits b of a float32 to
 * ~b for a negative (sign bit set, -0.0 included) and to b | 0x80000000 otherwise: unsigned order
 * on ord is numeric order on z, with -0.0 just below +0.0.  z is finite, so ord(z) >= 0x00800000
 * and a hit is never 0.  A cell holds the unsigned 64-bit maximum of the keys of the hits that
 * cover it: the highest surface, and among equal heights the larger payload.  A maximum does
 * not depend on the order of its operands, so a grid is the same bits call after call, whatever
 * the scheduling, the order in which clouds are added, and the form of the scatter.
 *
 * lea_dsm_splat_f32.  points: f32 [B, rows, 3] (an organised cloud flattened, or compact rows).
 * count: int32 [B] on the device or NULL; rows at and beyond min(max(count[b], 0), rows) are not
 * read (NULL: all rows).  colours: uint8 [B, rows, 3] or NULL.  G: f32 [12] per item on the
 * device, a row-major 3 x 4 matrix, item b's at G + b * g_bstride (floats; 0 = one matrix for
 * all, else >= 12), read at every launch and replay.  radius: in cells,
 * 0 <= radius <= LEA_DSM_MAX_RADIUS.  row_width: 0, or the width of the image the rows are the
 * pixels of (0 .. rows), a performance hint alone: the result does not depend on it.  staging:
 * LEA_DSM_STAGING_AUTO, _GLOBAL or _LDS; the result does not depend on it either.
 * Per row (X, Y, Z), every product and sum a separately rounded float32 operation, in this order:
 *   u = ((G[0][0] * X + G[0][1] * Y) + G[0][2] * Z) + G[0][3]
 *   v = ((G[1][0] * X + G[1][1] * Y) + G[1][2] * Z) + G[1][3]
 *   z = ((G[2][0] * X + G[2][1] * Y) + G[2][2] * Z) + G[2][3]
 * The row is skipped when X, Y, Z, u, v or z is not finite or |u| or |v| exceeds 2^30 (compared
 * as floats, before any conversion to an integer).  Cell i has its centre at the integer i.  The
 * row covers columns floorf((u - radius) + 0.5f) .. floorf((u + radius) + 0.5f) and rows
 * floorf((v - radius) + 0.5f) .. floorf((v + radius) + 0.5f), clipped to the grid: at most 5 x 5
 * cells, the nearest cell (floorf(u + 0.5f), floorf(v + 0.5f)) alone at radius 0.
 * Payload: with colours R << 16 | G << 8 | B; without, 0xFFFFFFFF - row (row within the item),
 * so that the smallest row wins among equal heights and lea_dsm_resolve_f32 gives it back.
 * hits: int32 [B, GH, GW] or NULL; hits[nearest cell] += 1 (an integer atomic add) for every row
 * that is not skipped and whose nearest cell is in the grid, whatever the radius.
 * The two forms of the scatter.  Global: one 64-bit atomic max on keys per covered cell.
 * LDS-staged: a workgroup takes 1024 rows (consecutive, or a 32 x 32 pixel patch with
 * row_width > 0) and the bounding box of the cells they cover; a box of at most 4096 cells is
 * zeroed in LDS (48 KB with the counts: three workgroups a CU), takes the hits with LDS
 * atomics and is flushed as contiguous runs of global atomics, non-empty cells only; a larger
 * box takes the global form.  The two give identical bits on every input.  Auto is the staged
 * form where it was measured not slower on model-like fields ("Surface model"): with
 * row_width > 0; the global form for runs of rows.
 * Any contents of points, count, G and colours are memory-safe (NaN, infinities, 1e30,
 * denormals, negative counts).  One launch; no lock, no spin, no workgroup waits for another, no
 * float atomics.
 * LEA_E_INVALID, before any launch: a null points, G or keys; B, rows, GH or GW < 1 (or B above
 * 65535, B*GH*GW or B*rows above 2^31 - 1); row_width outside 0 .. rows; a G stride that is
 * neither 0 nor >= 12; radius NaN or outside 0 .. LEA_DSM_MAX_RADIUS; staging outside 0 .. 2;
 * keys not 8-byte aligned; points, G, count or hits not 4-byte aligned; keys or hits overlapping
 * an input or each other.
 *
 * lea_dsm_resolve_f32.  keys as above, never written.  hits: the surface's counts or NULL; not
 * read, only kept apart from the outputs.  iterations (0 .. 1024) fill passes, each reading the
 * buffer the pass before wrote (the first reads keys): a cell empty at the start of the pass with
 * at least min_neighbours (1 .. 8) non-empty cells among its 8 neighbours inside the grid takes
 * the smallest of their keys (the lowest surface beside it, the background, as the left-right
 * fill and the forward warp choose; among equal heights the smaller payload); every other cell
 * keeps its key.  Then, per cell with key k after the passes:
 *   height (f32)        the float whose ord is k >> 32, bit for bit; nodata where k = 0
 *   rgb    (u8 [.., 3]) bits 16-23, 8-15, 0-7 of k; (0, 0, 0) where k = 0
 *   source (int32)      0xFFFFFFFF - (k & 0xFFFFFFFF); -1 where k = 0
 *   state  (u8)         0 measured (keys non-zero), 1 filled, 2 empty
 * each [B, GH, GW], each optional through NULL (never written), at least one required; rgb and
 * source are the two readings of one payload, at most one of them.  workspace:
 * lea_dsm_resolve_workspace_bytes(B, GH, GW) bytes on the device (0 for a non-positive size),
 * 8-byte aligned, contents need not be initialised; may be NULL with iterations = 0.
 * iterations + 1 launches, no atomics.
 * LEA_E_INVALID, before any launch: a null keys; every output null; both rgb and source; B, GH or
 * GW < 1 (or beyond the limits above); iterations outside 0 .. 1024; min_neighbours outside
 * 1 .. 8; a null workspace with iterations > 0; keys or the workspace not 8-byte aligned; height,
 * source or hits not 4-byte aligned; an output overlapping keys, hits, the workspace or another
 * output; the workspace overlapping keys or hits.
 *
 * lea_dsm_clear.  keys, and hits where given, set to 0.  One launch.  LEA_E_INVALID, before the
 * launch: a null keys; B, GH or GW < 1 (or beyond the limits above); misaligned keys or hits;
 * hits overlapping keys. */
#define LEA_DSM_MAX_RADIUS 2
#define LEA_DSM_STAGING_AUTO 0
#define LEA_DSM_STAGING_GLOBAL 1
#define LEA_DSM_STAGING_LDS 2
int lea_dsm_splat_f32(const float* points, const int32_t* count, const uint8_t* colours,
                      const float* G, int64_t g_bstride, int B, int rows, int row_width,
                      float radius, int staging, int GH, int GW, uint64_t* keys, int32_t* hits,
                      void* stream);
size_t lea_dsm_resolve_workspace_bytes(int B, int GH, int GW);
int lea_dsm_resolve_f32(const uint64_t* keys, const int32_t* hits, int B, int GH, int GW,
                        int iterations, int min_neighbours, float nodata, void* workspace,
                        float* height, uint8_t* rgb, int32_t* source, uint8_t* state, void* stream);
int lea_dsm_clear(uint64_t* keys, int32_t* hits, int B, int GH, int GW, void* stream);

/* ---- bf16 path (BASELINE configs 3 and 4) ----
 * Activations are bf16 in the "c8" layout: NCDHW with channels blocked by 8
 * innermost, x[b][c/8][d][h][w][c%8] (one voxel's 8 channels = one 16-byte word;
 * channel counts multiples of 8; a channel slice on a multiple of 8 is a block
 * slice, so the free-cat trick carries over).  Convs run on the bf16 matrix cores
 * (v_mfma_f32_16x16x32_bf16) with f32 accumulation and the f32 BN epilogue;
 * outputs are rounded to bf16.  Batch strides are in elements. */

/* Packed bf16 weights for a ConvBR of this shape (elements; 0 = unsupported), and
 * the packing of an f32 OIDHW weight into them (k in {1, 3}, cin % 8 == 0). */
size_t lea_conv3d_packed_elems_bf16(int cout, int cin, int k);
int lea_conv3d_pack_weights_bf16(const float* w, void* packed, int cout, int cin, int k,
                                 void* stream);

/* lea_conv3d_bnrelu on c8 tensors (cout, cin, cin2 multiples of 8). */
int lea_conv3d_bnrelu_bf16(const void* x, int64_t x_bstride, const void* x2, int64_t x2_bstride,
                           int cin2, const void* w_packed, const float* scale, const float* shift,
                           const void* residual, int64_t r_bstride, void* y, int64_t y_bstride,
                           int B, int cin, int cout, int D, int H, int W, int k, unsigned flags,
                           void* stream);

/* lea_conv3d_bnrelu_costvolume on c8 feature maps [B, C/8, H, W, 8] (C % 16 == 0). */
int lea_conv3d_bnrelu_costvolume_bf16(const void* left, const void* right, int64_t f_bstride,
                                      const void* w_packed, const float* scale, const float* shift,
                                      void* y, int64_t y_bstride, int B, int C, int cout, int D3,
                                      int H, int W, unsigned flags, void* stream);


/* Kernel instantiation the bf16 conv of this shape launches from one source without flags. */
const char* lea_conv3d_kernel_name_bf16(int B, int cout, int cin, int D, int H, int W, int k,
                                        int costvolume);
/* The same for the whole argument list of lea_conv3d_bnrelu_bf16 (cin2 of the cin input channels
 * in the second source; flags: LEA_PAIR_SUM selects the pair launch's kernel); NULL where the
 * launch refuses. */
const char* lea_conv3d_launch_kernel_name_bf16(int B, int cin, int cin2, int cout, int D, int H, int W, int k,
                                               unsigned flags, int costvolume);

/* 1 if lea_conv3d_bnrelu_bf16 takes LEA_PAIR_SUM for two sources of `cin` channels each
 * into `cout` (3x3x3) at this shape -- the planner's D-streaming form under the current
 * tuning (ABI 13) -- else 0; a caller falls back to two launches when 0. */
int lea_conv3d_bf16_pair_supported(int B, int cin, int cout, int D, int H, int W);

/* ConvBR 1x1 of a trilinearly resampled c8 input (align_corners=True): the cell
 * preprocess after a level change, skip_model_3d.py:44-53, without the resampled
 * tensor -- bit-identical to lea_resample3d_trilinear_bf16 (no epilogue) followed by
 * lea_conv3d_bnrelu_bf16 (k = 1).  x: [B, cin/8, Di, Hi, Wi, 8]; y: [B, cout/8, D, H, W, 8];
 * w_packed: the k = 1 packing of lea_conv3d_pack_weights_bf16; cin % 32 == 0 (<= 128),
 * cout in {16, 32, 64}; flags: LEA_RELU. */
int lea_conv1x1_resampled_bf16(const void* x, int64_t x_bstride, int Di, int Hi, int Wi,
                               const void* w_packed, const float* scale, const float* shift,
                               void* y, int64_t y_bstride, int B, int cin, int cout, int D, int H,
                               int W, unsigned flags, void* stream);

/* lea_resample3d_trilinear on c8 tensors (same source-index rule and epilogue). */
int lea_resample3d_trilinear_bf16(const void* x, int64_t x_bstride, void* y, int64_t y_bstride,
                                  int B, int C, int Di, int Hi, int Wi, int Do, int Ho, int Wo,
                                  int align_corners, const float* scale, const float* shift,
                                  unsigned flags, void* stream);


/* Layout converters: f32 NC[D]HW (vol = D*H*W voxels per channel) <-> bf16 c8. */
int lea_to_c8_bf16(const float* x, int64_t x_bstride, void* y, int64_t y_bstride, int B, int C,
                   int64_t vol, void* stream);
int lea_from_c8_bf16(const void* x, int64_t x_bstride, float* y, int64_t y_bstride, int B, int C,
                     int64_t vol, void* stream);

/* lea_tapsum_upsample also takes dtype LEA_BF16: q in the c8 layout, output f32. */

/* Feature-net ConvBR2d 3x3/s1/p1 (operations_2d.py:31-47) on c8 maps [B, C/8, 1, H, W, 8]
 * (the bf16 counterpart of lea_conv2d_bnrelu); weights [cout, cin, 3, 3] f32. */
size_t lea_conv2d_packed_elems_bf16(int cout, int cin);
int lea_conv2d_pack_weights_bf16(const float* w, void* packed, int cout, int cin, void* stream);
int lea_conv2d_bnrelu_bf16(const void* x, int64_t x_bstride, const void* w_packed,
                           const float* scale, const float* shift, const void* residual,
                           int64_t r_bstride, void* y, int64_t y_bstride, int B, int cin, int cout,
                           int H, int W, unsigned flags, void* stream);

/* ---- Winograd F(2,3) / F(4,3)-along-W ConvBR3d, k = 3, fp32 (csrc/conv3d_wino.hip) ----
 * Same operation and arguments as lea_conv3d_bnrelu / lea_conv3d_bnrelu_costvolume
 * (models/operations_3d.py:31-47, retrain/LEAStereo.py:34-48), computed as
 * y[w..w+F-1] = A^T[(G g) . (B^T x)] per (kd, kh): 2/3 (F = 2) or 1/2 (F = 4, on
 * widths that fill 64-wide tile rows) of the direct form's MFMA products, all in
 * fp32.  couts <= 8 run depth-paired (the couts of two output planes share one
 * 16-row MFMA tile, MT = 0 in the kernel name).  Weights are packed by
 * lea_conv3d_wino_pack_weights (a layout of their own, ending in a 256-float zero
 * tail: size the buffer with lea_conv3d_wino_packed_floats); cin (and the first
 * source's channels, and C for the cost volume) must be multiples of 4.        */
size_t lea_conv3d_wino_packed_floats(int cout, int cin);
int lea_conv3d_wino_pack_weights(const float* w, float* packed, int cout, int cin, void* stream);
int lea_conv3d_bnrelu_wino(const void* x, int64_t x_bstride, const void* x2, int64_t x2_bstride,
                           int cin2, const float* w_packed, const float* scale, const float* shift,
                           const void* residual, int64_t r_bstride, void* y, int64_t y_bstride,
                           int B, int cin, int cout, int D, int H, int W, unsigned flags, int dtype,
                           void* stream);
int lea_conv3d_bnrelu_costvolume_wino(const void* left, const void* right, int64_t f_bstride,
                                      const float* w_packed, const float* scale,
                                      const float* shift, void* y, int64_t y_bstride, int B, int C,
                                      int cout, int D3, int H, int W, unsigned flags, int dtype,
                                      void* stream);
/* Kernel instantiation the Winograd entries launch for this shape
 * ("conv3d_wino_kernel<F, Q, MT, NP, TD, CV>", or on the W x D engine
 * "conv3d_wino2_kernel<Q, WC, MTE, NW, OCC, PV, CV>" / "conv3d_wino2p_kernel"; cin = 0:
 * unknown, planned as a deep layer).  The engines' tuning hooks are in
 * leastereo_hip_tuning.h. */
const char* lea_conv3d_wino_kernel_name(int B, int cin, int cout, int D, int H, int W, int costvolume);
/* lea_conv3d_bnrelu_wino whose epilogue down-samples: instead of the layer's output it writes
 *   y [B, cout, D/2, H/2, W/2] = lea_resample3d_trilinear(ConvBR(x), align_corners = 1), bit
 * for bit (for in == 2 out every output voxel reads one aligned 2 x 2 x 2 block, which the
 * F(4,3) x F(4,3) tile's epilogue holds in registers: csrc/conv3d_wino44.hip), so a layer whose
 * only consumer reads it one level down (the matching net's stem1) never writes its
 * full-resolution output.  One source, no residual: LEA_RESIDUAL / LEA_PAIR_SUM are
 * LEA_E_UNSUPPORTED.  D and H even, W % 4 == 0 (else LEA_E_INVALID); y 16-byte aligned.  The
 * entry runs only where the planner puts the shape on the F(4,3) x F(4,3) tile in its default
 * instantiation (lea_conv3d_wino_down2_supported: 1; aligned operands assumed), otherwise
 * LEA_E_UNSUPPORTED and nothing is launched.  lea_conv3d_wino_down2_kernel_name: the
 * instantiation it launches ("conv3d_wino44_down2_kernel"), or NULL where unsupported. */
int lea_conv3d_wino_down2_supported(int B, int cin, int cout, int D, int H, int W);
const char* lea_conv3d_wino_down2_kernel_name(int B, int cin, int cout, int D, int H, int W);
int lea_conv3d_bnrelu_wino_down2(const void* x, int64_t x_bstride, const float* w_packed,
                                 const float* scale, const float* shift, void* y, int64_t y_bstride,
                                 int B, int cin, int cout, int D, int H, int W, unsigned flags, int dtype,
                                 void* stream);
/* The same on two sources, cat(x, x2) along the channels read in place as lea_conv3d_bnrelu_wino
 * takes it (cin2 of the cin channels come from x2; both counts multiples of 4, both sources
 * 16-byte aligned): the matching net's conv1, whose only reader sits one level down.  The
 * launch reports "conv3d_wino44_down2_cat_kernel"; the one-input entry and name are unchanged. */
int lea_conv3d_wino_down2_cat_supported(int B, int cin, int cin2, int cout, int D, int H, int W);
const char* lea_conv3d_wino_down2_cat_kernel_name(int B, int cin, int cin2, int cout, int D, int H, int W);
int lea_conv3d_bnrelu_wino_down2_cat(const void* x, int64_t x_bstride, const void* x2, int64_t x2_bstride,
                                     int cin2, const float* w_packed, const float* scale, const float* shift,
                                     void* y, int64_t y_bstride, int B, int cin, int cout, int D, int H,
                                     int W, unsigned flags, int dtype, void* stream);
/* The depth-paired tiles (couts <= 8) with the same epilogue, for a cell state whose only reader
 * sits one level down: besides y (NULL: not at all -- the residual is still read) the launch
 * writes y2 [B, cout, D/2, H/2, W/2] = lea_resample3d_trilinear(ConvBR(x) [+ residual],
 * align_corners = 1), bit for bit.  flags: LEA_RELU, LEA_RESIDUAL (residual may be y: the
 * accumulate form).  D and H even, W % 4 == 0, cout <= 8, and the planner's depth-paired tile
 * with the buffer-addressed epilogue (lea_conv3d_wino_dp_down2_supported: 1; aligned operands
 * assumed), otherwise LEA_E_UNSUPPORTED and nothing is launched.  y2 16-byte aligned, no
 * overlap with x, y or the residual.  lea_conv3d_wino_dp_down2_kernel_name: the instantiation
 * ("conv3d_wino_dp_down2_kernel<Q, ONLY>", ONLY = y is NULL), or NULL where unsupported. */
int lea_conv3d_wino_dp_down2_supported(int B, int cin, int cout, int D, int H, int W);
const char* lea_conv3d_wino_dp_down2_kernel_name(int B, int cin, int cout, int D, int H, int W, int only);
int lea_conv3d_bnrelu_wino_dp_down2(const void* x, int64_t x_bstride, const float* w_packed,
                                    const float* scale, const float* shift, const void* residual,
                                    int64_t r_bstride, void* y, int64_t y_bstride, void* y2,
                                    int64_t y2_bstride, int B, int cin, int cout, int D, int H, int W,
                                    unsigned flags, int dtype, void* stream);
/* lea_resample3d_trilinear (align_corners = 1) with a down-sampled side output (csrc/resample.hip):
 * besides y [B, C, Do, Ho, Wo] it writes
 *   y2 [B, C, Do/2, Ho/2, Wo/2] = lea_resample3d_trilinear(y -> half, align_corners = 1), bit for
 * bit and without reading y back: the level-down copy of an up-sampling cell preprocess's
 * output.  y is bit-identical to lea_resample3d_trilinear's.  Do and Ho even, Wo % 4 == 0,
 * Do >= Di (no down-sampling along D), rows that fit the LDS, LEA_F32
 * (lea_resample3d_down2_supported: 1), else LEA_E_UNSUPPORTED.  y 16-byte, y2 8-byte aligned.
 * flags: LEA_RELU. */
int lea_resample3d_down2_supported(int Di, int Hi, int Wi, int Do, int Ho, int Wo, int dtype);
int lea_resample3d_trilinear_down2(const void* x, int64_t x_bstride, void* y, int64_t y_bstride, void* y2,
                                   int64_t y2_bstride, int B, int C, int Di, int Hi, int Wi, int Do, int Ho,
                                   int Wo, const float* scale, const float* shift, unsigned flags, int dtype,
                                   void* stream);

/* ---- Matching-net stem0 over the cost volume, factored (csrc/cv_stem.hip) ----
 * Replaces retrain/LEAStereo.py:34-48 + skip_model_3d.py:141 like
 * lea_conv3d_bnrelu_costvolume, without a 3D convolution: every cost-volume plane is
 * a shifted copy of the feature maps, so with u = w - d
 *   conv(cost)[o, d, h, w] = sum_{kd: 0 <= d+kd-1 < D3} ( LK[kd][max(kd-u, 0)][o, h, w]
 *                                                       + Bk[kd][o, h, u-kd+1] )
 * (LK[kd][t] = 0 for kd - u >= 3; Bk[kd] at column -1 = K2[kd] at column 0; the last
 * column w = W-1 subtracts K2[kd][o, h, u-kd+2]), where LK, Bk, K2 are 2D 3x3 convs of
 * the left / right feature maps:
 *   lea_cv_stem_split_weights: stem0's [cout, 2C, 3, 3, 3] f32 weight ->
 *     wl [9 cout, C, 3, 3]: wl[(3 kd + t) cout + o][c][kh][kw] = W[o][c][kd][kh][kw] (kw >= t)
 *     wr [6 cout, C, 3, 3]: wr[kd cout + o] = W[o][C + c][kd]  (Bk)
 *                           wr[(3 + kd) cout + o][c][kh][1] = W[o][C + c][kd][kh][2]  (K2)
 *   maps: lea_conv2d_bnrelu (f32) / lea_conv2d_bnrelu_bf16 (c8) of left with wl and of
 *     right with wr, no BN/ReLU: lmaps [B, 9 cout, H, W], rmaps [B, 6 cout, H, W];
 *   lea_cv_stem_combine: the sum above, the folded BN and ReLU, written as
 *     y [B, cout, D3, H, W] (dtype LEA_F32: NCDHW, W % 4 == 0; LEA_BF16: c8 maps in,
 *     c8 out, cout % 8 == 0).  D3 >= 2.  Equal to the direct conv up to summation
 *     order (and, at bf16, the maps' rounding). */
int lea_cv_stem_split_weights(const float* w, float* wl, float* wr, int cout, int C, void* stream);
int lea_cv_stem_combine(const void* lmaps, int64_t l_bstride, const void* rmaps, int64_t r_bstride,
                        const float* scale, const float* shift, void* y, int64_t y_bstride, int B,
                        int cout, int D3, int H, int W, unsigned flags, int dtype, void* stream);
/* lea_cv_stem_combine (LEA_F32) with a down-sampled side output: besides y it writes
 *   y2 [B, cout, D3/2, H/2, W/2] = lea_resample3d_trilinear(y, align_corners = 1), bit for bit
 * (for in == 2 out every output voxel reads one aligned 2 x 2 x 2 block of y, which the
 * workgroup of a row pair holds in registers), so the matching net's first cell reads stem0
 * at its own level without a second pass over y.  y is bit-identical to lea_cv_stem_combine's.
 * lea_cv_stem_down2_supported: 1 where the entry takes the shape -- LEA_F32, D3 and H even,
 * W % 4 == 0 and every plane of a row pair in one workgroup's LDS (D3 <= 224); anything
 * else is LEA_E_UNSUPPORTED (the caller runs lea_cv_stem_combine and resamples).  y needs
 * 16-byte and y2 8-byte alignment (batch strides included) and they must not overlap
 * (LEA_E_INVALID).  flags: LEA_RELU (and LEA_CVS_TMAJOR, below) only. */
int lea_cv_stem_down2_supported(int cout, int D3, int H, int W, int dtype);
int lea_cv_stem_combine_down2(const void* lmaps, int64_t l_bstride, const void* rmaps, int64_t r_bstride,
                              const float* scale, const float* shift, void* y, int64_t y_bstride,
                              void* y2, int64_t y2_bstride, int B, int cout, int D3, int H, int W,
                              unsigned flags, int dtype, void* stream);

/* The f32 combine kernels read the masked left maps (t = 1, 2) and the K2 maps on a few
 * columns only, so those need not be computed elsewhere:
 *   LEA_CVS_TMAJOR (a flag of lea_cv_stem_combine and lea_cv_stem_combine_down2, LEA_F32):
 *     lmaps in the order (3 t + kd) cout + o -- the three full-width maps first, the six
 *     masked ones after them (rmaps are grouped already: Bk, then K2);
 *   lea_cv_stem_map_windows: the columns read -- left[0..1] = [begin, end) of the masked left
 *     maps, right[0..3] = the two [begin, end) of the K2 maps (derivation: csrc/cv_stem.hip);
 *   lea_conv2d_bnrelu_windowed: lea_conv2d_bnrelu (the direct engine's 2D tiles, no residual)
 *     that computes output channels [0, split) on every column and channels [split, cout) on
 *     the columns of up to two windows [w1_begin, w1_end), [w2_begin, w2_end) (the second
 *     empty when w2_begin >= w2_end; w1_end <= w2_begin), rounded outward to the 16-column
 *     tiles (lea_conv2d_windowed_tiles: tiles[0..3] = the windows in tile columns, as run;
 *     rounded windows that touch are one).  No workgroup exists for the other columns and
 *     nothing is written there.  w_packed: lea_conv2d_pack_weights of weight rows [0, split)
 *     followed by that of rows [split, cout) (only the latter when split = 0).  Where
 *     computed, a value is bit-identical to lea_conv2d_bnrelu's on the same engine. */
#define LEA_CVS_TMAJOR 8u
int lea_cv_stem_map_windows(int D3, int W, int* left, int* right);
int lea_conv2d_windowed_tiles(int W, int w1_begin, int w1_end, int w2_begin, int w2_end, int* tiles);
int lea_conv2d_bnrelu_windowed(const void* x, int64_t x_bstride, const float* w_packed,
                               const float* scale, const float* shift, void* y, int64_t y_bstride,
                               int B, int cin, int cout, int split, int H, int W, int w1_begin,
                               int w1_end, int w2_begin, int w2_end, unsigned flags, int dtype,
                               void* stream);

/* ---- host steps either side of forward ---- */

/* load_data + test_transform of predict.py, fused: replaces predict.py:162-184
 * (per image channel (x - mean) / std over the WHOLE image, np.mean / np.std in
 * float64, population std, stored float32) and predict.py:144-159 (zero-pad
 * top-left when H <= crop_h and W <= crop_w, else centre-crop at
 * start = int((H - crop) / 2); an image that neither fits nor covers the crop is
 * rejected, as the reference's copy into the crop fails).
 *   left/right: B uint8 HWC images [B, H, W, pix_stride] (RGB = 3, RGBA = 4; the
 *               first 3 channels are used, predict.py:170-182)
 *   out_left/out_right: [B, 3, crop_h, crop_w] float32
 *   workspace: lea_standardize_workspace_bytes(B) bytes of device memory (cleared
 *              by the call; holds the exact integer sums).                       */
size_t lea_standardize_workspace_bytes(int B);
int lea_standardize_crop_u8(const void* left, const void* right, int B, int H, int W,
                            int pix_stride, float* out_left, float* out_right, int crop_h,
                            int crop_w, void* workspace, void* stream);

/* set_rgb_layers + train_transform of the training loader, fused: replaces
 * dataloaders/datasets/common.py:119-131 (the standardisation above, whole-image
 * statistics) and :43-91 (pad, random crop, optional left-against-right shift, target
 * cut).  The random draws stay on the host (leastereo_amd/data.py sample_train_params
 * draws them in the reference's order); the call sees only their outcome:
 *   params: device int32 [B][5] = {src_y0, src_x0_left, src_x0_right, target_sub, flags}
 *     out_left[b][c][y][x] and out_target[b][0][y][x] read source pixel
 *       (y + src_y0, x + src_x0_left), out_right (y + src_y0, x + src_x0_right);
 *     a source pixel outside [0,H) x [0,W) is pad: 0 in the image planes, 1000 in the
 *     left disparity, 0 in the right disparity;
 *     out_target = source - (float)target_sub, one float32 subtraction, pad included;
 *     flags bit 0 = swap: out_left is cut from the right image, out_right from the left
 *     image, the target from disp_right (all pad when disp_right is NULL); other bits
 *     are ignored.
 *     With the reference's canvas Hc x Wc (image at its bottom-right, py = Hc - H,
 *     px = Wc - W): src_y0 = start_y - py, src_x0_left = start_x + shift_x - px,
 *     src_x0_right = start_x - px, target_sub = shift_x.
 *     The rows are not validated (they live in device memory so that a captured graph
 *     replays with fresh crops): coordinates are formed in 64 bits and bounds-tested
 *     before every read, so any five ints are memory-safe and give pad.
 *   left/right: B uint8 HWC images [B, H, W, pix_stride] (3 or 4)
 *   disp_left, disp_right: [B, H, W] float32; disp_right may be NULL
 *   out_left/out_right: [B, 3, crop_h, crop_w], out_target: [B, 1, crop_h, crop_w] float32
 *     (16-byte aligned when crop_w % 4 == 0)
 *   n_valid: optional device int32 [B], cleared by the call: the count of target pixels
 *     with t < maxdisp && t > 0.001f (train.py:116-118), float32 compares
 *   workspace: lea_train_transform_workspace_bytes(B) bytes, cleared by the call.
 * The statistics launch and the crop launch, behind a one-workgroup launch that clears
 * the workspace and n_valid (kernels only: a captured call holds no memset node); all
 * on `stream`, no host sync.                                                          */
size_t lea_train_transform_workspace_bytes(int B);
int lea_train_transform_u8(const void* left, const void* right, int B, int H, int W, int pix_stride,
                           const float* disp_left, const float* disp_right, const int* params,
                           float* out_left, float* out_right, float* out_target, int crop_h,
                           int crop_w, float maxdisp, int* n_valid, void* workspace, void* stream);

/* ---- whole-scene inference: overlapping tiles gathered and blended (not in the reference) ---- */

/* The gather: one pair of decoded scenes cut into N tiles, each standardised as
 * lea_standardize_crop_u8 standardises (the same exact sums, the same float64 -> float32
 * store) with the statistics of the WHOLE scene, as the reference standardises before it
 * crops.
 *   left/right: uint8 HWC scenes [H, W, pix_stride] (3 or 4)
 *   origins: device int32 [N][2] = {y, x}; tile k's pixel (y, x) reads scene pixel
 *     (y + origins[k][0], x + origins[k][1]) and is 0 where that lies outside the scene.
 *     The rows are not validated: coordinates are formed in 64 bits and bounds-tested
 *     before every read, so any N pairs of ints are memory-safe (a tile wholly outside the
 *     scene is all 0).
 *   out_left/out_right: [N, 3, tile_h, tile_w] float32 (16-byte aligned when tile_w % 4 == 0)
 *   workspace: lea_standardize_tiles_workspace_bytes() bytes, cleared by the call.
 * A clearing launch, the statistics launch and the tile launch (kernels only: a captured
 * call holds no memset node); all on `stream`, no host sync.  N in 1..65535.            */
size_t lea_standardize_tiles_workspace_bytes(void);
int lea_standardize_tiles_u8(const void* left, const void* right, int H, int W, int pix_stride,
                             const int* origins, int N, float* out_left, float* out_right, int tile_h,
                             int tile_w, void* workspace, void* stream);

/* The blend: the ny * nx per-tile maps of a separable plan (tile k = ky * nx + kx at origin
 * (ys[ky], xs[kx]), both in device memory, ny, nx <= 64) gathered into out [H, W].
 * Per axis (scene length S, tile length L, origin o, low / high guard g0 / g1) tile
 * coordinate i weighs
 *   lo = o > 0, hi = o + L < S, a = lo ? g0 : 0, b = hi ? g1 : 0
 *   w = 0 for i < a or i >= L - b, else min(lo ? i - a + 1 : ramp, hi ? (L - b) - i : ramp, ramp)
 * and a pixel's weight in a tile is the integer product wy * wx.  Over the tiles of positive
 * weight in ascending k: one tile -> its value copied; several -> (sum w * v) / (sum w) in
 * float32, each product, add and the divide rounded once; none -> 0.  A tile is never read
 * where its weight is 0.  The origins are not validated (any ints are memory-safe).
 *   tiles: [ny * nx, tile_h, tile_w] float32, tile_bstride elements from tile to tile
 *   guard_*: >= 0 (left-view maps: x guards (maxdisp + context, context); the right view's
 *     disparity: (context, maxdisp + context)); ramp: 1..256
 *   out: [H, W] float32 (16-byte aligned when W % 4 == 0), not aliasing tiles
 *   n_uncovered: optional device int32, cleared by the call (a launch): the number of
 *     pixels no tile covers.
 * One launch (two with n_uncovered) on `stream`, no host sync, no float atomics:
 * bit-reproducible.                                                                    */
int lea_tile_blend_f32(const float* tiles, int64_t tile_bstride, const int* ys, int ny, const int* xs,
                       int nx, int tile_h, int tile_w, int guard_y0, int guard_y1, int guard_x0,
                       int guard_x1, int ramp, float* out, int H, int W, int* n_uncovered, void* stream);

/* Disparity metrics of one batch, per pair b (device out[b][8], float64):
 *   [0] n    of evaluation.py:287 mask (gt >= 0.001 & gt <= maxdisp)
 *   [1] sum |pred - gt| over that mask          (EPE = [1] / [0], evaluation.py:288)
 *   [2] n    of utils/metrics.py:6-8 validity (gt > 0.001 & gt < maxdisp)
 *   [3] n correct, utils/metrics.py:16-19        (3-px error = 1 - [3] / [2])
 *   [4..6] n with abs_diff <= thr1..thr3, :41-43 (bad-thr = 1 - [4+i] / [2])
 * abs_diff follows the reference's int64 array: |gt - pred| truncated toward zero
 * on valid pixels, 10000 elsewhere.  round_pred applies evaluation.py:169
 * (pred.round() + z_shift, half-to-even) first.  correct (optional, [B, H*W]
 * uint8) receives the 3-px correct mask of calculate_3px_error_and_correct_mask.
 * pred/gt: [B, H, W] float32 with batch strides in elements.
 * workspace: lea_disparity_metrics_workspace_bytes(B, H, W) bytes.               */
size_t lea_disparity_metrics_workspace_bytes(int B, int H, int W);
int lea_disparity_metrics(const float* pred, int64_t pred_bstride, const float* gt,
                          int64_t gt_bstride, int B, int H, int W, float maxdisp, int round_pred,
                          int z_shift, int thr1, int thr2, int thr3, unsigned char* correct,
                          double* out, void* workspace, void* stream);

/* ---- training backward of ConvBR3d (operations_3d.py:31-47
 * as train.py:130-178 runs it: BatchNorm3d in train mode) ----
 * All tensors NCDHW contiguous fp32, V = D*H*W.  Composition (csrc/conv3d_grad.hip):
 *   forward  z = lea_conv3d_bnrelu(x, w; no scale/shift, flags 0)
 *            y = lea_bn_forward_f32(z)
 *   backward dz = lea_bn_backward_f32(dy, y, z)
 *            dx = lea_conv3d_bnrelu(dz, pack(lea_conv3d_flip_weights(w)); flags 0)
 *            dw = lea_conv3d_wgrad(x, dz)                                        */

/* dw[co][ci][kd][kh][kw] = sum_{b,d,h,w} dz[b][co][d][h][w] * x[b][ci][d+kd-k/2][h+kh-k/2][w+kw-k/2]
 * (zero padding; the weight gradient of a stride-1, pad k/2 Conv3d without bias,
 * which torch computes in aten's convolution_backward).  dw is overwritten;
 * workspace: lea_conv3d_wgrad_workspace_bytes(...) bytes (per-wave partials, summed
 * in a fixed order: the result is deterministic).  k in {1, 3}.                  */
size_t lea_conv3d_wgrad_workspace_bytes(int B, int cin, int cout, int D, int H, int W, int k);
int lea_conv3d_wgrad(const float* x, const float* dz, float* dw, void* workspace, size_t ws_bytes,
                     int B, int cin, int cout, int D, int H, int W, int k, void* stream);

/* The feature net's Conv2d 3x3 / stride 1 / pad 1 (operations_2d.py:31-47, the cells and
 * stem0/stem2 of new_model_2d.py:93-95): dw[co][ci][kh][kw] = sum_{b,h,w} dz[b][co][h][w] *
 * x[b][ci][h+kh-1][w+kw-1], the same deterministic MFMA reduction as lea_conv3d_wgrad.
 * x: [B, cin, H, W], dz: [B, cout, H, W], dw: [cout, cin, 3, 3].  The input gradient is
 * lea_conv2d_bnrelu of dz with w flipped along (kh, kw) and transposed to [cin, cout, 3, 3]. */
size_t lea_conv2d_wgrad_workspace_bytes(int B, int cin, int cout, int H, int W);
int lea_conv2d_wgrad(const float* x, const float* dz, float* dw, void* workspace, size_t ws_bytes,
                     int B, int cin, int cout, int H, int W, void* stream);

/* Backward of lea_conv2d_s3_bnrelu's convolution (stem1, new_model_2d.py:94; stride 3,
 * pad 1, 3x3: every input pixel is read by at most one output tap), w: [cout, cin, 3, 3]:
 *   dx[b][ci][y][x] = sum_co w[co][ci][(y+1)%3][(x+1)%3] * dz[b][co][(y+1)/3][(x+1)/3]
 *   (0 where (y+1)/3 = Ho or (x+1)/3 = Wo: the last row / column when Hi / Wi % 3 == 0)
 *   dw[co][ci][kh][kw] = sum_{b,oy,ox} dz[b][co][oy][ox] * x[b][ci][3oy+kh-1][3ox+kw-1]
 * x/dx: [B, cin, Hi, Wi]; dz: [B, cout, (Hi-1)/3+1, (Wi-1)/3+1]; contiguous fp32.
 * workspace: lea_conv2d_s3_wgrad_workspace_bytes(...) bytes (per-slice partials, summed
 * in a fixed order). */
int lea_conv2d_s3_backward_data(const float* dz, const float* w, float* dx, int B, int cin, int cout,
                                int Hi, int Wi, void* stream);
size_t lea_conv2d_s3_wgrad_workspace_bytes(int B, int cin, int cout, int Hi, int Wi);
int lea_conv2d_s3_wgrad(const float* x, const float* dz, float* dw, void* workspace, size_t ws_bytes,
                        int B, int cin, int cout, int Hi, int Wi, void* stream);

/* wt[ci][co][kd][kh][kw] = w[co][ci][k-1-kd][k-1-kh][k-1-kw]: the input gradient of a
 * stride-1, pad k/2 conv is the forward conv of dz with this weight.             */
int lea_conv3d_flip_weights(const float* w, float* wt, int cout, int cin, int k, void* stream);

/* BatchNorm3d + optional ReLU (flags LEA_RELU), operations_3d.py:44-46 in
 * torch.nn.BatchNorm3d's semantics: training = 1 normalises by the batch mean and
 * biased variance over (B, D, H, W) and updates running_mean / running_var with
 * momentum (unbiased variance; both may be NULL to skip the update); training = 0
 * uses the running stats.  gamma/beta NULL = 1/0.  y = relu((z - mean) * invstd *
 * gamma + beta); mean/invstd ([C], device) are written for the backward.
 * workspace: lea_bn_workspace_bytes(C) bytes (train mode).                      */
size_t lea_bn_workspace_bytes(int C);
int lea_bn_forward_f32(const float* z, float* y, int B, int C, int64_t V, const float* gamma,
                       const float* beta, float* running_mean, float* running_var, float momentum,
                       float eps, int training, unsigned flags, float* mean, float* invstd,
                       void* workspace, void* stream);

/* Backward of lea_bn_forward_f32: g = dy * [y > 0] (LEA_RELU) or dy;
 * dbeta = sum g, dgamma = sum g * xhat (xhat = (z - mean) * invstd, either may be NULL);
 * dz = gamma * invstd * (g - dbeta/N - xhat * dgamma/N) in train mode,
 * gamma * invstd * g in eval mode (N = B * V).  workspace: lea_bn_workspace_bytes(C). */
int lea_bn_backward_f32(const float* dy, const float* y, const float* z, float* dz, int B, int C,
                        int64_t V, const float* gamma, const float* mean, const float* invstd,
                        int training, unsigned flags, float* dgamma, float* dbeta, void* workspace,
                        void* stream);

/* Backward of lea_resample3d_trilinear without epilogue (F.interpolate trilinear,
 * skip_model_3d.py:48,50,162, align_corners 1; build_model_2d.py:53, 0):
 * dx[b][c] = interp^T(dy[b][c]), as three deterministic 1-D transposed passes with
 * the forward's source-index rule.  dy: [B, C, Do, Ho, Wo], dx: [B, C, Di, Hi, Wi],
 * contiguous; workspace: lea_resample3d_backward_workspace_bytes(...) bytes.     */
size_t lea_resample3d_backward_workspace_bytes(int B, int C, int Di, int Hi, int Wi, int Do, int Ho,
                                               int Wo);
int lea_resample3d_trilinear_backward(const float* dy, float* dx, void* workspace, size_t ws_bytes,
                                      int B, int C, int Di, int Hi, int Wi, int Do, int Ho, int Wo,
                                      int align_corners, void* stream);

/* Backward of lea_disparity_regression (build_model_2d.py:33-42,52-57): with
 * U = trilinear(cost, [maxdisp, 3H3, 3W3], align_corners=False), p = softmax(-U, d),
 * disp = sum_d d p_d (disp: the forward's output),
 *   dU[b, d, h, w] = -dout[b, h, w] * p_d * (d - disp[b, h, w]),
 * and writes dV = its transpose along D only (the depth lerp's two taps per d summed
 * onto the D3 cost planes): [B, D3, 3H3, 3W3].  dcost = the H/W part,
 * lea_resample3d_trilinear_backward(dV, [D3, H3, W3] <- [D3, 3H3, 3W3], align_corners = 0). */
int lea_disparity_regression_backward(const float* cost, const float* disp, const float* dout,
                                      float* dV, int B, int D3, int H3, int W3, int maxdisp,
                                      void* stream);

/* Backward of lea_build_cost_volume (retrain/LEAStereo.py:34-48):
 *   dleft[b,c,h,w]  = sum_{i <= w} dcost[b, c, i, h, w]
 *   dright[b,c,h,w] = sum_{i < W - w} dcost[b, C + c, i, h, w + i]
 * dcost: [B, 2C, D3, H, W]; dleft/dright: [B, C, H, W]; fp32.                    */
int lea_build_cost_volume_backward(const float* dcost, float* dleft, float* dright, int B, int C,
                                   int H, int W, int D3, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LEASTEREO_HIP_H */
