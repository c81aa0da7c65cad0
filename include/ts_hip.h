/*
 * ts_hip.h -- C ABI of libts_hip.so: the MI355X (gfx950) cost-volume stereo hot path.
 *
 * Drop-in boundary for the hot path of youmi-zym/TemporalStereo.
 * Every entry point replaces one python-level function of the reference; the reference
 * file:line is cited on each declaration.  The reference-side binding a maintainer would add
 * (a ctypes stub inside architecture/modeling/...) is shown in INTEGRATION.md.
 *
 * Conventions
 *   - all tensors are dense fp32, NCHW / NCDHW contiguous, device pointers owned by the caller;
 *     the library never allocates, frees or retains a pointer and never synchronises.
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).
 *   - return value: 0 = ok; negative = argument error (TS_ERR_*); positive = hipError_t of the
 *     failed launch.  ts_last_error_string() describes the last failure on the calling thread.
 *   - kernels needing scratch take `workspace` + a ts_*_workspace_bytes() query; 256-byte aligned.
 *   - re-entrant: no global mutable state besides the thread-local error string.
 */
#ifndef TS_HIP_H
#define TS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TS_OK 0
#define TS_ERR_NULL (-1)         /* a required pointer is NULL                         */
#define TS_ERR_SHAPE (-2)        /* sizes inconsistent / non-positive                  */
#define TS_ERR_UNSUPPORTED (-3)  /* valid for the reference but outside this build     */
#define TS_ERR_ALIGN (-4)        /* pointer not 16-byte aligned                        */

int ts_version(void);                     /* ABI version, bumps on any signature change */
const char* ts_last_error_string(void);   /* thread-local, never NULL                   */

/* ------------------------------------------------------------------------------------------
 * K1  cost-volume construction.
 * Replaces block_cost()  architecture/modeling/aggregation/utils/block_cost.py:16-83
 *   (+ groupwise_correlation :6-13, inverse_warp_3d  layers/inverse_warp_3d.py:4-58).
 * left,right [B,C,H,W]; C % 8 == 0; H,W >= 4; 1 <= scales <= 3.
 *   int path      (:34-45): out [B, C  + scales*C/8, D, H, W]
 *   sampled path  (:47-58): out [B, 2C + scales*C/8, D, H, W], disp [B,D,H,W], D >= 2
 * ---------------------------------------------------------------------------------------- */
size_t ts_block_cost_workspace_bytes(int B, int C, int H, int W, int D, int scales);

int ts_block_cost_int_fwd(const float* left, const float* right, float* out, void* workspace,
                          int B, int C, int H, int W, int D, int scales, void* stream);

int ts_block_cost_sampled_fwd(const float* left, const float* right, const float* disp, float* out,
                              void* workspace, int B, int C, int H, int W, int D, int scales,
                              void* stream);

/* Inference form of the sampled path: the first C channels of its output are `left` repeated D times
 * (block_cost.py:51), and the layer that consumes the volume is a (1,3,3) convolution, so
 *   conv(volume) = conv_{W[:, :C]}(left) broadcast over D  +  conv_{W[:, C:]}(volume[:, C:]).
 * This entry writes only volume[:, C:]  ->  out [B, C + scales*C/8, D, H, W]  (warped half, then the
 * correlation blocks); ts_conv3d_hw_fwd takes the left term as its `addend`. */
int ts_block_cost_sampled_warped_fwd(const float* left, const float* right, const float* disp, float* out,
                                     void* workspace, int B, int C, int H, int W, int D, int scales,
                                     void* stream);

/* Correlation blocks only (ABI 6): out [B, scales*C/8, D, H, W] = channels [2C:] of ts_block_cost_sampled_fwd.  The consumer is
 * ts_conv3d_hw_warp_fwd, which needs neither half of the 2C main channels as a volume. */
int ts_block_cost_sampled_corr_fwd(const float* left, const float* right, const float* disp, float* out,
                                   void* workspace, int B, int C, int H, int W, int D, int scales,
                                   void* stream);

/* Split-input forms: an input whose channels [0, Csplit) live in one allocation and [Csplit, C) in another is read in place
 * instead of being concatenated first.  Each base has its own batch stride (and, for the convolutions, channel stride) in elements
 * and is addressed through a buffer descriptor of its own extent.  Same kernels, same chunk order, same arithmetic: the results are
 * bit-identical to the plain entry on the concatenation.  Csplit must be a multiple of 32 (the widest K chunk a kernel stages, so no
 * chunk straddles the seam) with 0 < Csplit < C; anything else is TS_ERR_UNSUPPORTED, and the *_split_supported queries answer
 * beforehand (1 = the split entry takes the shape).
 *   ts_block_cost_sampled_corr_split_fwd  ts_block_cost_sampled_corr_fwd with left = [left | left2], right = [right | right2];
 *                                         planes are dense ([B][.][H][W]), the four batch strides are free
 *   ts_conv3d_hw_split_fwd                ts_conv3d_hw_fwd, not the transposed form; a split-K launch needs slices of whole
 *                                         32-channel chunks (ts_conv3d_hw_split_supported assumes the workspace is handed over)
 *   ts_conv3d_d_split_fwd                 ts_conv3d_d_fwd
 *   ts_conv3d_hw_x6_split_fwd             ts_conv3d_hw_x6_fwd (either of its kernels) */
int ts_block_cost_corr_split_supported(int C, int Csplit);
int ts_block_cost_sampled_corr_split_fwd(const float* left, const float* left2, const float* right, const float* right2,
                                         const float* disp, float* out, void* workspace, int B, int C, int Csplit, int H, int W,
                                         int D, int scales, long long left_bstride, long long left2_bstride,
                                         long long right_bstride, long long right2_bstride, void* stream);
int ts_conv3d_hw_split_supported(int B, int Cin, int Csplit, int Cout, int D, int H, int W, int stride, int dilation,
                                 int transposed);
int ts_conv3d_hw_split_fwd(const float* x, const float* x2, const float* w_t, const float* scale, const float* shift, float* y,
                           int B, int Cin, int Csplit, int Cout, int D, int H, int W, int stride, int dilation,
                           int transposed, int act, float act_param,
                           long long in_bstride, long long in_cstride, long long in2_bstride, long long in2_cstride,
                           long long out_bstride, long long out_cstride, const float* addend, long long addend_bstride,
                           void* workspace, size_t workspace_bytes, void* stream);
int ts_conv3d_d_split_supported(int Cin, int Csplit);
int ts_conv3d_d_split_fwd(const float* x, const float* x2, const float* w_t, const float* scale, const float* shift, float* y,
                          int B, int Cin, int Csplit, int Cout, int Din, int H, int W, int k, int stride, int dilation,
                          int padding, int transposed, int act, float act_param,
                          long long in_bstride, long long in_cstride, long long in2_bstride, long long in2_cstride,
                          long long out_bstride, long long out_cstride, void* stream);
int ts_conv3d_hw_x6_split_supported(int Cin, int Csplit, int Cout, int W, int dilation);
int ts_conv3d_hw_x6_split_fwd(const float* x, const float* x2, const void* w6, const float* scale, const float* shift, float* y,
                              int B, int Cin, int Csplit, int Cout, int D, int H, int W, int dilation, int act, float act_param,
                              long long in_bstride, long long in_cstride, long long in2_bstride, long long in2_cstride,
                              long long out_bstride, long long out_cstride, const float* addend, long long addend_bstride,
                              void* workspace, size_t workspace_bytes, void* stream);

/* Dense siblings of block_cost (forward only): any number of candidates D >= 2, C % 8 == 0.
 *   cat_fms  aggregation/utils/cat_fms.py:5-36   out [B,2C,D,H,W] = cat[left repeated over D, warped right]
 *   dif_fms  aggregation/utils/dif_fms.py:5-44   out [B, C,D,H,W] = |left - warped right|, elements whose warped
 *            value is not > 0 replaced by the maximum difference over the whole tensor (workspace: 256 bytes) */
int ts_cat_fms_fwd(const float* left, const float* right, const float* disp, float* out, int B, int C, int H, int W, int D,
                   void* stream);
/* inverse_warp_3d(img, disp, padding_mode='zeros', disp_Y=None)  layers/inverse_warp_3d.py:4-58, the function-level seam itself
 * (block_cost / cat_fms / dif_fms call it with -disp): img [B,C,H,W] (C % 8 == 0), disp [B,D,H,W], D >= 2, H, W >= 2 ->
 * out [B,C,D,H,W][b,c,d,y,x] = img[b,c,y, x + disp[b,d,y,x]] linearly interpolated, zeros outside [0, W-1].  The wrapper
 * (temporalstereo_amd.inverse_warp_3d) serves 5-D images, other channel counts and the gradients (ts_block_cost_sampled_bwd). */
int ts_inverse_warp_3d_fwd(const float* img, const float* disp, float* out, int B, int C, int H, int W, int D, void* stream);
size_t ts_dif_fms_workspace_bytes(void);
int ts_dif_fms_fwd(const float* left, const float* right, const float* disp, float* out, void* workspace, int B, int C,
                   int H, int W, int D, void* stream);

/* Correlation volumes, the native counterpart of the third-party SpatialCorrelationSampler the
 * reference imports optionally (aggregation/utils/correlation.py:4-7; unvendored and unpinned, so parity is pinned by the
 * sampler's published definition -- sum over channels, zeros outside the image -- through oracle/correlation.py):
 *   out[b, k, y, x] = leaky_relu_0.1( sum_c left[b,c,y,x] * right[b,c, y + k/pW - pH/2, x + k%pW - pW/2] ),  k < keep
 *   correlation   (correlation.py:10-29): patch (p, p), keep = p*p
 *   correlation1d (correlation.py:32-57): patch (1, 2*max_disp-1), keep = max_disp  (plane k = disparity max_disp-1-k)
 * Backward OVERWRITES grad_left / grad_right [B,C,H,W] (either may be NULL); deterministic. */
int ts_correlation_fwd(const float* left, const float* right, float* out, int B, int C, int H, int W, int patch_h, int patch_w,
                       int keep, void* stream);
int ts_correlation_bwd(const float* left, const float* right, const float* out, const float* grad_out, float* grad_left,
                       float* grad_right, int B, int C, int H, int W, int patch_h, int patch_w, int keep, void* stream);

/* Backward of the two paths (autograd of the reference's torch ops).  grad_out has the layout
 * of `out`.  grad_left/grad_right [B,C,H,W] and grad_disp [B,D,H,W] are OVERWRITTEN (any may be
 * NULL to skip).  grad_right / grad_disp accumulate with fp32 atomics (order not deterministic,
 * as in the reference's grid_sampler backward). */
size_t ts_block_cost_bwd_workspace_bytes(int B, int C, int H, int W, int D, int scales);

int ts_block_cost_int_bwd(const float* left, const float* right, const float* grad_out,
                          float* grad_left, float* grad_right, void* workspace,
                          int B, int C, int H, int W, int D, int scales, void* stream);

int ts_block_cost_sampled_bwd(const float* left, const float* right, const float* disp,
                              const float* grad_out, float* grad_left, float* grad_right,
                              float* grad_disp, void* workspace,
                              int B, int C, int H, int W, int D, int scales, void* stream);
/* ... of ts_block_cost_sampled_warped_fwd (ABI 9): grad_out [B, C + scales*C/8, D, H, W], the volume without its reference half */
int ts_block_cost_sampled_warped_bwd(const float* left, const float* right, const float* disp,
                                     const float* grad_out, float* grad_left, float* grad_right,
                                     float* grad_disp, void* workspace,
                                     int B, int C, int H, int W, int D, int scales, void* stream);

/* ------------------------------------------------------------------------------------------
 * BatchNorm (+ activation) of the convolution wrappers in TRAIN mode (layers/basic_layers.py:194-235: conv -> norm ->
 * activation).  x / out / dy / dx are [B,C,N] with N = D*H*W contiguous and explicit batch / channel strides (elements).
 *   ts_bn_stats_fwd       mean[C], var[C] (biased) of x over (B,N); deterministic.  running_mean / running_var (may be NULL) are
 *                         updated with `momentum` (running_var with the unbiased estimate, as nn.BatchNorm);
 *                         *num_batches_tracked (device int64, may be NULL) is incremented in the same launch
 *   ts_bn_apply_act_fwd   out = act((x - mean) * rsqrt(var + eps) * gamma + beta);  act 0 none | 1 SiLU | 2 ReLU
 *   ts_bn_act_bwd_reduce  sum_dz[C] = sum dz, sum_dz_xhat[C] = sum dz * xhat with dz = dy * act'(z)  (= grad beta, grad gamma)
 *   ts_bn_act_bwd_apply   train: dx = (dz - sum_dz/count - xhat * sum_dz_xhat/count) * invstd * gamma; eval: dx = dz * invstd * gamma
 * mean / var / the two sums are arguments so that cross-rank statistics (SyncBatchNorm) can be exchanged in between.
 * ---------------------------------------------------------------------------------------- */
size_t ts_bn_workspace_bytes(int B, int C, long long N);
/* SyncBatchNorm merge: gathered = the ranks' [mean(C) | biased var(C) | count] records of ts_bn_stats_fwd (world x (2C+1) floats, one
 * all_gather) -> statistics of the whole batch (parallel-variance formula, double), running statistics updated with momentum
 * (NULL: not tracked), *inv_count = 1 / total count on the device (the backward sums are scaled with it: no host read). */
int ts_bn_sync_merge(const float* gathered, int world, int C, float* mean, float* var, float* running_mean,
                     float* running_var, float momentum, float* inv_count, void* stream);
/* Single-rank training forms (nothing to exchange between the statistics and their use): statistics + normalise/activate in two
 * launches, backward sums + input gradient in two (each a partial-sums kernel, then one whose workgroups finish their channel's
 * sums themselves in the fixed order of the three-launch forms -- same values).  ts_bn_train_bwd: count = B*N elements.
 * ABI 9: channels of at most ts_bn_set_small_elems() elements (B*N; default below, TS_BN_SMALL_ELEMS) take ONE launch each way -- a
 * workgroup per channel does both passes (per-thread fp32 partial sums combined in double: the same statistics to rounding). */
long long ts_bn_set_small_elems(long long n);   /* returns the previous bound; n < 0 only queries */
/* out[c] = sum over batch and pixels of x [B,C,N] (a convolution's bias gradient), deterministic; workspace: ts_bn_workspace_bytes(B, C, N) */
int ts_channel_sum_fwd(const float* x, float* out, void* workspace, int B, int C, long long N, long long bstride, long long cstride,
                       void* stream);
int ts_bn_train_fwd(const float* x, float* mean, float* var, float* running_mean, float* running_var, float momentum,
                    long long* num_batches_tracked, const float* gamma, const float* beta, float* out, void* workspace,
                    int B, int C, long long N, long long x_bstride, long long x_cstride, long long out_bstride,
                    long long out_cstride, float eps, int act, void* stream);
int ts_bn_train_bwd(const float* x, const float* dy, const float* mean, const float* var, const float* gamma, const float* beta,
                    float* sum_dz, float* sum_dz_xhat, float* dx, void* workspace, int B, int C, long long N,
                    long long x_bstride, long long x_cstride, long long dy_bstride, long long dy_cstride, float eps, int act,
                    float count, void* stream);
int ts_bn_stats_fwd(const float* x, float* mean, float* var, float* running_mean, float* running_var, float momentum,
                    long long* num_batches_tracked, void* workspace, int B, int C, long long N, long long bstride,
                    long long cstride, void* stream);
int ts_bn_apply_act_fwd(const float* x, const float* mean, const float* var, const float* gamma, const float* beta, float* out,
                        int B, int C, long long N, long long x_bstride, long long x_cstride, long long out_bstride,
                        long long out_cstride, float eps, int act, void* stream);
int ts_bn_act_bwd_reduce(const float* x, const float* dy, const float* mean, const float* var, const float* gamma,
                         const float* beta, float* sum_dz, float* sum_dz_xhat, void* workspace, int B, int C, long long N,
                         long long x_bstride, long long x_cstride, long long dy_bstride, long long dy_cstride, float eps, int act,
                         void* stream);
int ts_bn_act_bwd_apply(const float* x, const float* dy, const float* mean, const float* var, const float* gamma,
                        const float* beta, const float* sum_dz, const float* sum_dz_xhat, float* dx, int B, int C, long long N,
                        long long x_bstride, long long x_cstride, long long dy_bstride, long long dy_cstride, float eps, int act,
                        int train, float count, void* stream);

/* ------------------------------------------------------------------------------------------
 * Loss side of the path's outputs.
 * ts_wasserstein_loss_*: WarssersteinDistanceLoss.loss_per_level  architecture/modeling/losses/warsserstein_distance_loss.py:52-78
 *   cost/offset/sample [B,D,H,W], gt [B,1,Hg,Wg] (full resolution; pooled to (H,W) after / (Wg/W): avg, or max when `sparse`).
 *   loss[0] = mean_{b,y,x} sum_d (softmax_d(cost)+0.25) |offset+sample-gt'| [start < gt' < max_disp/scale]; gt_scaled [B,H,W] is
 *   kept for the backward, which OVERWRITES grad_cost and grad_offset (== grad of sample); either may be NULL.
 * ts_disp_smooth_l1_*: DispSmoothL1Loss.loss_per_level (losses/smooth_l1_loss.py:49-76) of the disparity est [B,1,h,w] after the
 *   wrapper's rescale to the ground truth's size, F.interpolate(est * Wg / w, (Hg,Wg), bilinear, align_corners)
 *   (projects/TemporalStereo/TemporalStereo.py:305-309), evaluated in registers; (h,w) == (Hg,Wg) is the plain loss.
 *   loss_count[0] = mean smooth-L1 over the valid pixels (0 if none), loss_count[1] = their number (the backward reads it).
 * grad_loss: one float on the device (d objective / d loss).  Deterministic (fixed-order reductions, gather adjoint).
 * ---------------------------------------------------------------------------------------- */
size_t ts_wasserstein_loss_workspace_bytes(int B, int H, int W);
int ts_wasserstein_loss_fwd(const float* cost, const float* offset, const float* sample, const float* gt, float* loss,
                            float* gt_scaled, void* workspace, int B, int D, int H, int W, int Hg, int Wg, float max_disp,
                            float start_disp, int sparse, void* stream);
int ts_wasserstein_loss_bwd(const float* cost, const float* offset, const float* sample, const float* gt_scaled,
                            const float* grad_loss, float* grad_cost, float* grad_offset, int B, int D, int H, int W, int Wg,
                            float max_disp, float start_disp, void* stream);
size_t ts_disp_smooth_l1_workspace_bytes(int B, int Hg, int Wg);
int ts_disp_smooth_l1_fwd(const float* est, const float* gt, float* loss_count, void* workspace, int B, int h, int w, int Hg,
                          int Wg, float max_disp, float start_disp, void* stream);
int ts_disp_smooth_l1_bwd(const float* est, const float* gt, const float* grad_loss, const float* loss_count, float* grad_est,
                          int B, int h, int w, int Hg, int Wg, float max_disp, float start_disp, void* stream);

/* ------------------------------------------------------------------------------------------
 * Evaluation of the returned disparities (validation_step / test_step, projects/TemporalStereo/TemporalStereo.py:170-214).
 * ts_disp_metrics_fwd: log_metric (:463-486) of up to four levels in one call -- calc_error (data/evaluation/pixel_error.py:6-71)
 *   of each level and, when gt_right is given, do_occlusion_evaluation (data/evaluation/eval.py:45-105).
 *   est<l> [B,1,h<l>,w<l>] (n_est = 1..4; unused pointers may be NULL); a level smaller or larger than the ground truth is read
 *   through F.interpolate(est * Wg / w, (Hg,Wg), bilinear, align_corners) (:183) evaluated in registers.
 *   gt / gt_right [B,1,Hg,Wg]; gt_right NULL: only the `all` split (occ / noc written as 0); else Hg, Wg >= 2.
 *   flags bit0: lb given (valid needs gt > lb), bit1: ub given (gt < ub).
 *   out [n_est][3][5] fp32: split all / occ / noc x {1px, 2px, 3px, 5px, epe} (percent; 0 when no pixel is valid).
 *   Counts are exact integers, sums fp64 in a fixed order: bit-identical from run to run.  Two launches, no synchronisation.
 * ---------------------------------------------------------------------------------------- */
size_t ts_disp_metrics_workspace_bytes(int B, int Hg, int Wg);
int ts_disp_metrics_fwd(const float* est0, const float* est1, const float* est2, const float* est3, int n_est, int h0, int w0,
                        int h1, int w1, int h2, int w2, int h3, int w3, const float* gt, const float* gt_right, int B, int Hg,
                        int Wg, float lb, float ub, int flags, float* out, void* workspace, void* stream);

/* ------------------------------------------------------------------------------------------
 * Rendering of a frame's disparities (projects/TemporalStereo/video_inference.py:169-227 `visualize`, TemporalStereo.py:488-622
 * `log_image`; architecture/utils/visualization/disparity_colormap.py): colour maps and the 16-bit map, ready for one copy to the host.
 * ts_disp_render_fwd: est [B,1,h,w] is read at the size of the target (Hg,Wg) through F.interpolate(est * Wg / w, (Hg,Wg), bilinear,
 *   align_corners) (video_inference.py:182) evaluated in registers ((h,w) == (Hg,Wg): read as it is); gt [B,1,Hg,Wg] (NULL when no
 *   selected output needs it).  flags selects the outputs and their form:
 *     TS_RENDER_EST_COLOR / TS_RENDER_GT_COLOR  disp_to_color (:69-98) of est / gt into disp_color: [B,Hg,Wg,3], or with both set
 *                            [B,2Hg,Wg,3], est above gt.  The maximum is each map's own (np.max, per image), the one of both maps
 *                            with TS_RENDER_MAX_SHARED (video_inference.py:201-202), or max_disp[b] with TS_RENDER_MAX_GIVEN.
 *                            TS_RENDER_CLIP clamps the colours to [0,1] (the reference's callers do; disp_map itself extrapolates).
 *     TS_RENDER_ERR_CLASS    disp_err_to_color (:102-170) into err_class [B,Hg,Wg,3]
 *     TS_RENDER_ERR_JET      disp_err_to_colorbar (:172-219) into err_jet [B,Hg,Wg,3]; with TS_RENDER_BAR [B,Hg+50,Wg,3], the legend
 *                            below.  jet: the 256 x 3 fp32 table of the colour map (device pointer).
 *     TS_RENDER_U16          (est * scale16) truncated toward zero into disp_u16 [B,Hg,Wg] uint16, saturated to [0,65535], NaN -> 0
 *                            (video_inference.py:220)
 *     TS_RENDER_UINT8        colour outputs are uint8, floor(255 v + 0.5) after a clamp to [0,1], NaN -> 0; else fp32
 *     TS_RENDER_CHW          colour outputs are [B,3,rows,Wg] instead of [B,rows,Wg,3]
 *   stats [B][TS_RENDER_STATS_FLOATS] (written when a maximum is taken from the data or the jet map is selected; needs workspace):
 *     [0] max est  [1] max gt  [2] max of both  [3] max err, err = |est - gt| * (gt > 0)  [4] max(192, max err), 192 for a NaN
 *     [8..13] / [16..21] minimum / maximum of err inside (0,1] (1,2] (2,4] (4,12] (12,16] (16,[4]]  (+inf / -inf: no member)
 *     [24..29] the members' counts, int32 bit patterns.  Maxima propagate a NaN as np.max does.
 *   Two launches (statistics + finish) are skipped when stats is not needed; then the colour launch.  No atomics, no
 *   synchronisation; bit-identical from run to run.
 * ---------------------------------------------------------------------------------------- */
#define TS_RENDER_EST_COLOR 1
#define TS_RENDER_GT_COLOR 2
#define TS_RENDER_ERR_CLASS 4
#define TS_RENDER_ERR_JET 8
#define TS_RENDER_U16 16
#define TS_RENDER_UINT8 32
#define TS_RENDER_CHW 64
#define TS_RENDER_BAR 128
#define TS_RENDER_CLIP 256
#define TS_RENDER_MAX_SHARED 512
#define TS_RENDER_MAX_GIVEN 1024
#define TS_RENDER_STATS_FLOATS 32
size_t ts_disp_render_workspace_bytes(int B, int Hg, int Wg);
int ts_disp_render_fwd(const float* est, const float* gt, const float* max_disp, const float* jet, int B, int h, int w, int Hg,
                       int Wg, int flags, float scale16, void* disp_color, void* err_class, void* err_jet, void* disp_u16,
                       float* stats, void* workspace, void* stream);

/* ------------------------------------------------------------------------------------------
 * Optical flow: metrics, colour maps and the KITTI 16-bit decode (architecture/data/evaluation/flow_pixel_error.py:9-96
 * `flow_calc_error`, architecture/utils/visualization/flow_colormap.py:8-220, architecture/data/utils/load_flow.py:54-78 `load_png`).
 * A flow map is fp32 [B,2,h,w], or [B,h,w,2] with the call's *_HWC flag: either is read in place (quads where the rows are
 * 16-byte aligned and the width is a multiple of 4, single pixels otherwise).  Every quantity that feeds a decision is fp32 in the
 * reference's operation order, every operation rounded on its own.
 * ts_flow_metrics_fwd: flow_calc_error of up to four estimates against one ground truth in one call.
 *   est<l> [B,2,h<l>,w<l>] (n_est = 1..4; unused pointers may be NULL); a level whose size differs from the ground truth's is read
 *   through F.interpolate(est, (Hg,Wg), bilinear, align_corners) evaluated in registers, then u * Wg / w and v * Hg / h.
 *   gt [B,2,Hg,Wg].  Valid pixels: no NaN in gt, lb < sqrt(gt_u^2 + gt_v^2) < ub (strict), and with TS_FLOW_SPARSE not
 *   (|gt_u| < 1e-12 and |gt_v| < 1e-12).
 *   out [n_est][5] fp32: {1px, 2px, 3px, 5px, epe} of err = sqrt((gt_u - est_u)^2 + (gt_v - est_v)^2) (percent; 0 when no pixel is
 *   valid; a NaN estimate inside the mask leaves the counts alone and makes epe NaN).
 *   Counts are exact integers, sums fp64 in a fixed order: bit-identical from run to run.  Two launches, no synchronisation.
 * ts_flow_render_fwd: est [B,2,h,w] is read at the size of the target (Hg,Wg) as above; gt [B,2,Hg,Wg] (NULL when no selected
 *   output needs it); flags selects the outputs and their form:
 *     TS_FLOW_RENDER_EST_COLOR / TS_FLOW_RENDER_GT_COLOR  flow_to_color (:143-167) of est / gt into flow_color: [B,Hg,Wg,3], or with
 *                            both set [B,2Hg,Wg,3], est above gt.  Unknown pixels (|u| or |v| > 1e7, or NaN) count as 0 in the
 *                            maximum radius and are black.  The maximum is each map's own (per image), the one of both maps with
 *                            TS_FLOW_RENDER_MAX_SHARED, or max_rad[b] with TS_FLOW_RENDER_MAX_GIVEN.  wheel: the 55 x 3 fp32 table
 *                            of make_color_wheel (:8-56), values 0..255 (device pointer).
 *     TS_FLOW_RENDER_ERR_CLASS  flow_err_to_color (:170-220) into err_class [B,Hg,Wg,3]; gt_val (may be NULL) fp32 [B,Hg,Wg]
 *                            multiplies the error, and 0 gives black
 *     TS_FLOW_RENDER_STATS   stats is written although no selected output needs it
 *     TS_FLOW_RENDER_UINT8   colour outputs are uint8, floor(255 v + 0.5) after a clamp to [0,1], NaN -> 0; else fp32
 *     TS_FLOW_RENDER_CHW     colour outputs are [B,3,rows,Wg] instead of [B,rows,Wg,3]
 *   stats [B][TS_FLOW_STATS_FLOATS] (written with TS_FLOW_RENDER_STATS or when a maximum is taken from the data; needs workspace):
 *     [0] max radius of est  [1] of gt (0 without gt)  [2] of both  [4..13] the members' counts of the ten error classes, int32
 *     bit patterns (0 without gt)  [3], [14], [15] zero.
 *   Two launches (statistics + finish) are skipped when stats is not needed; then the colour launch.  No atomics, no
 *   synchronisation; bit-identical from run to run.
 * ts_flow_u16_decode_fwd: raw uint16 [B,H,W,3], or [B,3,H,W] with TS_FLOW_U16_CHW -> flow fp32 [B,2,H,W] = (raw - 2^15) / 64 (exact),
 *   both components 0 where the third channel is 0; valid (may be NULL) uint8 [B,1,H,W] = third channel != 0.  One launch.
 * ---------------------------------------------------------------------------------------- */
#define TS_FLOW_SPARSE 1
#define TS_FLOW_EST_HWC 2
#define TS_FLOW_GT_HWC 4
#define TS_FLOW_RENDER_EST_COLOR 1
#define TS_FLOW_RENDER_GT_COLOR 2
#define TS_FLOW_RENDER_ERR_CLASS 4
#define TS_FLOW_RENDER_STATS 8
#define TS_FLOW_RENDER_UINT8 16
#define TS_FLOW_RENDER_CHW 32
#define TS_FLOW_RENDER_MAX_SHARED 64
#define TS_FLOW_RENDER_MAX_GIVEN 128
#define TS_FLOW_RENDER_EST_HWC 256
#define TS_FLOW_RENDER_GT_HWC 512
#define TS_FLOW_STATS_FLOATS 16
#define TS_FLOW_U16_CHW 1
size_t ts_flow_metrics_workspace_bytes(int B, int Hg, int Wg);
int ts_flow_metrics_fwd(const float* est0, const float* est1, const float* est2, const float* est3, int n_est, int h0, int w0,
                        int h1, int w1, int h2, int w2, int h3, int w3, const float* gt, int B, int Hg, int Wg, float lb, float ub,
                        int flags, float* out, void* workspace, void* stream);
size_t ts_flow_render_workspace_bytes(int B, int Hg, int Wg);
int ts_flow_render_fwd(const float* est, const float* gt, const float* gt_val, const float* max_rad, const float* wheel, int B,
                       int h, int w, int Hg, int Wg, int flags, void* flow_color, void* err_class, float* stats, void* workspace,
                       void* stream);
int ts_flow_u16_decode_fwd(const void* raw, int B, int H, int W, int flags, float* flow, void* valid, void* stream);

/* ------------------------------------------------------------------------------------------
 * Preparation of the input frames (projects/TemporalStereo/video_inference.py:100-110 `read_image`, :135-140 `read_disparity`, :246-251;
 * architecture/data/datasets/base.py:99-187 `do_transform`, :231-248 the intrinsics pyramid): uint8 frames in, the batch's tensors out.
 * ts_frames_prepare_fwd: one launch for the whole batch and both eyes.
 *   left / right  uint8 [B,Hs,Ws,3], or [B,3,Hs,Ws] with TS_PREPARE_CHW; right may be NULL (then color_r / color_aug_r must be).
 *   color_*       fp32 [B,3,Hc,Wc] = byte / 255 (ToTensor), image b at color_* + b * color_stride (floats, >= 3 Hc Wc)
 *   color_aug_*   fp32 [B,3,H,W] = ((byte / 255) - mean[c]) / std[c] (normalize; both divisions correctly rounded), then
 *                 image b at color_aug_* + b * color_aug_stride (floats, >= 3 H W).  Any output pointer may be NULL, not all.
 *   crop NULL, (H,W) == (Hs,Ws)   the values as they are; (Hc,Wc) = (Hs,Ws)
 *   crop NULL, (H,W) != (Hs,Ws)   color_aug = F.interpolate(normalised, (H,W), bilinear, align_corners=True) (base.py:183,
 *                                 video_inference.py:108), any ratio; normalised first, then interpolated; (Hc,Wc) = (Hs,Ws)
 *   crop given                    DEVICE pointer to int32 [B,2] = (ch, cw) per image: rows ch..ch+H-1, columns cw..cw+W-1 of both
 *                                 outputs (base.py:155); (Hc,Wc) = (H,W); needs H <= Hs, W <= Ws.  The origins are read by the
 *                                 kernel, so the host cannot refuse them: an origin outside [0,Hs-H] x [0,Ws-W] is CLAMPED into it
 *                                 (nothing is read out of bounds).
 *   No workspace, no atomics; bit-identical from run to run.
 * ts_intrinsics_pyramid_fwd: K_norm [B,4,4] fp32 (is_fp64 0) or fp64 (1), the "K / (h, w)" form -> K, inv_K fp32 [B,S,4,4]:
 *   rows 0 / 1 times kw >> s / kh >> s (base.py:241-242), the inverse by cofactors in fp64 rounded once (the reference: np.linalg.pinv
 *   in fp64, then .float()).  K_norm must be invertible and kh >> (S-1), kw >> (S-1) positive.
 * ts_disp_u16_decode_fwd: raw uint16 [B,H,W] -> disp fp32 [B,1,H,W] = raw / scale where raw > 0 (exact for a power of two such as
 *   256), else 0; valid (may be NULL) uint8 [B,1,H,W] = raw > 0.
 * ---------------------------------------------------------------------------------------- */
#define TS_PREPARE_CHW 1
int ts_frames_prepare_fwd(const void* left, const void* right, int B, int Hs, int Ws, int flags, float mean0, float mean1,
                          float mean2, float std0, float std1, float std2, int H, int W, const int* crop, float* color_l,
                          float* color_r, long long color_stride, float* color_aug_l, float* color_aug_r,
                          long long color_aug_stride, void* stream);
int ts_intrinsics_pyramid_fwd(const void* K_norm, int is_fp64, int B, int kh, int kw, int S, float* K, float* inv_K, void* stream);
int ts_disp_u16_decode_fwd(const void* raw, int B, int H, int W, float scale, float* disp, void* valid, void* stream);

/* ------------------------------------------------------------------------------------------
 * Augmentation of the training frames (architecture/data/datasets/base.py:65-187: ColorJitter in a random order, AdjustGamma, the
 * crop, the occlusion rectangles on the right eye's color_aug).  The random draws are made on the host and handed over as ONE table:
 * table  DEVICE pointer to int32 [eyes,B,TS_AUGMENT_ROW_INTS], eyes = 2 with a right image, else 1; the words of a row:
 *     [0]      flags: TS_AUGMENT_GAMMA = the row's gamma table is applied after the colour operations
 *     [1]      the order: byte k (k = 0 lowest) is the k-th operation, 0 brightness, 1 contrast, 2 saturation, 3 hue, 4 none;
 *              an operation appears at most once
 *     [2..4]   the factors of brightness, contrast, saturation (fp32 bit patterns)      [5] the hue shift in bytes, 0..255
 *     [6],[7]  the crop origin (ch, cw); outside [0,Hs-H] x [0,Ws-W] it is CLAMPED (the kernel reads it, the host cannot refuse it)
 *     [8]      the number of rectangles, 0..TS_AUGMENT_MAX_RECTS   [9..24] (sh, sw, occh, occw) each, window coordinates, in the order
 *              they are applied (a later one overwrites an earlier one); the part outside the window is ignored
 *     [25],[26] the noise seed, low and high word                   [27..31] zero
 *     [32..95] the gamma table, 256 bytes, byte e of word 32 + e / 4 at bits 8 (e % 4)
 * ts_frames_augment_fwd: two launches for the whole batch and both eyes (grey-level sums of the full frames for contrast, then
 *   the window).  left / right / flags / mean / std / strides as ts_frames_prepare_fwd; H <= Hs, W <= Ws.
 *   color_*      fp32 [B,3,H,W] = byte / 255 of the window of the frame as it came
 *   color_aug_*  fp32 [B,3,H,W] = the window of normalize(gamma(operations(frame))) in PIL's uint8 arithmetic, bit for bit; inside a
 *                rectangle (n - mean[c]) / std[c], n ~ N(0, 0.1) from Philox-4x32-10 keyed by the row's seed and counted by
 *                (column, row in the rectangle, channel, rectangle): independent of B, of the image's place and of the strides.
 *   workspace    ts_frames_augment_workspace_bytes(B, Hs, Ws) bytes, 8-byte aligned; need not be zeroed.  No atomics; bit-identical
 *                from run to run.
 * ts_disp_u16_window_fwd: ts_disp_u16_decode_fwd of the window [ch:ch+H, cw:cw+W] whose origin is words [6],[7] of row b of the
 *   table (the left eye's rows), clamped alike: raw uint16 [B,Hs,Ws] -> disp fp32 [B,1,H,W], valid (may be NULL) uint8 [B,1,H,W].
 * ---------------------------------------------------------------------------------------- */
#define TS_AUGMENT_ROW_INTS 96
#define TS_AUGMENT_MAX_RECTS 4
#define TS_AUGMENT_GAMMA 1
size_t ts_frames_augment_workspace_bytes(int B, int Hs, int Ws);
int ts_frames_augment_fwd(const void* left, const void* right, int B, int Hs, int Ws, int flags, float mean0, float mean1,
                          float mean2, float std0, float std1, float std2, int H, int W, const int* table, float* color_l,
                          float* color_r, long long color_stride, float* color_aug_l, float* color_aug_r,
                          long long color_aug_stride, void* workspace, size_t workspace_bytes, void* stream);
int ts_disp_u16_window_fwd(const void* raw, int B, int Hs, int Ws, int H, int W, const int* table, float scale, float* disp,
                           void* valid, void* stream);

/* ------------------------------------------------------------------------------------------
 * K4  disparity regression.  cost / sample / offset are [B,D,H,W].
 * ts_topk_softargmax_*: predict_disp()  .../aggregation/TemporalStereo/coarse.py:69-75
 *   (== fine.py:70-76, precise.py:61-67): top-k (1 <= k <= 8, ties: lowest index first) ->
 *   softmax -> gather(sample+offset) -> weighted sum.  disp [B,1,H,W]; topk_* [B,k,H,W];
 *   topk_index (int32, may be NULL in fwd) is what the backward needs.  Backward overwrites
 *   grad_cost and grad_sample ([B,D,H,W]; grad of offset == grad of sample); any grad_* input may be NULL.
 * ts_softargmin_*: SOFTARGMIN.forward  architecture/modeling/prediction/soft_argmin.py:38-59
 * ts_argmax_select_fwd: ARGMIN.forward  architecture/modeling/prediction/argmin.py:35-46
 * ---------------------------------------------------------------------------------------- */
int ts_topk_softargmax_fwd(const float* cost, const float* sample, const float* offset, float* disp,
                           float* topk_disp, float* topk_cost, int* topk_index,
                           int B, int D, int H, int W, int k, void* stream);

/* ABI 19 -- ts_topk_softargmax_fwd followed by ts_convex_upsample_candidates_fwd on its disparity, as one launch (the tail of the
 * coarse and fine levels of an inference pass): mask [B,9*factor^2,H,W]; out / low / high [B,1,factor*H,factor*W] and the
 * candidate planes exactly as ts_convex_upsample_candidates_fwd writes them.  The disparity at level resolution and the top-k
 * planes are not written.  Results are bit-identical to the two launches.  factor <= 8. */
int ts_regress_convex_upsample_fwd(const float* cost, const float* sample, const float* offset, const float* mask,
                                   float* out, float* low, float* high, float* candidates, int B, int D, int H, int W,
                                   int k, int factor, float disp_scale, float range, int channel_offset,
                                   int channels_total, void* stream);

/* ABI 19 -- ts_topk_softargmax_fwd followed by ts_resize_bilinear_pair_fwd of its top-k planes to (H/2, W/2) with value scales 0.5
 * and 1 (the tail of the 1/4 level, precise.py:100-103), as one launch: disp [B,1,H,W]; mem_sample / mem_cost [B,k,H/2,W/2].  The
 * full-size top-k planes are not written.  Bit-identical to the two launches.  Odd H or W: TS_ERR_UNSUPPORTED. */
int ts_topk_softargmax_half_fwd(const float* cost, const float* sample, const float* offset, float* disp,
                                float* mem_sample, float* mem_cost, int B, int D, int H, int W, int k, void* stream);

int ts_topk_softargmax_bwd(const float* topk_disp, const float* topk_cost, const int* topk_index,
                           const float* disp, const float* grad_disp, const float* grad_topk_disp,
                           const float* grad_topk_cost, float* grad_cost, float* grad_sample,
                           int B, int D, int H, int W, int k, void* stream);

int ts_softargmin_fwd(const float* cost, const float* sample, float* disp, float temperature,
                      int normalize, int B, int D, int H, int W, void* stream);

int ts_softargmin_bwd(const float* cost, const float* sample, const float* disp, const float* grad_disp,
                      float* grad_cost, float* grad_sample, float temperature, int normalize,
                      int B, int D, int H, int W, void* stream);

int ts_argmax_select_fwd(const float* cost, const float* sample, float* disp, int* index,
                         int B, int D, int H, int W, void* stream);

/* ------------------------------------------------------------------------------------------
 * K2  temporal cost warp.
 * ts_softsplat_sum_*: the three kernels of architecture/modeling/layers/softsplat.py:8-177
 *   (updateOutput :14-52, updateGradInput :63-105, updateGradFlow :116-176); input/output [B,C,H,W],
 *   flow [B,2,H,W] (x then y).  fwd zero-fills `output` itself.  fp32 atomics: order not deterministic.
 * ts_softsplat_softmax_fwd: FunctionSoftsplat(..., 'softmax')  softsplat.py:334-360 fused for the
 *   detached use in update_map (projects/TemporalStereo/TemporalStereo.py:415-419): metric [B,1,H,W].
 * ts_project_to_3d_fwd: project_to_3d()  architecture/modeling/layers/inverse_warp.py:92-178;
 *   depth [B,C,H,W], K [B,k,k] (k = 3|4), inv_K [B,ik,ik], T [B,4,4] -> triangular_depth [B,C,H,W],
 *   optical_flow [B,2C,H,W], flow_mask [B,C,H,W] (uint8); any output may be NULL.
 * ---------------------------------------------------------------------------------------- */
int ts_softsplat_sum_fwd(const float* input, const float* flow, float* output,
                         int B, int C, int H, int W, void* stream);
/* order-independent summation splat (64-bit fixed-point accumulation, integer atomics): bit-identical from
 * run to run; workspace B*C*H*W*8 bytes; |values| < 2^22 */
int ts_softsplat_sum_fwd_deterministic(const float* input, const float* flow, float* output, void* workspace,
                                       int B, int C, int H, int W, void* stream);
int ts_softsplat_sum_bwd_input(const float* flow, const float* grad_output, float* grad_input,
                               int B, int C, int H, int W, void* stream);
int ts_softsplat_sum_bwd_flow(const float* input, const float* flow, const float* grad_output,
                              float* grad_flow, int B, int C, int H, int W, void* stream);
size_t ts_softsplat_softmax_workspace_bytes(int B, int C, int H, int W);
int ts_softsplat_softmax_fwd(const float* input, const float* flow, const float* metric, float* output,
                             void* workspace, int B, int C, int H, int W, void* stream);
int ts_project_to_3d_fwd(const float* depth, const float* K, const float* inv_K, const float* T,
                         float* triangular_depth, float* optical_flow, unsigned char* flow_mask,
                         int B, int C, int H, int W, int k_dim, int inv_k_dim, float eps, void* stream);

/* ------------------------------------------------------------------------------------------
 * The 2-D inverse warp (ABI 14).
 * Replaces inverse_warp()  architecture/modeling/layers/inverse_warp.py:6-77 -- pixel grid, normalisation, the [B,H,W,2] grid
 * tensor and F.grid_sample(align_corners=True) -- and, in depth mode, the project_to_3d() it calls (:92-178), in ONE launch.
 *   img [B,C,Hi,Wi]; motion [B,1,H,W] (disparity, depth) or [B,2,H,W] (flow: x then y); out [B,C,H,W].  The image may differ in
 *   size from the motion map: the reference normalises with H, W and grid_sample un-normalises with Hi, Wi.  All four >= 2.
 *   mode    TS_WARP_DISPARITY  X = x + m, Y = y
 *           TS_WARP_FLOW       X = x + m0, Y = y + m1
 *           TS_WARP_DEPTH      (X, Y) = src_pixel_coord of project_to_3d(motion, K, inv_K, T, eps): K [B,k,k] (k = 3|4),
 *                              inv_K [B,ik,ik], T [B,4,4], all three required; the arithmetic is ts_project_to_3d_fwd's, bit for bit
 *   position  gx = (2 X) / (W - 1) - 1, ix = ((gx + 1) / 2) * (Wi - 1), each step rounded as the reference's fp32 run rounds it;
 *             likewise for y with H, Hi
 *   pad     TS_WARP_ZEROS taps outside contribute 0; TS_WARP_BORDER position clipped to [0, size - 1]; TS_WARP_REFLECTION
 *           reflected over [0, size - 1] as often as needed, then clipped
 *   interp  TS_WARP_BILINEAR; TS_WARP_NEAREST (round half to even); TS_WARP_BICUBIC is TS_ERR_UNSUPPORTED
 *   The position is clamped to a finite range before any conversion to int: no motion, however large or non-finite, indexes
 *   outside the image (the value there is unspecified).
 *   Side outputs of depth mode, each may be NULL (ignored in the other modes): triangular_depth [B,1,H,W], src_pixel_coord
 *   [B,2,H,W], optical_flow [B,2,H,W], flow_mask [B,1,H,W] (uint8), homo_points_3d [B,4,H*W].
 * ts_inverse_warp_bwd: grad_out [B,C,H,W].  Either gradient may be NULL, not both.
 *   grad_img    [B,C,Hi,Wi] is ACCUMULATED with fp32 hardware atomics into what the caller zero-filled: the summation order is not
 *               deterministic (the contract of ts_softsplat_sum_fwd)
 *   grad_motion (the motion's shape) is OVERWRITTEN and deterministic: the tap differences reduced over the channels, times
 *               (Wi - 1) / (W - 1) resp. (Hi - 1) / (H - 1); 0 where TS_WARP_BORDER clipped the position, sign flipped on odd
 *               reflections, 0 everywhere for TS_WARP_NEAREST; in depth mode through d src_pixel_coord / d depth.  Needs img.
 *   K, inv_K and T are constants: no gradient reaches them.
 * Checks, before any launch: sizes (TS_ERR_SHAPE, also any of H, W, Hi, Wi < 2), then codes (TS_ERR_UNSUPPORTED), then pointers
 * (TS_ERR_NULL, also depth mode without K, inv_K or T).
 * ---------------------------------------------------------------------------------------- */
#define TS_WARP_DISPARITY 0
#define TS_WARP_FLOW 1
#define TS_WARP_DEPTH 2
#define TS_WARP_BILINEAR 0
#define TS_WARP_NEAREST 1
#define TS_WARP_BICUBIC 2
#define TS_WARP_ZEROS 0
#define TS_WARP_BORDER 1
#define TS_WARP_REFLECTION 2
int ts_inverse_warp_fwd(const float* img, const float* motion, const float* K, const float* inv_K, const float* T, float* out,
                        float* triangular_depth, float* src_pixel_coord, float* optical_flow, unsigned char* flow_mask,
                        float* homo_points_3d, int B, int C, int Hi, int Wi, int H, int W, int mode, int interp, int pad,
                        int k_dim, int inv_k_dim, float eps, void* stream);
int ts_inverse_warp_bwd(const float* img, const float* motion, const float* K, const float* inv_K, const float* T,
                        const float* grad_out, float* grad_img, float* grad_motion, int B, int C, int Hi, int Wi, int H, int W,
                        int mode, int interp, int pad, int k_dim, int inv_k_dim, float eps, void* stream);

/* ------------------------------------------------------------------------------------------
 * CorrBlock: the RAFT-Stereo correlation pyramid and its windowed lookup (ABI 15).
 * Replaces CorrBlock  architecture/modeling/aggregation/utils/raft_corr.py:4-67.  fmap1, fmap2 [B,C,H,W], disp [B,1,H,W];
 * n = (b*H + y)*W + x numbers the pixels, N = B*H*W, W_i = W >> i.
 *   P_0[n][x'] = sum_c fmap1[b,c,y,x] * fmap2[b,c,y,x'] / sqrt(C);  P_i[n][m] = (P_{i-1}[n][2m] + P_{i-1}[n][2m+1]) / 2, m < W_i
 *   out[b, i*(2r+1)+k, y, x] = (1 - 2^-(i+1)) * lerp0(P_i[n][:], ((x - disp[n]) / 2^i + (k - r)) * W_i / (W - 1) - 0.5)
 *   (linear interpolation, zeros outside the row; both the mixed normalisation and the level weights are the reference's).
 * pyramid: ONE buffer of N * (W_0 + ... + W_{L-1}) floats; level i is [N][W_i] contiguous at float offset N * (W_0 + ... + W_{i-1}).
 * ts_raft_corr_pyramid_fwd  builds every level in one launch (v_mfma_f32_16x16x4_f32; level 0 is not read back).
 * ts_raft_corr_lookup_fwd   out [B, L*(2r+1), H, W], one launch.
 * ts_raft_corr_lookup_bwd   grad_out as out.  grad_disp [B,1,H,W] (needs pyramid) and grad_pyramid are OVERWRITTEN; either may be
 *                           NULL, not both.  fold != 0: grad_pyramid is G [N][W], the cotangent of level 0 with levels 1..L-1
 *                           folded in by the pooling's own backward (what ts_raft_corr_pyramid_bwd takes with levels = 1);
 *                           fold == 0: grad_pyramid has the pyramid's layout, every level written.  No atomics: bit-reproducible.
 * ts_raft_corr_pyramid_bwd  grad_pyramid with `levels` levels (1: a folded G).  grad_fmap1 = G fmap2^T / sqrt(C) and grad_fmap2 =
 *                           G^T fmap1^T / sqrt(C) per image row, OVERWRITTEN; either may be NULL, not both.  Deterministic.
 * Checks, before any launch: sizes (TS_ERR_SHAPE: non-positive, W < 2, num_levels < 1, radius < 0, W >> (num_levels - 1) < 1 --
 * the reference's avg_pool2d raises there), num_levels > 7 or radius > 1024 (TS_ERR_UNSUPPORTED), then pointers (TS_ERR_NULL).
 * ---------------------------------------------------------------------------------------- */
int ts_raft_corr_pyramid_fwd(const float* fmap1, const float* fmap2, float* pyramid, int B, int C, int H, int W, int num_levels,
                             void* stream);
int ts_raft_corr_lookup_fwd(const float* pyramid, const float* disp, float* out, int B, int H, int W, int num_levels, int radius,
                            void* stream);
int ts_raft_corr_lookup_bwd(const float* pyramid, const float* disp, const float* grad_out, float* grad_disp, float* grad_pyramid,
                            int B, int H, int W, int num_levels, int radius, int fold, void* stream);
int ts_raft_corr_pyramid_bwd(const float* grad_pyramid, const float* fmap1, const float* fmap2, float* grad_fmap1, float* grad_fmap2,
                             int B, int C, int H, int W, int levels, void* stream);

/* ------------------------------------------------------------------------------------------
 * FlowCorrBlock: the RAFT all-pairs correlation pyramid for optical flow and its windowed lookup (ABI 16).
 * Replaces FlowCorrBlock + bilinear_sampler  architecture/modeling/aggregation/utils/raft_corr.py:71-160.  fmap1, fmap2 [B,C,H,W],
 * coords [B,2,H,W] (channel 0 = x, 1 = y, level-0 scale); N = H*W, n / m number the pixels of frame 1 / frame 2 row-major,
 * H_i = H >> i, W_i = W >> i, K = 2r + 1.
 *   P_0[b,n,m] = (f1_n.f1_m - 2 f1_n.f2_m + f2_n.f2_m) / sqrt(C)   (the reference's full Gram matrices; = (f1_n.D_m - D_n.f2_m) / sqrt(C),
 *   D = f1 - f2, which is how it is evaluated);  P_i[b,n] = avg_pool2d(P_{i-1}[b,n] as an H_{i-1} x W_{i-1} image, 2, 2)
 *   out[b, i*K*K + a*K + bb, y, x] = bilinear(P_i[b,n], x_t / 2^i + (a - r), y_t / 2^i + (bb - r)), zeros outside: the FIRST window
 *   index moves x (the reference's meshgrid(dy, dx)); the position takes bilinear_sampler's and grid_sample's fp32 steps in order.
 * pyramid: ONE buffer; level i is [B*N][H_i*W_i] contiguous at float offset B*N * sum_{l<i} H_l*W_l.
 * ts_flow_corr_pyramid_fwd  builds every level in one launch (v_mfma_f32_16x16x4_f32; level 0 is not read back).
 * ts_flow_corr_lookup_fwd   out [B, L*K*K, H, W], one launch.
 * ts_flow_corr_lookup_bwd   grad_out as out.  grad_coords [B,2,H,W] (needs pyramid) and grad_pyramid are OVERWRITTEN; either may be
 *                           NULL, not both.  fold != 0: grad_pyramid is G [B*N][N], the cotangent of level 0 with levels 1..L-1
 *                           folded in by the pooling's own backward (what ts_flow_corr_pyramid_bwd takes with levels = 1);
 *                           fold == 0: grad_pyramid has the pyramid's layout, every level written.  No atomics: bit-reproducible.
 * ts_flow_corr_pyramid_bwd  grad_pyramid with `levels` levels (1: a folded G).  Per batch grad_fmap1 = ((G + G^T) f1 - 2 G f2) / sqrt(C),
 *                           grad_fmap2 = ((G + G^T) f2 - 2 G^T f1) / sqrt(C), OVERWRITTEN; either may be NULL, not both.  Deterministic.
 * Checks, before any launch: sizes (TS_ERR_SHAPE: non-positive, num_levels < 1, radius < 0, a level smaller than 2 x 2 -- the
 * reference divides by H_i - 1 and W_i - 1), num_levels > 4 or radius > 1024 or a window too large for LDS (TS_ERR_UNSUPPORTED),
 * then pointers (TS_ERR_NULL).
 * ---------------------------------------------------------------------------------------- */
int ts_flow_corr_pyramid_fwd(const float* fmap1, const float* fmap2, float* pyramid, int B, int C, int H, int W, int num_levels,
                             void* stream);
int ts_flow_corr_lookup_fwd(const float* pyramid, const float* coords, float* out, int B, int H, int W, int num_levels, int radius,
                            void* stream);
int ts_flow_corr_lookup_bwd(const float* pyramid, const float* coords, const float* grad_out, float* grad_coords, float* grad_pyramid,
                            int B, int H, int W, int num_levels, int radius, int fold, void* stream);
int ts_flow_corr_pyramid_bwd(const float* grad_pyramid, const float* fmap1, const float* fmap2, float* grad_fmap1, float* grad_fmap2,
                             int B, int C, int H, int W, int levels, void* stream);

/* ------------------------------------------------------------------------------------------
 * SPP3D: the memory-bound pieces of the 3-D pyramid pooling module (ABI 18).
 * Replaces the avg_pool3d / interpolate / cat of SPP3D.forward  architecture/modeling/aggregation/utils/SPP3D.py:38-49; its
 * convolutions run on the (k,1,1) and (1,3,3) families above.  x [B,C,D,H,W] (batch / channel strides in elements, D*H*W dense).
 * Level i of stride s_i (num_levels <= 4, unused strides ignored): box k_i = (min(D,s_i), min(H,s_i), min(W,s_i)), n_i = floor(dim / k_i)
 * cells per axis, a trailing remainder is dropped.
 *   pooled: ONE buffer; level i is [B][C][n_i] contiguous at float offset B*C * sum_{l<i} |n_l|.
 * ts_spp3d_pool_fwd    every level in one launch; a level whose box is a whole multiple of the previous level's is summed from that
 *                      level's partial sums (LDS), the others from x.
 * ts_spp3d_pool_bwd    grad_x[v] = addend[v] + sum_i g_i[cell_i(v)] / |k_i| over the levels whose covered region holds v, OVERWRITTEN;
 *                      g_i [B,C,n_i] dense, one pointer per level (the cotangents arrive as separate tensors); addend (strided like x, may be NULL) is the part of the concat gradient that belongs to x.
 * ts_spp3d_expand_fwd  cat [B, C + Cl*L, D, H, W] = [x | resize(lv0) | ...]: lv_i [B,Cl,n_i] dense, resized trilinearly with
 *                      align_corners (the framework's fp32 order: scale (n_in-1)/(n_out-1), pos = scale*o, floor, upper index clamped).
 * ts_spp3d_expand_bwd  g_i [B,Cl,n_i] OVERWRITTEN from channels [C, C + Cl*L) of grad_cat (strided); one wave per coarse cell gathers
 *                      over that cell's support.  (The gradient of x through the concat is a view of grad_cat: no kernel.)
 * ts_depth_sum3_fwd    y[d] = act(scale[c] * (z0[d-1] + z1[d] + z2[d+1]) + shift[c]), planes outside [0,D) zero; scale / shift may be
 *                      NULL (1 / 0); act 0 none, 1 SiLU, 2 ReLU; y may be z1.  With z0 and z2 exchanged it sums the three data
 *                      gradients of a 3x3x3 convolution run as three (1,3,3) convolutions.
 * No atomics: every entry is bit-reproducible.  Checks, before any launch: sizes (TS_ERR_SHAPE: non-positive, num_levels < 1, a stride
 * < 1, overlapping strides), num_levels > 4, an axis >= 2^20, B * channels > 65535 (TS_ERR_UNSUPPORTED), then pointers (TS_ERR_NULL).
 * ---------------------------------------------------------------------------------------- */
int ts_spp3d_pool_fwd(const float* x, float* pooled, int B, int C, int D, int H, int W, int num_levels, int s0, int s1, int s2, int s3,
                      long long x_bstride, long long x_cstride, void* stream);
int ts_spp3d_pool_bwd(const float* g0, const float* g1, const float* g2, const float* g3, const float* addend, float* grad_x, int B,
                      int C, int D, int H, int W, int num_levels, int s0, int s1, int s2, int s3, long long addend_bstride,
                      long long addend_cstride, long long gx_bstride, long long gx_cstride, void* stream);
int ts_spp3d_expand_fwd(const float* x, const float* lv0, const float* lv1, const float* lv2, const float* lv3, float* cat, int B, int C,
                        int Cl, int D, int H, int W, int num_levels, int s0, int s1, int s2, int s3, long long x_bstride,
                        long long x_cstride, void* stream);
int ts_spp3d_expand_bwd(const float* grad_cat, float* g0, float* g1, float* g2, float* g3, int B, int C, int Cl, int D, int H, int W,
                        int num_levels, int s0, int s1, int s2, int s3, long long g_bstride, long long g_cstride, void* stream);
int ts_depth_sum3_fwd(const float* z0, const float* z1, const float* z2, const float* scale, const float* shift, float* y, int B, int C,
                      int D, int H, int W, int act, long long z0_bstride, long long z0_cstride, long long z1_bstride,
                      long long z1_cstride, long long z2_bstride, long long z2_cstride, long long y_bstride, long long y_cstride,
                      void* stream);

/* Train-mode BatchNorm -> activation backward for FEW values per channel (B * N <= 4096; a coarse SPP3D level has down to two), carried
 * in fp64 up to the final rounding: y [B,C,N] the raw convolution output, g the incoming cotangent, dy OVERWRITTEN (all three strided),
 * sum_g [C] = sum of the cotangent behind the activation (the gradient of beta), sum_gx [C] = its sum against xhat (the gradient of
 * gamma).  The batch statistics are formed again from y.  With two values per channel the result is what a cancellation leaves,
 * O(eps / var) of its terms: an fp32 rounding of xhat costs 2^-24 var / eps of it.  gamma / beta may be NULL (1 / 0); act 0 | 1 | 2.
 * Checks: sizes, one value per channel, overlapping strides (TS_ERR_SHAPE), B * N > 4096 (TS_ERR_UNSUPPORTED), pointers (TS_ERR_NULL). */
int ts_bn_small_train_bwd(const float* y, const float* g, const float* gamma, const float* beta, float* sum_g, float* sum_gx, float* dy,
                          int B, int C, int N, long long y_bstride, long long y_cstride, long long g_bstride, long long g_cstride,
                          long long dy_bstride, long long dy_cstride, float eps, int act, void* stream);

/* ------------------------------------------------------------------------------------------
 * ConvGRU: the gated recurrent cell of layers/conv_gru.py:4-28 as two launches, fp32 throughout (ABI 20).
 *   z = sigmoid(convz([h, x]))  r = sigmoid(convr([h, x]))  q = tanh(convq([r*h, x]))  hidden = (1 - z) * h + z * q
 * h [B,Ch,H,W] and x [B,Cx,H,W] are read in place (batch / channel strides in elements, H*W dense): no concatenation is written.
 * Every other plane is dense [B,Ch,H,W].  The three 3x3 convolutions (padding 1, bias) run on the f32-input MFMA: an fmaf chain.
 * ts_conv_gru_weight_layout  wz, wr, wq [Ch][Ch+Cx][3][3] (the framework's, contiguous) -> w_l, ts_conv_gru_weight_bytes(Ch, Cx) bytes,
 *                            16-byte aligned: the gate rows [z | r] and the candidate rows in the kernels' chunked order.
 * ts_conv_gru_gates_fwd      z and rh = r * h OVERWRITTEN; r too unless it is NULL (only a backward pass reads it).
 * ts_conv_gru_out_fwd        out = hidden OVERWRITTEN from rh, x, z, h; q too unless it is NULL.  h strides as in the gates call.
 * ts_conv_gru_gate_bwd_a     dq_pre = dout z (1 - q^2) (dense), dz_pre = dout (q - h) z (1 - z) (strided: a half of the gates' [dz | dr]
 *                            buffer), dh = dout (1 - z) (dense), all OVERWRITTEN; N = H*W.
 * ts_conv_gru_gate_bwd_b     d_rh (strided: the first Ch channels of the candidate convolution's input gradient), r, h ->
 *                            dr_pre = d_rh h r (1 - r) (strided) OVERWRITTEN, dh += d_rh r.
 * ts_conv_gru_grad_sum       dcat_g / dcat_q [B,Ch+Cx,N] dense, the input gradients of the gate / candidate convolutions
 *                            (ts_conv3d_hw_bwd_data, D = 1): dh += dcat_g[:, :Ch]; dx [B,Cx,N] = dcat_g[:, Ch:] + dcat_q[:, Ch:] OVERWRITTEN,
 *                            skipped when dx is NULL.
 * The weight and bias gradients run on ts_conv3d_hw_bwd_weight (per gate and per source) and ts_channel_sum_fwd.  No atomics: every
 * entry is bit-reproducible.  Checks, before any launch: sizes (TS_ERR_SHAPE: non-positive, overlapping strides), then
 * Ch > 64, Cx > 64, an axis >= 2^20, a grid that does not fit (TS_ERR_UNSUPPORTED), then pointers (TS_ERR_NULL; r, q, dx may be NULL).
 * ---------------------------------------------------------------------------------------- */
size_t ts_conv_gru_weight_bytes(int Ch, int Cx);
int ts_conv_gru_weight_layout(const float* wz, const float* wr, const float* wq, float* w_l, int Ch, int Cx, void* stream);
int ts_conv_gru_gates_fwd(const float* h, const float* x, const float* w_l, const float* bz, const float* br, float* z, float* rh,
                          float* r, int B, int Ch, int Cx, int H, int W, long long h_bstride, long long h_cstride,
                          long long x_bstride, long long x_cstride, void* stream);
int ts_conv_gru_out_fwd(const float* rh, const float* x, const float* w_l, const float* bq, const float* z, const float* h, float* out,
                        float* q, int B, int Ch, int Cx, int H, int W, long long h_bstride, long long h_cstride,
                        long long x_bstride, long long x_cstride, void* stream);
int ts_conv_gru_gate_bwd_a(const float* dout, const float* z, const float* q, const float* h, float* dq_pre, float* dz_pre, float* dh,
                           int B, int Ch, long long N, long long h_bstride, long long h_cstride, long long dz_bstride,
                           long long dz_cstride, void* stream);
int ts_conv_gru_gate_bwd_b(const float* d_rh, const float* r, const float* h, float* dr_pre, float* dh, int B, int Ch, long long N,
                           long long drh_bstride, long long drh_cstride, long long h_bstride, long long h_cstride,
                           long long dr_bstride, long long dr_cstride, void* stream);
int ts_conv_gru_grad_sum(const float* dcat_g, const float* dcat_q, float* dh, float* dx, int B, int Ch, int Cx, long long N,
                         void* stream);

/* ------------------------------------------------------------------------------------------
 * FeatureDecoder: the layers of the backbone's three-level decoder, backbone/TemporalStereo.py:78-90,125-138, fp32 throughout (ABI 21).
 *   y = act(conv3x3(cat([resize(up), skip], 1)) * scale + shift)      stride 1, padding 1, on the f32-input MFMA: an fmaf chain
 * ts_decoder_conv_fwd       up [B,Cu,h,w] is read THROUGH the align-corners bilinear resize to (H,W) (the coordinates of
 *                           ts_resize_bilinear_fwd), skip [B,Cs,H,W] is read in place; neither the resized map nor the concatenation is
 *                           written.  The zero padding applies to the resized map.  Channel order [up | skip].  Cu = 0 (up, h, w
 *                           ignored) is the plain convolution; Cs > 0 always (skip sets the output plane).  y [B,Cout,H,W] OVERWRITTEN.
 *                           act 0 none | 1 SiLU; scale / shift [Cout] may be NULL (1 / 0).  up, skip and y have batch / channel
 *                           strides in elements, their planes dense.
 * ts_decoder_weight_layout  w [Cout][Cin][3][3] (the framework's, contiguous), Cin = Cu + Cs -> w_l, ts_decoder_weight_bytes(Cin, Cout)
 *                           bytes (0 outside the envelope), 16-byte aligned: the kernel's chunked order, one launch.
 * ts_resize_bilinear_bwd    the adjoint of the align-corners bilinear resize (h,w) -> (H,W) as a gather: dx [B,C,h,w] OVERWRITTEN from
 *                           dy [B,C,H,W], both with batch / channel strides.  Each coarse pixel sums, in a fixed order, the fine pixels
 *                           whose two source indices include it.  No atomics: bit-reproducible.
 * The other gradients run on ts_conv3d_hw_bwd_data (D = 1, over the concatenation's channels), ts_conv3d_hw_bwd_weight (per source and
 * per slice of <= 64 output channels), ts_bn_* and ts_channel_sum_fwd.  Checks, before any launch: sizes (TS_ERR_SHAPE: non-positive,
 * an unknown activation, overlapping strides), then Cu + Cs > 512, Cout > 512, an axis >= 2^20, a grid that does not fit
 * (TS_ERR_UNSUPPORTED), then pointers (TS_ERR_NULL; scale, shift, and up when Cu = 0 may be NULL), then the alignment of w_l
 * (TS_ERR_ALIGN), then the aliasing rule of ts_decoder_conv_fwd (ABI 24, TS_ERR_SHAPE): y lies apart from up and from skip, judged on
 * the operands' bounding extents as for ts_conv3x3_s_fwd below (other workgroups read the neighbours of what a workgroup writes).
 * ---------------------------------------------------------------------------------------- */
size_t ts_decoder_weight_bytes(int Cin, int Cout);
int ts_decoder_weight_layout(const float* w, float* w_l, int Cin, int Cout, void* stream);
int ts_decoder_conv_fwd(const float* up, const float* skip, const float* w_l, const float* scale, const float* shift, float* y, int B,
                        int Cu, int Cs, int Cout, int h, int w, int H, int W, int act, long long up_bstride, long long up_cstride,
                        long long skip_bstride, long long skip_cstride, long long y_bstride, long long y_cstride, void* stream);
int ts_resize_bilinear_bwd(const float* dy, float* dx, int B, int C, int h, int w, int H, int W, long long dy_bstride,
                           long long dy_cstride, long long dx_bstride, long long dx_cstride, void* stream);

/* ------------------------------------------------------------------------------------------
 * MemoryInvertedResidual: the encoder's inverted-residual block with the feature memory spliced into its input,
 * backbone/TemporalStereo.py:165-218, fp32 throughout, no atomics (ABI 22).  Eval form, four launches:
 *   e = silu(conv1x1(cat([memory, input[:, mc:]], 1)) * scale + shift)            ts_mbconv_expand_fwd
 *   d = silu(depthwise3x3(e) * scale + shift), plane_sum = sum over the plane of d  ts_depthwise3x3_fwd
 *   gate = sigmoid(w_expand . silu(w_reduce . (plane_sum * inv_hw) + b_reduce) + b_expand)      ts_se_gate_fwd
 *   y = conv1x1(d * gate) * scale + shift + residual                              ts_mbconv_project_fwd
 * Both 1x1 convolutions run on the f32-input MFMA with blocked sums (chains of 256 products, then a chain of blocks); an output's
 * bits do not depend on the batch or the launch geometry.
 * ts_mbconv_weight_layout     w [Cout][Cin] (the framework's 1x1 weight, contiguous) -> w_l, ts_mbconv_weight_bytes(Cin, Cout) bytes
 *                             (0 outside 1..2048 each), 16-byte aligned: the transpose, zero padded; one launch.
 * ts_mbconv_expand_fwd        input channels [0, mc) are read from memory [B,mc,H,W], channels [mc, C) from input [B,C,H,W] (its first mc
 *                             channels are not read), each in place; the concatenation is not written.  memory NULL: input alone (the
 *                             first frame; mc and the memory strides are ignored).  y [B,Cmid,H,W] OVERWRITTEN.
 * ts_mbconv_project_fwd       x [B,Cmid,H,W] times gate [B][Cmid] (dense) per channel while it is read; the gated map is not written.
 *                             residual and y [B,C,H,W]; y OVERWRITTEN.
 * ts_depthwise3x3_fwd         x, y [B,C,H,W], w [C][9], stride 1, padding 1; act 0 none | 1 SiLU; flip 1 reverses the nine taps (with
 *                             no epilogue: the input gradient of dy).  plane_sum [B][C] may be NULL; a plane's sum is taken in an order
 *                             fixed by (H, W): the same bits whatever B and C are.  One workgroup per (b, c) plane.
 * ts_depthwise3x3_bwd_weight  dw [C][9] OVERWRITTEN: dw[c][t] = sum over b, y, x of dy[b,c,y,x] x[b,c,y+t/3-1,x+t%3-1], fixed order.
 * ts_se_gate_fwd              plane_sum, gate [B][Cmid]; w_reduce [Cr][Cmid], b_reduce [Cr], w_expand [Cmid][Cr], b_expand [Cmid], all
 *                             dense; one launch of B x ceil(Cmid / 256) workgroups, each of which repeats the reduce step for its
 *                             batch element and then computes 256 gate channels.  A reduce row is read in 16-byte pieces when
 *                             Cmid % 4 == 0 and w_reduce is 16-byte aligned, an expand row when Cr % 4 == 0 and w_expand is: the
 *                             summation order of a row depends on those three facts (not on B), and so do its bits.
 * scale / shift (per output channel) may be NULL (1 / 0).  Tensors with strides have batch / channel strides in elements and dense
 * planes.  Checks, before any launch: sizes (TS_ERR_SHAPE: non-positive, mc outside [0, C], an unknown activation or flip, overlapping
 * strides), then C > 512, Cmid > 2048, Cr > 512, an axis >= 2^20, a plane >= 2^31 pixels, a grid that does not fit
 * (TS_ERR_UNSUPPORTED), then pointers (TS_ERR_NULL), then the alignment of w_l (TS_ERR_ALIGN), then the aliasing rules (ABI 24,
 * TS_ERR_SHAPE; "overlap" is judged on the operands' bounding extents, as for ts_conv3x3_s_fwd below):
 *   ts_mbconv_expand_fwd    y lies apart from memory and from input;
 *   ts_mbconv_project_fwd   y lies apart from x; y is either the residual's own elements (the same pointer and strides: the in-place
 *                           residual) or apart from it;
 *   ts_depthwise3x3_fwd     y lies apart from x.
 * ---------------------------------------------------------------------------------------- */
size_t ts_mbconv_weight_bytes(int Cin, int Cout);
int ts_mbconv_weight_layout(const float* w, float* w_l, int Cin, int Cout, void* stream);
int ts_mbconv_expand_fwd(const float* memory, const float* input, const float* w_l, const float* scale, const float* shift, float* y,
                         int B, int C, int mc, int Cmid, int H, int W, long long mem_bstride, long long mem_cstride,
                         long long in_bstride, long long in_cstride, long long y_bstride, long long y_cstride, void* stream);
int ts_mbconv_project_fwd(const float* x, const float* gate, const float* w_l, const float* scale, const float* shift,
                          const float* residual, float* y, int B, int Cmid, int C, int H, int W, long long x_bstride,
                          long long x_cstride, long long r_bstride, long long r_cstride, long long y_bstride, long long y_cstride,
                          void* stream);
int ts_depthwise3x3_fwd(const float* x, const float* w, const float* scale, const float* shift, float* y, float* plane_sum, int B,
                        int C, int H, int W, int act, int flip, long long x_bstride, long long x_cstride, long long y_bstride,
                        long long y_cstride, void* stream);
int ts_depthwise3x3_bwd_weight(const float* x, const float* dy, float* dw, int B, int C, int H, int W, long long x_bstride,
                               long long x_cstride, long long dy_bstride, long long dy_cstride, void* stream);
int ts_se_gate_fwd(const float* plane_sum, const float* w_reduce, const float* b_reduce, const float* w_expand, const float* b_expand,
                   float* gate, int B, int Cmid, int Cr, float inv_hw, void* stream);

/* ------------------------------------------------------------------------------------------
 * The encoder's large planes: the stem, block0's ConvBnAct members and the fused-MBConv (EdgeResidual) members of block1 / block2,
 * backbone/TemporalStereo.py:62-70,105-113, fp32 throughout, no atomics (ABI 23).  Eval forms:
 *   y = act(conv3x3(x, stride s, padding 1) * scale + shift) (+ residual)        ts_conv3x3_s_fwd        a ConvBnAct, the stem, a
 *                                                                                                        fused block's expansion
 *   y = conv1x1(x) * scale + shift (+ residual)                                  ts_fused_project_fwd    a fused block's projection
 * Both run on the f32-input MFMA through the cores of the decoder (3x3, blocked sums of 288 products) and of the memory block (1x1,
 * blocked sums of 256 products); an output's bits do not depend on the batch or the launch geometry.
 * ts_conv3x3_s_weight_layout  w [Cout][Cin][3][3] (contiguous) -> w_l, ts_conv3x3_s_weight_bytes(Cin, Cout, stride) bytes (0 outside the
 *                             envelope), 16-byte aligned; one launch.  stride 2: the image of the phase form -- a stride-1 3x3 over
 *                             the 4 Cin phase channels x[c, 2y + py, 2x + px] whose taps at offsets {-1, 0} carry the weights, zeros
 *                             elsewhere.  An image serves the stride it was made for only.
 * ts_conv3x3_s_fwd            x [B,Cin,H,W]; y and residual [B,Cout,ceil(H/s),ceil(W/s)]; s 1 | 2; act 0 none | 1 SiLU.  The residual is
 *                             added AFTER the activation and is accepted at s = 1 only (TS_ERR_SHAPE otherwise).  y OVERWRITTEN.
 * ts_fused_project_fwd        x [B,Cmid,H,W]; y and residual [B,Cout,H,W]; w_l is ts_mbconv_weight_layout's image of [Cout][Cmid].
 *                             y OVERWRITTEN.
 * Aliasing (both entries, TS_ERR_SHAPE): y may not overlap x, and y is either the residual's own elements (the same pointer and
 * strides) or apart from it.  "Overlap" is judged on the operands' bounding extents [p, p + (B - 1) bstride + (C - 1) cstride + plane):
 * two interleaved channel slices of one wider buffer are refused although they share no element.
 * scale / shift (per output channel) and residual may each be NULL (1 / 0 / nothing added).  Tensors have batch / channel strides in
 * elements and dense planes.  Checks, before any launch: sizes (TS_ERR_SHAPE: non-positive, another stride or activation, a residual
 * at stride 2, overlapping strides), then Cin (s = 1) or 4 Cin (s = 2) > 512, Cout > 512, Cmid > 2048, an axis >= 2^20, a grid that
 * does not fit (TS_ERR_UNSUPPORTED), then pointers (TS_ERR_NULL), then the alignment of w_l (TS_ERR_ALIGN), then the aliasing rule
 * (TS_ERR_SHAPE).
 * ---------------------------------------------------------------------------------------- */
size_t ts_conv3x3_s_weight_bytes(int Cin, int Cout, int stride);
int ts_conv3x3_s_weight_layout(const float* w, float* w_l, int Cin, int Cout, int stride, void* stream);
int ts_conv3x3_s_fwd(const float* x, const float* w_l, const float* scale, const float* shift, const float* residual, float* y, int B,
                     int Cin, int Cout, int H, int W, int stride, int act, long long x_bstride, long long x_cstride,
                     long long r_bstride, long long r_cstride, long long y_bstride, long long y_cstride, void* stream);
int ts_fused_project_fwd(const float* x, const float* w_l, const float* scale, const float* shift, const float* residual, float* y,
                         int B, int Cmid, int Cout, int H, int W, long long x_bstride, long long x_cstride, long long r_bstride,
                         long long r_cstride, long long y_bstride, long long y_cstride, void* stream);

/* K2c  the temporal state update of one frame, fused: update_map's closures update_local_map and
 * update_past_cost, projects/TemporalStereo/TemporalStereo.py:340-384 / :386-426, three launches.
 *   prev_disp  full-resolution disparity of the previous frame, [B,1,full_h,full_w] (disp_bstride elements
 *              between batch items); resized to (h,w) with value scale w/full_w  (:357-359)
 *   mem_disp / mem_cost [B,k,h,w]  top-k candidates and costs kept from the previous frame (k may be 0)
 *   local_map [B,n_local_in,h,w]   previous local maps (may be NULL when n_local_out <= 1);
 *              planes re-projected = [resized prev_disp | local_map][: n_local_out]      (:365-367)
 *   K [B,k_dim,k_dim] full-resolution intrinsics (rows 0,1 divided by `factor` = full_w / w inside; when 4x4 the
 *              last row must be 0 0 0 1); T = T_a * T_b (T_b NULL: T = T_a), [B,4,4]     (:333-338)
 *   baseline   per-item array [B] or NULL -> the scalar `baseline`
 *   out_disp / out_cost [B,k,h,w], out_local [B,n_local_out,h,w]: soft-max splat with metric
 *              clamp(d - mean(d), +-50) of the resized disparity (global mean, :374)     (:373-379, :415-419)
 * fp32 atomics in the splat: summation order not deterministic (as the reference's atomicAdd). */
size_t ts_reproject_memory_workspace_bytes(int B, int h, int w, int k, int n_local_out);
int ts_reproject_memory_fwd(const float* prev_disp, long long disp_bstride, int full_h, int full_w,
                            const float* mem_disp, const float* mem_cost, int k,
                            const float* local_map, int n_local_in, int n_local_out,
                            const float* K, int k_dim, const float* T_a, const float* T_b,
                            const float* baseline_ptr, float baseline, float factor,
                            float* out_disp, float* out_cost, float* out_local, void* workspace,
                            int B, int h, int w, void* stream);

/* ------------------------------------------------------------------------------------------
 * K3  3-D aggregation pyramid, inference form (BatchNorm folded into per-channel scale/shift,
 * activation fused: act 0 none, 1 SiLU, 2 ReLU, 3 tanh(x/100).clamp(-1,1)*act_param, 4 = channel 0 none and
 * channel 1 as 3 (both PredictionHeads outputs from one block-diagonal convolution, hw family only)).
 * Tensors may be channel slices of larger buffers: *_bstride / *_cstride are element strides of
 * the batch and channel axes.  Weights are pre-laid out by the host with the output channel
 * contiguous and zero-padded to ts_conv_cout_pad(Cout): [Cin][taps][CoutPad]; scale/shift [CoutPad].
 * ts_conv3d_hw_fwd: Conv3d (1,3,3) / ConvTranspose3d (1,3,3) of DepthwiseConv3D /
 *   DepthwiseConvTranspose3D (.../TemporalStereo/module.py:111-184) through the Conv3d wrappers
 *   (layers/basic_layers.py:194-235,340-388); also every 3x3 Conv2d (D = 1).
 * ts_conv3d_d_fwd: the (k,1,1) halves, Conv3d(5,1,1) of PyramidFusion (:408), Conv3d(3,1,1) of
 *   PredictionHeads (:369-378), 1x1 convolutions (k = 1).
 * ---------------------------------------------------------------------------------------- */
int ts_conv_cout_pad(int cout);
/* out[a][t][b] = b < nb ? w[a*stride_a + b*stride_b + (flip ? T-1-t : t)*stride_t] : 0, out [A][T][bpad]: the [Cin][taps][CoutPad]
 * layouts of ts_conv3d_*_fwd / *_bwd_data from a framework weight ([Cout][Cin][taps] or [Cin][Cout][taps]) in one launch. */
int ts_conv_weight_layout(const float* w, float* out, int A, int T, int nb, int bpad, long long stride_a, long long stride_b,
                          long long stride_t, int flip, void* stream);
/* The same for n weights in one launch (training: every convolution weight is re-laid once per optimizer update).
 * table: n entries in DEVICE memory; blocks_x: 256-thread workgroups per entry (grid-stride over larger entries). */
typedef struct {
  const float* w; float* out;
  int A, T, nb, bpad;
  long long stride_a, stride_b, stride_t;
  int flip, reserved;
} ts_weight_layout_desc;               /* 64 bytes */
int ts_conv_weight_layout_many(const void* table, int n, int blocks_x, void* stream);
/* General form (ABI 9): out[a*out_stride_a + t*out_stride_t + col0 + b] = w[a*stride_a + b*stride_b + (flip ? T-1-t : t)*stride_t] for
 * b < nb -- only those elements are written (padding is the caller's, zeroed once).  One entry per (destination region, source):
 * concatenations along Cout, block-diagonal pairs and re-pitched arrays are entries over the framework's own parameters, so an
 * inference engine re-folds ALL its kernel-layout weights after an optimizer step in one launch (aggregation/native.py Tape). */
typedef struct {
  const float* w; float* out;
  int A, T, nb, col0;
  long long stride_a, stride_b, stride_t;
  long long out_stride_a, out_stride_t;
  int flip, reserved;
} ts_weight_layout_desc2;              /* 80 bytes */
int ts_conv_weight_layout_many2(const void* table, int n, int blocks_x, void* stream);
/* Deferred finishes of ts_conv3d_{hw,d}_bwd_weight (ABI 9): between ts_conv_wgrad_defer(1) and (0) the calls ON THIS HOST THREAD leave
 * their partial sums in the caller's workspaces -- which must stay alive -- and dw unwritten; ts_conv_wgrad_take moves the kept
 * descriptors into a HOST table (48 bytes each), which the caller copies to the device and hands to ts_conv_wgrad_finish_many: one
 * launch sums every layer's partials (same sums, same order as the per-layer finish).  A training step saves ~95 launches with it. */
typedef struct { const float* part; float* dw; int gx, nitems, cob, Cin, Cout, KT, ciblocks, block0; } ts_wgrad_finish_desc;   /* 48 bytes */
int ts_conv_wgrad_defer(int on);           /* returns the previous setting */
int ts_conv_wgrad_pending(void);
int ts_conv_wgrad_take(void* host_table, size_t capacity_bytes, int* n, int* total_blocks);
int ts_conv_wgrad_finish_many(const void* table, int n, int total_blocks, void* stream);
/* Upper bound (8 | 16 | 32, default 32) on the input-channel chunk -- hence the LDS footprint -- of the
 * convolution launches that follow on this host thread: short chunks when kernels of several streams
 * should share the CUs, long chunks for a lone dependent chain.  Recordable in a plan. */
int ts_conv_set_chunk_cap(int cap);
int ts_conv3d_hw_fwd(const float* x, const float* w_t, const float* scale, const float* shift, float* y,
                     int B, int Cin, int Cout, int D, int H, int W, int stride, int dilation,
                     int transposed, int act, float act_param,
                     long long in_bstride, long long in_cstride, long long out_bstride,
                     long long out_cstride, const float* addend, long long addend_bstride,
                     void* workspace, size_t workspace_bytes, void* stream);
/* addend (may be NULL): [B, Cout, Ho, Wo] (batch stride addend_bstride elements), added to the raw sum of
 * EVERY depth plane before scale / shift / activation -- the D-invariant part of a convolution over a
 * volume whose leading channels are a broadcast (see ts_block_cost_sampled_warped_fwd). */
/* ABI 6 -- the first (1,3,3) layer of a sampled level without its warped input volume (reference
 * precise.py:88-91, fine.py:96-103 over block_cost.py:47-81).  The warp of block_cost's sampled path is a two-tap interpolation along
 * x whose weights do not depend on the channel, and the convolution contracts over channels, so the two commute:
 *     sum_c W[co][c][t] warp(right)[c][d][p]  ==  lerp(Q[t*Cout + co][row of p], x_p - disp[d][p]),
 *     Q[t*Cout + co] = sum_c W[co][C + c][t] right[c]      (a 1x1 convolution, [B, 9*Cout, H, W], made with ts_conv3d_d_fwd, k = 1)
 * i.e. layer(cat[left x D | warp | corr]) = act(scale * (conv_{W[:, 2C:]}(corr) + T) + shift),
 *     T[co][d][y][x] = base[co][y][x] + sum_{t=(ky,kx)} lerp(Q[t*Cout+co][y+(ky-1)dil], x+(kx-1)dil - disp[d][y+(ky-1)dil][x+(kx-1)dil])
 * with zero for tap pixels outside the image (the convolution's padding) and for columns outside the row (the warp's padding).
 *   corr [B,Cc,D,H,W] (ts_block_cost_sampled_corr_fwd), w_t [Cc][9][CoutPad], scale/shift [CoutPad], q [B,9*Cout,H,W] dense,
 *   disp [B,D,H,W] dense, base [B,Cout,H,W] (the left term conv_{W[:, :C]}(left), or NULL), y [B,Cout,D,H,W].
 *   workspace: ts_conv3d_hw_warp_workspace_bytes(B, Cout, D, H, W) bytes (T).  Strides in elements as for ts_conv3d_hw_fwd. */
size_t ts_conv3d_hw_warp_workspace_bytes(int B, int Cout, int D, int H, int W);
int ts_conv3d_hw_warp_fwd(const float* corr, const float* w_t, const float* scale, const float* shift, float* y,
                          const float* q, const float* disp, const float* base,
                          int B, int Cc, int Cout, int D, int H, int W, int dilation, int act, float act_param,
                          long long in_bstride, long long in_cstride, long long out_bstride, long long out_cstride,
                          long long base_bstride, void* workspace, size_t workspace_bytes, void* stream);

/* scratch ts_conv3d_hw_fwd can use to split a long reduction over more workgroups (0 = never splits at
 * this shape; passing NULL / too little simply disables the split) */
size_t ts_conv3d_hw_workspace_bytes(int B, int Cin, int Cout, int D, int H, int W, int stride, int transposed);
/* The stride-1 (1,3,3) convolution with every fp32 product assembled from bf16 pieces on the bf16 matrix pipe:
 * a = a0 + a1 + a2 (bf16 parts), a*b ~= a0b0 + a0b1 + a1b0 + a1b1 + a0b2 + a2b0, fp32 accumulation -- dropped terms are below
 * 2^-24 of the product, every 16-channel chunk summed apart and added to the running sum in fp32; measured max error against an
 * fp64 convolution 0.15e-6 ... 0.26e-6 of the output's magnitude for Cin 16 ... 512 (ts_conv3d_hw_fwd's f32 MFMA chain: 0.3e-6
 * ... 0.7e-6; tests/test_conv_x6_gpu.py), at 3/8 of its matrix time (f32-input MFMA = 1/16 of the bf16 rate on gfx950).
 *   ts_conv3d_hw_x6_supported     1 when the layer can take this path (Cin >= 16, 8 < Cout <= 512, W % 4 == 0, stride 1, dilation 1 | 2)
 *   ts_conv3d_hw_x6_weight_split  w_t (the [Cin][9][CoutPad] array of ts_conv3d_hw_fwd) -> w6, ts_conv3d_hw_x6_weight_bytes
 *                                 bytes: [Cin/16][part 3][tap slot 10][group 2][CoutPad][8] bf16
 *   ts_conv3d_hw_x6_fwd           arguments as ts_conv3d_hw_fwd with stride 1, not transposed; workspace (ABI 5): scratch of
 *                                 ts_conv3d_hw_x6_workspace_bytes bytes for the split-K form of small grids (a grid of a few dozen
 *                                 workgroups is cut into 2 | 4 | 8 slices of the input channels, summed in a fixed order by a second
 *                                 launch); NULL / too little: unsplit */
int ts_conv3d_hw_x6_supported(int Cin, int Cout, int W, int stride, int dilation, int transposed);
size_t ts_conv3d_hw_x6_weight_bytes(int Cin, int Cout);
size_t ts_conv3d_hw_x6_workspace_bytes(int B, int Cin, int Cout, int D, int H, int W);
int ts_conv3d_hw_x6_weight_split(const float* w_t, void* w6, int Cin, int Cout, void* stream);
/* ... the same from the FRAMEWORK's weight in one launch (ABI 9; training re-splits per call): element (ci, co, tap) of the
 * convolution being run = w[ci*stride_ci + co*stride_co + tap*stride_t], taps reversed when flip (input gradient of a stride-1 layer) */
int ts_conv3d_hw_x6_weight_split_from(const float* w, void* w6, int Cin, int Cout, long long stride_ci, long long stride_co,
                                      long long stride_t, int flip, void* stream);
int ts_conv3d_hw_x6_fwd(const float* x, const void* w6, const float* scale, const float* shift, float* y,
                        int B, int Cin, int Cout, int D, int H, int W, int dilation, int act, float act_param,
                        long long in_bstride, long long in_cstride, long long out_bstride, long long out_cstride,
                        const float* addend, long long addend_bstride, void* workspace, size_t workspace_bytes, void* stream);
/* Small-message exchange between the ranks of one node as kernels over peer-mapped (hipIpc, xGMI) memory (ABI 8; csrc/peer.hip):
 * the statistics exchanges of SyncBatchNorm (reference: Lightning's sync_batchnorm=True, projects/TemporalStereo/dist_train.py:94)
 * without a communicator launch per layer, and capturable in a hipGraph.  Set-up: every rank ts_peer_alloc()s its mailbox, the
 * 64-byte handles travel through any out-of-band channel (torch.distributed all_gather), every rank ts_peer_open()s the others and
 * fills a ts_peer_ctx.  All ranks must issue the same sequence of exchanges.  At most ts_peer_max_floats() floats per exchange. */
typedef struct ts_peer_ctx {
  void* region[8];        /* mailbox of rank r as mapped in this process (region[rank]: the local allocation) */
  int rank, world;
} ts_peer_ctx;
size_t ts_peer_region_bytes(void);
int ts_peer_max_floats(void);
int ts_peer_max_ranks(void);
int ts_peer_alloc(void** region, void* handle64);
int ts_peer_open(const void* handle64, void** region);
int ts_peer_close(void* region);
int ts_peer_free(void* region);
/* status: 0, or 1 + r when rank r did not answer an exchange within the bound (that exchange's results and every later one's are
 * undefined until ts_peer_reset).  ts_peer_status synchronises the stream; ts_peer_status_async (ABI 9) copies the word into PINNED
 * host memory behind the queued work, to be read once an event recorded after the call has completed. */
int ts_peer_status(const void* ctx, int* status, void* stream);
int ts_peer_status_async(const void* ctx, int* host_status, void* stream);
/* bound of one wait in milliseconds (default 120 000, or TS_PEER_TIMEOUT_MS); returns the previous one; ms <= 0 only queries */
long long ts_peer_set_timeout_ms(long long ms);
/* clears this rank's flags / sequence number / err word; every rank calls it, nothing in flight, between two barriers */
int ts_peer_reset(const void* ctx, void* stream);
/* dst [world][n] <- every rank's src [n] */
int ts_peer_all_gather(const void* ctx, const float* src, float* dst, int n, void* stream);
/* buf [n] <- (sum over the ranks in rank order: bit-identical everywhere) * (*scale, a device scalar, if not NULL) */
int ts_peer_all_reduce_sum(const void* ctx, float* buf, int n, const float* scale, void* stream);

/* The same bf16-split arithmetic for the STRIDED and TRANSPOSED forms (ABI 7; csrc/conv_x6s.hip), which ts_conv3d_hw_fwd /
 * ts_deconv2d_k4s2_fwd run on the f32-input MFMA.  mode 0: Conv3d (1,3,3) stride 2, padding 1 (Ho = (H-1)/2+1);  mode 1:
 * ConvTranspose3d (1,3,3) stride 2, padding 1, output_padding 1 (Ho = 2H);  mode 2: ConvTranspose2d 4x4 stride 2, padding 1
 * (D = 1, Ho = 2H) -- reference: aggregation/TemporalStereo/module.py:111-184,453-457.  K chunks of 8 input channels, four taps per MFMA.
 *   ts_conv3d_hw_x6s_supported     1 when the layer can take this path (Cin >= 16, Cout <= 512, W % 4 == 0, Wo % 4 == 0)
 *   ts_conv3d_hw_x6s_weight_split  w_t [Cin][9 | 16][w_pad] (the array of ts_conv3d_hw_fwd / ts_deconv2d_k4s2_fwd) -> w6,
 *                                  ts_conv3d_hw_x6s_weight_bytes bytes: [Cin/8][part 3][tap slot 12 | 16][Cout up to 16][8] bf16
 *   ts_conv3d_hw_x6s_fwd           scale / shift [>= Cout] or NULL; strides in elements (x / y may be channel slices) */
int ts_conv3d_hw_x6s_supported(int Cin, int Cout, int H, int W, int mode);
size_t ts_conv3d_hw_x6s_weight_bytes(int Cin, int Cout, int mode);
int ts_conv3d_hw_x6s_weight_split(const float* w_t, void* w6, int Cin, int Cout, int w_pad, int mode, void* stream);
int ts_conv3d_hw_x6s_fwd(const float* x, const void* w6, const float* scale, const float* shift, float* y,
                         int B, int Cin, int Cout, int D, int H, int W, int mode, int act, float act_param,
                         long long in_bstride, long long in_cstride, long long out_bstride, long long out_cstride, void* stream);
/* ABI 19 -- ts_conv3d_hw_x6s_fwd (mode 2, D = 1, no activation, 9 <= Cout <= 16) followed by ts_unet_upsample_fwd on its first nine
 * output planes, as one launch: x [B,Cin,H,W] with H = 2h, W = 2w even; disp [B,1,h,w]; out [B,1,4h,4w].  The logit planes stay in
 * the workgroup's LDS.  Bit-identical to the two launches.  Anything else: TS_ERR_UNSUPPORTED. */
int ts_deconv2d_k4s2_unet_upsample_fwd(const float* x, const void* w6, const float* scale, const float* shift,
                                       const float* disp, float* out, int B, int Cin, int Cout, int H, int W,
                                       long long in_bstride, long long in_cstride, void* stream);
int ts_conv3d_d_fwd(const float* x, const float* w_t, const float* scale, const float* shift, float* y,
                    int B, int Cin, int Cout, int Din, int H, int W, int k, int stride, int dilation,
                    int padding, int transposed, int act, float act_param,
                    long long in_bstride, long long in_cstride, long long out_bstride,
                    long long out_cstride, void* stream);
/* Backward of the two families (training: raw convolutions; BatchNorm / activation stay framework ops in
 * train mode because they need batch statistics).  Geometry arguments always describe the FORWARD call.
 * scale / shift of the forward entries may be NULL (= 1 / 0): that is the raw convolution these invert.
 *   bwd_data  : dy (forward output shape) -> dx (forward input shape).  w_b is the weight re-laid by the host,
 *               [Cout][taps][ts_conv_cout_pad(Cin)]: taps flipped for a stride-1 forward, unflipped for a
 *               stride-2 forward (runs as the transposed form, cropped to the input size) and for a
 *               transposed forward (runs as a stride-2 convolution of dy).
 *   bwd_weight: x, dy -> dw [Cout][Cin][taps] in the framework's layout, OVERWRITTEN.  Every workgroup
 *               leaves its partial sums in `workspace` (ts_conv3d_bwd_weight_workspace_bytes(Cin, Cout,
 *               taps) bytes, taps = 9 | k; contents undefined afterwards) and a second launch adds them in a
 *               fixed order: the result is deterministic (no atomics).  Cout <= 64.
 *               Transposed forward: call with x := dy, dy := x, stride 2 -> [Cin][Cout][taps]
 *               (and size the workspace with the exchanged channel counts). */
size_t ts_conv3d_bwd_weight_workspace_bytes(int Cin, int Cout, int taps);
int ts_conv3d_hw_bwd_data(const float* dy, const float* w_b, float* dx, int B, int Cin, int Cout, int D, int H, int W,
                          int stride, int dilation, int transposed, long long dy_bstride, long long dy_cstride,
                          long long dx_bstride, long long dx_cstride, void* stream);
int ts_conv3d_hw_bwd_weight(const float* x, const float* dy, float* dw, int B, int Cin, int Cout, int D, int H, int W,
                            int stride, int dilation, long long x_bstride, long long x_cstride, long long dy_bstride,
                            long long dy_cstride, void* workspace, size_t workspace_bytes, void* stream);
int ts_conv3d_d_bwd_data(const float* dy, const float* w_b, float* dx, int B, int Cin, int Cout, int Din, int H, int W,
                         int k, int stride, int dilation, int padding, int transposed, long long dy_bstride,
                         long long dy_cstride, long long dx_bstride, long long dx_cstride, void* stream);
int ts_conv3d_d_bwd_weight(const float* x, const float* dy, float* dw, int B, int Cin, int Cout, int Din, int H, int W,
                           int k, int stride, int dilation, int padding, long long x_bstride, long long x_cstride,
                           long long dy_bstride, long long dy_cstride, void* workspace, size_t workspace_bytes,
                           void* stream);
/* ResidualBlock3D up-steps: out = act(trilinear_align_corners(a -> (D,H,W)) + add)  module.py:285-295 */
int ts_resize3d_add_act_fwd(const float* a, const float* add, float* out, int B, int C, int Da, int Ha, int Wa,
                            int D, int H, int W, int act, long long a_bstride, long long a_cstride,
                            long long add_bstride, long long add_cstride, long long out_bstride,
                            long long out_cstride, void* stream);
/* PyramidFusion pooling branch: avg_pool3d + max_pool3d, kernel 5, stride 1, padding 2  module.py:415-417 */
int ts_pool3d5_avgmax_fwd(const float* x, float* out_avg, float* out_max, int B, int C, int D, int H, int W,
                          long long x_bstride, long long x_cstride, long long avg_bstride, long long avg_cstride,
                          long long max_bstride, long long max_cstride, void* stream);
/* temporal merge: past_conv(1->C)+BN+SiLU on the K memory costs, cat along D, stable sort of the
 * D0+K candidates, gather of the volume  coarse.py:84-105 / fine.py:105-122.  sample NULL = 0..D0-1;
 * mem_sample / mem_cost NULL = zeros. */
int ts_merge_candidates_fwd(const float* volume, const float* sample, const float* mem_sample, const float* mem_cost,
                            const float* past_w, const float* past_scale, const float* past_shift,
                            float* out_sample, float* out_volume, int B, int C, int D0, int K, int H, int W,
                            long long vol_bstride, long long vol_cstride, long long out_bstride,
                            long long out_cstride, void* stream);
/* K5 upsamplers: ConvexUpsample.forward module.py:336-353 (mask [B,9*f*f,H,W]); UNet.upsample :468-482
 * (mask [B,9,Ho,Wo]); ConvTranspose2d(4, stride 2, padding 1) of UNet :453-457 (w_t [Cin][4][4][CoutPad],
 * CoutPad = ts_conv_cout_pad(Cout) = 8 | 16 | 32 as for every other convolution entry since ABI 9; up to ABI 8 this entry
 * alone wanted 16 | 32, which its own training-side caller did not honour for Cout <= 8); bilinear align_corners resize
 * with a value scale. */
int ts_convex_upsample_fwd(const float* mask, const float* disp, float* out, int B, int H, int W, int factor,
                           float disp_scale, void* stream);
/* ts_convex_upsample_fwd + ts_range_candidates_fwd (on the upsampled map) as one launch */
int ts_convex_upsample_candidates_fwd(const float* mask, const float* disp, float* out, float* low, float* high,
                                      float* candidates, int B, int H, int W, int factor, float disp_scale, float range,
                                      int channel_offset, int channels_total, void* stream);
int ts_unet_upsample_fwd(const float* mask, const float* disp, float* out, int B, int h, int w, int Ho, int Wo,
                         void* stream);
/* Backward of the two upsamplers (training form).  grad_out has the output's shape; grad_mask / grad_disp are OVERWRITTEN
 * (ts_convex_upsample_bwd: either may be NULL; ts_unet_upsample_bwd: grad_disp may be NULL; workspace B*9*Ho*Wo floats).
 * Gather formulations: deterministic, no atomics. */
int ts_convex_upsample_bwd(const float* mask, const float* disp, const float* grad_out, float* grad_mask, float* grad_disp,
                           int B, int H, int W, int factor, float disp_scale, void* stream);
int ts_unet_upsample_bwd(const float* mask, const float* disp, const float* grad_out, float* grad_mask, float* grad_disp,
                         void* workspace, int B, int h, int w, int Ho, int Wo, void* stream);
int ts_deconv2d_k4s2_fwd(const float* x, const float* w_t, const float* scale, const float* shift, float* y,
                         int B, int Cin, int Cout, int H, int W, int act, long long out_bstride, void* stream);
int ts_resize_bilinear_fwd(const float* x, float* out, int B, int C, int h, int w, int Ho, int Wo, float value_scale,
                           long long out_bstride, void* stream);
/* two same-shaped dense maps in one launch (the top-k memory's candidates and costs, precise.py:100-103, coarse.py:91-96) */
int ts_resize_bilinear_pair_fwd(const float* x0, const float* x1, float* out0, float* out1, int B, int C, int h, int w,
                                int Ho, int Wo, float value_scale0, float value_scale1, void* stream);
/* search range of the next level and its five candidates from an upsampled disparity:
 * low = d - range, high = d + range (aggregation/TemporalStereo/TemporalStereo.py:110,119);
 * candidates[:, off+i] = |high-low| * {0,3,4,5,8}/8 + min(low,high)  (fine.py:82-87, precise.py:73-78) */
int ts_range_candidates_fwd(const float* disp, float* low, float* high, float* candidates, int B, int H, int W,
                            float range, int channel_offset, int channels_total, void* stream);

/* Backward of the element stages (training; dense NCDHW tensors, outputs OVERWRITTEN, fp32 atomics where a
 * gradient is a scatter -- the same non-deterministic order as the framework's own backward kernels):
 *   resize3d_add_act_bwd : d out / d(a, add) of ts_resize3d_add_act_fwd (grad_add may be NULL)
 *   pool3d5_avgmax_bwd   : grad_x = box5^3(grad_avg)/125 + grad_max routed to each window's arg-max
 *                          (first occurrence in (d,y,x) order, as max_pool3d_with_indices)
 *   merge_candidates_bwd : the sort + gather half of ts_merge_candidates_fwd (its K = 0 form):
 *                          grad_volume[:, j] = grad_out_volume[:, rank_j], likewise the samples */
int ts_resize3d_add_act_bwd(const float* a, const float* add, const float* grad_out, float* grad_a, float* grad_add,
                            int B, int C, int Da, int Ha, int Wa, int D, int H, int W, int act, void* stream);
int ts_pool3d5_avgmax_bwd(const float* x, const float* grad_avg, const float* grad_max, float* grad_x,
                          int B, int C, int D, int H, int W, void* stream);
int ts_merge_candidates_bwd(const float* sample, const float* grad_out_volume, const float* grad_out_sample,
                            float* grad_volume, float* grad_sample, int B, int C, int DT, int H, int W, void* stream);

/* dst[r * dst_pitch + c] = src[r * src_pitch + c] (elements): writes a tensor into a channel slice of
 * another -- the torch.cat / slice.copy_ of precise.py:60-63 and module.py:486-489 without torch. */
/* Channel splice of the backbone's per-frame feature memory (architecture/modeling/backbone/TemporalStereo.py:
 * 183-197: `torch.cat([memory, input[:, mc:]], 1)` in front of every residual block):
 *   out[b][c] = c < mc ? first[b][c] : second[b][c];  first [B, mc, N] (NULL = zeros: the adjoint towards `input`), second / out
 *   [B, C, N]; *_bstride in elements. */
int ts_channel_splice_fwd(const float* first, const float* second, float* out, int B, int C, int mc, long long N,
                          long long first_bstride, long long second_bstride, long long out_bstride, void* stream);
int ts_copy_rows_fwd(const float* src, float* dst, long long rows, long long row_elems, long long src_pitch,
                     long long dst_pitch, void* stream);

/* ------------------------------------------------------------------------------------------
 * Training-side glue (csrc/train_ops.hip): the element-wise steps around the levels that the framework otherwise runs
 * as ~280 tiny launches per training step, the pieces that run the UNet decoder's ConvTranspose2d(4, stride 2, padding 1)
 * (module.py:453-457) on the convolution kernels in training, and the optimizer step.
 *   candidates_in_range : candidates[:, off+i] = |high-low| * {0,3,4,5,8}/8 + min(low,high) (fine.py:82-87, precise.py:73-78)
 *                         from separate low / high maps [B,1,H,W]; bwd: d/d low, d/d high (|.|' = sign, min' split at ties)
 *   offset_head         : y = clamp(tanh(x/100), -1, 1) * delta  (PredictionHeads.regress_offset, module.py:384-390)
 *   space_to_depth2     : z[b][(py*2+px)*C + c][y][x] = x[b][c][2y+py][2x+px]   (x [B,C,2H,2W] -> z [B,4C,H,W])
 *   deconv2d_k4s2_weight_to_conv3 : w [Cin][Cout][4][4] -> out [(4*Cout)][9][cin_pad], the ts_conv3d_hw_fwd weight of the 3x3
 *                         stride-1 convolution of space_to_depth2(dy) that is d/dx of the transposed convolution
 *   deconv2d_k4s2_wgrad_from_conv3: dw3 [Cin][4*Cout][9] (ts_conv3d_hw_bwd_weight of that convolution) -> dw [Cin][Cout][4][4]
 *   clip_rmsprop_step   : clip_grad_norm_(max_norm) + RMSprop(lr, alpha, eps; no momentum / centring / weight decay) over
 *                         a DEVICE table of ts_opt_entry; two launches, deterministic; workspace's last float <- total norm
 * ---------------------------------------------------------------------------------------- */
typedef struct ts_opt_entry { float* param; const float* grad; float* square_avg; long long n; } ts_opt_entry;
int ts_candidates_in_range_fwd(const float* low, const float* high, float* candidates, int B, int H, int W,
                               int channel_offset, int channels_total, void* stream);
int ts_candidates_in_range_bwd(const float* low, const float* high, const float* grad_candidates, float* grad_low,
                               float* grad_high, int B, int H, int W, int channel_offset, int channels_total, void* stream);
int ts_offset_head_fwd(const float* x, float* y, long long n, float delta, void* stream);
int ts_offset_head_bwd(const float* x, const float* grad_y, float* grad_x, long long n, float delta, void* stream);
int ts_space_to_depth2_fwd(const float* x, float* z, int B, int C, int H, int W, void* stream);
int ts_deconv2d_k4s2_weight_to_conv3(const float* w, float* out, int Cin, int Cout, int cin_pad, void* stream);
int ts_deconv2d_k4s2_wgrad_from_conv3(const float* dw3, float* dw, int Cin, int Cout, void* stream);
/* eval-mode BatchNorm folded into the convolution epilogue for a whole step in one launch: table = n ts_bn_fold_entry in DEVICE memory;
 * scale[c] = gamma / sqrt(var + eps), shift[c] = beta + (bias - mean) * scale for c < C, 0 for C <= c < pad (gamma / beta / bias may be NULL;
 * mean / var NULL (ABI 9) = no BatchNorm behind the convolution: scale 1, shift = bias) */
typedef struct ts_bn_fold_entry { const float* gamma; const float* beta; const float* mean; const float* var; const float* bias;
                                  float* scale; float* shift; int C, pad; } ts_bn_fold_entry;
int ts_bn_fold_many(const void* table, int n, float eps, void* stream);
size_t ts_clip_rmsprop_workspace_bytes(int n_tensors);
int ts_clip_rmsprop_step(const void* table, int n_tensors, float max_norm, float lr, float alpha, float eps,
                         void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Native replay runtime (no reference counterpart; the reference runs eagerly under PyTorch).
 * A plan is the recorded sequence of launching calls of one pass -- device pointers, shapes and
 * streams baked in, the contract of a CUDA graph with static buffers -- re-issued by one host call.
 * ts_plan_add_call: `name` is one of the int-returning launch entry points above, `words` holds its
 * arguments in order, one 64-bit word each (ints / floats in the low bytes).
 * ts_stream_fork: to_stream waits for the work enqueued so far on from_stream.
 * ---------------------------------------------------------------------------------------- */
typedef struct ts_plan ts_plan;
ts_plan* ts_plan_create(void);
void ts_plan_destroy(ts_plan* plan);
int ts_plan_length(const ts_plan* plan);
int ts_plan_add_call(ts_plan* plan, const char* name, const unsigned long long* words, int n_words);
int ts_plan_run(ts_plan* plan);
int ts_stream_fork(void* from_stream, void* to_stream);
/* Named events (slot 0..255): record on one stream now, wait from another stream in a LATER call (an edge that spans
 * replays: "the pass that last used these buffers is done").  Waiting on a never-recorded slot is a no-op. */
int ts_event_record(int slot, void* stream);
int ts_event_wait(int slot, void* stream);

/* ------------------------------------------------------------------------------------------
 * Measurement support (no reference counterpart): float4 streams used by bench.py to calibrate
 * what this box sustains.  kind 0 = fill dst (write-only), 1 = copy src->dst, 2 = read src
 * (dst = 4-byte sink).  nbytes % 16 == 0.
 * ---------------------------------------------------------------------------------------- */
int ts_calib_stream(int kind, void* dst, const void* src, size_t nbytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TS_HIP_H */
