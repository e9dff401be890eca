/*
 * lanefit.h -- C ABI of liblanefit_hip.so, the MI355X (gfx950) implementation of the
 * LaneDetection_End2End hot path: ERFNet backbone -> weighted-least-squares lane fit ->
 * area / back-projection / segmentation losses, forward and backward.
 *
 * The reference has no FFI boundary of its own (it is pure PyTorch): its
 * operator API is the nn.Module surface.  Each entry point below therefore names the
 * reference nn.Module / function it replaces (file:line under /root/reference, with
 * BEV/ = Birds_Eye_View_Loss/, BP/ = Backprojection_Loss/).  The Python host layer in
 * lanedetection_end2end_amd/ binds these with ctypes (INTEGRATION.md shows the stub).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless its name ends in _host;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream);
 *   - plain C types only: no torch / ATen / HIP types in any signature;
 *   - return value: 0 = launches enqueued, <0 = argument error (lf_last_error() has text).
 *     Numerical failure (singular normal matrix) is reported asynchronously through a
 *     device-side `status` word the caller reads back (1 = singular, 2 = not positive
 *     definite) so that the host can raise RuntimeError like torch.inverse does
 *     (BEV/main.py:213-219 catches exactly that);
 *   - activation tensors inside the backbone are NHWC fp32; the module boundary
 *     (input image, logits, weight maps) is NCHW fp32 as in the reference.
 */
#ifndef LANEFIT_H
#define LANEFIT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LF_ABI_VERSION 5      /* 5 (round 6): lf_erfnet_workspace_bytes_for added; lf_erfnet_set_precision refuses the removed modes 1 and 4;
                                 lf_erfnet_forward_range / _backward_range take precision mode 2.
                                 Later ADDITIONS that leave every existing entry point's contract as it was keep the number:
                                 lf_convchain_set_precision / _workspace_bytes_for, lf_poolflat_bf16_*, lf_pointwise_bf16_*, and
                                 lf_erfnet_backward's grad_encoder in mode 2 (the --clas heads and only_encode in bf16);
                                 additions since 5 (inference engine): lf_erfnet_infer*, lf_erfnet_infer_range*, lf_convchain_infer*,
                                 lf_head_fit, lf_lane_infer*;
                                 additions since 5 (homography through the fit): lf_theta_grid, lf_theta_grid_bwd*, lf_wls_fwd_theta,
                                 lf_wls_bwd_theta*, lf_wls_bwd_grid;
                                 additions since 5 (scoring of decoded lanes): lf_lane_eval;
                                 additions since 5 (whole-step criterion): lf_step_loss, lf_step_loss_workspace_bytes, lf_step_loss_bwd;
                                 additions since 5 (BEV lane decoding): lf_lane_decode_bev;
                                 additions since 5 (segmentation-mode step criterion): lf_seg_step, lf_seg_step_workspace_bytes,
                                 lf_seg_step_bwd;
                                 additions since 5 (resident dataset's label batch): lf_label_batch_bp, lf_label_batch_bev;
                                 additions since 5 (gradient-norm clipping): lf_grad_norm_workspace_bytes, lf_grad_sumsq,
                                 lf_grad_norm_finish, lf_grad_scale_inplace, lf_adam_step_clipped, lf_sgd_step_clipped,
                                 lf_rmsprop_step_clipped;
                                 additions since 5 (segmentation-mode detect): lf_head_fit_seg, lf_lane_infer_seg_workspace_bytes,
                                 lf_lane_infer_seg;
                                 additions since 5 (input-image gradient): lf_stem_bwd_data, lf_erfnet_backward_input (and
                                 lf_erfnet_backward_range writes a non-NULL gx for first = 0);
                                 additions since 5 (frozen single-frame detector): lf_erfnet_infer_fold, lf_lane_infer_folded,
                                 lf_lane_infer_seg_folded;
                                 additions since 5 (frozen --clas heads): lf_convchain_infer_fold, lf_convchain_infer_folded,
                                 lf_clas_tail_workspace_bytes, lf_clas_tail;
                                 additions since 5 (camera frames): lf_pipeline_frame_stem_ok, lf_pipeline_frame_stem_lds_bytes,
                                 lf_pipeline_frame_stem_tile, lf_lane_infer_u8_workspace_bytes, lf_lane_infer_seg_u8_workspace_bytes,
                                 lf_lane_infer_folded_u8, lf_lane_infer_seg_folded_u8;
                                 additions since 5 (frame formats): lf_pipeline_plan_set_format, lf_pipeline_frame_bytes;
                                 additions since 5 (surfaces): lf_pipeline_plan_set_layout, lf_pipeline_surface_span */

/* activation applied to the backbone logits: BEV/Networks/LSQ_layer.py:43-63 */
enum { LF_ACT_SQUARE = 0, LF_ACT_ABS = 1, LF_ACT_RELU = 2, LF_ACT_SIGMOID = 3,
       LF_ACT_SOFTPLUS = 4, LF_ACT_NONE = 5 };
/* normal-equation solver: torch.inverse path (LSQ_layer.py:128-130) or GELS/Cholesky (BP/Networks/gels.py) */
enum { LF_SOLVE_LU = 0, LF_SOLVE_CHOLESKY = 1 };
/* Area_Loss weightings: BEV/Loss_crit.py:103-121 */
enum { LF_WF_NONE = 0, LF_WF_LINEAR = 1, LF_WF_QUADRATIC = 2 };
enum { LF_F32 = 0, LF_F64 = 1 };

int lf_abi_version(void);
const char* lf_last_error(void);

/* ------------------------------------------------------------------------------------
 * Fitting head.  Replaces Net.forward steps 2-4 (activation, row mask, grid, WLS):
 * BEV/Networks/LSQ_layer.py:310-325 and Weighted_least_squares.forward :103-167
 * (BP/Networks/LSQ_layer.py:85-154), plus the GELS option (BP/Networks/gels.py:10-15).
 *
 *   logits   (N,K,H,W) fp32 NCHW backbone output `output`
 *   grid_xy  (H*W,2) fp32 (x', y') of every pixel; grid_batch_stride = 0 when shared by
 *            all images (always the case in the reference), else floats between images
 *   zero_rows  rows [0,zero_rows) of every map are masked to 0 (LSQ_layer.py:257-258,316)
 *   order 0..3, reg = --reg_ls added to the diagonal for BOTH solvers (BEV adds it before either factorisation,
 *     LSQ_layer.py:120-126; BP's GELS has no regulariser, gels.py:10-15: its caller passes reg = 0),
 *     y_offset = 1 (BEV :109) or 255 (BP :94)
 *   beta     out (N,K,order+1) fp64, coefficients highest power first
 *   zinv     out (N,K,(order+1)^2) fp64, (Y0^T Y0 + reg I)^-1 -- saved for backward
 *   masked   out (N,K,H,W) fp32 weight maps after activation+mask, or NULL to skip
 *   partials workspace, >= lf_wls_workspace_bytes(N,K,order) bytes
 *   status   out (N*K) int32: 0 ok, 1 singular, 2 not positive definite
 * ---------------------------------------------------------------------------------- */
size_t lf_wls_workspace_bytes(int N, int K, int order);
int lf_wls_fwd(const float* logits, const float* grid_xy, long grid_batch_stride,
               int N, int K, int H, int W, int zero_rows, int order, double reg,
               double y_offset, int act_kind, int solver,
               double* beta, double* zinv, float* masked, void* partials, int32_t* status,
               void* stream);
/* d loss / d logits from d loss / d beta (autograd of the bmm/inverse chain; gels.py:17-25).
 *   grad_beta (N,K,order+1) fp64; lanes whose beta received no gradient pass zeros.
 *   grad_logits out (N,K,H,W) fp32 (masked rows are written as 0). */
int lf_wls_bwd(const float* logits, const float* grid_xy, long grid_batch_stride,
               int N, int K, int H, int W, int zero_rows, int order, double y_offset,
               int act_kind, const double* beta, const double* zinv, const double* grad_beta,
               float* grad_logits, void* stream);

/* GELS.forward / GELS.backward -- BP/Networks/gels.py:9-25: x = (A^T A)^-1 A^T b by Cholesky of the normal
 * equations (no regulariser) and the hand-written backward of the reference.
 *   A (N,P,D) fp32, b (N,P) fp32, D <= 4; x out (N,D) fp32; zinv out (N,D,D) fp64 (saved for backward);
 *   partials >= lf_gels_workspace_bytes(N,D); status out (N) int32 (2 = not positive definite).
 *   backward: grad_out (N,D) fp32 -> grad_A (N,P,D), grad_b (N,P) fp32. */
size_t lf_gels_workspace_bytes(int N, int D);
int lf_gels_fwd(const float* A, const float* b, int N, long P, int D, float* x, double* zinv, void* partials,
                int32_t* status, void* stream);
int lf_gels_bwd(const float* A, const float* b, const float* x, const double* zinv, const float* grad_out,
                int N, long P, int D, float* grad_A, float* grad_b, void* stream);

/* Area_Loss.forward -- BEV/Loss_crit.py:98-134.  beta (N,order+1) with element stride
 * beta_stride between images, gt (N,order+1) contiguous; dtype LF_F32/LF_F64 for both.
 * loss out: 1 element of dtype; grad out: (N,order+1) of dtype = d loss / d beta. */
int lf_area_loss(const void* beta, long beta_stride, const void* gt, int N, int order,
                 int weight_funct, int dtype, void* loss, void* grad, void* stream);

/* MSE_Loss.forward -- BEV/Loss_crit.py:137-150 (BP/Loss_crit.py:147-160): nn.MSELoss() of params.squeeze(-1) against
 * gt_params = mean over ALL n = N * (order + 1) elements of the squared difference (--loss_policy mse).  params, gt: n
 * contiguous elements of dtype (LF_F32 / LF_F64); loss out: 1 element; grad out: n elements = 2 (params - gt) / n. */
int lf_mse_loss(const void* params, const void* gt, long n, int dtype, void* loss, void* grad, void* stream);

/* backprojection_loss.forward -- BP/Loss_crit.py:202-218 (constants of :166-200 passed in).
 *   beta (N,order+1) fp64 (stride beta_stride), x_gt/valid (N,S) fp64, Y (S,order+1) fp64,
 *   y_prime (S) fp64, minv_host: 9 doubles (row-major M^-1) read on the HOST at call time.
 *   loss out fp64 scalar; x_cal_valid out (N,S) fp64; grad out (N,order+1) fp64. */
int lf_backproj_loss(const double* beta, long beta_stride, const double* x_gt, const double* valid,
                     const double* Y, const double* y_prime, const double* minv_host,
                     int N, int S, int order, double* loss, double* x_cal_valid, double* grad,
                     void* stream);

/* Class-weighted pixel cross entropy, weighted-mean reduction: BEV/Loss_crit.py:61-75,
 * BP/Loss_crit.py:64-65.  logits (N,C,H,W) fp32, target (N,H,W) int64, weights (C) fp32.
 * acc: 3 doubles of scratch: weighted loss sum, weight sum, and the NUMBER OF TARGETS OUTSIDE [0, C) -- those pixels get
 * weight 0 in loss and gradient, and the host raises when the count is non-zero (torch's NLLLoss asserts on them).
 * loss out fp32 scalar. */
int lf_ce2d_fwd(const float* logits, const int64_t* target, const float* weights,
                int N, int C, int H, int W, double* acc, float* loss, void* stream);
/* grad_logits (N,C,H,W) = upstream * d loss / d logits; `acc` as left by lf_ce2d_fwd. */
int lf_ce2d_bwd(const float* logits, const int64_t* target, const float* weights,
                int N, int C, int H, int W, const double* acc, const float* upstream,
                float* grad_logits, void* stream);

/* ------------------------------------------------------------------------------------
 * ERFNet backbone engine.  Replaces ERFNet.Net.forward (BEV/Networks/ERFNet.py:151-157;
 * DownsamplerBlock :11-22, non_bottleneck_1d :25-60, Encoder :63-95, UpsamplerBlock :98-107,
 * Decoder :109-142; BP/Networks/ERFNet.py is the same network) and its autograd backward.
 *
 * A plan is built once per input shape (host-side object, no device allocation); every call
 * runs the whole pass on `stream` out of a caller-owned workspace that must stay untouched
 * between a forward and its backward (it holds the saved activations, NHWC fp32).
 *
 *   params: the model's parameter tensors in state_dict() order, buffers excluded (weights,
 *     biases, BN weight/bias; 228 of them for one head, +2 with the `pretrained` second head),
 *     given both as a HOST array of device pointers and as a DEVICE array of the same pointers;
 *   running: 2 * lf_erfnet_num_bn() device pointers (running_mean, running_var per BN, module
 *     order); updated in training mode exactly like nn.BatchNorm2d (momentum 0.1, eps 1e-3);
 *   dropmask: Dropout2d keep-masks (0 or 1/(1-p) per (image, channel)) for the 13 encoder blocks
 *     with p > 0 (ERFNet.py:41,57-58), laid out per lf_erfnet_dropmask_offset(); NULL = no dropout;
 *   head: 0 = decoder.output_conv, 1 = decoder.output_conv2 (Decoder.forward flag, :134-141);
 *   logits: (N, out_channels + head, H, W) fp32 NCHW.
 * ---------------------------------------------------------------------------------- */
typedef struct lf_erfnet_plan lf_erfnet_plan;
lf_erfnet_plan* lf_erfnet_plan_create(int N, int H, int W, int in_channels, int out_channels, int n_heads);
void lf_erfnet_plan_destroy(lf_erfnet_plan* plan);
/* Precision mode of the backbone (there is no reference for modes 2 and 3 -- the reference is fp32 only):
 * 0 = fp32 matrix cores (v_mfma_f32_16x16x4_f32), fp32 tensors: the default, the parity path, the BASELINE headline;
 * 2 = bf16 tensors (BASELINE config 3): every activation / gradient tensor of the workspace stored as bf16, convolutions, data
 *     gradients and weight gradients on the bf16 matrix cores with fp32 accumulation; parameters, their gradients, BatchNorm
 *     statistics and the logits stay fp32;
 * 3 = fp32 results on the bf16 matrix cores: tensors and accumulation as in mode 0, every product of the 64- and 128-channel
 *     convolutions and data gradients formed from exact 3-way bf16 splits of both fp32 operands (all 9 partial products, i.e.
 *     exact products); parity as mode 0 (tests/test_backbone_gpu.py); launches the split kernel cannot take (other channel
 *     counts, pixel counts not a multiple of 512) and the weight gradient run on the fp32 matrix cores.
 * (Modes 1 and 4 -- bf16 operands with fp32 tensors, and the 6-term split -- existed through ABI 4; no BASELINE configuration
 * used them and they were removed in round 6: the call returns an error for them.) */
int lf_erfnet_set_precision(const lf_erfnet_plan* plan, int mode);
size_t lf_erfnet_workspace_bytes(const lf_erfnet_plan* plan);   /* follows the precision mode (bf16 tensors: larger partial-row regions): query it after lf_erfnet_set_precision */
size_t lf_erfnet_workspace_bytes_for(const lf_erfnet_plan* plan, int mode);   /* the same for a named mode, whatever the plan's current setting (0: unknown mode) */
long lf_erfnet_activation_floats(const lf_erfnet_plan* plan);   /* elements of the saved activations (all layers): bench.py's HBM roofline */
int lf_erfnet_num_params(const lf_erfnet_plan* plan);
int lf_erfnet_num_bn(const lf_erfnet_plan* plan);
int lf_erfnet_num_dropout(const lf_erfnet_plan* plan);
long lf_erfnet_dropmask_floats(const lf_erfnet_plan* plan);
long lf_erfnet_dropmask_offset(const lf_erfnet_plan* plan, int i);      /* float offset of block i */
int lf_erfnet_dropmask_channels(const lf_erfnet_plan* plan, int i);
long lf_erfnet_encoder_offset(const lf_erfnet_plan* plan);             /* float offset of the encoder output (N,H/8,W/8,128) NHWC */
long lf_erfnet_activation_offset(const lf_erfnet_plan* plan, int layer, int slot);
/* float offset of a BatchNorm's folded per-channel fp32 vector in the workspace (parity tests: the values the forward pass decided
 * its ReLU masks with).  bn: 0 / 1 within the layer (non_bottleneck_1d: bn1, bn2); which: 0 scale = gamma * rstd, 1 shift =
 * beta - mean * scale, 2 rstd, 3 -mean * rstd.  Valid after lf_erfnet_forward; -1 when out of range. */
long lf_erfnet_bn_vector_offset(const lf_erfnet_plan* plan, int layer, int bn, int which);
/* head = 0 / 1 selects output_conv / output_conv2; head = -1 = ENCODER ONLY (Net.forward(only_encode=True),
 * BEV/Networks/ERFNet.py:151-153): the decoder does not run (its BatchNorm running statistics stay untouched, as in the
 * reference, where the decoder is never called on that branch), logits may be NULL; the matching backward takes
 * head = -1 too, with grad_encoder as the incoming gradient. */
int lf_erfnet_forward(const lf_erfnet_plan* plan, const float* img, const float* const* params_host,
                      const float* const* params_dev, float* const* running_host, const float* dropmask,
                      int training, int head, float* logits, void* workspace, size_t workspace_bytes, void* stream);
/* Gradients are written (not accumulated) into grads_host[i]; NULL entries are skipped.
 * grad_encoder: optional (N,H/8,W/8,128) NHWC gradient w.r.t. the encoder output (`shared_encoder`,
 * BP/Networks/LSQ_layer.py:275), added where the decoder's gradient reaches the encoder; NULL = none.  It has the storage
 * type of the encoder output: fp32, or bf16 elements in precision mode 2 (the --clas heads and only_encode in bf16); the
 * encoder-only backward (head = -1) takes it in every mode.
 * training: the mode the matching forward ran in.  1 = batch statistics (autograd of nn.BatchNorm2d in train mode);
 * 0 = running statistics (net.eval() with gradients enabled, e.g. fine-tuning with frozen statistics): BatchNorm is then
 * a per-channel affine map and its data gradient is gamma * rstd * dy, as torch computes it. */
int lf_erfnet_backward(const lf_erfnet_plan* plan, const float* img, const float* grad_logits,
                       const float* grad_encoder, const float* const* params_host, float* const* grads_host,
                       const float* dropmask, int training, int head, void* workspace, size_t workspace_bytes, void* stream);
int lf_nhwc_to_nchw(const float* src, float* dst, int N, int H, int W, int C, void* stream);

/* Inference engine: the eval-mode forward of ERFNet.Net (model.eval() under torch.no_grad() in validate(),
 * Birds_Eye_View_Loss/main.py:373-388 and Backprojection_Loss/main.py:429-452, and test_model, Backprojection_Loss/test.py:35-58)
 * with nothing a backward reads: every BatchNorm is folded into the convolution that feeds it from its running statistics, per
 * call (one fold-and-pack launch), so a call after a training step sees the new statistics; no statistics, dropout, saved
 * activations or partial rows.  Precision mode as set by lf_erfnet_set_precision (0, 2, 3).
 * lf_erfnet_infer_workspace_bytes(plan, mode): its workspace for a named mode (0 for an unknown mode), about 1/20 of
 * lf_erfnet_workspace_bytes_for at the headline size.  lf_erfnet_infer_encoder_offset: float offset of the encoder output
 * (N,H/8,W/8,128) NHWC in it -- fp32, or bf16 elements in mode 2, the layout lf_erfnet_forward leaves -- the same in every mode.
 * lf_erfnet_infer: arguments as lf_erfnet_forward without dropout mask and training flag; head = -1 = encoder only (logits may
 * be NULL); the running statistics are read, never written. */
size_t lf_erfnet_infer_workspace_bytes(const lf_erfnet_plan* plan, int mode);
long lf_erfnet_infer_encoder_offset(const lf_erfnet_plan* plan);
int lf_erfnet_infer(const lf_erfnet_plan* plan, const float* img, const float* const* params_host, const float* const* params_dev,
                    float* const* running_host, int head, float* logits, void* workspace, size_t workspace_bytes, void* stream);

/* The inference engine for a layer range: lf_erfnet_forward_range (below) in eval mode without gradients -- DownsamplerBlock /
 * non_bottleneck_1d / UpsamplerBlock.forward(input), Encoder.forward(input), Decoder.forward(input, flag) under model.eval() and
 * torch.no_grad() (BEV/Networks/ERFNet.py:19-22,44-60,86-95,104-107,129-142).  Layers [first, last) (+ head when last = the layer
 * count) on an NCHW fp32 input -> NCHW fp32 output, precision mode as set by lf_erfnet_set_precision (0, 2, 3); the contract of
 * lf_erfnet_forward_range without dropout mask and training flag, the schedule, kernels and folded weights of lf_erfnet_infer: the
 * encoder range followed by the decoder range gives lf_erfnet_infer's logits bit for bit.  Running statistics are read, never
 * written.  The workspace equals lf_erfnet_infer_workspace_bytes of the mode (the fold-and-pack launch covers the whole plan; input
 * and output are staged through the activation buffers); 0 for an unknown mode or an empty / reversed range. */
size_t lf_erfnet_infer_range_workspace_bytes(const lf_erfnet_plan* plan, int first, int last, int mode);
int lf_erfnet_infer_range(const lf_erfnet_plan* plan, int first, int last, int head, const float* x, const float* const* params_host,
                          const float* const* params_dev, float* const* running_host, float* y, void* workspace,
                          size_t workspace_bytes, void* stream);

/* Fused head + fit (inference): decoder.output_conv = ConvTranspose2d(16, K, 2, stride 2) (BEV/Networks/ERFNet.py:123,139) and
 * Net.forward steps 2-4 (activation, row mask, grid, WLS: BEV/Networks/LSQ_layer.py:310-325, BP/Networks/LSQ_layer.py:298-313) in
 * one pass over the last decoder layer's tensor: the logits are written only on request, the masked weight maps never.
 *   x (N,h,w,16) NHWC: fp32 (x_bf16 = 0) or bf16 bit patterns (1); head_w (16,K,2,2), head_b (K) fp32, K <= 8;
 *   grid_xy ... solver, beta, zinv, partials (>= lf_wls_workspace_bytes(N,K,order)), status: as lf_wls_fwd on the (N,K,2h,2w) maps;
 *   logits_or_null (N,K,2h,2w) fp32.  With logits NULL, input rows that feed only output rows < zero_rows are never read (nor
 *   is the grid on those rows); with logits requested every row is computed for them, and the fit still skips the masked rows.
 * lf_lane_infer: image -> lane polynomials in one call = lf_erfnet_infer's schedule up to the last decoder layer, lf_head_fit on
 * head 0 (K = the plan's out_channels), the solve; validate() / test_model of the reference consume exactly these outputs
 * (Backprojection_Loss/test.py:35-88).  beta (N,K,order+1) fp64 and status (N*K) as lf_wls_fwd; reg_ls is added to the diagonal
 * for both solvers (pass 0 for BP's GELS).  The encoder output stays at lf_erfnet_infer_encoder_offset of the workspace for the
 * --clas heads.  lf_lane_infer_workspace_bytes: 0 for an unknown mode, K != out_channels or order outside 0..3. */
int lf_head_fit(const void* x, int x_bf16, const float* head_w, const float* head_b, const float* grid_xy, long grid_batch_stride,
                int N, int h, int w, int K, int zero_rows, int order, double reg, double y_offset, int act_kind, int solver,
                float* logits_or_null, double* beta, double* zinv, void* partials, int32_t* status, void* stream);
size_t lf_lane_infer_workspace_bytes(const lf_erfnet_plan* plan, int mode, int K, int order);
int lf_lane_infer(const lf_erfnet_plan* plan, const float* img, const float* const* params_host, const float* const* params_dev,
                  float* const* running_host, const float* grid_xy, long grid_batch_stride, int zero_rows, int order, double reg_ls,
                  double y_offset, int act_kind, int use_cholesky, float* logits_or_null, double* beta, int32_t* status,
                  void* workspace, size_t workspace_bytes, void* stream);

/* additions since 5 -- homography through the fit (BEV/Networks/LSQ_layer.py:84-87 ProjectiveGridGenerator.forward as a kernel, and
 * the gradients the reference's autograd carries to the grid and to theta):
 *   theta  (3,3) fp32 shared by all images (theta_batch_stride = 0) or (N,3,3) per image (theta_batch_stride = 9)
 *   xs (W), ys (H)  fp32 base coordinates, made on the host with the reference's torch.linspace calls (xs 16-byte aligned)
 *   (a, b, c) = theta [xs[j], ys[i], 1];  grid = (a / c, b / c) in fp32
 * lf_theta_grid       grid_xy out (N | 1, H*W, 2) fp32.
 * lf_theta_grid_bwd   grad_grid (same shape) -> grad_theta (N | 1, 3, 3) fp64; pixels whose grad_grid is exactly (0, 0) are
 *                     skipped (masked rows: a pole there contributes nothing); workspace >= lf_theta_grid_bwd_workspace_bytes(N).
 * lf_wls_fwd_theta    lf_wls_fwd with the grid computed inline: same outputs, same bits as lf_wls_fwd on lf_theta_grid's grid.
 * lf_wls_bwd_theta    lf_wls_bwd's grad_logits plus grad_theta (N | 1, 3, 3) fp64 in the same pass: fp64 per-workgroup partials
 *                     in workspace (>= lf_wls_bwd_theta_workspace_bytes(N,K)), added in a fixed order by a second launch; no
 *                     atomics, no (N,H*W,2) gradient tensor.
 * lf_wls_bwd_grid     d loss / d grid_xy of lf_wls_fwd (arguments as lf_wls_bwd): grad_grid (N,H*W,2) fp32, or (H*W,2) summed
 *                     over images and lanes in a fixed order when grid_batch_stride = 0; masked rows are written as 0. */
int lf_theta_grid(const float* theta, long theta_batch_stride, const float* xs, const float* ys, int N, int H, int W,
                  float* grid_xy, void* stream);
size_t lf_theta_grid_bwd_workspace_bytes(int N);
int lf_theta_grid_bwd(const float* theta, long theta_batch_stride, const float* xs, const float* ys, const float* grad_grid,
                      int N, int H, int W, double* grad_theta, void* workspace, void* stream);
int lf_wls_fwd_theta(const float* logits, const float* theta, long theta_batch_stride, const float* xs, const float* ys,
                     int N, int K, int H, int W, int zero_rows, int order, double reg, double y_offset, int act_kind, int solver,
                     double* beta, double* zinv, float* masked, void* partials, int32_t* status, void* stream);
size_t lf_wls_bwd_theta_workspace_bytes(int N, int K);
int lf_wls_bwd_theta(const float* logits, const float* theta, long theta_batch_stride, const float* xs, const float* ys,
                     int N, int K, int H, int W, int zero_rows, int order, double y_offset, int act_kind, const double* beta,
                     const double* zinv, const double* grad_beta, float* grad_logits, double* grad_theta, void* workspace,
                     void* stream);
int lf_wls_bwd_grid(const float* logits, const float* grid_xy, long grid_batch_stride, int N, int K, int H, int W,
                    int zero_rows, int order, double y_offset, int act_kind, const double* beta, const double* zinv,
                    const double* grad_beta, float* grad_grid, void* stream);

/* Block-level surface (round 4): a contiguous range [first, last) of the plan's layers (module order: 0 =
 * encoder.initial_block, 1..15 = encoder.layers[0..14], 16..21 = decoder.layers[0..5]) as one call, inside the plan of the
 * whole network at the matching input size -- what makes the reference's sub-modules callable on their own:
 *   DownsamplerBlock.forward(input)            BEV/Networks/ERFNet.py:19-22
 *   non_bottleneck_1d.forward(input)           :44-60
 *   UpsamplerBlock.forward(input)              :104-107
 *   Encoder.forward(input, predict=False)      :86-95   (range 0..16; predict = lf_pointwise_fwd on top)
 *   Decoder.forward(input, flag)               :129-142 (range 16..22 with head = 0 / 1)
 * x / y / gy / gx are NCHW fp32 like the reference's tensors; head >= 0 (only with last = the layer count) appends
 * output_conv (0) / output_conv2 (1) and makes y the logits.  Only the range's parameters are read / receive gradients
 * (grads_host entries outside it are left untouched); BatchNorm running statistics of the range are updated in train mode.
 * lf_erfnet_backward_range must follow lf_erfnet_forward_range on the same workspace.  Every precision mode (in mode 2 the
 * range's input and the incoming gradient are rounded to bf16 on their way into the workspace, outputs widened on their way out).
 * The workspace of a range is COMPACT (ABI 4): lf_erfnet_range_workspace_bytes(plan, first, last) = the range's own activations
 * + the plan's globals (packed weights, statistics rows, one partial-row region, three gradient buffers), so that a loop over
 * the blocks of a network keeps the activations of ONE network alive until backward, not one whole-network workspace per block.
 * gx may be NULL for any range.  For first = 0 a non-NULL gx receives the image's gradient (N,Cin,H,W) from one extra launch,
 * lf_stem_bwd_data, as lf_erfnet_backward_input's grad_img does; with NULL the stem runs its weight gradient only. */
int lf_erfnet_num_layers(const lf_erfnet_plan* plan);
size_t lf_erfnet_range_workspace_bytes(const lf_erfnet_plan* plan, int first, int last);
int lf_erfnet_layer_io(const lf_erfnet_plan* plan, int layer, int* out6_host);   /* Cin, Hin, Win, Cout, Hout, Wout */
int lf_erfnet_forward_range(const lf_erfnet_plan* plan, int first, int last, int head, const float* x,
                            const float* const* params_host, const float* const* params_dev, float* const* running_host,
                            const float* dropmask, int training, float* y, void* workspace, size_t workspace_bytes, void* stream);
int lf_erfnet_backward_range(const lf_erfnet_plan* plan, int first, int last, int head, const float* x, const float* gy,
                             const float* const* params_host, float* const* grads_host, const float* dropmask, int training,
                             float* gx, void* workspace, size_t workspace_bytes, void* stream);
/* encoder.output_conv = nn.Conv2d(128, num_classes, 1): the `predict=True` branch of Encoder.forward that
 * Net.forward(input, flag, only_encode=True) returns (BEV/Networks/ERFNet.py:84,86-95,151-153).
 * x (N,h,w,C) NHWC fp32 (the encoder output, read in place), w (K,C) = the weight (K,C,1,1), b (K) or NULL -> y (N,K,h,w) NCHW.
 * Backward: gy (N,K,h,w) -> gx (N,h,w,C) NHWC (or NULL), gw (K,C) and gb (K) (or NULL); scratch >= lf_pointwise_scratch_floats(). */
int lf_pointwise_fwd(const float* x, const float* w, const float* b, float* y, int N, int h, int w_, int C, int K, void* stream);
long lf_pointwise_scratch_floats(int N, int h, int w_, int C, int K);
int lf_pointwise_bwd(const float* x, const float* gy, const float* w, float* gx, float* gw, float* gb, int N, int h, int w_,
                     int C, int K, float* scratch, void* stream);
/* The same on the bf16 encoder output of precision mode 2 (ERFNet.py:84,86-95,151-153 in Net(precision="bf16")): x (N,h,w,C) NHWC
 * bf16 (bit patterns, read in place), C % 8 == 0; y, w, b, gy, gw, gb fp32 as above; gx (N,h,w,C) NHWC is written as bf16 -- the
 * grad_encoder that the encoder-only lf_erfnet_backward takes in mode 2.  Scratch as lf_pointwise_scratch_floats(). */
int lf_pointwise_bf16_fwd(const uint16_t* x, const float* w, const float* b, float* y, int N, int h, int w_, int C, int K,
                          void* stream);
int lf_pointwise_bf16_bwd(const uint16_t* x, const float* gy, const float* w, uint16_t* gx, float* gw, float* gb, int N, int h,
                          int w_, int C, int K, float* scratch, void* stream);
/* ------------------------------------------------------------------------------------
 * Cold-path arithmetic natively (round 4): the nn.Linear tails of the --clas heads and the segmentation-mode fit input.
 *
 * lf_linear_fwd: y (N,O) = act(x (N,K) @ w (O,K)^T + b (O) or NULL), act = identity or ReLU (relu = 1).  Replaces
 *   F.relu(self.fully_connected1(x)), self.fully_connected_line1(x), self.fully_connected_horizon(x)
 *   (BP/Networks/LSQ_layer.py:186-189,199-207; BEV/Networks/LSQ_layer.py:198-205,218-226).  fp32, fixed summation order.
 * lf_linear_bwd: gy (N,O) [+ y, the forward's output, when relu] -> gx (N,K), gw (O,K), gb (O); NULL outputs are skipped
 *   (gb needs gw).  Written, not accumulated.
 * lf_seg_maps: logits (N,C,H,W) -> maps (N,L,H,W): per-lane maps valued k where the arg-max over the C class logits is k
 *   (first maximum, like torch.max), rows < zero_rows zeroed (index_fill), lanes flagged in gt_line (N,L fp32, or NULL) set to
 *   map [0,0] -- Net.forward(end_to_end=False): BEV/Networks/LSQ_layer.py:302-308,316; BP/Networks/LSQ_layer.py:279-293,298,308-311. */
int lf_linear_fwd(const float* x, const float* w, const float* b, float* y, int N, int K, int O, int relu, void* stream);
int lf_linear_bwd(const float* x, const float* w, const float* y, const float* gy, float* gx, float* gw, float* gb, int N, int K,
                  int O, int relu, void* stream);
int lf_seg_maps(const float* logits, const float* gt_line, float* maps, int N, int C, int L, int H, int W, int zero_rows,
                void* stream);
/* Roofline instrumentation (bench.py): HIP event pairs around every matrix-core launch of the engine.
 * out6 = {ms, algorithmic FLOPs, launches} for family 0 (tap-GEMM forward + data gradient) and
 * family 1 (weight gradient), accumulated since the last read. */
int lf_erfnet_profile(const lf_erfnet_plan* plan, int enable);
/* csv_path_host: optional file receiving one line per recorded launch (family, layer, shape, us, TFLOP/s); NULL = none */
int lf_erfnet_profile_read(const lf_erfnet_plan* plan, double* out6_host, const char* csv_path_host);

/* ------------------------------------------------------------------------------------
 * Fused Adam step over all parameter tensors in ONE launch ("next" row 8f-1).  Replaces optimizer.step() of the
 * torch.optim.Adam the reference builds (BEV/Networks/utils.py:411-420, BEV/main.py:266); same arithmetic.
 *   tensors_dev: n records {float* p; const float* g; float* m; float* v; long numel; long step[2]} on the device: the
 *     step count is PER TENSOR like torch.optim.Adam's (a head that starts training late has its own bias correction) and
 *     lives in the record, double-buffered;
 *   work_dev: nblocks int2 {tensor index, chunk index}, chunk = lf_adam_chunk() elements;
 *   parity: the slot of step[] holding each tensor's count of updates so far; the launch writes count + 1 to the other slot
 *     (alternate parity between calls); grad_scale: multiplies every gradient first (1/world size).
 * ---------------------------------------------------------------------------------- */
int lf_adam_chunk(void);
int lf_adam_step(const void* tensors_dev, const void* work_dev, int nblocks, float lr, float beta1, float beta2,
                 float eps, float weight_decay, int parity, float grad_scale, void* stream);
/* The other optimizers of define_optim (BEV/Networks/utils.py:414-417), same tables (record field m = momentum buffer,
 * v = RMSprop's square average; the step slots are unused): torch.optim.SGD(momentum, dampening 0, no Nesterov) and
 * torch.optim.RMSprop(alpha, eps, momentum, not centered), L2 weight decay folded into the gradient as torch does. */
int lf_sgd_step(const void* tensors_dev, const void* work_dev, int nblocks, float lr, float momentum, float weight_decay,
                float grad_scale, void* stream);
int lf_rmsprop_step(const void* tensors_dev, const void* work_dev, int nblocks, float lr, float alpha, float eps,
                    float momentum, float weight_decay, float grad_scale, void* stream);

/* additions since 5 -- gradient-norm clipping: nn.utils.clip_grad_norm(model.parameters(), args.clip_grad_norm) between
 * loss.backward() and optimizer.step() (BP/main.py:334-335) as ONE read of the gradients plus a scalar in device memory that the
 * step picks up; the host never waits.  All entry points take the record / work tables of lf_adam_step.
 *   lf_grad_sumsq: one workgroup per work item adds the squares of its gradient elements -- each widened to fp64 before it is
 *     squared, so 1e30 does not overflow -- and writes one fp64 partial to workspace slot slot0 + block.  Call it once per param
 *     group with consecutive slot ranges; workspace holds lf_grad_norm_workspace_bytes(total_blocks) bytes, 8-byte aligned.
 *   lf_grad_norm_finish: one workgroup adds the total_blocks partials in a fixed order and writes two fp32 values,
 *     out2[0] = total_norm = fl32(grad_scale * sqrt(sum))   (the norm of the gradients the step will use: under summed
 *                                                            data-parallel gradients and grad_scale = 1/world, of their average),
 *     out2[1] = coef = max_norm / (total_norm + 1e-6), replaced by 1 where that exceeds 1   (fp32, torch's clamp(max=1.0)).
 *     No floating-point atomics anywhere: two runs on the same inputs give the same bits.
 *   lf_grad_scale_inplace: g = fl32(fl32(g * grad_scale) * coef_dev[0]) on every element inside a tensor's numel and nowhere
 *     else -- the drop-in form, what torch leaves in p.grad.
 *   lf_*_step_clipped: the step of lf_*_step on the effective gradient fl32(fl32(g * grad_scale) * coef_dev[0]), two separately
 *     rounded products; the gradients are not written.  lf_grad_scale_inplace followed by lf_*_step with grad_scale 1 leaves the
 *     same bits.  Adam's per-tensor step counts and the parity slot work as in lf_adam_step.
 * Non-finite gradients behave as under torch's clip_grad_norm_(error_if_nonfinite=False); there is no step skip.  An Inf gradient
 * gives total_norm = Inf and coef = 0: every finite gradient then counts as 0 and the Inf element as NaN.  A NaN gradient gives
 * total_norm = coef = NaN, hence NaN everywhere.  All-zero gradients give total_norm 0 and coef 1. */
size_t lf_grad_norm_workspace_bytes(int total_blocks);
int lf_grad_sumsq(const void* tensors_dev, const void* work_dev, int nblocks, int slot0, void* workspace, void* stream);
int lf_grad_norm_finish(const void* workspace, int total_blocks, float grad_scale, float max_norm, float* out2, void* stream);
int lf_grad_scale_inplace(const void* tensors_dev, const void* work_dev, int nblocks, float grad_scale, const float* coef_dev,
                          void* stream);
int lf_adam_step_clipped(const void* tensors_dev, const void* work_dev, int nblocks, float lr, float beta1, float beta2,
                         float eps, float weight_decay, int parity, float grad_scale, const float* coef_dev, void* stream);
int lf_sgd_step_clipped(const void* tensors_dev, const void* work_dev, int nblocks, float lr, float momentum, float weight_decay,
                        float grad_scale, const float* coef_dev, void* stream);
int lf_rmsprop_step_clipped(const void* tensors_dev, const void* work_dev, int nblocks, float lr, float alpha, float eps,
                            float momentum, float weight_decay, float grad_scale, const float* coef_dev, void* stream);

/* ------------------------------------------------------------------------------------
 * "Next" row 8f-3: the `--clas` heads and the inference-side post-processing of BP/test.py.
 *
 * lf_convchain_*: a chain of [Conv2d(k, stride 1, pad k/2, bias) -> BatchNorm2d -> ReLU] blocks on an NHWC fp32
 * tensor = the trunk of `Classification` (BP/Networks/LSQ_layer.py:150-181,192-196: conv1..conv4 + BNs) that the
 * line-type and horizon heads run on the encoder output.  Plan per shape; channels[0..L] multiples of 16,
 * ksize[i] in {1,3}.  params: 4 per block (conv.weight (Co,Ci,k,k), conv.bias, bn.weight, bn.bias) as a HOST
 * and a DEVICE array of device pointers; running_host: 2 per block.  x is read in place from the backbone
 * workspace (lf_erfnet_encoder_offset); y = last block's post-ReLU output, NHWC.  The workspace holds the
 * saved pre-BN tensors until lf_convchain_backward, which writes every parameter gradient and (if gx != NULL)
 * the NHWC input gradient to hand to lf_erfnet_backward(grad_encoder).
 * Precision (lf_convchain_set_precision): mode 0 (default) = fp32 tensors on the fp32 matrix cores; mode 2 = the backbone's
 * "bf16" mode for the same trunk (BP/Networks/LSQ_layer.py:150-181 in Net(precision="bf16")): x, y, gy, gx and the saved pre-BN
 * tensors hold bf16 elements (the pointers keep their float* type, as in lf_erfnet_*), the convolutions, their data gradients
 * and weight gradients run on the bf16 matrix cores; BatchNorm statistics come from the fp32 values before the bf16 store;
 * parameters, running statistics and parameter gradients stay fp32.  lf_convchain_workspace_bytes follows the mode the plan
 * is set to; lf_convchain_workspace_bytes_for(plan, mode) names it (0 bytes for a mode other than 0 and 2), and a workspace
 * sized for mode 2 serves mode 0 too.
 * Limits of lf_convchain_backward (lf_convchain_plan_create, _forward and _infer take every multiple of 16 and every W; the backward
 * call then returns < 0 with lf_last_error set, having written no parameter gradient of the refused block or of any block below
 * it, and the plan and its workspace stay usable for further forward calls):
 *   - the weight gradient is compiled for (C_in, C_out) channel pairs in which each side is a multiple of 64, 16 or 48 -- a side of
 *     32, 80, 96, ... that is no multiple of 64 is refused, and so is the pair (48, 48);
 *   - W must be a multiple of 4;
 *   - the LAST block's channel count must be a power of two (its BatchNorm backward reduces whole pixels per lane group;
 *     with any other count the call fails before it writes anything).
 * ---------------------------------------------------------------------------------- */
typedef struct lf_convchain_plan lf_convchain_plan;
lf_convchain_plan* lf_convchain_plan_create(int N, int H, int W, int nlayers, const int* channels_host,
                                            const int* ksize_host);
void lf_convchain_plan_destroy(lf_convchain_plan* plan);
size_t lf_convchain_workspace_bytes(const lf_convchain_plan* plan);
size_t lf_convchain_workspace_bytes_for(const lf_convchain_plan* plan, int mode);
int lf_convchain_set_precision(const lf_convchain_plan* plan, int mode);      /* 0 or 2; anything else is refused */
int lf_convchain_forward(const lf_convchain_plan* plan, const float* x, const float* const* params_host,
                         const float* const* params_dev, float* const* running_host, int training, float momentum,
                         float eps, float* y, void* workspace, size_t workspace_bytes, void* stream);
/* training = the mode of the matching forward (0: running statistics; see lf_erfnet_backward) */
int lf_convchain_backward(const lf_convchain_plan* plan, const float* x, const float* y, const float* gy,
                          const float* const* params_host, float* const* grads_host, float* gx, int training,
                          void* workspace, size_t workspace_bytes, void* stream);
/* The trunk in eval mode without gradients (Classification.forward under model.eval() and torch.no_grad(),
 * BP/Networks/LSQ_layer.py:192-196 in validate() / test_model): every BatchNorm folded into its convolution from the running
 * statistics, per call (one fold-and-pack launch), then one convolution launch per block with a bias + ReLU epilogue; nothing saved.
 * Mode as lf_convchain_set_precision (0; 2 reads the bf16 encoder output in place and writes y as bf16).  x, y, params and running
 * pointers as lf_convchain_forward; the running statistics are read, never written.  Workspace: 0 bytes for a mode other than 0, 2. */
size_t lf_convchain_infer_workspace_bytes(const lf_convchain_plan* plan, int mode);
int lf_convchain_infer(const lf_convchain_plan* plan, const float* x, const float* const* params_host,
                       const float* const* params_dev, float* const* running_host, float eps, float* y, void* workspace,
                       size_t workspace_bytes, void* stream);
/* Pool + flatten in front of the heads' fully connected layers (LSQ_layer.py:183-187,197-201):
 * mode 0 = MaxPool2d(2,2) -> (N, C*(H/2)*(W/2)); mode 1 = AvgPool2d((1,W)) -> (N, C*H); input NHWC,
 * output in the NCHW flatten order nn.Linear's weights expect.  The Linear layers themselves are plain
 * library GEMMs (rocBLAS through torch.nn.functional.linear). */
int lf_poolflat_fwd(const float* y, int N, int H, int W, int C, int mode, float* out, void* stream);
int lf_poolflat_bwd(const float* y, const float* gout, int N, int H, int W, int C, int mode, float* gy, void* stream);
/* The same on the bf16 NHWC trunk output of precision mode 2 (bit patterns): features and gout stay fp32 (the nn.Linear tails are
 * fp32 in every mode), gy is written as bf16; the max-pool backward keeps ATen's first-maximum rule on the bf16 values. */
int lf_poolflat_bf16_fwd(const uint16_t* y, int N, int H, int W, int C, int mode, float* out, void* stream);
int lf_poolflat_bf16_bwd(const uint16_t* y, const float* gout, int N, int H, int W, int C, int mode, uint16_t* gy, void* stream);

/* Projections.compute_coordinates (BP/test.py:172-186) + the gating of test_model (:77-88) in one launch:
 * x = resize(M_inv . [poly(beta, y_eval), y_prime, 1]) per (image, lane, sample height); then
 * line_flag[n][l] == 0 -> fill; sample index < bound[n] (python slice semantics) -> fill; x > hi or x < lo -> fill.
 * beta (N,L,order+1) fp64, highest power first; y_eval / y_prime (S) fp64; minv_host 9 doubles;
 * line_flag (N,L) fp32 or NULL; bound (N) int32 or NULL; lo > hi disables the range gate.
 * Outputs (either may be NULL): x_out (N,L,S) fp64, x_int (N,L,S) int32 = round-half-even(x). */
int lf_lane_decode(const double* beta, const double* y_eval, const double* y_prime, const double* minv_host,
                   double scale, const float* line_flag, const int* bound, double lo, double hi, double fill,
                   int N, int L, int S, int order, double* x_out, int* x_int, void* stream);

/* additions since 5 -- scoring of decoded lanes (BP/eval_lane.py:15-57, LaneEval.bench, one wave per image):
 *   pred (N,P,S) int32 x coordinates, pred_count (N) or NULL (= P lanes each; the first pred_count[n] lanes are scored);
 *   gt (M,G,S) int32 + gt_count (M): the resident label table; image n is scored against row index[n] (int32), or row n with
 *   index NULL (N <= M);  y_samples (S) fp64 shared by all rows (y_stride 0) or (M,S) per row (y_stride S);
 *   run_time (N) fp32 or NULL (= 20, what test_model writes).  P, G <= 8, 1 <= S <= 256.
 * Per gt lane: k = least-squares slope of x on y over its samples with x >= 0 (0 with fewer than two),
 * thresh = pixel_thresh * sqrt(1 + k^2); negative coordinates on either side become -100; a sample hits when |pred - gt| < thresh;
 * max_acc = max over pred lanes of hits / S (lowest index on a tie).  fn = gt lanes with max_acc < pt_thresh, fp = P_n - matched;
 * with G_n > 4 one fn is forgiven and the smallest max_acc leaves the sum; run_time > 200 or G_n + 2 < P_n scores (0, 0, 1).
 *   per_image (N,3) fp64 = accuracy, fp, fn -- the sum over gt lanes runs in ascending order in fp64;
 *   best_acc (N,G) fp64 / best_pred (N,G) int32 or NULL: max_acc per gt lane (0 past G_n) and the pred lane reaching it (-1: none);
 *   totals (3) fp64 or NULL: sums (not means) of per_image over the N images, by a second single-workgroup launch in a fixed order;
 *   bad_index: device int32, incremented once per image whose index lies outside [0, M); such an image scores (0, 0, 1) and
 *   reads nothing out of range (the host raises IndexError from the count, as with lf_pipeline_*_indexed). */
int lf_lane_eval(const int32_t* pred, const int32_t* pred_count, const int32_t* gt, const int32_t* gt_count,
                 const int32_t* index, const double* y_samples, long y_stride, const float* run_time,
                 int N, int M, int P, int G, int S, double pixel_thresh, double pt_thresh,
                 double* per_image, double* best_acc, int32_t* best_pred, double* totals, int32_t* bad_index, void* stream);

/* additions since 5 -- BEV lane decoding (BEV/Dataloader/Load_Data_new.py:334-420 write_lsq_results, the tail of validate(),
 * BEV/main.py:445-488): predicted polynomials -> image-space lane points, one wave per image against the resident label table
 * lf_lane_eval reads (gt, gt_count, index, h_samples + h_stride exactly as there; S <= 256, G <= 8).
 *   beta (N,L,order+1) contiguous, highest power first, beta_dtype LF_F32 | LF_F64, order 0..2 (missing leading coefficients are 0,
 *   the reference's [0]*(3-len(p)) + p), L <= 8;  line_id (N,4) int32 or NULL;  horizon (N,R) fp32 holding 0/1 or NULL, factor =
 *   640/resize;  m_host / minv_host: 9 doubles each (row-major M and M_inv);  nclasses >= L output rows per image.
 * Per image n (row = index ? index[n] : n), all in fp64:
 *   extent of lane j < L: count, min h and max h over the samples of gt lane j with x != -2 (ballot + fixed butterflies, any order
 *     of h; a gt lane j >= gt_count[row] counts as all -2 -- the reference raises IndexError there);
 *   without all_branches_ready a lane without a valid gt sample is skipped; with it lane 2 is skipped when line_id[n][0] == 0 and
 *     lane 3 when line_id[n][3] == 0, a lane without a valid gt sample uses (minimum, maximum) = (250, 710), and with horizon_on
 *     as well minimum = (sum_r horizon[n][r]) * factor + 80;
 *   y_d = (h - 80)/639, y' = (M11 y_d + M12)/(M21 y_d + M22);  ortho: y = 1 - y', x' = a y^2 + b y + c,
 *     x = (Minv row 0 . [x', y', 1]) / (Minv row 2 . [x', y', 1]);  no_ortho: y = 1 - y_d, x = a y^2 + b y + c, no homography;
 *   lanes[n][j][s] = round-half-even(1279 x) where max(210, minimum) <= h <= maximum, else -2; there is no range clamp (negative x
 *     is written as it is); the int32 store saturates and NaN becomes INT32_MIN.  Skipped lanes and rows L <= j < nclasses are -2.
 *   bad_index: device int32, incremented once per image whose row lies outside [0, M); its rows are all -2 and nothing out of
 *     range is read.  No other atomics: two launches give identical bits. */
int lf_lane_decode_bev(const void* beta, int beta_dtype, const int32_t* gt, const int32_t* gt_count, const int32_t* index,
                       const double* h_samples, long h_stride, const int32_t* line_id, const float* horizon, int R, double factor,
                       const double* m_host, const double* minv_host, int N, int M, int L, int G, int S, int order, int nclasses,
                       int all_branches_ready, int horizon_on, int no_ortho, int32_t* lanes, int32_t* bad_index, void* stream);

/* additions since 5 -- whole-step criterion: every criterion statement of one training / validation step as ONE launch
 * (BP/main.py:296-326 and :459-501 with BP/Loss_crit.py:202-218; BEV/main.py:223-253 and :395-431 with BEV/Loss_crit.py:98-134;
 * the two head criteria are BP/main.py:109-110 and BEV/main.py:88-89).  One 256-thread workgroup per task (K lanes, line, horizon);
 * the last one to arrive (a device-scope ticket in the workspace, left at zero) adds the task values up in the loop's order.
 * No workgroup waits for another and a result is bit-identical from call to call.
 *   tree: LF_TREE_BP -- fit = (sum over lanes) / nclasses, line head = BCEWithLogits on (N,4) logits against fp32 {0,1} targets;
 *         LF_TREE_BEV -- fit = plain sum, lanes 2 and 3 have their coefficients multiplied by the lane-present mask first
 *         (BEV/main.py:226-234), line head = unweighted mean cross entropy of (N,3,4) logits against (N,4) int64 labels (a label outside
 *         [0,3) carries weight 0 and is counted in out[6], the lf_ce2d_fwd convention).
 *   kind: LF_LANE_BACKPROJECT (orders 0-3; target = x_gt, valid: (N,Kt,S) fp64 with target_stride = Kt*S elements per image; Y, y_prime,
 *         minv_host exactly as for lf_backproj_loss; x_cal_valid (N,K,S) fp64 out), LF_LANE_AREA (orders 1-2, weight_funct; target = gt
 *         coefficients (N,Kt,D) in beta's type, target_stride = Kt*D; an image whose gt has a zero coefficient is dropped, a lane with
 *         every image dropped contributes 0), LF_LANE_MSE (orders 0-3; mean over the N*D elements).  valid, Y, y_prime, minv_host and
 *         x_cal_valid may be NULL for the last two.
 *   beta_lanes: HOST array of K (1..4) device pointers, lane k's coefficients of image n at beta_lanes[k] + n*beta_stride (the unbind
 *         views of one (N,K,D) tensor are read in place); beta_dtype LF_F32 | LF_F64.
 *   heads: line_logits / line_target / horizon_logits (N,R) fp32 / horizon_target (N,R) fp32 {0,1}: all four or all NULL.  Horizon loss =
 *         mean BCEWithLogits, max(x,0) - x*y + log1p(exp(-|x|)); a prediction is x > 0 (BP line, horizon) or the first arg-max over
 *         the class axis (BEV line); accuracies = hits / (R*N) and hits / (nclasses*N) (BP/main.py:491-497, BEV/main.py:421-427).
 *   total = fit*weight_fit + (line + horizon)*weight_class with the heads, fit without.  All arithmetic is fp64.
 *   out (10 fp64): total, fit, line, horizon, acc_line, acc_horizon, bad line labels, line hits, horizon hits, 0.
 *   grad: the gradient of total, flat: (N,K,D) in beta's type, then the line logits' and the horizon logits' in fp32 (with the heads).
 *   meters (8 fp64, may be NULL; never read for the results above): += total*N, N, fit*N, N, acc_line, 1, acc_horizon, 1.
 *   workspace: lf_step_loss_workspace_bytes() bytes, zeroed ONCE when allocated; calls sharing it must be ordered on one stream.
 * lf_step_loss_bwd: grad_out = grad * upstream[0] (device fp64 scalar) over the n_beta coefficient and n_head fp32 head elements. */
enum { LF_TREE_BP = 0, LF_TREE_BEV = 1 };
enum { LF_LANE_BACKPROJECT = 0, LF_LANE_AREA = 1, LF_LANE_MSE = 2 };
size_t lf_step_loss_workspace_bytes(void);
int lf_step_loss(int tree, int kind, int K, int N, int order, int weight_funct, int nclasses,
                 const void* const* beta_lanes, long beta_stride, int beta_dtype,
                 const void* target, const double* valid, long target_stride, int S,
                 const double* Y, const double* y_prime, const double* minv_host,
                 const float* line_logits, const void* line_target, const float* horizon_logits, const float* horizon_target, int R,
                 double weight_fit, double weight_class,
                 double* out, double* x_cal_valid, void* grad, double* meters, void* workspace, void* stream);
int lf_step_loss_bwd(const void* grad, int beta_dtype, long n_beta, long n_head, const double* upstream, void* grad_out, void* stream);

/* additions since 5 -- segmentation-mode step criterion: what a step of Net.forward(end_to_end=False) does behind the backbone
 * (criterion_seg(output_net, gt) and its gradient, BEV/Loss_crit.py:61-75; the arg-max lane maps and their fit,
 * BP/Networks/LSQ_layer.py:279-314, BEV/Networks/LSQ_layer.py:302-325) in one read of the logits, one read of the target and one
 * write of the gradient.  Three launches: a label pass (per-class pixel counts of the target as integers: the normaliser sum w[t] is
 * exact), the streaming pass (per-workgroup loss and moment partials into fixed workspace slots) and a finish (partials added in a
 * fixed order, the solve).  No floating-point atomics, no workgroup waits for another; two calls on the same inputs give identical
 * bits in out, grad_logits and beta.
 *   logits (N,C,H,W) fp32, target (N,H,W) int64, weights (C) fp32: as lf_ce2d_fwd (C <= 8; a label outside [0, C) carries weight 0
 *     in the loss and the gradient and is counted in out[3]).  The per-pixel arithmetic is lf_ce2d_fwd's / lf_ce2d_bwd's (fp32),
 *     the sums are fp64.
 *   grid_xy (H*W,2) fp32 with grid_batch_stride 0, or (N,H*W,2) with 2*H*W, y_offset, reg, solver: as lf_wls_fwd; NULL = no fit
 *     (beta, status, maps, gt_line unused; L, order, zero_rows ignored).  On rows >= zero_rows a pixel whose first arg-max (NaN
 *     counts as maximal, as lf_seg_maps) is class l + 1 <= L adds weight (l + 1)^2 to lane l's moments: the sums lf_wls_fwd forms
 *     for the map lf_seg_maps writes.  Grid points of masked rows and of pixels of no lane are not read.  L <= 4, order 0..3.
 *   gt_line (N,L) fp32 or NULL: a flagged lane is solved from the moments of lane (0, 0) ("prevent singular matrix").
 *   grad_logits (N,C,H,W) fp32 or NULL: d loss / d logits for upstream 1.
 *   maps (N,L,H,W) fp32 or NULL: exactly what lf_seg_maps writes (one more small launch when gt_line is given as well).
 *   beta (N,L,order+1) fp64, status (N*L) int32: as lf_wls_fwd.
 *   out (4 fp64): loss = out[1] / out[2], the weighted loss sum, the weight sum, the number of labels outside [0, C).
 *   meters (2 fp64) or NULL: += loss * N, N.
 *   workspace: lf_seg_step_workspace_bytes(N, C, L, H, W, order) bytes (L = 0 without the fit), zeroed ONCE when allocated (the
 *     finish leaves the label counts at zero); calls sharing it must be ordered on one stream.
 * lf_seg_step_bwd: grad_logits (n elements) *= upstream[0] (device fp32 scalar), in place; every workgroup returns at once when the
 *   scalar is exactly 1.0, the case of the loops' loss.backward(). */
size_t lf_seg_step_workspace_bytes(int N, int C, int L, int H, int W, int order);
int lf_seg_step(const float* logits, const int64_t* target, const float* weights,
                const float* grid_xy, long grid_batch_stride, const float* gt_line,
                int N, int C, int L, int H, int W, int zero_rows, int order, double reg, double y_offset, int solver,
                float* grad_logits, float* maps, double* beta, int32_t* status, double* out, double* meters,
                void* workspace, void* stream);
int lf_seg_step_bwd(float* grad_logits, long n, const float* upstream, void* stream);

/* "Next" row 8f-2: polynomial.trapezoidal (BEV/Loss_crit.py:26-35): area between two parabolas by the
 * trapezium rule on [a, b] with n intervals; p, q (B,3) rows [a2, a1, a0]; fp32 or fp64; out (B). */
int lf_trapezoid(const void* p, const void* q, int B, double a, double b, int n, int is_double, void* out,
                 void* stream);

/* ------------------------------------------------------------------------------------
 * "Next" row 8f-4: the input pipeline on the device.  Replaces the per-sample PIL/torchvision work of
 * LaneDataset.__getitem__ (BEV/Dataloader/Load_Data_new.py:77-101, BP/Dataloader/Load_Data_new.py:126-173):
 * F.crop(bottom rows) -> F.resize((R,2R), BILINEAR | NEAREST) -> class remap -> F.hflip -> ToTensor, with
 * Pillow's fixed-point resampling arithmetic reproduced bit for bit (see csrc/lf_pipeline.hip).
 *   plan: host object holding the resampling tables for one geometry; upload them once to a device buffer of
 *     lf_pipeline_table_bytes() and pass that buffer to every call;
 *   lf_pipeline_image: frames (N,Hin,Win,3) uint8 HWC -> out (N,3,out_h,out_w) fp32 in [0,1];
 *   lf_pipeline_label: labels (N,Hin,Win) uint8 -> out (N,1,out_h,out_w) int64 through lut (256 int64 =
 *     (ToTensor(v)*255).long()), mode bit 0: zero classes 3,4 (BEV; BP with nclasses < 3), bit 1: BP's flip
 *     statement order (pre-flip masks of 3/4 applied to the flipped map, Load_Data_new.py:152-165);
 *     horizon (N,out_h) fp32 = ones above the first labelled row (BEV :103-105) or NULL;
 *   flip: (N) uint8 per-sample horizontal flip flags or NULL.
 * ---------------------------------------------------------------------------------- */
typedef struct lf_pipeline_plan lf_pipeline_plan;
lf_pipeline_plan* lf_pipeline_plan_create(int Hin, int Win, int crop_top, int crop_h, int out_h, int out_w);
void lf_pipeline_plan_destroy(lf_pipeline_plan* plan);
size_t lf_pipeline_table_bytes(const lf_pipeline_plan* plan);
int lf_pipeline_upload(const lf_pipeline_plan* plan, void* tables_dev, void* stream);
int lf_pipeline_tables_host(const lf_pipeline_plan* plan, int* ksx_host, int* ksy_host, int* bx_host, int* kx_host,
                            int* by_host, int* ky_host, int* ntx_host, int* nty_host);
int lf_pipeline_image(const lf_pipeline_plan* plan, const uint8_t* frames, int N, const void* tables_dev,
                      const uint8_t* flip, float* out, void* stream);
int lf_pipeline_label(const lf_pipeline_plan* plan, const uint8_t* labels, int N, const void* tables_dev,
                      const uint8_t* flip, int mode, const int64_t* lut, int64_t* out, float* horizon, void* stream);
/* The same two calls reading a RESIDENT POOL of decoded frames / label maps (pool_frames entries): batch element n is pool entry
 * sel[n] (int64 on the device).  The index batch of a cached dataset (SubsetRandomSampler's draw,
 * BEV/Dataloader/Load_Data_new.py:305-320) is gathered inside the kernels instead of by a copy of N frames first.
 * bad_index (device int32, may be NULL): incremented once per batch element whose sel[n] lies outside [0, pool_frames); such an
 * element reads pool entry 0 -- never out of bounds -- and the host raises from the count, as the reference's tensor indexing
 * raises IndexError (ABI 4: pool_frames on the label call, bad_index on both). */
int lf_pipeline_image_indexed(const lf_pipeline_plan* plan, const uint8_t* pool, long pool_frames, const int64_t* sel, int N,
                              const void* tables_dev, const uint8_t* flip, float* out, int* bad_index, void* stream);
int lf_pipeline_label_indexed(const lf_pipeline_plan* plan, const uint8_t* pool, long pool_frames, const int64_t* sel, int N,
                              const void* tables_dev, const uint8_t* flip, int mode, const int64_t* lut, int64_t* out, float* horizon,
                              int* bad_index, void* stream);

/* ------------------------------------------------------------------------------------
 * The LABEL half of LaneDataset.__getitem__ for a whole batch in one launch (csrc/lf_labels.hip), next to the pixel half above:
 * the parsed label tables of a resident dataset of M rows stay on the device, batch element n is table row sel[n].
 * Shared by both entry points:
 *   lines     (M,10) int8   the "lines" list of label_new.json;
 *   file_idx  (M)    int64  the reference's `idx`, file number - 1;
 *   is_valid  (M)    uint8  1 = the row belongs to the validation split;
 *   valid_pos (M)    int32  position in the dataset's valid_idx list, -1 for a training row;
 *   sel       (N)    int64  pool rows of the batch;  flip (N) uint8 the drawn flip flags, or NULL = none;
 *   idx (N) int64 = file_idx[sel];  index (N) int64 = valid_pos[sel];
 *   flipped   (N)    uint8  the EFFECTIVE flip, flip[n] && !is_valid[sel[n]] (`if idx not in self.valid_idx and hflip_input`) --
 *                           hand it to lf_pipeline_*_indexed as their flip so that pixels and labels agree;
 *   bad (device int32, may be NULL): incremented once per element whose sel[n] lies outside [0, M); row 0 is read in its place.
 * lf_label_batch_bp (BP/Dataloader/Load_Data_new.py:133-197):
 *   lanes (M,4,56) int32 raw TuSimple x, left-padded with -2 to 56 columns;  h_samples (M,56) fp64 the label's heights (the first
 *   h_count[m] entries are read);  h_count (M) int32 <= 56;  resize = R.
 *   valid_points (N,4,56) fp64 = lanes > 0 with columns 0..7 zero (never flipped);  lanes_out (N,4,56) fp64 = x / 2.5, -2 where that
 *   is negative, under the flip (2R - 1) - x with rows [1,0,3,2];  horizon (N,R) fp32 = ones on [0 : int(floor(y_val))] in Python's
 *   slice meaning, y_val the smallest h / 2.5 - 32 of a present point, pairing padded lane column i with height i (R if none);
 *   gt_line (N,4) fp32 = clamp(mirror?(lines)[3:7] + 1, 0, 1).
 * lf_label_batch_bev (BEV/Dataloader/Load_Data_new.py:74,86-111):
 *   params (M,4,3) fp64 -> params_out (N,4,3) fp32; flipped: rows [1,0,3,2], negated, last coefficient 1 + (-c), in fp64, then cast;
 *   gt_line (N,4) int64 = mirror?(lines)[3:7] + 1.
 * ---------------------------------------------------------------------------------- */
int lf_label_batch_bp(const int32_t* lanes, const double* h_samples, const int32_t* h_count, const int8_t* lines,
                      const int64_t* file_idx, const uint8_t* is_valid, const int32_t* valid_pos, long M, const int64_t* sel,
                      const uint8_t* flip, int N, int resize, double* valid_points, double* lanes_out, float* horizon,
                      float* gt_line, int64_t* idx, int64_t* index, uint8_t* flipped, int* bad, void* stream);
int lf_label_batch_bev(const double* params, const int8_t* lines, const int64_t* file_idx, const uint8_t* is_valid,
                       const int32_t* valid_pos, long M, const int64_t* sel, const uint8_t* flip, int N, float* params_out,
                       int64_t* gt_line, int64_t* idx, int64_t* index, uint8_t* flipped, int* bad, void* stream);

/* ------------------------------------------------------------------------------------
 * Kernel-level entry points: one factorised convolution of non_bottleneck_1d
 * (nn.Conv2d(C, C, (3,1)|(1,3), padding = dilation = d), BEV/Networks/ERFNet.py:29-37) on NHWC fp32
 * tensors, outside the plan: forward, data gradient (optionally times the ReLU mask of mask_src),
 * weight + bias gradient.  w / gw use the nn.Conv2d layout (C, C, 3) flattened; axis 0 = 3x1 (along H),
 * 1 = 1x3 (along W); C a multiple of 16; scratch >= lf_conv1d_scratch_floats() floats.
 * ---------------------------------------------------------------------------------- */
long lf_conv1d_scratch_floats(int N, int H, int W, int C);
int lf_conv1d_fwd(const float* x, const float* w, const float* bias, float* y, int N, int H, int W, int C,
                  int axis, int dilation, int relu, float* scratch, void* stream);
int lf_conv1d_bwd_data(const float* gy, const float* w, const float* mask_src, float* gx, int N, int H, int W,
                       int C, int axis, int dilation, float* scratch, void* stream);
int lf_conv1d_bwd_weight(const float* x, const float* gy, float* gw, float* gb, int N, int H, int W, int C,
                         int axis, int dilation, float* scratch, void* stream);

/* additions since 5 -- frozen single-frame detector: at deployment the weights and running statistics do not change between
 * frames, so the BatchNorm fold of the inference engine is done ONCE into a persistent workspace and every call after it is the
 * kernels alone.
 * lf_erfnet_infer_fold: the fold-table upload and the one fold-and-pack launch that lf_erfnet_infer / lf_lane_infer /
 *   lf_lane_infer_seg do on every call, in the plan's current precision mode (lf_erfnet_set_precision), into `workspace`.  The
 *   folded region is the common prefix of the workspaces of lf_erfnet_infer_workspace_bytes, lf_lane_infer_workspace_bytes and
 *   lf_lane_infer_seg_workspace_bytes: a workspace sized by any of them can be folded and then handed to the matching call.
 *   Fold again after any change of a parameter, a running statistic or the plan's precision mode.
 * lf_lane_infer_folded / lf_lane_infer_seg_folded: lf_lane_infer / lf_lane_infer_seg on such a workspace -- the same schedule and
 *   the same results bit for bit, nothing uploaded, nothing folded.  params_host is still read (the stem and head kernels take
 *   their raw weights from it); params_dev and running_host are not.  flags: LF_INFER_THIN routes the tap-GEMM launches whose
 *   regular grid cannot fill the device (one camera frame) to a thin tiling with the same bits, in precision mode fp32 (fp32 tensors,
 *   fp32 matrix cores) and bf16 (bf16 tensors, bf16 matrix cores); 0 in the split-operand mode, which has no thin kernel. */
enum { LF_INFER_THIN = 1 };
int lf_erfnet_infer_fold(const lf_erfnet_plan* plan, const float* const* params_host, const float* const* params_dev,
                         float* const* running_host, void* workspace, size_t workspace_bytes, void* stream);
int lf_lane_infer_folded(const lf_erfnet_plan* plan, const float* img, const float* const* params_host,
                         const float* const* params_dev, float* const* running_host, const float* grid_xy, long grid_batch_stride,
                         int zero_rows, int order, double reg_ls, double y_offset, int act_kind, int use_cholesky,
                         float* logits_or_null, double* beta, int32_t* status, void* workspace, size_t workspace_bytes, int flags,
                         void* stream);
int lf_lane_infer_seg_folded(const lf_erfnet_plan* plan, const float* img, const float* const* params_host,
                             const float* const* params_dev, float* const* running_host, const float* grid_xy,
                             long grid_batch_stride, const float* gt_line_or_null, int L, int zero_rows, int order, double reg_ls,
                             double y_offset, int use_cholesky, uint8_t* classes_or_null, double* beta, int32_t* status,
                             void* workspace, size_t workspace_bytes, int flags, void* stream);

/* additions since 5 -- frozen --clas heads (the frozen single-frame detector carried through the line-type / horizon heads to the
 * lanes of the frame):
 * lf_convchain_infer_fold: the fold-table upload and the one fold-and-pack launch of lf_convchain_infer, in the plan's current
 *   precision mode (lf_convchain_set_precision), into a workspace of lf_convchain_infer_workspace_bytes that the caller keeps.
 *   Fold again after any change of a parameter, a running statistic or the plan's precision mode.
 * lf_convchain_infer_folded: the convolution launches of lf_convchain_infer on such a workspace -- the same results bit for bit,
 *   nothing uploaded, folded or allocated.  flags: LF_INFER_THIN, as for lf_lane_infer_folded.
 * lf_clas_tail: everything behind the two trunks, three dependent launches.  y_line / y_hor (N,H,W,C) NHWC trunk outputs (fp32, or
 *   bf16 elements with bf16 != 0; H and W even); w1 (O1, C*(H/2)*(W/2)), b1: fully_connected1 (+ReLU); wl (4, O1), bl:
 *   fully_connected_line1; wh (R, C*H), bh: fully_connected_horizon; beta (N,L,order+1) fp64, L in 1..4; y_eval, y_prime (S), minv_host,
 *   scale, lo, hi, fill as lf_lane_decode.  Outputs: line (N,4) and horizon (N,R) fp32 logits (the bits of lf_poolflat_* +
 *   lf_linear_fwd), line_flags (N,4) fp32 = round(sigmoid(line)), horizon_row (N) int32 = round((sum sigmoid(horizon) * 2.5 + 80) /
 *   10) * 10 (the sum in fp64, a fixed order), lanes (N,L,S) int32 = lf_lane_decode's x_int with line_flag[n][l] = line_flags[n][{1,2,0,3}[l]]
 *   and bound[n] = trunc((horizon_row[n] - 160) / 10) (BP/test.py:60-88).  Workspace: lf_clas_tail_workspace_bytes; nothing persists
 *   in it between calls. */
int lf_convchain_infer_fold(const lf_convchain_plan* plan, const float* const* params_host, const float* const* params_dev,
                            float* const* running_host, float eps, void* workspace, size_t workspace_bytes, void* stream);
int lf_convchain_infer_folded(const lf_convchain_plan* plan, const float* x, float* y, void* workspace, size_t workspace_bytes,
                              int flags, void* stream);
size_t lf_clas_tail_workspace_bytes(int N, int H, int W, int C, int O1);
int lf_clas_tail(const void* y_line, const void* y_hor, int bf16, int N, int H, int W, int C, const float* w1, const float* b1,
                 int O1, const float* wl, const float* bl, const float* wh, const float* bh, int R, const double* beta, int L,
                 int order, const double* y_eval, const double* y_prime, int S, const double* minv_host, double scale, double lo,
                 double hi, double fill, float* line, float* horizon, float* line_flags, int32_t* horizon_row, int32_t* lanes,
                 void* workspace, size_t workspace_bytes, void* stream);

/* additions since 5 -- camera frames: the frozen detector's calls from decoded uint8 HWC camera frames (N,Hin,Win,3), what the
 * reference's LaneTestSet.__getitem__ starts from (BP/Dataloader/Load_Data_new.py:55-65: crop, Pillow BILINEAR resize, ToTensor), in
 * the place of the fp32 (N,3,H,W) image.  `pipe` is an lf_pipeline_plan whose output size is the network plan's H x W, tables_dev
 * the buffer lf_pipeline_upload filled.  RGB only: the network plan has 3 input channels (frames in BGR, NV12 or YUYV become RGB in
 * the staging: "additions since 5 -- frame formats" below).
 * lf_lane_infer_folded_u8 / lf_lane_infer_seg_folded_u8: lf_lane_infer_folded / lf_lane_infer_seg_folded with (pipe, tables_dev,
 *   frames) for img; the results are those of lf_pipeline_image followed by the call on its output, bit for bit.  The resize and the
 *   stem run as ONE launch (the resized image stays in LDS) where lf_pipeline_frame_stem_ok(pipe) is 1; where it is 0 (the source
 *   window of a tile does not fit 64 KB of LDS: 640 x 1280 -> 64 x 128) or with LF_INFER_FRAME_TWO_LAUNCH in flags, as two launches
 *   through an fp32 image slot at the end of the workspace.
 * lf_lane_infer_u8_workspace_bytes / lf_lane_infer_seg_u8_workspace_bytes: lf_lane_infer_workspace_bytes /
 *   lf_lane_infer_seg_workspace_bytes + that image slot, always: one workspace serves both forms.  The folded prefix is the same
 *   (lf_erfnet_infer_fold).
 * lf_pipeline_frame_stem_ok: 1 where the one-launch kernel takes the plan's geometry (even output size, a tile that fits), else 0;
 *   lf_pipeline_frame_stem_lds_bytes: the LDS bytes of one of its workgroups (0 where it does not fit);
 *   lf_pipeline_frame_stem_tile: its tile of stem output pixels (0 x 0 where it does not fit). */
enum { LF_INFER_FRAME_TWO_LAUNCH = 2 };
int lf_pipeline_frame_stem_ok(const lf_pipeline_plan* plan);
size_t lf_pipeline_frame_stem_lds_bytes(const lf_pipeline_plan* plan);
int lf_pipeline_frame_stem_tile(const lf_pipeline_plan* plan, int* tile_h, int* tile_w);
size_t lf_lane_infer_u8_workspace_bytes(const lf_erfnet_plan* plan, int mode, int K, int order);
size_t lf_lane_infer_seg_u8_workspace_bytes(const lf_erfnet_plan* plan, int mode, int L, int order);
int lf_lane_infer_folded_u8(const lf_erfnet_plan* plan, const lf_pipeline_plan* pipe, const void* tables_dev, const uint8_t* frames,
                            const float* const* params_host, const float* const* params_dev, float* const* running_host,
                            const float* grid_xy, long grid_batch_stride, int zero_rows, int order, double reg_ls, double y_offset,
                            int act_kind, int use_cholesky, float* logits_or_null, double* beta, int32_t* status, void* workspace,
                            size_t workspace_bytes, int flags, void* stream);
int lf_lane_infer_seg_folded_u8(const lf_erfnet_plan* plan, const lf_pipeline_plan* pipe, const void* tables_dev,
                                const uint8_t* frames, const float* const* params_host, const float* const* params_dev,
                                float* const* running_host, const float* grid_xy, long grid_batch_stride,
                                const float* gt_line_or_null, int L, int zero_rows, int order, double reg_ls, double y_offset,
                                int use_cholesky, uint8_t* classes_or_null, double* beta, int32_t* status, void* workspace,
                                size_t workspace_bytes, int flags, void* stream);

/* additions since 5 -- frame formats: what the frames pointer of a plan holds.  Decoders write NV12, USB / CSI cameras deliver YUYV,
 * OpenCV decodes to BGR; the staging of a source window converts to RGB in registers, and everything behind it (both resize passes,
 * ToTensor, the fused stem) runs on those uint8 RGB values as on packed RGB frames.  Contiguous uint8, pitch = width:
 *   LF_FRAME_RGB, LF_FRAME_BGR  (N,Hin,Win,3) packed;
 *   LF_FRAME_NV12               (N,Hin*3/2,Win): Hin rows of Y, then Hin/2 rows of interleaved Cb Cr pairs; Hin and Win even;
 *   LF_FRAME_YUYV               (N,Hin,Win,2): Y0 Cb Y1 Cr per pixel pair; Win even.
 * The chroma of pixel (y, x) is the pair at chroma row y >> 1, column x >> 1 (NV12) / of pixel pair x >> 1 in row y (YUYV), y the row
 * in the FULL frame (an odd crop_top is legal): replicated, not interpolated.  YCbCr -> RGB is this Q16 form, arithmetic shift:
 *   y' = Y - y_off;  u = Cb - 128;  v = Cr - 128
 *   R = clamp8((c_y y' + c_rv v + 32768) >> 16)
 *   G = clamp8((c_y y' - c_gu u - c_gv v + 32768) >> 16)
 *   B = clamp8((c_y y' + c_bu u + 32768) >> 16)
 * with coef = {c_y, y_off, c_rv, c_gu, c_gv, c_bu}: {65536, 0, 91881, 22554, 46802, 116130} is full-range BT.601 as libjpeg's
 * decoder computes it, bit for bit (the default); {76309, 16, 117489, 13975, 34925, 138438} is limited-range BT.709.
 * Bit contract: every result of a call on frames in format F equals the same call on an LF_FRAME_RGB plan of the same geometry, fed the
 * RGB frames this definition makes from them.
 * lf_pipeline_plan_set_format: sets the format of a plan (host only, no device is touched).  coef may be NULL for LF_FRAME_RGB /
 *   LF_FRAME_BGR (it is ignored there) and for the YCbCr formats (the default above).  Refuses an unknown format, an odd Hin or Win
 *   for NV12, an odd Win for YUYV, and coefficients with which an intermediate could leave int32.  A plan that never gets this call
 *   is an LF_FRAME_RGB plan.  Every entry point that takes a plan and a frames pointer (lf_pipeline_image, lf_pipeline_image_indexed,
 *   lf_lane_infer_folded_u8, lf_lane_infer_seg_folded_u8) reads the format from the plan; labels know no format.
 * lf_pipeline_frame_bytes: the bytes of one frame in the plan's format (Hin Win 3, Hin Win 3 / 2, Hin Win 2); 0 for a NULL plan.  No
 *   load reaches past N (pool_frames) times this many bytes behind the frames pointer. */
enum { LF_FRAME_RGB = 0, LF_FRAME_BGR = 1, LF_FRAME_NV12 = 2, LF_FRAME_YUYV = 3 };
int lf_pipeline_plan_set_format(lf_pipeline_plan* plan, int format, const int coef[6]);
size_t lf_pipeline_frame_bytes(const lf_pipeline_plan* plan);

/* additions since 5 -- surfaces: frames as a decoder leaves them.  A hardware decoder writes NV12 with a row pitch aligned to 256
 * bytes and the chroma plane behind an aligned height (720 -> 736 rows), often in an allocation of its own; a batch of cameras is N
 * surfaces of a pool; software decoders give planar I420, compositors and capture cards 4-byte RGBX / BGRX.  A frame layout on the
 * plan lifts "contiguous, pitch = width" of the block above: the staging reads the surface where it lies, no repacking pass.
 * Planes, rows x row bytes (Hin x Win pixels):
 *   LF_FRAME_RGB, LF_FRAME_BGR    one plane, Hin x 3 Win;
 *   LF_FRAME_RGBX, LF_FRAME_BGRX  one plane, Hin x 4 Win: R G B X / B G R X per pixel, the fourth byte is ignored;
 *   LF_FRAME_YUYV                 one plane, Hin x 2 Win; Win even;
 *   LF_FRAME_NV12                 Y: Hin x Win; CbCr: Hin/2 x Win; Hin and Win even;
 *   LF_FRAME_I420                 Y: Hin x Win; Cb: Hin/2 x Win/2; Cr: Hin/2 x Win/2; Hin and Win even.  YV12 is I420 with the
 *                                 offsets (or the pointers) of planes 1 and 2 exchanged.
 * The chroma of I420 pixel (y, x) is sample (y >> 1, x >> 1) of each chroma plane, replicated as for NV12; the Q16 YCbCr -> RGB form
 * and coef are those of the block above.
 * lf_frame_layout: pitch[p] bytes between rows of plane p (0 = the row's own bytes); plane_offset[p] bytes from a frame's base to
 *   plane p ([0] must be 0; 0 for p > 0 = directly behind plane p - 1, its rows x its pitch); frame_stride bytes between the frames
 *   of a contiguous batch (0 = the end of the furthest plane at full pitch).  plane_pointers = 0: `frames` is the base of a
 *   contiguous batch, 4-byte aligned.  plane_pointers = 1: `frames` is a DEVICE array (N, planes) of plane base pointers, row n the
 *   planes of batch element n -- separate allocations, surfaces of a pool in any order; plane_offset and frame_stride are then not
 *   looked at, whatever they hold (nor, in either mode, the values of planes the format lacks).
 *   Each pointer must be 4-byte aligned (2 bytes suffice for the NV12 CbCr plane): no host-only call can check a device table, it is
 *   the caller's contract.  For a CbCr pointer that is only 2-byte aligned the staging loads the aligned dword that holds the plane's
 *   first two bytes, i.e. it reads the 2 bytes in front of the pointer too (the same memory granule; they reach no result).
 * lf_pipeline_plan_set_layout: sets format and layout of a plan (host only); coef as for lf_pipeline_plan_set_format (NULL: keeps the
 *   plan's).  Returns != 0, leaves the plan untouched and sets lf_last_error for: a NULL plan or layout; an unknown format; an odd
 *   Hin or Win for NV12 / I420, an odd Win for YUYV; a negative value; a pitch below the row's bytes; plane_offset[0] != 0;
 *   coefficients that overflow int32; and the alignment the staging relies on --
 *     YUYV, RGBX, BGRX: pitch, plane offset and frame stride multiples of 4 (every pixel group is one aligned dword);
 *     NV12: CbCr pitch and offset even, and the frame stride even (it moves the CbCr plane of every frame but the first).
 *   RGB, BGR and I420 take any pitch, offset and stride (odd ones too).  LF_FRAME_I420, _RGBX and _BGRX are reachable only through this
 *   call: lf_pipeline_plan_set_format keeps refusing codes >= 4, and after a set_layout it resets the plan to a tight plan of its format.
 * lf_pipeline_surface_span: plane >= 0 -- (rows_p - 1) pitch_p + row bytes_p, the bytes a plane pointer must grant (0 for a plane the
 *   format does not have); plane < 0 -- the furthest byte of one frame, max over p of plane_offset_p + span_p.  On a plan without a
 *   layout: those of its tight frames.
 * lf_pipeline_frame_bytes returns the frame stride on a layout plan.
 * Bit contract: that of the frame formats -- every result of every entry point that takes a plan and a frames pointer
 *   (lf_pipeline_image, lf_pipeline_image_indexed, lf_lane_infer_folded_u8, lf_lane_infer_seg_folded_u8) equals the same call on a
 *   tight LF_FRAME_RGB plan fed the RGB frames the definition makes from the surface's pixels.  No padding byte influences a result.
 * Bounds: contiguous mode -- no load reaches past (N - 1) frame_stride + span(-1) bytes behind `frames` (N = pool_frames for the
 *   indexed call); pointer mode -- no load for plane p of frame n reaches past span(p) bytes behind that pointer.
 * lf_pipeline_image_indexed on a plane_pointers plan is refused at the call: it covers contiguous pools only.
 * Tight plans run the kernels they always ran; a layout plan runs resize_surface_kernel / frame_surface_stem_kernel. */
enum { LF_FRAME_I420 = 4, LF_FRAME_RGBX = 5, LF_FRAME_BGRX = 6 };
typedef struct lf_frame_layout {
    int  format;            /* any LF_FRAME_* 0..6 */
    int  plane_pointers;    /* 0: `frames` is the base of a contiguous batch; 1: `frames` is a device array (N, planes) of plane base pointers */
    long pitch[3];          /* bytes between rows of plane p; 0 = tight (the row's own bytes) */
    long plane_offset[3];   /* bytes from a frame's base to plane p; [0] must be 0; 0 for p > 0 = directly behind plane p-1 (its rows x its pitch) */
    long frame_stride;      /* bytes between frames of a contiguous batch; 0 = tight (end of the last plane at full pitch) */
} lf_frame_layout;
int    lf_pipeline_plan_set_layout(lf_pipeline_plan* plan, const lf_frame_layout* layout, const int coef[6]);
size_t lf_pipeline_surface_span(const lf_pipeline_plan* plan, int plane);

/* additions since 5 -- input-image gradient: d loss / d input of Net.forward, what `input.requires_grad_()` before the forward and
 * `loss.backward()` (BEV/main.py:264-266) give in the reference -- the data gradient of the stem DownsamplerBlock's
 * cat[conv3x3 s2 p1 (input), max_pool2d(input, 2)] (BEV/Networks/ERFNet.py:11-22,66), the one layer that had none.
 * lf_stem_bwd_data: gcat (N,H/2,W/2,16) NHWC = the gradient of the block's pre-BatchNorm concat buffer (fp32, or bf16 bit patterns
 *   with s16 = 1, widened exactly), img (N,Cin,H,W) NCHW fp32, w (16-Cin,Cin,3,3) the raw convolution weight -> gimg (N,Cin,H,W)
 *   NCHW fp32: every element WRITTEN (not accumulated), by a gather without atomics (the same bits on every launch); fp32
 *   products and sums.  The pooled channels' gradient goes to the first maximum of each 2x2 window in scan order (ATen's
 *   max_pool2d rule); every other pixel of the window takes exactly nothing from it.  Cin 1..4, any even H and W, both tensors
 *   within 32-bit byte offsets.
 * lf_erfnet_backward_input: lf_erfnet_backward with grad_img (N,Cin,H,W) in front of the workspace.  NULL: lf_erfnet_backward
 *   itself, launch for launch.  Otherwise ONE launch more, lf_stem_bwd_data behind the stem's weight gradient (also when the stem's
 *   weight is frozen and takes none); every precision mode, training 0 / 1, head -1 / 0 / 1, with and without grad_encoder; no
 *   workspace beyond lf_erfnet_workspace_bytes_for. */
int lf_stem_bwd_data(const float* gcat, const float* img, const float* w, int N, int Cin, int H, int W, int s16, float* gimg,
                     void* stream);
int lf_erfnet_backward_input(const lf_erfnet_plan* plan, const float* img, const float* grad_logits,
                             const float* grad_encoder, const float* const* params_host, float* const* grads_host,
                             const float* dropmask, int training, int head, float* grad_img, void* workspace,
                             size_t workspace_bytes, void* stream);

/* additions since 5 -- segmentation-mode detect: the test-time path of a model trained with end_to_end = False (the reference's
 * baseline and its pre-training epochs), Net.forward's arg-max branch (BEV/Networks/LSQ_layer.py:302-308,
 * BP/Networks/LSQ_layer.py:279-293,308-311) fused with decoder.output_conv and the fit.
 * lf_head_fit_seg: one pass over the last decoder layer's tensor -> the C class logits of every output pixel (lf_head_fit's head),
 *   their arg-max (first maximum, NaN maximal), the L lane maps valued l + 1 where class l + 1 wins and the moment pass of their fit
 *   (activation none); neither the logits nor the maps are written.  beta, zinv and status equal lf_seg_maps + lf_wls_fwd on the
 *   head's logits BIT FOR BIT (the same partition of the pixels over threads, the same order of every fp64 addition).
 *     x (N,h,w,16) NHWC fp32 (x_bf16 = 0) or bf16 bit patterns (1); head_w (16,C,2,2), head_b (C) fp32; C <= 5, L <= 4; L >= C is
 *       allowed (a lane whose class does not exist never wins: singular); w must be even (4 output pixels of a unit share a row);
 *     grid_xy, grid_batch_stride, zero_rows, order, reg, y_offset, solver, beta (N,L,order+1), zinv, partials
 *       (>= lf_wls_workspace_bytes(N,L,order)), status (N*L): as lf_wls_fwd on the (N,L,2h,2w) maps.  Input rows that feed only
 *       output rows < zero_rows are never read, nor is the grid on those rows;
 *     gt_line_or_null (N,L) fp32 flags as lf_seg_maps (BP's "prevent singular matrix"): a flagged lane (n, l) fits the map of image
 *       0, lane 0 against image n's grid; lane (0, 0) itself is left as it is;
 *     classes_or_null (N,2h,2w) uint8: the arg-max class of every pixel; when requested every row is computed for it (the fit
 *       still skips the masked rows).
 * lf_lane_infer_seg: image -> lane polynomials in one call = lf_erfnet_infer's schedule up to the last decoder layer, then
 *   lf_head_fit_seg on head 0 with C = the plan's out_channels; every precision mode.  Arguments as lf_lane_infer.
 * lf_lane_infer_seg_workspace_bytes: the inference workspace + the chunk partials and saved inverses of N * L lanes; 0 for an
 *   unknown mode, order outside 0..3 or L outside 1..4. */
int lf_head_fit_seg(const void* x, int x_bf16, const float* head_w, const float* head_b, const float* grid_xy, long grid_batch_stride,
                    const float* gt_line_or_null, int N, int h, int w, int C, int L, int zero_rows, int order, double reg,
                    double y_offset, int solver, uint8_t* classes_or_null, double* beta, double* zinv, void* partials,
                    int32_t* status, void* stream);
size_t lf_lane_infer_seg_workspace_bytes(const lf_erfnet_plan* plan, int mode, int L, int order);
int lf_lane_infer_seg(const lf_erfnet_plan* plan, const float* img, const float* const* params_host, const float* const* params_dev,
                      float* const* running_host, const float* grid_xy, long grid_batch_stride, const float* gt_line_or_null, int L,
                      int zero_rows, int order, double reg_ls, double y_offset, int use_cholesky, uint8_t* classes_or_null,
                      double* beta, int32_t* status, void* workspace, size_t workspace_bytes, void* stream);
#ifdef __cplusplus
}
#endif
#endif /* LANEFIT_H */
