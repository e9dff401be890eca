// Test / tooling hooks of liblanefit_hip.so (NOT part of the public C ABI in include/lanefit.h): the phase-stamp entries of
// tools/kbench.py and the precision selector of the kernel-level lf_conv1d_* parity tests.  Exported with C linkage so
// that ctypes can reach them; process-global state, never touched by the product path.
#pragma once
#ifdef __cplusplus
extern "C" {
#endif
/* 1: the split kernels also take launches below their shipped size rule (kernel-level tests at small shapes) */
void lf_debug_set_split_any_size(int v);
/* which bf16-tensor tap-GEMM kernels run: 4 (shipped) wave-private kernel at 64 channels, whole-line kernel at 128, 16-channel kernels
   where they apply, else the ring; 3 the whole-line kernel at 64 channels too (round 5's routing); 2 the ring for every launch it takes;
   0 the streaming kernel only (A/B timing, bit-identity of the forms: tools/bf16_ab.py, tests/test_bf16_kernels_gpu.py) */
void lf_debug_set_bf16_lds(int v);
/* 1: bf16-tensor launches whose source-channel count is no multiple of 32 (16, 48) decline the compiled-in whole-step forms of
   tapgemm_bf16_kernel and run on its run-time-flag form, which clamps a partial step's channel offsets inside the pixel; 0 (shipped):
   the compiled-in forms.  The two agree bit for bit (tests/test_bf16_stride2_kernels_gpu.py) */
void lf_debug_set_bf16_no_partial_fast(int v);
/* launches with Cs % 32 != 0 that took one of those compiled-in forms since the process started: which form a launch selected */
long lf_debug_partial_fast_launches(void);
/* launches tapgemm_bf16_ring_kernel (the persistent LDS-DMA ring) took since the process started: which bf16 kernel a launch selected */
long lf_debug_bf16_ring_launches(void);
/* v > 0 caps grid.x of the resident bf16-tensor launches (ring, whole-line, wave-private kernels), so that one workgroup walks several
   items -- across tiles and output slabs -- at small shapes; 0 (shipped) leaves every launch as it is.  Capped and uncapped runs agree
   bit for bit (tests/test_bf16_stride2_kernels_gpu.py, tests/test_bf16_kernels_gpu.py) */
void lf_debug_set_bf16_max_workgroups(int v);
/* precision mode of the lf_conv1d_* calls: 0 fp32, 2 bf16 matrix cores on bf16 tensors (x, y, gx, gy, mask_src hold bf16; w, bias,
 * gw, gb stay fp32), 9 fp32 from 9-term split operands (modes 1 and 6 were removed in round 6 and select 0) */
void lf_debug_set_ops_precision(int mode);
/* lf_conv1d_fwd + per-wave s_memrealtime stamps (100 MHz) (start, tap table built, main loop done, stores
 * retired; 8 words per wave) */
int lf_debug_conv1d_fwd_phases(const float* x, const float* w, const float* bias, float* y, int N, int H, int W, int C,
                               int axis, int dilation, float* scratch, unsigned long long* dbg, void* stream);
/* the weight-gradient launch of lf_conv1d_bwd_weight with the same stamps (start, first operands, main loop done, partials
 * stored, HW id); returns the number of waves launched, -1 on error */
// lf_conv1d_fwd with the BN+ReLU operand prologue and the ReLU epilogue (the third convolution of a non_bottleneck_1d block):
// y = relu(conv1d(relu(x * sc + sh)) + bias); sc, sh: [C] fp32.  Kernel-level tests of the prologue forms (tests/test_bf16_kernels_gpu.py)
int lf_debug_conv1d_fwd_pro(const float* x, const float* w, const float* bias, const float* sc, const float* sh, float* y, int N, int H,
                            int W, int C, int axis, int dilation, float* scratch, void* stream);
/* the read-once bf16 weight gradient (lf_wgrad_ro.hip): mode 0 = off (tapwgrad_kernel's job form takes every launch), 1 = shipped;
 * cap64 / cap128 > 0: workgroups per launch at 64 / 128 channels (A/B runs; at most the shipped 512 / 256 the buffers are sized for) */
void lf_debug_set_wgrad_ro(int mode, int cap64, int cap128);
/* the fp32 3-tap C -> C tap-GEMM launches at 64 / 128 channels and whole-row waves (tapstream_kernel, lf_conv.hip): mode 0 =
 * tapgemm_kernel takes every launch, 1 = the shipped routing, 2 = every variant tapstream_kernel is compiled for; max_workgroups > 0
 * caps the grid, so that one workgroup walks several tiles at small shapes.  The kernels agree bit for bit (tests/test_fp32_stream_gpu.py) */
void lf_debug_set_fp32_stream(int mode, int max_workgroups);
/* the 3x1 -> 1x3 forward pairs of the non_bottleneck_1d blocks on fp32 tensors (tappair_kernel, csrc/lf_conv_pair.hip): mode 0 = two
 * launches, 1 = the shipped routing (the forms that lowered the step), 2 = every compiled form, 4 * m = the compiled forms of bit mask m
 * (1 / 2: 64 channels without / with the BN+ReLU prologue, 4 / 8: 128 channels; A/B runs in the step); max_workgroups > 0 caps the grid, so
 * that one workgroup walks several tiles at small shapes.  One launch and two agree bit for bit (tests/test_fwd_pair_gpu.py) */
void lf_debug_set_fwd_pair(int mode, int max_workgroups);
/* One pair on caller tensors, routed as the network routes it (lf_debug_set_fwd_pair; a pair the fused kernel does not take runs as
 * two launches):  t = relu(conv3x1(pro(x)) + ba),  y = conv1x3(t) + bb, both with the dilation given; pro = relu(x * sc + sh) when sc
 * and sh ([C] fp32) are given, else the identity.  x, t, y (N,H,W,C) NHWC fp32; wa, wb (C,C,3).  stats: [2][C][rows] BatchNorm forward
 * rows of y (sum, M2 about the row's own mean), rows = ceil(N * H * W / 256).  scratch: lf_conv1d_scratch_floats floats.  Returns 1
 * where the pair ran as one launch, 0 as two, -1 on error. */
int lf_debug_conv1d_fwd_pair(const float* x, const float* wa, const float* ba, const float* wb, const float* bb, const float* sc,
                             const float* sh, float* t, float* y, float* stats, int N, int H, int W, int C, int dilation, float* scratch,
                             void* stream);
/* fp32 16-channel 3-tap convolutions in backward: 0 = weight gradient and data gradient as two launches, 1 = the shipped routing
 * (tapbwd16_kernel, csrc/lf_bwd16.hip, takes the pairs it is routed for in one launch), 2 * m = exactly the forms of bit mask m
 * (1 mask, 2 recomputed-BN mask + sums with the prologue, 4 residual + mask + sums, 8 residual: A/B runs in the step) */
void lf_debug_set_bwd16_fused(int mode);
/* One fused backward launch of a 16 -> 16 channel 3-tap convolution (fp32 tensors) followed by the immediate reduction of its
 * weight-gradient rows, as lf_conv1d_bwd_weight runs it:
 *   gx = epilogue(conv1d^T(gy))   with the flag set epi of csrc/lf_conv.h -- one of the four sets the kernel is compiled for;
 *   gw, gb = the weight and bias gradient against pro(x), pro = relu(x * pro_sc + pro_sh) when pro_sc is given.
 * The mask (LF_EPI_MASK) and the MASKBN / BN-sums operand of the MASKBN form are x itself; add_src and, beside LF_EPI_MASK, aux are
 * tensors of their own.  stats: [2][C][rows], rows = ceil(N * H * W / 256).  scratch: lf_debug_conv1d_bwd_pair_scratch_floats floats.
 * Returns the statistics rows written (0 without a sums flag), -1 on error -- also where the fused kernel does not take the launch. */
long lf_debug_conv1d_bwd_pair_scratch_floats(int N, int H, int W, int C);
int lf_debug_conv1d_bwd_pair(const float* x, const float* gy, const float* w, int epi, const float* add_src, const float* aux,
                             const float* msc, const float* msh, const float* pro_sc, const float* pro_sh, float* gx, float* gw, float* gb,
                             float* stats, int N, int H, int W, int C, int axis, int dilation, float* scratch, void* stream);
/* lf_conv1d_bwd_weight with the BN+ReLU operand prologue on x (the weight gradient of a non_bottleneck_1d block's third convolution):
 * gw = d/dw of conv1d(relu(x * sc + sh)), gb = column sums of gy */
int lf_debug_conv1d_wgrad_pro(const float* x, const float* gy, const float* sc, const float* sh, float* gw, float* gb, int N, int H, int W,
                              int C, int axis, int dilation, float* scratch, void* stream);
/* lf_conv1d_bwd_data with the THREE-TENSOR epilogue of the network's last data gradient per block (ADD + MASK + BN-backward sums,
 * ERFNet.py:44-60 backward): gx = (conv1d^T(gy) + add_src) * [mask_src > 0]; stats receives the per-tile partial rows
 * [2][C][rows] (channel-major: element (kind, c, row)) = (sum gx, sum gx * aux) -- raw, as lf_bn_bwd_finalize consumes them.  Returns the number of rows, -1 on error. */
int lf_debug_conv1d_bwd_data_epi3(const float* gy, const float* w, const float* mask_src, const float* add_src, const float* aux,
                                  float* gx, float* stats, int N, int H, int W, int C, int axis, int dilation, float* scratch, void* stream);
/* one convolution launch with any epilogue flag set of csrc/lf_conv.h (1 ReLU, 2 mask by mask_src > 0, 4 + add_src, 8 BN forward sums,
 * 16 mask by aux * msc + msh > 0, 32 BN-backward sums over aux); transposed = 1: the data gradient's weights.  Returns the number of
 * statistics rows written (channel-major [2][C][rows]; BN forward sums: kind 1 = M2 about the row's own mean), 0 without a sums flag, -1 on error.  (tests/test_lean_gpu.py) */
int lf_debug_conv1d_epi(const float* src, const float* w, const float* bias, float* dst, int transposed, int epi, const float* mask_src,
                        const float* add_src, const float* aux, const float* msc, const float* msh, float* stats, int N, int H, int W, int C,
                        int axis, int dilation, float* scratch, void* stream);
/* one tap-GEMM launch of a stride-2 layer, with the geometry and the weight gather the ERFNet plan builds (lf_plan.h), any epilogue flag
 * set of csrc/lf_conv.h and the precision of lf_debug_set_ops_precision (0 fp32, 2 bf16 tensors).  (N, H, W): the LARGER tensor, H and W even.
 *   kind 0  DownsamplerBlock conv forward: Conv2d(Cin, Cout, 3, stride 2, pad 1); src (N,H,W,Cin) -> channels [0, Cout) of dst
 *           (N,H/2,W/2,Cin+Cout), the block's concat buffer; w (Cout,Cin,3,3)
 *   kind 1  its data gradient, sub-pixel phase (a, b) = (phase >> 1, phase & 1): src (N,H/2,W/2,Cin+Cout) read at channels [0, Cout)
 *           -> pixels (2i+a, 2j+b) of dst (N,H,W,Cin)
 *   kind 2  UpsamplerBlock forward phase: ConvTranspose2d(Cin, Cout, 3, stride 2, pad 1, output_padding 1), w (Cin,Cout,3,3);
 *           src (N,H/2,W/2,Cin) -> pixels (2i+a, 2j+b) of dst (N,H,W,Cout)
 *   kind 3  its data gradient: src (N,H,W,Cout) -> dst (N,H/2,W/2,Cin)
 * mask_src, add_src, aux: tensors of the destination's layout; bias fp32 [produced channels]; scratch: 9 * roundup(Kc, 32) * Nc floats.
 * stats: [2][produced channels][rows], rows = ceil(logical pixels / 256).  Returns the rows written (0 without a sums flag), -1 on error. */
int lf_debug_stride2_epi(int kind, int phase, const float* src, const float* w, const float* bias, float* dst, int epi, const float* mask_src,
                         const float* add_src, const float* aux, float* stats, int N, int H, int W, int Cin, int Cout, float* scratch,
                         void* stream);
/* the weight + bias gradient of a stride-2 layer as the ERFNet plan issues it (run_wgrad, lf_erfnet.hip): tapwgrad_kernel over the plan's
 * forward geometries (lf_plan.h) and one of the two reductions, in the precision of lf_debug_set_ops_precision (0 fp32, 2: x and g hold
 * bf16; partial rows, gw, gb stay fp32).  (N, H, W): the LARGER tensor, H and W even.  Its own kind numbering (NOT lf_debug_stride2_epi's):
 *   kind 0  DownsamplerBlock conv: x (N,H,W,Cin), g (N,H/2,W/2,Cin+Cout) read at channels [0, Cout); gw (Cout,Cin,3,3); one launch
 *   kind 2  UpsamplerBlock transposed conv: x (N,H/2,W/2,Cin), g (N,H,W,Cout); gw (Cin,Cout,3,3); four sub-pixel-phase launches, which
 *           reduce into disjoint 3x3 elements of gw and into ONE bias gradient
 *   reduce 0  immediate: lf_wgrad_reduce_launch behind every launch from one shared partial region, the bias accumulating for phases
 *             1..3 (run_wgrad with batch_off)
 *   reduce 1  batched: every launch keeps its own partial region, the phases' bias rows are chained end to end (LfBiasChain, lf_plan.h:
 *             only the last job carries a bias pointer) and one lf_wgrad_reduce_batch_launch follows
 * gb [Cout] may be null (a bias that does not require grad: no bias rows are written).  scratch: lf_debug_stride2_wgrad_scratch_floats
 * floats -- exactly what the call may touch: [weight regions][bias regions], each sized from lf_tapwgrad_splits_bound as the plan
 * sizes its own, without padding.  Returns the partial rows written, summed over the launches; -1 on error. */
long lf_debug_stride2_wgrad_scratch_floats(int kind, int reduce, int N, int H, int W, int Cin, int Cout);
int lf_debug_stride2_wgrad(int kind, int reduce, const float* x, const float* g, float* gw, float* gb, int N, int H, int W, int Cin,
                           int Cout, float* scratch, void* stream);
/* the stem's weight gradient (stem_wgrad_kernel + its row sums, lf_stem.hip): img (N,Cin,H,W) fp32 NCHW, gcat (N,H/2,W/2,16) -- bf16 in
 * mode 2 -- read at channels [0, 16 - Cin); gw (16 - Cin,Cin,3,3), gb [16 - Cin] or null.  reduce 0: lf_rows_reduce_launch per tensor;
 * 1: the row-sum jobs of row_sums_finish (lf_plan.h) in one lf_wgrad_reduce_batch_launch.  scratch: [rows][gw elements] then
 * [rows][gb elements], rows = the workgroups of the launch (at most 1024).  Returns the rows written, -1 on error. */
long lf_debug_stem_wgrad_scratch_floats(int N, int Cin, int H, int W);
int lf_debug_stem_wgrad(int reduce, const float* img, const float* gcat, float* gw, float* gb, int N, int Cin, int H, int W, float* scratch,
                        void* stream);
/* the head's weight gradient (head_wgrad_kernel + its row sums): x (N,h,w,16) -- bf16 in mode 2 --, gout (N,K,2h,2w) fp32 NCHW;
 * gw (16,K,2,2), gb [K] or null; reduce, scratch layout and return value as above */
long lf_debug_head_wgrad_scratch_floats(int N, int h, int w, int K);
int lf_debug_head_wgrad(int reduce, const float* x, const float* gout, float* gw, float* gb, int N, int h, int w, int K, float* scratch,
                        void* stream);
/* ---- ONE launch of a bandwidth-bound backbone kernel (csrc/lf_eltwise.h: BatchNorm finalise / apply / backward, max-pool branch, stem
 * forward, head forward / data gradient), as the ERFNet plan issues it.  (tests/test_eltwise_gpu.py)
 * Common to all of them: activation and gradient tensors are NHWC fp32 (s16 = 0) or NHWC bf16 (s16 = 1; the pointers still travel as
 * float*) -- s16 is an argument, lf_debug_set_ops_precision is NOT read; per-channel vectors, statistics rows, the image, the logits and
 * every parameter are fp32 either way.  Tensor and vector pointers are 16-byte aligned.  Every hook checks its pointers and sizes on the
 * host and returns -1 (lf_last_error) WITHOUT launching where the launcher's own geometry would not hold.
 *
 * A source of partial rows is eight flat arguments (rows, nrows, ld, C, ch_off, tile_pix, seg_rows, seg_pix) = LfStatPart:
 *   rows      [2][C][ld] fp32, CHANNEL-MAJOR: element (kind, c, row) = rows[(kind * C + c) * ld + row]; only row < nrows is read -- the
 *             floats in [nrows, ld) may hold anything.  ld >= nrows, ld % 4 == 0, rows 16-byte aligned.  rows = NULL: no such source.
 *   C, ch_off the source covers channels [ch_off, ch_off + C) of the layer (multiples of 4); a channel no source covers sums to zero.
 *   tile_pix  0: RAW rows, kind 0 = sum v, kind 1 = sum v^2 (backward: sum g, sum g * t).
 *             > 0: CENTRED rows, kind 0 = sum v, kind 1 = M2 = sum (v - row mean)^2; row r covers pixels (r % seg_rows) * tile_pix .. of a
 *             launch of seg_pix pixels -- n_r = min(tile_pix, seg_pix - (r % seg_rows) * tile_pix) --, nrows % seg_rows == 0 (the four
 *             sub-pixel phases of a transposed convolution: nrows = 4 * seg_rows), (seg_rows - 1) * tile_pix < seg_pix <= seg_rows * tile_pix.
 *
 * lf_debug_bn_finalize_fwd: up to two sources, then the arguments of lf_bn_finalize_fwd.  training = 1: mean / biased variance (clamped
 * at 0) of `count` values per channel from the rows' fp64 column sums, running_mean / running_var updated in place (momentum; unbiased
 * variance, count / (count - 1), unless count == 1); training = 0: the running statistics are used and left alone, and zero sources are
 * allowed.  Writes, [C] each: scale = gamma * rstd, shift = beta - mean * scale, asc = rstd = 1 / sqrt(var + eps), ash = -mean * rstd.
 * Returns 0. */
int lf_debug_bn_finalize_fwd(const float* rows0, int nrows0, int ld0, int C0, int ch_off0, int tile_pix0, int seg_rows0, long seg_pix0,
                             const float* rows1, int nrows1, int ld1, int C1, int ch_off1, int tile_pix1, int seg_rows1, long seg_pix1,
                             int C, double count, const float* gamma, const float* beta, float* running_mean, float* running_var,
                             float momentum, float eps, int training, float* scale, float* shift, float* asc, float* ash, void* stream);
/* one or two sources of RAW backward rows (sum gm, sum gm * t; t = the pre-BatchNorm tensor), then the arguments of lf_bn_bwd_finalize:
 * with S1, S2 the column sums, gbeta = S1, ggamma = asc * S2 + ash * S1 (= sum gm * xhat), c1 = gbeta / count, c2 = ggamma / count --
 * c1 = c2 = 0 with training = 0 (the forward normalised with the running statistics).  [C] each.  Returns 0. */
int lf_debug_bn_bwd_finalize(const float* rows0, int nrows0, int ld0, int C0, int ch_off0, int tile_pix0, int seg_rows0, long seg_pix0,
                             const float* rows1, int nrows1, int ld1, int C1, int ch_off1, int tile_pix1, int seg_rows1, long seg_pix1,
                             int C, double count, const float* asc, const float* ash, float* c1, float* c2, float* ggamma, float* gbeta,
                             int training, void* stream);
/* y = relu((x * sc + sh) [* dm[n][c]] [+ res]); x, res, y (npix, C), pixel p belongs to image n = p / pix_per_image; dm [npix /
 * pix_per_image][C] fp32 (Dropout2d's per-image channel mask, already scaled) or NULL; res NULL: no residual.  C % 4 == 0.  Returns 0. */
int lf_debug_bn_act(const float* x, const float* sc, const float* sh, const float* dm, const float* res, float* y, long npix, int C,
                    long pix_per_image, int s16, void* stream);
/* gm = g * [y > 0] (y NULL: no mask) * dm (NULL: none); rows [2][C][ld] receives RAW partial rows (sum gm, sum gm * t), each over one
 * contiguous run of at most roundup(ceil(npix / rows), 256) pixels: row count = min(ceil(npix / 64), 1024) <= ld, which is also the
 * return value (lf_bn_bwd_reduce_rows); the floats of [rows, ld) are not written.  C / 4 a power of two <= 64.  asc / ash are not read. */
int lf_debug_bn_bwd_reduce(const float* g, const float* y, const float* t, const float* asc, const float* ash, const float* dm, float* rows,
                           int ld, long npix, int C, long pix_per_image, int s16, void* stream);
/* g_t = gamma * asc * (gm - c1 - (t * asc + ash) * c2), gm as above; g_z (optional) = g * [y > 0], BEFORE the dropout mask: the
 * gradient of the residual branch.  Returns 0. */
int lf_debug_bn_bwd_apply(const float* g, const float* y, const float* t, const float* asc, const float* ash, const float* gamma,
                          const float* c1, const float* c2, const float* dm, float* g_t, float* g_z, long npix, int C, long pix_per_image,
                          int s16, void* stream);
/* DownsamplerBlock pool branch: channels [choff, choff + Cin) of cat (N,H/2,W/2,cat_pix) = maxpool2x2(x), x (N,H,W,Cin); the other
 * channels of cat are not touched.  rows [2][Cin][ld] (or NULL) receives RAW partial rows (sum v, sum v^2) of the STORED values, row count
 * = min(ceil(N * H/2 * W/2 / 64), 1024) <= ld = the return value (lf_pool_rows), with or without rows; a row covers one contiguous
 * run of at most roundup(ceil(pixels / rows), 256) output pixels.  H, W even; Cin / 4 a power of two;
 * choff, cat_pix multiples of 4 (bf16: the 8-channel kernels need Cin, choff, cat_pix multiples of 8, else one quad per thread). */
int lf_debug_pool_concat_fwd(const float* x, int N, int H, int W, int Cin, float* cat, int cat_pix, int choff, float* rows, int ld, int s16,
                             void* stream);
/* inference form: cat[..., choff + c] = relu(maxpool2x2(x)[c] * sc[c] + sh[c]), sc / sh [Cin]; the affine map AFTER the max.  Returns 0. */
int lf_debug_pool_affine_fwd(const float* x, int N, int H, int W, int Cin, float* cat, int cat_pix, int choff, const float* sc, const float* sh,
                             int s16, void* stream);
/* gx (N,H,W,Cin): every element written -- gcat[..., choff + c] at the window's FIRST maximum in the scan order (0,0), (0,1), (1,0),
 * (1,1) (strict >, ATen's rule), zero at the other three.  Returns 0. */
int lf_debug_pool_bwd(const float* x, const float* gcat, int N, int H, int W, int Cin, int cat_pix, int choff, float* gx, int s16, void* stream);
/* stem, DownsamplerBlock(Cin, 16) on the NCHW fp32 image (N,Cin,H,W), Cin 1..4, H and W even: cat (N,H/2,W/2,16) = [Conv2d(Cin, 16 - Cin,
 * 3, stride 2, pad 1) | maxpool2x2]; w (16 - Cin,Cin,3,3), b [16 - Cin].
 *   sc = sh = NULL  training form: rows [2][16][ld] (or NULL) receives RAW partial rows (sum v, sum v^2) of the values before rounding to
 *                   the storage type, one per 256 output pixels; returns that count, ceil(N * H/2 * W/2 / 256) <= ld (lf_stem_rows)
 *   sc, sh [16]     inference form (lf_stem_fwd_infer): cat = relu(v * sc + sh), after the max for the pooled channels; rows and ld are
 *                   ignored; returns 0 */
int lf_debug_stem_fwd(const float* img, int N, int Cin, int H, int W, const float* w, const float* b, const float* sc, const float* sh, float* cat,
                      float* rows, int ld, int s16, void* stream);
/* frame_stem_kernel alone (csrc/lf_frame_stem.hip): frames (N,Hin,Win,3) uint8 HWC -> cat (N,out_h/2,out_w/2,16) = the inference form of
 * lf_debug_stem_fwd (Cin = 3; sc, sh [16]) on lf_pipeline_image's output, bit for bit, in one launch.  plan / tables_dev: an
 * lf_pipeline_plan and its uploaded tables.  Returns 0; -1 (lf_last_error) WITHOUT launching for a null pointer, a plan with an odd
 * out_h / out_w or one whose geometry does not fit the kernel (lf_pipeline_frame_stem_ok = 0).  (tests/test_frame_stem_gpu.py) */
struct lf_pipeline_plan;
int lf_debug_frame_stem(const struct lf_pipeline_plan* plan, const unsigned char* frames, int N, const void* tables_dev, const float* w,
                        const float* b, const float* sc, const float* sh, float* cat, int s16, void* stream);
/* head, ConvTranspose2d(16, K, 2, stride 2), K 1..8: x (N,h,w,16) NHWC -> out (N,K,2h,2w) NCHW fp32; w (16,K,2,2), b [K].  Returns 0. */
int lf_debug_head_fwd(const float* x, const float* w, const float* b, float* out, int N, int h, int w_, int K, int s16, void* stream);
/* its data gradient: gout (N,K,2h,2w) NCHW fp32 -> gx (N,h,w,16) NHWC.  Returns 0. */
int lf_debug_head_bwd_data(const float* gout, const float* w, float* gx, int N, int h, int w_, int K, int s16, void* stream);
/* tap-GEMM launches that took a compiled-in bias + residual + ReLU epilogue (the inference engine's block tail) since the process
 * started: which kernel form a launch selected (tests/test_infer_gpu.py) */
long lf_debug_bias_residual_launches(void);
/* the thin fp32 tap-GEMM (tapgemm_thin_kernel, csrc/lf_conv.hip: one 16-pixel tile per wave, for launches that cannot fill the device).
 * mode 0 (shipped): LfTapArgs::thin -- set by the frozen detector's calls only -- and the grid size decide; 2: every launch the kernel is
 * compiled for (fp32 tensors, an output slab of 32 channels or more, no prologue, bias + ReLU or bias + residual + ReLU) takes it, whatever
 * the flag and the grid.  nt 0: the launcher picks the 16-channel slabs per wave; 1..4: forced where it divides Cd / 16.  The kernels agree
 * bit for bit (tests/test_thin_conv_gpu.py) */
void lf_debug_set_thin(int mode, int nt);
/* launches that kernel took since the process started */
long lf_debug_thin_launches(void);
/* the thin bf16 tap-GEMM (tapgemm_bf16_thin_kernel, csrc/lf_conv_bf16.hip: the same tiling on bf16 tensors and the bf16 matrix cores), with
 * a switch and a counter of its own -- lf_debug_set_thin leaves bf16 launches alone, and this pair fp32 launches.  mode 0 (shipped):
 * LfTapArgs::thin and the grid size decide; 2: every launch the kernel is compiled for (bf16 tensors, an output slab of 32 channels or
 * more, source channels a multiple of 32 or 16, no prologue, bias + ReLU or bias + residual + ReLU) takes it.  nt as above.  The kernels
 * agree bit for bit (tests/test_thin_bf16_conv_gpu.py) */
void lf_debug_set_thin_bf16(int mode, int nt);
/* launches that kernel took since the process started */
long lf_debug_thin_bf16_launches(void);
/* fold-and-pack launches (lf_fold_pack_launch: the inference engine's per-call fold, lf_erfnet_infer_fold, the --clas heads' chains)
 * since the process started */
long lf_debug_fold_pack_launches(void);
int lf_debug_conv1d_wgrad_phases(const float* x, const float* gy, int N, int H, int W, int C, int axis, int dilation,
                                 float* scratch, unsigned long long* dbg, void* stream);
/* where lf_convchain_forward leaves block `block`'s saved state in its training workspace, as a FLOAT offset (the same in both
 * precision modes: in mode 2 the region of z holds bf16 elements from that offset on): which 0 = z, the pre-BatchNorm tensor
 * (N,H,W,C_block+1) NHWC; 1 = sc, 2 = sh (the folded scale and shift the next block's prologue and the ReLU masks use); 3 = asc (rstd),
 * 4 = ash (-mean * rstd) -- [C] fp32 each.  -1 for a null plan or a block / which out of range.  (tests/test_convchain_shapes_gpu.py) */
struct lf_convchain_plan;
long lf_debug_convchain_offset(const struct lf_convchain_plan* plan, int block, int which);
#ifdef __cplusplus
}
#endif
