// Internal interface of the tap-GEMM convolution kernels (gfx950; fp32 MFMA 16x16x4 by default, bf16 MFMA 16x16x32 in the
// bf16 and split precision modes).
//
// Every convolution-like layer of the ERFNet backbone (1-D factorised 3x1 / 1x3 convs with
// dilation, 3x3 stride-2 convs, 3x3 stride-2 transposed convs by sub-pixel phase, and all of
// their data gradients) is ONE kernel family: for every logical pixel p and output channel co
//     dst[dpix(p)][co] = epi( bias[co] + sum_t sum_ci pro(src[spix(p,t)][ci]) * Wp[t][ci][co] )
// with NHWC fp32 activations, K = (taps x source channels) contracted on the matrix cores.
// Weight gradients are the transposed contraction over pixels (lf_tapwgrad).
#pragma once
#include <atomic>

#include "lf_common.h"

#define LF_MAX_TAPS 9
struct TapIdx { int v[LF_MAX_TAPS]; };     // a kernel argument: packed tap t <- weight element v[t] of the layer's kernel

struct LfTapGeom {
    int N, Hl, Wl;                 // logical pixel grid the kernel iterates over
    int Hs, Ws, s_pix, s_choff;    // source tensor: spatial dims, floats per pixel, channel offset
    int ssh, ssw;                  // source coord = logical * ss + tap offset
    int Hd, Wd, d_pix, d_choff;    // destination tensor
    int dsh, dsw, dah, daw;        // dest coord = logical * ds + da
    int Cs, Cd;                    // contracted channels (multiple of 16), produced channels (multiple of 16)
    int ntaps;
    int tdh[LF_MAX_TAPS], tdw[LF_MAX_TAPS];
};

enum { LF_PRO_NONE = 0, LF_PRO_BNRELU = 1 };
enum {
    LF_EPI_RELU = 1,        // v = max(v, 0)
    LF_EPI_MASK = 2,        // v = mask_src > 0 ? v : 0        (ReLU backward from the saved output)
    LF_EPI_ADD = 4,         // v += add_src                    (residual / accumulated gradient)
    LF_EPI_STATS_SQ = 8,    // per-channel sum v, sum v^2      (BatchNorm forward statistics)
    LF_EPI_MASKBN = 16,     // v = (aux*msc+msh) > 0 ? v : 0   (ReLU backward through a recomputed BN)
    LF_EPI_STATS_XHAT = 32, // per-channel sum v, sum v*aux (RAW: lf_bn_bwd_finalize turns the pair into sum v*xhat, xhat = aux*rstd - mean*rstd, in fp64)
    LF_EPI_BIAS = 64        // compile-time selector only (never passed to lf_tapgemm_launch): the compiled-in epilogue keeps its bias
                            // vector beside ADD -- the inference engine's folded residual tail relu(conv + b' + x)
};

struct LfTapArgs {
    const float* src;
    const float* wp;        // packed weights [tap][Cs/4][Cd][4]
    int s16;                // 1: src / dst / mask_src / add_src / aux hold bf16 elements (needs wp16)
    const void* wp16;       // non-null selects the bf16 matrix-core kernel: packed bf16 weights [tap][ceil(Cs/32)*4][Cd][8]
    int split;              // 9: fp32 on the bf16 matrix cores from 3-way split operands, all nine partial products (tapgemm_split_kernel);
    const void* wp48;       //   its weights, split by the pack kernel: bf16 [tap][Cs/8][Cd][3][8]; launches the split
                            //   kernel cannot take (Cs % 32, Cd % 64) fall back to the fp32 matrix cores (wp)
    const float* bias;      // [Cd] or null
    float* dst;
    const float* pro_sc;    // prologue BN scale / shift per source channel
    const float* pro_sh;
    const float* mask_src;  // dest-geometry tensors
    const float* add_src;
    const float* aux;
    const float* msc;       // [Cd] forward BN scale/shift (MASKBN)
    const float* msh;
    const float* asc;       // (unused since round 3: the BatchNorm-backward sums are written raw)
    const float* ash;
    const float* dm;        // optional Dropout2d keep-mask [N][Cd] applied to the STATS_XHAT sums only (gm = v * dm)
    float* stats;           // per-workgroup partial sums, channel-major: [2][Cd][stats_ld], row r = 256-pixel tile r of the launch
    int stats_ld;           //   (rows = lf_tapgemm_stat_rows(); stats_ld >= rows: lf_eltwise.h, LfStatPart)
    unsigned long long* dbg;  // optional: per-wave phase timestamps (s_memtime), 8 words per wave (tools/kbench.py --phases)
    int thin;               // host-side routing flag (no kernel reads it): a launch whose regular grid cannot fill the device takes
                            //   tapgemm_thin_kernel (fp32 tensors: lf_conv.hip, launch_fp32_route) / tapgemm_bf16_thin_kernel (bf16 tensors:
                            //   lf_conv_bf16.hip, lf_tapgemm_bf16_route) where that kernel is compiled for it; 0 everywhere but the frozen
                            //   detector's calls (LF_INFER_THIN)
};

// ---- lf_conv.hip: forward and data-gradient launches, the fp32 kernels' routing switches and the counters of both routes ----
void lf_tapgemm_set_split_any_size(int v);
void lf_tapgemm_set_fp32_stream(int mode, int max_workgroups);   // tapstream_kernel routing (lf_debug_set_fp32_stream, lf_debug.h)
void lf_tapgemm_set_thin(int mode, int nt);          // tapgemm_thin_kernel routing (lf_debug_set_thin, lf_debug.h)
long lf_tapgemm_thin_launches();                     // launches tapgemm_thin_kernel took since the process started
// what the two thin routes (fp32 here, bf16 in lf_conv_bf16.hip) share: the CU count of the current device (cached), and the 16-channel
// slabs per wave of a thin launch -- `forced` (1..4) where it divides Cd / 16, else the largest of 4, 3, 2, 1 dividing Cd / 16 that
// still gives one workgroup (64 pixels x nt slabs) per CU, else 1
int lf_tapgemm_device_cus();
int lf_tapgemm_thin_pick_nt(const LfTapGeom& g, int forced);
int lf_tapgemm_stat_rows(const LfTapGeom& g);                          // upper bound over the kernels (buffer sizing)
int lf_tapgemm_stat_rows_for(const LfTapGeom& g, const LfTapArgs& a);  // rows the launch with these arguments writes
int lf_tapgemm_launch(const LfTapGeom& g, const LfTapArgs& a, int pro, int epi, hipStream_t st);
// the same launch WITHOUT the in-order barrier on its dispatch packet (hipExtAnyOrderLaunch; fp32 tap-GEMM kernels only, the other
// kernels launch in order): it may overlap the previous launch of the stream, which the caller guarantees to be independent of it
int lf_tapgemm_launch_unordered(const LfTapGeom& g, const LfTapArgs& a, int pro, int epi, hipStream_t st);
bool lf_tapgemm_split_ok(const LfTapGeom& g);
// launches that took a compiled-in bias + residual + ReLU epilogue since the process started (kernel-level tests)
long lf_tapgemm_bias_residual_launches();
extern std::atomic<long> g_bres_launches;           // ... the counter itself: ONE object, which both routes increment

// ---- lf_conv_pair.hip: a non_bottleneck_1d block's 3x1 -> 1x3 forward pair in one launch (tappair_kernel; fp32 tensors) ----
// ga / aa: the convolution along H with the ReLU epilogue (pro: its operand prologue), gb / ab: the one along W with the BatchNorm
// statistics epilogue, ab.src == aa.dst.  Takes: precision mode 0, C -> C at a compiled channel count (64), 3 taps each, dense
// stride-1 tensors, Wl % 64 == 0 and 256 % Wl == 0 (a 256-pixel tile is whole image rows), epi_a == LF_EPI_RELU and epi_b ==
// LF_EPI_STATS_SQ (training).  Both tensors and the statistics rows are the two launches' bit for bit.  False too where the runtime
// refuses the kernel's LDS budget on this device; the caller then takes the two launches.
bool lf_tappair_ok(const LfTapGeom& ga, const LfTapGeom& gb, const LfTapArgs& aa, const LfTapArgs& ab, int pro, int epi_a, int epi_b);
int lf_tappair_launch(const LfTapGeom& ga, const LfTapGeom& gb, const LfTapArgs& aa, const LfTapArgs& ab, int pro, hipStream_t st);
void lf_tappair_set(int mode, int max_workgroups);   // lf_debug_set_fwd_pair (lf_debug.h)
bool lf_tappair_routed(int C, int pro);              // the network takes the fused launch for this form (the forms that lowered the step)

// ---- lf_conv_bf16.hip: the kernels on bf16 tensors, their route, routing switches and counters ----
// lf_tapgemm_launch's route for a launch with packed bf16 weights (a.wp16), after its checks: epis, npix, nt and grid are its values
int lf_tapgemm_bf16_route(const LfTapGeom& g, const LfTapArgs& a, int pro, int epi, int epis, long npix, int nt, dim3 grid, hipStream_t st);
void lf_tapgemm_set_bf16_lds(int v);
int lf_tapgemm_bf16_lds();                          // the value set (the 16-channel weight gradient's LDS rings follow it: lf_wgrad.hip)
void lf_tapgemm_set_bf16_no_partial_fast(int v);   // 1: launches with Cs % 32 != 0 decline the compiled-in whole-step forms (tests)
long lf_tapgemm_partial_fast_launches();            // launches with Cs % 32 != 0 that took a compiled-in whole-step form since the process started (tests)
long lf_tapgemm_bf16_ring_launches();               // launches tapgemm_bf16_ring_kernel took since the process started (tests)
void lf_tapgemm_set_bf16_max_workgroups(int v);     // > 0: caps grid.x of the resident bf16 launches (ring, whole-line, wave-private); 0: shipped (tests)
void lf_tapgemm_set_thin_bf16(int mode, int nt);    // tapgemm_bf16_thin_kernel routing (lf_debug_set_thin_bf16, lf_debug.h)
long lf_tapgemm_thin_bf16_launches();               // launches tapgemm_bf16_thin_kernel took since the process started

// ---- lf_wgrad.hip: weight gradients and their split-K reductions (lf_tapwgrad_ro_*: lf_wgrad_ro.hip) ----
struct LfWgradArgs {
    const float* x;         // source-side tensor (gathered by taps), geometry = source fields of LfTapGeom
    const float* g;         // dest-side gradient tensor, geometry = dest fields
    const float* pro_sc;    // optional BN+ReLU recompute on x
    const float* pro_sh;
    int s16;                // 1: x and g hold bf16 elements (partials and bias rows stay fp32)
    int split;              // (unused since round 6: the weight gradient of the split mode runs on the fp32 matrix cores)
    float* partial;         // [splits][ntaps][Cs][Cd]
    float* bias_partial;    // [bias_rows][Cd] or null
    unsigned long long* dbg = nullptr;   // tools/kbench.py --phases: 8 words per wave (start, first operands, loop done, end, HW id)
};
// number of k-split rows the kernel will write for this geometry
int lf_tapwgrad_splits(const LfTapGeom& g);          // upper bound over the kernels that take fp32 tensors
int lf_tapwgrad_splits_bound(const LfTapGeom& g, int s16);   // ... by storage type: bf16 tensors add the read-once kernel's rows
long lf_tapwgrad_wave_pixels(const LfTapGeom& g);    // pixels per wave of those kernels (rows = ceil(pixels / (4 * this)))
// rows the launch with these arguments writes (bf16 tensors: the read-once kernel's row count)
int lf_tapwgrad_splits_for(const LfTapGeom& g, const LfWgradArgs& a, int pro);
int lf_tapwgrad_launch(const LfTapGeom& g, const LfWgradArgs& a, int pro, hipStream_t st);

// Weight gradient AND data gradient of a 16 -> 16 channel 3-tap stride-1 convolution on fp32 tensors in one pass (lf_bwd16.hip).
// gf: the forward (weight-gradient) geometry, gd: the data gradient's -- the plan builds them equal, the data gradient's weights
// are packed flipped.  w.x is the convolution's input, w.g == a.src the gradient; a.mask_src (MASK) / a.aux (MASKBN) must be w.x.
// The partial rows are lf_tapwgrad_launch's (lf_tapwgrad_splits_for rows), the statistics rows lf_tapgemm_launch's.
bool lf_tapbwd16_ok(const LfTapGeom& gf, const LfTapGeom& gd, const LfWgradArgs& w, const LfTapArgs& a, int pro, int epi);
int lf_tapbwd16_launch(const LfTapGeom& gf, const LfTapGeom& gd, const LfWgradArgs& w, const LfTapArgs& a, int pro, int epi, hipStream_t st);
void lf_tapbwd16_set(int mode);          // 0: lf_tapbwd16_routed() declines every form; 1: the shipped routing; 2 * m: the forms of bit mask m
bool lf_tapbwd16_routed(int pro, int epi);   // the network takes the fused launch for this form (the forms that were faster in the step)

// Read-once weight gradient of the 3-tap C -> C convolutions on bf16 tensors (lf_wgrad_ro.hip; C = 64, 128, stride 1, Wl % 16 == 0):
// one workgroup owns all taps of a 64-channel x-block against every g-channel for its pixel range.  lf_tapwgrad_launch routes to it.
bool lf_tapwgrad_ro_ok(const LfTapGeom& g, int s16);
int lf_tapwgrad_ro_rows_bound(const LfTapGeom& g);     // partial rows at the shipped workgroup caps (buffer sizing; 0 = geometry not taken)
int lf_tapwgrad_ro_rows(const LfTapGeom& g);           // rows the launch writes ([rows][3][C][C] fp32 + [rows][C] bias rows)
int lf_tapwgrad_ro_launch(const LfTapGeom& g, const LfWgradArgs& a, int pro, hipStream_t st);
void lf_tapwgrad_ro_set(int mode, int cap64, int cap128);   // tools / A-B runs: 0 = off; workgroups per launch at 64 / 128 channels

// dst[k*sk + n*sn + tapidx[t]] = sum_s partial[s][t][k][n]
// ... and, in the same launch, bias_grad[n] (+)= sum_r bias_rows[r][n] when bias_rows != null
int lf_wgrad_reduce_launch(const float* partial, int splits, int ntaps, int Cs, int Cd, float* grad, long sk, long sn,
                           const int* tapidx_host, const float* bias_rows, int n_bias_rows, float* bias_grad,
                           int bias_accumulate, hipStream_t st);
// The same reduction for up to LF_REDUCE_BATCH independent weight gradients in ONE launch (the jobs travel as kernel
// arguments): lf_erfnet collects the reductions of a whole backward pass -- each weight gradient keeps its partial rows
// in its own region of the workspace -- and issues them at the end instead of one 6 us launch behind every wgrad.
#define LF_REDUCE_BATCH 32
struct LfReduceJob {
    const float* partial; float* grad; const float* bias_rows; float* bias_grad;
    long sk, sn;
    int splits, ntaps, Cs, Cd, n_bias_rows;
    int tapidx[LF_MAX_TAPS];
};
int lf_wgrad_reduce_batch_launch(const LfReduceJob* jobs_host, int njobs, hipStream_t st);
// dst[n] (+)= sum_r rows[r][n]
int lf_rows_reduce_launch(const float* rows, int nrows, int C, float* dst, int accumulate, hipStream_t st);

// ---- lf_pack.hip: weight packing and the inference fold-and-pack ----
// wp[((t*(Kc/4) + k/4)*Nc + n)*4 + k%4] = w[k*sk + n*sn + tapidx[t]]
struct LfPackEntry {
    long src_off;   // float offset into the flat parameter arena / or pointer index, see lf_erfnet
    long dst_off;   // float offset into the packed-weight arena
    int Kc, Nc, ntaps;
    long sk, sn;
    int tapidx[LF_MAX_TAPS];
    int param;      // index of the parameter tensor holding the weights
    long dst16_off; // bf16-element offset into the bf16 packed arena (precision mode "bf16")
};
int lf_pack_weights_launch(const LfPackEntry* entries_dev, int nentries, const float* const* params_dev, float* arena,
                           hipStream_t st);
long lf_pack_bf16_elems(int Kc, int Nc, int ntaps);
// split weights: 3 bf16 pieces per element, entry e at 3 * e.dst16_off of arena48 (entries with Kc % 32 != 0 are skipped)
int lf_pack_weights_split_launch(const LfPackEntry* entries_dev, int nentries, const float* const* params_dev, void* arena48,
                                 hipStream_t st);

// Inference fold-and-pack (eval-mode BatchNorm folded into the convolution that feeds it), one entry per forward convolution and
// one per per-channel affine (the max-pool channels of a down-sampler, the stem): with s = gamma / sqrt(var + eps) in fp64,
// packed weights w' = fl(w * s[n]), bias b' = fl((b - mean) * s + beta); an entry without gamma copies w and b; a vector-only
// entry (pk.ntaps == 0) writes sc = fl(s), sh = fl(beta - mean * s) for its C channels.  BatchNorm channel = ch_off + n.
struct LfFoldEntry {
    LfPackEntry pk;         // the pack entry (dst_off / dst16_off into the INFERENCE arenas); pk.ntaps = 0: vector-only
    int ch_off, C;          // BatchNorm channels [ch_off, ch_off + C) (C = pk.Nc for a convolution)
    const float* gamma;     // null: no BatchNorm after this convolution
    const float* beta;
    const float* mean;      // running statistics
    const float* var;
    const float* bias;      // conv bias [Nc]
    long out_off;           // float offset into the launch's vector region: the folded bias [Nc] (convolutions), or the per-channel
                            // scale [C] followed by the shift [C] (vector-only entries) -- relative, so the table holds no workspace address
};
// arenas: fp32 [pk.dst_off], bf16 [pk.dst16_off] and split [3 * pk.dst16_off]; a null arena is not written; vec: the vector region
int lf_fold_pack_launch(const LfFoldEntry* entries_dev, int nentries, const float* const* params_dev, float eps, float* vec, float* arena,
                        void* arena16, void* arena48, hipStream_t st);
long lf_fold_pack_launches();       // lf_fold_pack_launch calls that launched since the process started (lf_debug_fold_pack_launches)
int lf_pack_weights_bf16_launch(const LfPackEntry* entries_dev, int nentries, const float* const* params_dev, void* arena16,
                                hipStream_t st);
