// Kernel-level C-ABI entry points: one factorised 1-D convolution (forward, data gradient, weight
// gradient) on NHWC fp32 tensors, outside the ERFNet plan.  Used by the kernel-level parity tests
// and by tools/kbench.py (roofline micro-benchmarks, kernel A/B switches).
// Replaces nn.Conv2d(C, C, (3,1)|(1,3), padding=d, dilation=d) of non_bottleneck_1d (ERFNet.py:29-37).
#include "lf_conv.h"
#include "lf_debug.h"
#include "lf_eltwise.h"
#include "lf_plan.h"

namespace {

TapIdx conv1d_taps(int flip) {
    TapIdx ti;
    memset(&ti, 0, sizeof(ti));
    for (int t = 0; t < 3; ++t) ti.v[t] = flip ? 2 - t : t;
    return ti;
}

__global__ __launch_bounds__(256) void pack_one_kernel(const float* __restrict__ w, float* __restrict__ dst, int Kc, int Nc,
                                                      int ntaps, long sk, long sn, const TapIdx ti) {
    const long total = (long)ntaps * Kc * Nc;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int k4 = (int)(i & 3);
        long r = i >> 2;
        const int n = (int)(r % Nc);
        r /= Nc;
        const int kb = (int)(r % (Kc >> 2));
        const int t = (int)(r / (Kc >> 2));
        dst[i] = w[(kb * 4 + k4) * sk + n * sn + ti.v[t]];
    }
}

// bf16 operand order of tapgemm_bf16_kernel: [tap][ceil(Kc/32)*4][Nc][8], zero beyond Kc
__global__ __launch_bounds__(256) void pack_one_bf16_kernel(const float* __restrict__ w, __bf16* __restrict__ dst, int Kc, int Nc,
                                                           int ntaps, long sk, long sn, const TapIdx ti) {
    const int kb_per_tap = ((Kc + 31) >> 5) * 4;
    const long total = (long)ntaps * kb_per_tap * Nc * 8;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int k8 = (int)(i & 7);
        long r = i >> 3;
        const int n = (int)(r % Nc);
        r /= Nc;
        const int kb = (int)(r % kb_per_tap);
        const int t = (int)(r / kb_per_tap);
        const int k = kb * 8 + k8;
        dst[i] = (__bf16)(k < Kc ? w[k * sk + n * sn + ti.v[t]] : 0.f);
    }
}

// split operand order of tapgemm_split_kernel: [tap][Kc/8][Nc][3][8] bf16 (pieces h, m, l; h + m + l == w exactly)
__global__ __launch_bounds__(256) void pack_one_split_kernel(const float* __restrict__ w, __bf16* __restrict__ dst, int Kc, int Nc,
                                                            int ntaps, long sk, long sn, const TapIdx ti) {
    const int kb_per_tap = Kc >> 3;
    const long total = (long)ntaps * kb_per_tap * Nc * 8;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int k8 = (int)(i & 7);
        const long row = i >> 3;
        long r = row;
        const int n = (int)(r % Nc);
        r /= Nc;
        const int kb = (int)(r % kb_per_tap);
        const int t = (int)(r / kb_per_tap);
        const float v = w[(kb * 8 + k8) * sk + n * sn + ti.v[t]];
        const __bf16 vh = (__bf16)v;
        const float r1 = v - (float)vh;
        const __bf16 vm = (__bf16)r1;
        dst[row * 24 + k8] = vh; dst[row * 24 + 8 + k8] = vm; dst[row * 24 + 16 + k8] = (__bf16)(r1 - (float)vm);
    }
}

int g_ops_bf16 = 0;     // 0 fp32 cores, 2 bf16 cores on bf16 tensors, 9 fp32 from 9-term split operands on the bf16 cores

// pack into scratch in the order the selected kernel wants; returns the LfTapArgs weight fields
void pack_conv1d(LfTapArgs& a, const float* w, float* scratch, int C, long sk, long sn, int flip, hipStream_t st) {
    if (g_ops_bf16 == 9) {
        hipLaunchKernelGGL(pack_one_kernel, dim3(64), dim3(256), 0, st, w, scratch, C, C, 3, sk, sn, conv1d_taps(flip));
        if (C % 32 == 0) {
            hipLaunchKernelGGL(pack_one_split_kernel, dim3(64), dim3(256), 0, st, w, reinterpret_cast<__bf16*>(scratch + 3L * C * C),
                               C, C, 3, sk, sn, conv1d_taps(flip));
            a.split = g_ops_bf16;
            a.wp48 = scratch + 3L * C * C;
        }
    } else if (g_ops_bf16 == 2) {
        hipLaunchKernelGGL(pack_one_bf16_kernel, dim3(64), dim3(256), 0, st, w, reinterpret_cast<__bf16*>(scratch), C, C, 3, sk, sn, conv1d_taps(flip));
        a.wp16 = scratch;
        a.s16 = 1;
    } else {
        hipLaunchKernelGGL(pack_one_kernel, dim3(64), dim3(256), 0, st, w, scratch, C, C, 3, sk, sn, conv1d_taps(flip));
    }
    a.wp = scratch;
}

LfTapGeom conv1d_geom(int N, int H, int W, int C, int axis, int d) {
    LfTapGeom g;
    memset(&g, 0, sizeof(g));
    g.N = N; g.Hl = H; g.Wl = W; g.Hs = H; g.Ws = W; g.s_pix = C; g.ssh = 1; g.ssw = 1;
    g.Hd = H; g.Wd = W; g.d_pix = C; g.dsh = 1; g.dsw = 1; g.Cs = C; g.Cd = C; g.ntaps = 3;
    for (int t = 0; t < 3; ++t) { g.tdh[t] = axis == 0 ? (t - 1) * d : 0; g.tdw[t] = axis == 1 ? (t - 1) * d : 0; }
    return g;
}

}  // namespace

extern "C" {

void lf_debug_set_split_any_size(int v) { lf_tapgemm_set_split_any_size(v); }
void lf_debug_set_bf16_lds(int v) { lf_tapgemm_set_bf16_lds(v); }
void lf_debug_set_bf16_no_partial_fast(int v) { lf_tapgemm_set_bf16_no_partial_fast(v); }
// precision mode of the kernel-level conv1d calls below (tests, kbench): 0 fp32, 2 bf16 matrix cores on bf16 tensors (x, y, gx, gy,
// mask_src then hold bf16 elements; w, bias, gw, gb stay fp32), 9 fp32 from 9-term split operands; anything else (the removed
// modes 1 and 6) selects 0
void lf_debug_set_ops_precision(int mode) { g_ops_bf16 = (mode == 2 || mode == 9) ? mode : 0; }

void lf_debug_set_wgrad_ro(int mode, int cap64, int cap128) { lf_tapwgrad_ro_set(mode, cap64, cap128); }
void lf_debug_set_fp32_stream(int mode, int max_workgroups) { lf_tapgemm_set_fp32_stream(mode, max_workgroups); }
void lf_debug_set_bwd16_fused(int mode) { lf_tapbwd16_set(mode); }
void lf_debug_set_fwd_pair(int mode, int max_workgroups) { lf_tappair_set(mode, max_workgroups); }
long lf_debug_bias_residual_launches(void) { return lf_tapgemm_bias_residual_launches(); }
void lf_debug_set_thin(int mode, int nt) { lf_tapgemm_set_thin(mode, nt); }
long lf_debug_thin_launches(void) { return lf_tapgemm_thin_launches(); }
void lf_debug_set_thin_bf16(int mode, int nt) { lf_tapgemm_set_thin_bf16(mode, nt); }
long lf_debug_thin_bf16_launches(void) { return lf_tapgemm_thin_bf16_launches(); }
long lf_debug_fold_pack_launches(void) { return lf_fold_pack_launches(); }
long lf_debug_partial_fast_launches(void) { return lf_tapgemm_partial_fast_launches(); }
long lf_debug_bf16_ring_launches(void) { return lf_tapgemm_bf16_ring_launches(); }
void lf_debug_set_bf16_max_workgroups(int v) { lf_tapgemm_set_bf16_max_workgroups(v); }

// same as lf_conv1d_fwd with per-wave phase timestamps: dbg receives 8 uint64 per wave
// (start, tap table built, main loop done, stores retired); waves = ceil(N*H*W/256)*4*(C/64)
int lf_debug_conv1d_fwd_phases(const float* x, const float* w, const float* bias, float* y, int N, int H, int W, int C,
                               int axis, int dilation, float* scratch, unsigned long long* dbg, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const LfTapGeom g = conv1d_geom(N, H, W, C, axis, dilation);
    LfTapArgs a;
    memset(&a, 0, sizeof(a));
    pack_conv1d(a, w, scratch, C, 3L, 3L * C, 0, st);
    a.src = x; a.bias = bias; a.dst = y; a.dbg = dbg;
    return lf_tapgemm_launch(g, a, LF_PRO_NONE, 0, st);
}

int lf_debug_conv1d_fwd_pro(const float* x, const float* w, const float* bias, const float* sc, const float* sh, float* y, int N, int H,
                            int W, int C, int axis, int dilation, float* scratch, void* stream) {
    LF_REQUIRE(x && w && y && sc && sh && scratch, "lf_debug_conv1d_fwd_pro: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const LfTapGeom g = conv1d_geom(N, H, W, C, axis, dilation);
    LfTapArgs a;
    memset(&a, 0, sizeof(a));
    pack_conv1d(a, w, scratch, C, 3L, 3L * C, 0, st);
    a.src = x; a.bias = bias; a.dst = y; a.pro_sc = sc; a.pro_sh = sh;
    return lf_tapgemm_launch(g, a, LF_PRO_BNRELU, LF_EPI_RELU, st);
}

// one 3x1 -> 1x3 forward pair, routed as forward_layers (lf_erfnet.hip) routes it; scratch: [packed wa 3 C C][packed wb 3 C C]
int lf_debug_conv1d_fwd_pair(const float* x, const float* wa, const float* ba, const float* wb, const float* bb, const float* sc,
                             const float* sh, float* t, float* y, float* stats, int N, int H, int W, int C, int dilation, float* scratch,
                             void* stream) {
    if (!(x && wa && wb && t && y && stats && scratch) || (sc != nullptr) != (sh != nullptr)) { lf_fail("lf_debug_conv1d_fwd_pair: null pointer"); return -1; }
    if (N < 1 || H < 1 || W < 1 || C < 16 || C % 16 != 0 || dilation < 1) { lf_fail("lf_debug_conv1d_fwd_pair: bad arguments"); return -1; }
    if (g_ops_bf16 != 0) { lf_fail("lf_debug_conv1d_fwd_pair: fp32 tensors in precision mode 0 only"); return -1; }
    hipStream_t st = (hipStream_t)stream;
    const LfTapGeom ga = conv1d_geom(N, H, W, C, 0, dilation), gb = conv1d_geom(N, H, W, C, 1, dilation);
    LfTapArgs aa, ab;
    memset(&aa, 0, sizeof(aa));
    memset(&ab, 0, sizeof(ab));
    pack_conv1d(aa, wa, scratch, C, 3L, 3L * C, 0, st);
    pack_conv1d(ab, wb, scratch + 3L * C * C, C, 3L, 3L * C, 0, st);
    aa.src = x; aa.bias = ba; aa.dst = t; aa.pro_sc = sc; aa.pro_sh = sh;
    ab.src = t; ab.bias = bb; ab.dst = y; ab.stats = stats;
    ab.stats_ld = lf_tapgemm_stat_rows(gb);        // the caller's buffer: [2][C][rows], rows = ceil(N * H * W / 256)
    const int pro = sc ? LF_PRO_BNRELU : LF_PRO_NONE;
    if (lf_tappair_routed(C, pro) && lf_tappair_ok(ga, gb, aa, ab, pro, LF_EPI_RELU, LF_EPI_STATS_SQ))
        return lf_tappair_launch(ga, gb, aa, ab, pro, st) ? -1 : 1;
    if (lf_tapgemm_launch(ga, aa, pro, LF_EPI_RELU, st) || lf_tapgemm_launch(gb, ab, LF_PRO_NONE, LF_EPI_STATS_SQ, st)) return -1;
    return 0;
}

// the weight gradient of lf_conv1d_bwd_weight (no reduction) with per-wave phase timestamps; returns the number of waves
int lf_debug_conv1d_wgrad_phases(const float* x, const float* gy, int N, int H, int W, int C, int axis, int dilation,
                                 float* scratch, unsigned long long* dbg, void* stream) {
    const LfTapGeom g = conv1d_geom(N, H, W, C, axis, dilation);
    LfWgradArgs a;
    a.x = x; a.g = gy; a.pro_sc = nullptr; a.pro_sh = nullptr; a.s16 = 0; a.split = 0;
    a.partial = scratch; a.bias_partial = nullptr; a.dbg = dbg;
    const int rc = lf_tapwgrad_launch(g, a, LF_PRO_NONE, (hipStream_t)stream);
    return rc ? -1 : lf_tapwgrad_splits_for(g, a, LF_PRO_NONE) * 3 * (C / 64) * (C / 64) * 4;
}

// scratch floats needed by the three calls below (packed weights / split-K partials)
long lf_conv1d_scratch_floats(int N, int H, int W, int C) {
    const LfTapGeom g = conv1d_geom(N, H, W, C, 0, 1);
    long a = 8L * C * C;        // fp32-packed weights + their 3-piece bf16 split (4.5 C^2 floats)
    const long rows = lf_tapwgrad_splits_bound(g, 1);          // either storage type
    long b = rows * 3 * C * C + rows * C;
    return a > b ? a : b;
}

// y = [relu](conv1d(x) + bias); x,y (N,H,W,C) NHWC; w in the nn.Conv2d layout (C,C,3) flattened; axis 0 = 3x1, 1 = 1x3
int lf_conv1d_fwd(const float* x, const float* w, const float* bias, float* y, int N, int H, int W, int C, int axis,
                  int dilation, int relu, float* scratch, void* stream) {
    LF_REQUIRE(x && w && y && scratch, "lf_conv1d_fwd: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const LfTapGeom g = conv1d_geom(N, H, W, C, axis, dilation);
    LfTapArgs a;
    memset(&a, 0, sizeof(a));
    pack_conv1d(a, w, scratch, C, 3L, 3L * C, 0, st);
    a.src = x; a.bias = bias; a.dst = y;
    return lf_tapgemm_launch(g, a, LF_PRO_NONE, relu ? LF_EPI_RELU : 0, st);
}

// gx = conv1d^T(gy) [* (mask_src > 0)]
int lf_conv1d_bwd_data(const float* gy, const float* w, const float* mask_src, float* gx, int N, int H, int W, int C,
                       int axis, int dilation, float* scratch, void* stream) {
    LF_REQUIRE(gy && w && gx && scratch, "lf_conv1d_bwd_data: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const LfTapGeom g = conv1d_geom(N, H, W, C, axis, dilation);
    LfTapArgs a;
    memset(&a, 0, sizeof(a));
    pack_conv1d(a, w, scratch, C, 3L * C, 3L, 1, st);
    a.src = gy; a.dst = gx; a.mask_src = mask_src;
    return lf_tapgemm_launch(g, a, LF_PRO_NONE, mask_src ? LF_EPI_MASK : 0, st);
}

int lf_debug_conv1d_bwd_data_epi3(const float* gy, const float* w, const float* mask_src, const float* add_src, const float* aux,
                                  float* gx, float* stats, int N, int H, int W, int C, int axis, int dilation, float* scratch, void* stream) {
    if (!(gy && w && mask_src && add_src && aux && gx && stats && scratch)) { lf_fail("lf_debug_conv1d_bwd_data_epi3: null pointer"); return -1; }
    hipStream_t st = (hipStream_t)stream;
    const LfTapGeom g = conv1d_geom(N, H, W, C, axis, dilation);
    LfTapArgs a;
    memset(&a, 0, sizeof(a));
    pack_conv1d(a, w, scratch, C, 3L * C, 3L, 1, st);
    a.src = gy; a.dst = gx; a.mask_src = mask_src; a.add_src = add_src; a.aux = aux; a.stats = stats;
    a.stats_ld = lf_tapgemm_stat_rows(g);        // the caller's buffer: [2][C][rows], rows = ceil(N * H * W / 256)
    if (lf_tapgemm_launch(g, a, LF_PRO_NONE, LF_EPI_ADD | LF_EPI_MASK | LF_EPI_STATS_XHAT, st)) return -1;
    return lf_tapgemm_stat_rows_for(g, a);
}

// one tap-GEMM launch with any of the network's epilogue flag sets (LF_EPI_*, lf_conv.h); transposed = 1: data-gradient weights.
// Tensors a flag does not name may be null.  Returns the number of statistics rows written (0 without a STATS flag), -1 on error.
int lf_debug_conv1d_epi(const float* src, const float* w, const float* bias, float* dst, int transposed, int epi, const float* mask_src,
                        const float* add_src, const float* aux, const float* msc, const float* msh, float* stats, int N, int H, int W, int C,
                        int axis, int dilation, float* scratch, void* stream) {
    if (!(src && w && dst && scratch)) { lf_fail("lf_debug_conv1d_epi: null pointer"); return -1; }
    hipStream_t st = (hipStream_t)stream;
    const LfTapGeom g = conv1d_geom(N, H, W, C, axis, dilation);
    LfTapArgs a;
    memset(&a, 0, sizeof(a));
    if (transposed) pack_conv1d(a, w, scratch, C, 3L * C, 3L, 1, st);
    else pack_conv1d(a, w, scratch, C, 3L, 3L * C, 0, st);
    a.src = src; a.dst = dst; a.bias = bias; a.mask_src = mask_src; a.add_src = add_src; a.aux = aux; a.msc = msc; a.msh = msh; a.stats = stats;
    a.stats_ld = lf_tapgemm_stat_rows(g);        // the caller's buffer: [2][C][rows], rows = ceil(N * H * W / 256)
    if (lf_tapgemm_launch(g, a, LF_PRO_NONE, epi, st)) return -1;
    return (epi & (LF_EPI_STATS_SQ | LF_EPI_STATS_XHAT)) ? lf_tapgemm_stat_rows_for(g, a) : 0;
}

// One launch of a stride-2 layer (see lf_debug.h); the geometry and the weight gather are the plan's own (lf_plan.h)
int lf_debug_stride2_epi(int kind, int phase, const float* src, const float* w, const float* bias, float* dst, int epi, const float* mask_src,
                         const float* add_src, const float* aux, float* stats, int N, int H, int W, int Cin, int Cout, float* scratch,
                         void* stream) {
    if (!(src && w && dst && scratch)) { lf_fail("lf_debug_stride2_epi: null pointer"); return -1; }
    if (kind < 0 || kind > 3 || phase < 0 || phase > 3 || N < 1 || H < 2 || W < 2 || (H & 1) || (W & 1) || Cin < 16 || Cout < 16) {
        lf_fail("lf_debug_stride2_epi: bad arguments (kind %d phase %d N %d H %d W %d Cin %d Cout %d)", kind, phase, N, H, W, Cin, Cout);
        return -1;
    }
    if (g_ops_bf16 != 0 && g_ops_bf16 != 2) { lf_fail("lf_debug_stride2_epi: precision mode 0 or 2 only"); return -1; }
    hipStream_t st = (hipStream_t)stream;
    LfStride2Op one, four[4];
    if (kind <= 1) lf_down_conv_ops(N, H, W, Cin, Cout, Cin + Cout, one, four);
    else lf_up_conv_ops(N, H / 2, W / 2, Cin, Cout, four, one);
    const LfStride2Op& op = (kind == 0 || kind == 3) ? one : four[phase];
    const LfTapGeom& g = op.geom;
    TapIdx ti;
    memset(&ti, 0, sizeof(ti));
    for (int t = 0; t < g.ntaps; ++t) ti.v[t] = op.tapidx[t];
    LfTapArgs a;
    memset(&a, 0, sizeof(a));
    if (g_ops_bf16 == 2) {
        hipLaunchKernelGGL(pack_one_bf16_kernel, dim3(64), dim3(256), 0, st, w, reinterpret_cast<__bf16*>(scratch), op.Kc, op.Nc, g.ntaps, op.sk, op.sn, ti);
        a.wp16 = scratch;
        a.s16 = 1;
    } else {
        hipLaunchKernelGGL(pack_one_kernel, dim3(64), dim3(256), 0, st, w, scratch, op.Kc, op.Nc, g.ntaps, op.sk, op.sn, ti);
    }
    a.wp = scratch;
    a.src = src; a.dst = dst; a.bias = bias; a.mask_src = mask_src; a.add_src = add_src; a.aux = aux; a.stats = stats;
    a.stats_ld = lf_tapgemm_stat_rows(g);        // the caller's buffer: [2][Cd][rows], rows = ceil(logical pixels / 256)
    if (lf_tapgemm_launch(g, a, LF_PRO_NONE, epi, st)) return -1;
    return (epi & (LF_EPI_STATS_SQ | LF_EPI_STATS_XHAT)) ? lf_tapgemm_stat_rows_for(g, a) : 0;
}

namespace {
// the weight-gradient launches of a stride-2 layer: the plan's forward geometries (run_wgrad differentiates L.cv[0].fwd / .fph[ph])
int stride2_wgrad_ops(int kind, int N, int H, int W, int Cin, int Cout, LfStride2Op ops[4]) {
    LfStride2Op one, four[4];
    if (kind == 0) { lf_down_conv_ops(N, H, W, Cin, Cout, Cin + Cout, ops[0], four); return 1; }
    lf_up_conv_ops(N, H / 2, W / 2, Cin, Cout, ops, one);
    return 4;
}
bool stride2_wgrad_ok(const char* who, int kind, int reduce, int N, int H, int W, int Cin, int Cout) {
    if ((kind != 0 && kind != 2) || (reduce != 0 && reduce != 1) || N < 1 || H < 2 || W < 2 || (H & 1) || (W & 1) || Cin < 16 || Cout < 16) {
        lf_fail("%s: bad arguments (kind %d reduce %d N %d H %d W %d Cin %d Cout %d)", who, kind, reduce, N, H, W, Cin, Cout);
        return false;
    }
    if (g_ops_bf16 != 0 && g_ops_bf16 != 2) { lf_fail("%s: precision mode 0 or 2 only", who); return false; }
    return true;
}
// floats of the weight / bias partial-row regions: one shared region (immediate route) or one per launch, end to end (batched route)
void stride2_wgrad_regions(const LfStride2Op* ops, int nops, int reduce, long& wtot, long& btot) {
    const int s16 = g_ops_bf16 == 2;
    wtot = btot = 0;
    for (int i = 0; i < nops; ++i) {
        const long w = lf_wgrad_wneed(ops[i].geom, s16), b = lf_wgrad_bneed(ops[i].geom, s16);
        wtot = reduce ? wtot + w : lf_maxl(wtot, w);
        btot = reduce ? btot + b : lf_maxl(btot, b);
    }
}
}  // namespace

long lf_debug_stride2_wgrad_scratch_floats(int kind, int reduce, int N, int H, int W, int Cin, int Cout) {
    if (!stride2_wgrad_ok("lf_debug_stride2_wgrad_scratch_floats", kind, reduce, N, H, W, Cin, Cout)) return -1;
    LfStride2Op ops[4];
    const int nops = stride2_wgrad_ops(kind, N, H, W, Cin, Cout, ops);
    long wtot, btot;
    stride2_wgrad_regions(ops, nops, reduce, wtot, btot);
    return wtot + btot;
}

// The weight + bias gradient of a stride-2 layer as run_wgrad (lf_erfnet.hip) issues it: one launch per forward geometry of the
// plan, then the immediate or the batched reduction.  The jobs and the bias chain are lf_plan.h's, shared with run_wgrad; what is
// this hook's own is where the partial-row regions lie: scratch = [weight regions][bias regions], unpadded, so that a row written
// past its region lands in the next one or in the caller's guard band.
int lf_debug_stride2_wgrad(int kind, int reduce, const float* x, const float* g, float* gw, float* gb, int N, int H, int W, int Cin,
                           int Cout, float* scratch, void* stream) {
    if (!(x && g && gw && scratch)) { lf_fail("lf_debug_stride2_wgrad: null pointer"); return -1; }
    if (!stride2_wgrad_ok("lf_debug_stride2_wgrad", kind, reduce, N, H, W, Cin, Cout)) return -1;
    hipStream_t st = (hipStream_t)stream;
    const int s16 = g_ops_bf16 == 2;
    LfStride2Op ops[4];
    const int nops = stride2_wgrad_ops(kind, N, H, W, Cin, Cout, ops);
    long wtot, btot;
    stride2_wgrad_regions(ops, nops, reduce, wtot, btot);
    LfBiasChain chain;
    LfReduceJob jobs[4];
    long woff = 0, boff = 0;
    int rows = 0;
    for (int ph = 0; ph < nops; ++ph) {
        const LfStride2Op& op = ops[ph];
        float* bregion = scratch + wtot + boff;
        LfWgradArgs a;
        a.x = x; a.g = g; a.pro_sc = nullptr; a.pro_sh = nullptr; a.s16 = s16; a.split = 0;
        a.partial = scratch + woff;
        a.bias_partial = gb ? bregion : nullptr;
        if (reduce && nops == 4) {
            float* chained = lf_bias_chain_rows(chain, bregion, op.geom.Cd);
            if (a.bias_partial) a.bias_partial = chained;
        }
        if (lf_tapwgrad_launch(op.geom, a, LF_PRO_NONE, st)) return -1;
        const int nsplit = lf_tapwgrad_splits_for(op.geom, a, LF_PRO_NONE);
        if (nsplit < 1 || nsplit > lf_tapwgrad_splits_bound(op.geom, s16)) {
            lf_fail("lf_debug_stride2_wgrad: phase %d wrote %d rows, its region holds %d", ph, nsplit, lf_tapwgrad_splits_bound(op.geom, s16));
            return -1;
        }
        rows += nsplit;
        if (reduce) {
            jobs[ph] = lf_wgrad_reduce_job(op.geom, a.partial, nsplit, gw, op.sk, op.sn, op.tapidx, a.bias_partial, gb);
            if (nops == 4) lf_bias_chain_job(chain, jobs[ph], nsplit, a.bias_partial != nullptr);
            woff += lf_wgrad_wneed(op.geom, s16); boff += lf_wgrad_bneed(op.geom, s16);
        } else if (lf_wgrad_reduce_launch(a.partial, nsplit, op.geom.ntaps, op.geom.Cs, op.geom.Cd, gw, op.sk, op.sn, op.tapidx,
                                          a.bias_partial, nsplit, gb, ph > 0, st)) {
            return -1;
        }
    }
    if (reduce && lf_wgrad_reduce_batch_launch(jobs, nops, st)) return -1;
    return rows;
}

namespace {
// the stem's / head's partial rows summed as row_sums_finish (lf_erfnet.hip) sums them: immediately, or as lf_plan.h's row-sum jobs
int debug_row_sums(int reduce, const float* wrows, const float* brows, int rows, int nw, float* gw, int nb, float* gb, hipStream_t st) {
    if (!reduce) {
        if (lf_rows_reduce_launch(wrows, rows, nw, gw, 0, st)) return -1;
        if (gb && lf_rows_reduce_launch(brows, rows, nb, gb, 0, st)) return -1;
        return rows;
    }
    LfReduceJob jobs[2];
    int n = 0;
    jobs[n++] = lf_row_sum_job(wrows, rows, nw, gw);
    if (gb) jobs[n++] = lf_row_sum_job(brows, rows, nb, gb);
    return lf_wgrad_reduce_batch_launch(jobs, n, st) ? -1 : rows;
}
bool ends_wgrad_ok(const char* who, int reduce, bool dims_ok) {
    if ((reduce != 0 && reduce != 1) || !dims_ok) { lf_fail("%s: bad arguments", who); return false; }
    if (g_ops_bf16 != 0 && g_ops_bf16 != 2) { lf_fail("%s: precision mode 0 or 2 only", who); return false; }
    return true;
}
}  // namespace

long lf_debug_stem_wgrad_scratch_floats(int N, int Cin, int H, int W) {
    if (N < 1 || Cin < 1 || Cin > 4 || H < 2 || W < 2) return -1;
    return (long)lf_stem_wgrad_rows(N, H, W) * ((16 - Cin) * Cin * 9 + (16 - Cin));
}

int lf_debug_stem_wgrad(int reduce, const float* img, const float* gcat, float* gw, float* gb, int N, int Cin, int H, int W, float* scratch,
                        void* stream) {
    if (!(img && gcat && gw && scratch)) { lf_fail("lf_debug_stem_wgrad: null pointer"); return -1; }
    if (!ends_wgrad_ok("lf_debug_stem_wgrad", reduce, N >= 1 && Cin >= 1 && Cin <= 4 && H >= 2 && W >= 2)) return -1;
    hipStream_t st = (hipStream_t)stream;
    const int Cc = 16 - Cin, rows = lf_stem_wgrad_rows(N, H, W), nw = Cc * Cin * 9;
    float *wrows = scratch, *brows = scratch + (long)rows * nw;
    if (lf_stem_wgrad(img, gcat, N, Cin, H, W, wrows, brows, g_ops_bf16 == 2, st)) return -1;
    return debug_row_sums(reduce, wrows, brows, rows, nw, gw, Cc, gb, st);
}

long lf_debug_head_wgrad_scratch_floats(int N, int h, int w, int K) {
    if (N < 1 || h < 1 || w < 1 || K < 1 || K > 5) return -1;
    return (long)lf_head_wgrad_rows(N, h, w) * (16 * K * 4 + K);
}

int lf_debug_head_wgrad(int reduce, const float* x, const float* gout, float* gw, float* gb, int N, int h, int w, int K, float* scratch,
                        void* stream) {
    if (!(x && gout && gw && scratch)) { lf_fail("lf_debug_head_wgrad: null pointer"); return -1; }
    if (!ends_wgrad_ok("lf_debug_head_wgrad", reduce, N >= 1 && h >= 1 && w >= 1 && K >= 1 && K <= 5)) return -1;
    hipStream_t st = (hipStream_t)stream;
    const int rows = lf_head_wgrad_rows(N, h, w), nw = 16 * K * 4;
    float *wrows = scratch, *brows = scratch + (long)rows * nw;
    if (lf_head_wgrad(x, gout, wrows, brows, N, h, w, K, g_ops_bf16 == 2, st)) return -1;
    return debug_row_sums(reduce, wrows, brows, rows, nw, gw, K, gb, st);
}

// ---- one launch of a bandwidth-bound backbone kernel (lf_eltwise.h): pass-throughs to the launchers the plan calls, with the
// host checks the plan's own geometry makes unnecessary there (lf_debug.h has the contracts)
namespace {
bool al16(const void* p) { return ((size_t)p & 15) == 0; }
// channel counts the row-writing kernels take: quads that divide a 256-thread workgroup
bool quads_ok(int C) { return C >= 4 && C % 4 == 0 && 256 % (C / 4) == 0; }
// builds parts[] from the flat source arguments (a null rows pointer = no such source); the number of sources, -1 on a bad one
int debug_stat_parts(const char* who, const float* const rows[2], const int nrows[2], const int ld[2], const int Cs[2], const int ch_off[2],
                     const int tile_pix[2], const int seg_rows[2], const long seg_pix[2], int C, LfStatPart parts[2]) {
    int n = 0;
    for (int i = 0; i < 2; ++i) {
        if (!rows[i]) continue;
        if (nrows[i] < 1 || ld[i] < nrows[i] || ld[i] % 4 != 0 || !al16(rows[i])) {
            lf_fail("%s: source %d needs a 16-byte aligned base and a leading dimension >= nrows, multiple of 4 (ld=%d nrows=%d)", who, i, ld[i], nrows[i]);
            return -1;
        }
        if (Cs[i] < 4 || Cs[i] % 4 != 0 || ch_off[i] < 0 || ch_off[i] % 4 != 0 || ch_off[i] + Cs[i] > C) {
            lf_fail("%s: source %d covers channels [%d, %d) of %d: multiples of 4 inside the layer", who, i, ch_off[i], ch_off[i] + Cs[i], C);
            return -1;
        }
        if (tile_pix[i] < 0 || (tile_pix[i] > 0 && (seg_rows[i] < 1 || nrows[i] % seg_rows[i] != 0 || seg_pix[i] > (long)seg_rows[i] * tile_pix[i] ||
                                                    seg_pix[i] <= (long)(seg_rows[i] - 1) * tile_pix[i]))) {
            lf_fail("%s: source %d: centred rows need the launch geometry (nrows=%d seg_rows=%d seg_pix=%ld tile_pix=%d)", who, i, nrows[i],
                    seg_rows[i], seg_pix[i], tile_pix[i]);
            return -1;
        }
        parts[n] = {rows[i], nrows[i], Cs[i], ch_off[i], ld[i]};
        parts[n].tile_pix = tile_pix[i]; parts[n].seg_rows = seg_rows[i]; parts[n].seg_pix = seg_pix[i];
        ++n;
    }
    return n;
}
bool stream_ok(const char* who, long npix, int C, long pix_per_image, const float* dm) {
    if (npix < 1 || C < 4 || C % 4 != 0 || pix_per_image < 1 || (dm && npix % pix_per_image != 0)) {
        lf_fail("%s: bad arguments (npix %ld C %d pix_per_image %ld)", who, npix, C, pix_per_image);
        return false;
    }
    return true;
}
bool pool_ok(const char* who, int N, int H, int W, int Cin, int cat_pix, int choff) {
    if (N < 1 || H < 2 || W < 2 || (H & 1) || (W & 1) || !quads_ok(Cin) || choff < 0 || choff % 4 != 0 || cat_pix % 4 != 0 || choff + Cin > cat_pix) {
        lf_fail("%s: bad arguments (N %d H %d W %d Cin %d cat_pix %d choff %d)", who, N, H, W, Cin, cat_pix, choff);
        return false;
    }
    return true;
}
}  // namespace

int lf_debug_bn_finalize_fwd(const float* rows0, int nrows0, int ld0, int C0, int ch_off0, int tile_pix0, int seg_rows0, long seg_pix0,
                             const float* rows1, int nrows1, int ld1, int C1, int ch_off1, int tile_pix1, int seg_rows1, long seg_pix1,
                             int C, double count, const float* gamma, const float* beta, float* running_mean, float* running_var,
                             float momentum, float eps, int training, float* scale, float* shift, float* asc, float* ash, void* stream) {
    if (!(gamma && beta && running_mean && running_var && scale && shift && asc && ash)) { lf_fail("lf_debug_bn_finalize_fwd: null pointer"); return -1; }
    if (C < 4 || C % 4 != 0 || !(count >= 1.0)) { lf_fail("lf_debug_bn_finalize_fwd: bad arguments (C %d count %g)", C, count); return -1; }
    const float* const rows[2] = {rows0, rows1};
    const int nrows[2] = {nrows0, nrows1}, ld[2] = {ld0, ld1}, Cs[2] = {C0, C1}, ch_off[2] = {ch_off0, ch_off1}, tile_pix[2] = {tile_pix0, tile_pix1},
              seg_rows[2] = {seg_rows0, seg_rows1};
    const long seg_pix[2] = {seg_pix0, seg_pix1};
    LfStatPart parts[2];
    const int n = debug_stat_parts("lf_debug_bn_finalize_fwd", rows, nrows, ld, Cs, ch_off, tile_pix, seg_rows, seg_pix, C, parts);
    if (n < 0) return -1;
    if (training && n == 0) { lf_fail("lf_debug_bn_finalize_fwd: training mode needs a source of partial rows"); return -1; }
    return lf_bn_finalize_fwd(parts, n, C, count, gamma, beta, running_mean, running_var, momentum, eps, training, scale, shift, asc, ash,
                              (hipStream_t)stream) ? -1 : 0;
}

int lf_debug_bn_bwd_finalize(const float* rows0, int nrows0, int ld0, int C0, int ch_off0, int tile_pix0, int seg_rows0, long seg_pix0,
                             const float* rows1, int nrows1, int ld1, int C1, int ch_off1, int tile_pix1, int seg_rows1, long seg_pix1,
                             int C, double count, const float* asc, const float* ash, float* c1, float* c2, float* ggamma, float* gbeta,
                             int training, void* stream) {
    if (!(asc && ash && c1 && c2 && ggamma && gbeta)) { lf_fail("lf_debug_bn_bwd_finalize: null pointer"); return -1; }
    if (C < 4 || C % 4 != 0 || !(count >= 1.0)) { lf_fail("lf_debug_bn_bwd_finalize: bad arguments (C %d count %g)", C, count); return -1; }
    const float* const rows[2] = {rows0, rows1};
    const int nrows[2] = {nrows0, nrows1}, ld[2] = {ld0, ld1}, Cs[2] = {C0, C1}, ch_off[2] = {ch_off0, ch_off1}, tile_pix[2] = {tile_pix0, tile_pix1},
              seg_rows[2] = {seg_rows0, seg_rows1};
    const long seg_pix[2] = {seg_pix0, seg_pix1};
    LfStatPart parts[2];
    const int n = debug_stat_parts("lf_debug_bn_bwd_finalize", rows, nrows, ld, Cs, ch_off, tile_pix, seg_rows, seg_pix, C, parts);
    if (n < 0) return -1;
    if (n == 0) { lf_fail("lf_debug_bn_bwd_finalize: no source of partial rows"); return -1; }
    return lf_bn_bwd_finalize(parts, n, C, count, asc, ash, c1, c2, ggamma, gbeta, training, (hipStream_t)stream) ? -1 : 0;
}

int lf_debug_bn_act(const float* x, const float* sc, const float* sh, const float* dm, const float* res, float* y, long npix, int C,
                    long pix_per_image, int s16, void* stream) {
    if (!(x && sc && sh && y)) { lf_fail("lf_debug_bn_act: null pointer"); return -1; }
    if (!(al16(x) && al16(sc) && al16(sh) && al16(dm) && al16(res) && al16(y))) { lf_fail("lf_debug_bn_act: pointers must be 16-byte aligned"); return -1; }
    if (!stream_ok("lf_debug_bn_act", npix, C, pix_per_image, dm)) return -1;
    return lf_bn_act(x, sc, sh, dm, res, y, npix, C, pix_per_image, s16 != 0, (hipStream_t)stream) ? -1 : 0;
}

int lf_debug_bn_bwd_reduce(const float* g, const float* y, const float* t, const float* asc, const float* ash, const float* dm, float* rows,
                           int ld, long npix, int C, long pix_per_image, int s16, void* stream) {
    if (!(g && t && asc && ash && rows)) { lf_fail("lf_debug_bn_bwd_reduce: null pointer"); return -1; }
    if (!(al16(g) && al16(y) && al16(t) && al16(dm))) { lf_fail("lf_debug_bn_bwd_reduce: pointers must be 16-byte aligned"); return -1; }
    if (!stream_ok("lf_debug_bn_bwd_reduce", npix, C, pix_per_image, dm)) return -1;
    if (!quads_ok(C)) { lf_fail("lf_debug_bn_bwd_reduce: unsupported channel count %d", C); return -1; }
    const int nrows = lf_bn_bwd_reduce_rows(npix);
    if (ld < nrows) { lf_fail("lf_debug_bn_bwd_reduce: ld %d below the %d rows of the launch", ld, nrows); return -1; }
    return lf_bn_bwd_reduce(g, y, t, asc, ash, dm, rows, ld, npix, C, pix_per_image, s16 != 0, (hipStream_t)stream) ? -1 : nrows;
}

int lf_debug_bn_bwd_apply(const float* g, const float* y, const float* t, const float* asc, const float* ash, const float* gamma,
                          const float* c1, const float* c2, const float* dm, float* g_t, float* g_z, long npix, int C, long pix_per_image,
                          int s16, void* stream) {
    if (!(g && t && asc && ash && gamma && c1 && c2 && g_t)) { lf_fail("lf_debug_bn_bwd_apply: null pointer"); return -1; }
    if (!(al16(g) && al16(y) && al16(t) && al16(asc) && al16(ash) && al16(gamma) && al16(c1) && al16(c2) && al16(dm) && al16(g_t) && al16(g_z))) {
        lf_fail("lf_debug_bn_bwd_apply: pointers must be 16-byte aligned");
        return -1;
    }
    if (!stream_ok("lf_debug_bn_bwd_apply", npix, C, pix_per_image, dm)) return -1;
    return lf_bn_bwd_apply(g, y, t, asc, ash, gamma, c1, c2, dm, g_t, g_z, npix, C, pix_per_image, s16 != 0, (hipStream_t)stream) ? -1 : 0;
}

int lf_debug_pool_concat_fwd(const float* x, int N, int H, int W, int Cin, float* cat, int cat_pix, int choff, float* rows, int ld, int s16,
                             void* stream) {
    if (!(x && cat) || !al16(x) || !al16(cat)) { lf_fail("lf_debug_pool_concat_fwd: null or misaligned pointer"); return -1; }
    if (!pool_ok("lf_debug_pool_concat_fwd", N, H, W, Cin, cat_pix, choff)) return -1;
    const int nrows = lf_pool_rows((long)N * (H / 2) * (W / 2));
    if (rows && ld < nrows) { lf_fail("lf_debug_pool_concat_fwd: ld %d below the %d rows of the launch", ld, nrows); return -1; }
    return lf_pool_concat_fwd(x, N, H, W, Cin, cat, cat_pix, choff, rows, ld, s16 != 0, (hipStream_t)stream) ? -1 : nrows;
}

int lf_debug_pool_affine_fwd(const float* x, int N, int H, int W, int Cin, float* cat, int cat_pix, int choff, const float* sc, const float* sh,
                             int s16, void* stream) {
    if (!(x && cat && sc && sh) || !al16(x) || !al16(cat) || !al16(sc) || !al16(sh)) { lf_fail("lf_debug_pool_affine_fwd: null or misaligned pointer"); return -1; }
    if (!pool_ok("lf_debug_pool_affine_fwd", N, H, W, Cin, cat_pix, choff)) return -1;
    return lf_pool_affine_fwd(x, N, H, W, Cin, cat, cat_pix, choff, sc, sh, s16 != 0, (hipStream_t)stream) ? -1 : 0;
}

int lf_debug_pool_bwd(const float* x, const float* gcat, int N, int H, int W, int Cin, int cat_pix, int choff, float* gx, int s16, void* stream) {
    if (!(x && gcat && gx) || !al16(x) || !al16(gcat) || !al16(gx)) { lf_fail("lf_debug_pool_bwd: null or misaligned pointer"); return -1; }
    if (!pool_ok("lf_debug_pool_bwd", N, H, W, Cin, cat_pix, choff)) return -1;
    return lf_pool_bwd(x, gcat, N, H, W, Cin, cat_pix, choff, gx, s16 != 0, (hipStream_t)stream) ? -1 : 0;
}

int lf_debug_stem_fwd(const float* img, int N, int Cin, int H, int W, const float* w, const float* b, const float* sc, const float* sh, float* cat,
                      float* rows, int ld, int s16, void* stream) {
    if (!(img && w && b && cat) || !al16(cat)) { lf_fail("lf_debug_stem_fwd: null or misaligned pointer"); return -1; }
    if (N < 1 || Cin < 1 || Cin > 4 || H < 2 || W < 2 || (H & 1) || (W & 1)) {
        lf_fail("lf_debug_stem_fwd: bad arguments (N %d Cin %d H %d W %d)", N, Cin, H, W);
        return -1;
    }
    if ((sc == nullptr) != (sh == nullptr)) { lf_fail("lf_debug_stem_fwd: scale and shift come together"); return -1; }
    hipStream_t st = (hipStream_t)stream;
    if (sc) return lf_stem_fwd_infer(img, N, Cin, H, W, w, b, sc, sh, cat, s16 != 0, st) ? -1 : 0;
    const int nrows = lf_stem_rows(N, H, W);
    if (rows && ld < nrows) { lf_fail("lf_debug_stem_fwd: ld %d below the %d rows of the launch", ld, nrows); return -1; }
    return lf_stem_fwd(img, N, Cin, H, W, w, b, cat, rows, ld, s16 != 0, st) ? -1 : nrows;
}

int lf_debug_head_fwd(const float* x, const float* w, const float* b, float* out, int N, int h, int w_, int K, int s16, void* stream) {
    if (!(x && w && b && out) || !al16(x) || ((size_t)out & 7)) { lf_fail("lf_debug_head_fwd: null or misaligned pointer"); return -1; }
    if (N < 1 || h < 1 || w_ < 1 || K < 1 || K > 8) { lf_fail("lf_debug_head_fwd: bad arguments (N %d h %d w %d K %d)", N, h, w_, K); return -1; }
    return lf_head_fwd(x, w, b, out, N, h, w_, K, s16 != 0, (hipStream_t)stream) ? -1 : 0;
}

int lf_debug_head_bwd_data(const float* gout, const float* w, float* gx, int N, int h, int w_, int K, int s16, void* stream) {
    if (!(gout && w && gx) || !al16(gx) || ((size_t)gout & 7)) { lf_fail("lf_debug_head_bwd_data: null or misaligned pointer"); return -1; }
    if (N < 1 || h < 1 || w_ < 1 || K < 1 || K > 8) { lf_fail("lf_debug_head_bwd_data: bad arguments (N %d h %d w %d K %d)", N, h, w_, K); return -1; }
    return lf_head_bwd_data(gout, w, gx, N, h, w_, K, s16 != 0, (hipStream_t)stream) ? -1 : 0;
}

namespace {
int conv1d_bwd_weight(const float* x, const float* gy, const float* sc, const float* sh, float* gw, float* gb, int N, int H, int W, int C,
                      int axis, int dilation, float* scratch, hipStream_t st) {
    const LfTapGeom g = conv1d_geom(N, H, W, C, axis, dilation);
    const int pro = sc ? LF_PRO_BNRELU : LF_PRO_NONE;
    LfWgradArgs a;
    a.x = x; a.g = gy; a.pro_sc = sc; a.pro_sh = sh; a.s16 = g_ops_bf16 == 2;
    a.split = 0;
    a.partial = scratch;
    a.bias_partial = gb ? scratch + (long)lf_tapwgrad_splits_bound(g, 1) * 3 * C * C : nullptr;
    int rc = lf_tapwgrad_launch(g, a, pro, st);
    if (rc) return rc;
    const int idx[3] = {0, 1, 2};
    const int nsplit = lf_tapwgrad_splits_for(g, a, pro);
    return lf_wgrad_reduce_launch(a.partial, nsplit, 3, C, C, gw, 3L, 3L * C, idx, a.bias_partial, nsplit, gb, 0, st);
}
}  // namespace

// gw (C,C,3) and gb (C) from x and gy
int lf_conv1d_bwd_weight(const float* x, const float* gy, float* gw, float* gb, int N, int H, int W, int C, int axis,
                         int dilation, float* scratch, void* stream) {
    LF_REQUIRE(x && gy && gw && scratch, "lf_conv1d_bwd_weight: null pointer");
    return conv1d_bwd_weight(x, gy, nullptr, nullptr, gw, gb, N, H, W, C, axis, dilation, scratch, (hipStream_t)stream);
}

// scratch of lf_debug_conv1d_bwd_pair: [packed data-gradient weights 3 C C][partial rows: rows x 3 C C][bias rows: rows x C]
long lf_debug_conv1d_bwd_pair_scratch_floats(int N, int H, int W, int C) {
    if (N < 1 || H < 1 || W < 1 || C < 1) return -1;
    const long rows = lf_tapwgrad_splits(conv1d_geom(N, H, W, C, 0, 1));
    return 3L * C * C + rows * (3L * C * C + C);
}

int lf_debug_conv1d_bwd_pair(const float* x, const float* gy, const float* w, int epi, const float* add_src, const float* aux,
                             const float* msc, const float* msh, const float* pro_sc, const float* pro_sh, float* gx, float* gw, float* gb,
                             float* stats, int N, int H, int W, int C, int axis, int dilation, float* scratch, void* stream) {
    if (!(x && gy && w && gx && gw && gb && scratch)) { lf_fail("lf_debug_conv1d_bwd_pair: null pointer"); return -1; }
    if (N < 1 || H < 1 || W < 1 || C < 1 || dilation < 1 || (axis != 0 && axis != 1)) { lf_fail("lf_debug_conv1d_bwd_pair: bad arguments"); return -1; }
    if (g_ops_bf16 == 2) { lf_fail("lf_debug_conv1d_bwd_pair: fp32 tensors only"); return -1; }
    hipStream_t st = (hipStream_t)stream;
    const LfTapGeom g = conv1d_geom(N, H, W, C, axis, dilation);
    const long rows = lf_tapwgrad_splits(g);
    LfTapArgs a;
    memset(&a, 0, sizeof(a));
    LfWgradArgs wa;
    wa.x = x; wa.g = gy; wa.pro_sc = pro_sc; wa.pro_sh = pro_sh; wa.s16 = 0; wa.split = 0;
    wa.partial = scratch + 3L * C * C;
    wa.bias_partial = wa.partial + rows * 3L * C * C;
    a.wp = scratch;
    a.src = gy; a.dst = gx; a.add_src = add_src; a.msc = msc; a.msh = msh; a.stats = stats;
    a.mask_src = (epi & LF_EPI_MASK) ? x : nullptr;
    a.aux = (epi & LF_EPI_MASKBN) ? x : aux;
    a.stats_ld = lf_tapgemm_stat_rows(g);        // the caller's buffer: [2][C][rows], rows = ceil(N * H * W / 256)
    const int pro = pro_sc ? LF_PRO_BNRELU : LF_PRO_NONE;
    if (!lf_tapbwd16_ok(g, g, wa, a, pro, epi)) {
        lf_fail("lf_debug_conv1d_bwd_pair: the fused kernel does not take this launch (epi %d, prologue %d, %d x %d x %d x %d)", epi, pro, N, H, W, C);
        return -1;
    }
    hipLaunchKernelGGL(pack_one_kernel, dim3(64), dim3(256), 0, st, w, scratch, C, C, 3, 3L * C, 3L, conv1d_taps(1));
    if (lf_tapbwd16_launch(g, g, wa, a, pro, epi, st)) return -1;
    const int idx[3] = {0, 1, 2};
    const int nsplit = lf_tapwgrad_splits_for(g, wa, pro);
    if (lf_wgrad_reduce_launch(wa.partial, nsplit, 3, C, C, gw, 3L, 3L * C, idx, wa.bias_partial, nsplit, gb, 0, st)) return -1;
    return (epi & LF_EPI_STATS_XHAT) ? lf_tapgemm_stat_rows_for(g, a) : 0;
}

int lf_debug_conv1d_wgrad_pro(const float* x, const float* gy, const float* sc, const float* sh, float* gw, float* gb, int N, int H, int W,
                              int C, int axis, int dilation, float* scratch, void* stream) {
    LF_REQUIRE(x && gy && sc && sh && gw && scratch, "lf_debug_conv1d_wgrad_pro: null pointer");
    return conv1d_bwd_weight(x, gy, sc, sh, gw, gb, N, H, W, C, axis, dilation, scratch, (hipStream_t)stream);
}

}  // extern "C"
