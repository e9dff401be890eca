// Small host-side helpers shared by the plan builders (lf_erfnet.hip, lf_convchain.hip) and the kernel-level hooks (lf_ops.hip).
#pragma once
#include <string.h>

#include "lf_conv.h"

#define LF_TRY(expr)              \
    do {                          \
        int rc_ = (expr);         \
        if (rc_ != 0) return rc_; \
    } while (0)

struct LfBump {   // workspace layout: float offsets, 256-byte aligned
    long cur = 0;
    long take(long nfloats) { long o = cur; cur += (nfloats + 63) / 64 * 64; return o; }
};

inline long lf_maxl(long a, long b) { return a > b ? a : b; }

inline LfTapArgs lf_no_args() { LfTapArgs a; memset(&a, 0, sizeof(a)); return a; }

// logical grid == source grid == destination grid, unit strides, no taps yet
inline LfTapGeom lf_base_geom(int N, int Hl, int Wl, int Hs, int Ws, int Cs_pix, int Hd, int Wd, int Cd_pix, int Cs, int Cd) {
    LfTapGeom g;
    memset(&g, 0, sizeof(g));
    g.N = N; g.Hl = Hl; g.Wl = Wl;
    g.Hs = Hs; g.Ws = Ws; g.s_pix = Cs_pix; g.s_choff = 0; g.ssh = 1; g.ssw = 1;
    g.Hd = Hd; g.Wd = Wd; g.d_pix = Cd_pix; g.d_choff = 0; g.dsh = 1; g.dsw = 1; g.dah = 0; g.daw = 0;
    g.Cs = Cs; g.Cd = Cd; g.ntaps = 0;
    return g;
}

// One tap-GEMM launch of a stride-2 layer: its geometry and how its packed weights are gathered from the layer's (.., .., 3, 3)
// weight tensor -- wp[t][k][n] = w[k * sk + n * sn + tapidx[t]].  Built here, once, for the plan (lf_erfnet.hip) and for the
// kernel-level hook (lf_debug_stride2_epi, lf_ops.hip): the tests of the hook test the plan's geometry.
struct LfStride2Op {
    LfTapGeom geom;
    int Kc, Nc;
    long sk, sn;
    int tapidx[LF_MAX_TAPS];
};

// sub-pixel phase tap sets shared by "3x3 s2 conv data-gradient" and "3x3 s2 transposed conv forward"
inline int lf_phase_taps(int a, int* k, int* off) {
    if (a == 0) { k[0] = 1; off[0] = 0; return 1; }
    k[0] = 0; off[0] = 1; k[1] = 2; off[1] = 0;
    return 2;
}
// the taps of phase (a, b) appended to g; ti: the 3x3 kernel element of each
inline void lf_phase_geom_taps(LfTapGeom& g, int a, int b, int* ti) {
    int kh[2], oh[2], kw[2], ow[2];
    const int na = lf_phase_taps(a, kh, oh), nb = lf_phase_taps(b, kw, ow);
    for (int i = 0; i < na; ++i)
        for (int j = 0; j < nb; ++j) { g.tdh[g.ntaps] = oh[i]; g.tdw[g.ntaps] = ow[j]; ti[g.ntaps] = kh[i] * 3 + kw[j]; ++g.ntaps; }
}
// the 9 taps of a 3x3 stride-2 window appended to g (source stride 2)
inline void lf_window9_taps(LfTapGeom& g, int* ti) {
    g.ssh = 2; g.ssw = 2; g.ntaps = 9;
    for (int kh = 0; kh < 3; ++kh)
        for (int kw = 0; kw < 3; ++kw) { g.tdh[kh * 3 + kw] = kh - 1; g.tdw[kh * 3 + kw] = kw - 1; ti[kh * 3 + kw] = kh * 3 + kw; }
}

// DownsamplerBlock conv: Conv2d(Cin, Cc, 3, stride 2, pad 1), weight (Cc,Cin,3,3), writing channels [0,Cc) of the Ccat-wide concat
// buffer; dg[a * 2 + b]: the data gradient's sub-pixel phase (a, b), reading the Ccat-wide gradient at Cs = Cc
inline void lf_down_conv_ops(int N, int H, int W, int Cin, int Cc, int Ccat, LfStride2Op& fwd, LfStride2Op dg[4]) {
    const int Ho = H / 2, Wo = W / 2;
    fwd.geom = lf_base_geom(N, Ho, Wo, H, W, Cin, Ho, Wo, Ccat, Cin, Cc);
    lf_window9_taps(fwd.geom, fwd.tapidx);
    fwd.Kc = Cin; fwd.Nc = Cc; fwd.sk = 9; fwd.sn = (long)Cin * 9;
    for (int a = 0; a < 2; ++a)
        for (int b = 0; b < 2; ++b) {
            LfStride2Op& d = dg[a * 2 + b];
            d.geom = lf_base_geom(N, Ho, Wo, Ho, Wo, Ccat, H, W, Cin, Cc, Cin);
            d.geom.dsh = 2; d.geom.dsw = 2; d.geom.dah = a; d.geom.daw = b;
            lf_phase_geom_taps(d.geom, a, b, d.tapidx);
            d.Kc = Cc; d.Nc = Cin; d.sk = (long)Cin * 9; d.sn = 9;
        }
}

// UpsamplerBlock conv: ConvTranspose2d(Cin, Co, 3, stride 2, pad 1, output_padding 1), weight (Cin,Co,3,3); fph[a * 2 + b]: the
// forward's sub-pixel phase (a, b); dg: its data gradient (9 taps, stride 2)
inline void lf_up_conv_ops(int N, int Hi, int Wi, int Cin, int Co, LfStride2Op fph[4], LfStride2Op& dg) {
    for (int a = 0; a < 2; ++a)
        for (int b = 0; b < 2; ++b) {
            LfStride2Op& f = fph[a * 2 + b];
            f.geom = lf_base_geom(N, Hi, Wi, Hi, Wi, Cin, 2 * Hi, 2 * Wi, Co, Cin, Co);
            f.geom.dsh = 2; f.geom.dsw = 2; f.geom.dah = a; f.geom.daw = b;
            lf_phase_geom_taps(f.geom, a, b, f.tapidx);
            f.Kc = Cin; f.Nc = Co; f.sk = (long)Co * 9; f.sn = 9;
        }
    dg.geom = lf_base_geom(N, Hi, Wi, 2 * Hi, 2 * Wi, Co, Hi, Wi, Cin, Co, Cin);
    lf_window9_taps(dg.geom, dg.tapidx);
    dg.Kc = Co; dg.Nc = Cin; dg.sk = 9; dg.sn = (long)Co * 9;
}

// ---- Weight-gradient reductions: how a launch's partial rows become a reduction job, and how the four sub-pixel phases of a
// transposed convolution share one bias gradient.  Built here, once, for the plan (run_wgrad / row_sums_finish, lf_erfnet.hip) and
// for the kernel-level hooks (lf_debug_stride2_wgrad, lf_debug_stem_wgrad, lf_debug_head_wgrad, lf_ops.hip): the tests of the hooks
// test the plan's own jobs.

// floats of the partial-row regions of one weight-gradient launch (upper bound over the kernels that may take it)
inline long lf_wgrad_wneed(const LfTapGeom& g, int s16) { return (long)lf_tapwgrad_splits_bound(g, s16) * g.ntaps * g.Cs * g.Cd; }
inline long lf_wgrad_bneed(const LfTapGeom& g, int s16) { return (long)lf_tapwgrad_splits_bound(g, s16) * g.Cd; }

// the batched reduction of one weight-gradient launch that wrote nsplit rows: grad[k * sk + n * sn + tapidx[t]] = sum_s partial[s][t][k][n],
// bias_grad[n] = sum_r bias_rows[r][n] (bias_rows / bias_grad may be null)
inline LfReduceJob lf_wgrad_reduce_job(const LfTapGeom& g, const float* partial, int nsplit, float* grad, long sk, long sn,
                                       const int* tapidx, const float* bias_rows, float* bias_grad) {
    LfReduceJob j;
    memset(&j, 0, sizeof(j));
    j.partial = partial; j.grad = grad; j.bias_rows = bias_rows; j.bias_grad = bias_grad;
    j.sk = sk; j.sn = sn; j.splits = nsplit; j.ntaps = g.ntaps; j.Cs = g.Cs; j.Cd = g.Cd;
    j.n_bias_rows = nsplit;
    for (int t = 0; t < g.ntaps; ++t) j.tapidx[t] = tapidx[t];
    return j;
}

// The four sub-pixel phases of a transposed convolution have ONE bias gradient: in batched mode their bias partial rows are laid
// end to end (the phases' own bias regions are adjacent) and summed by the last phase's reduction job
struct LfBiasChain { float* base = nullptr; int rows = 0; int phase = 0; };
// where the next phase writes its bias rows; region: that phase's own bias region (the chain starts at phase 0's)
inline float* lf_bias_chain_rows(LfBiasChain& ch, float* region, int Cd) {
    if (ch.phase == 0) ch.base = region;
    return ch.base + (long)ch.rows * Cd;
}
// the phase wrote nsplit rows: its job sums no bias rows, except the last phase's, which sums the whole chain (has_bias: the
// launches wrote bias rows at all)
inline void lf_bias_chain_job(LfBiasChain& ch, LfReduceJob& j, int nsplit, bool has_bias) {
    ch.rows += nsplit;
    const bool last = ++ch.phase == 4;
    j.bias_rows = (last && has_bias) ? ch.base : nullptr;
    j.n_bias_rows = ch.rows;
    if (!last) j.bias_grad = nullptr;
}

// plain column sums as a batched job: dst[n] = sum_r rows[r][n], n < width (the stem / head weight-gradient rows)
inline LfReduceJob lf_row_sum_job(const float* rows, int nrows, int width, float* dst) {
    LfReduceJob j;
    memset(&j, 0, sizeof(j));
    j.partial = rows; j.grad = dst; j.sk = 0; j.sn = 1; j.splits = nrows; j.ntaps = 1; j.Cs = 1; j.Cd = width;
    return j;
}
