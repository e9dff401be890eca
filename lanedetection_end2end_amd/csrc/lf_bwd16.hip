// Backward of the fp32 16 -> 16 channel 3-tap convolutions (the decoder's full-resolution non_bottleneck_1d blocks) in ONE pass
// over the pixels: the weight gradient of tapwgrad16_f32_kernel (lf_wgrad.hip) and the data gradient of tapgemm_lean_kernel
// (lf_conv.hip) read the same two tensors -- the gradient g at the three tap positions and at the centre, the convolution's input x
// at the three tap positions and, as the data gradient's ReLU mask / recomputed-BN operand, at the centre.  As two launches each
// tensor crosses the fabric twice; these launches are bound by bytes.
//
// tapbwd16_kernel keeps the weight gradient's ownership: a wave walks a contiguous pixel range (wgrad_cfg's, so the partial rows are
// the same rows) one 16-pixel group at a time through a PRIVATE LDS-DMA ring, no barrier in the loop.  A stage holds 1 KB tiles
// (16 pixels x 64 bytes, whole pixels, lane-linear): g at taps 0 1 2, x at taps 0 1 2, and -- the forms that have them -- the
// residual (add_src) and the BN-backward operand (aux) at the group itself.  A padding position carries the out-of-range offset and
// lands as zeros.  From one stage:
//   weight gradient   ds_read_b32 fragments, lane (channel l & 15, pixel slot l >> 4), K = 4 pixels per v_mfma_f32_16x16x4_f32:
//                     the instruction order of tapwgrad16_f32_kernel, the same 4-wave reduction -> gw / gb bit for bit;
//   data gradient     ds_read_b128 of the g tiles, lane (pixel l & 15, channels 4 (l >> 4) ..), the packed weights in 12 registers:
//                     one 16-product chain per tap, the three summed in tap order -> gx bit for bit tapgemm_lean_kernel's;
//   epilogue          the shared text of lf_conv_epi.h on the one 16-pixel tile, its operand loads redirected to the stage
//                     (the mask is the centre x tile); each lane stores its 16 bytes of a 64-byte pixel.
// Ring order per wave and group:  s_waitcnt lgkmcnt(0) (my reads of the slot restaged next have retired) ; issue the group STAGES - 1
// ahead ; s_waitcnt vmcnt(N) ; read ; MFMAs ; epilogue.  N = the DMA instructions of the STAGES - 1 younger stages.  The loop's
// other vector-memory instructions are the output store and, every 16th group, the statistics row: they are younger than the
// awaited stage too, so N under-counts and the wait can only be longer than needed (vmcnt retires in issue order).  No load of the
// loop goes through the compiler's own counting: a counted load behind an uncounted DMA would drain the ring.
// Statistics rows ([2][16][rows], one per 256 pixels): a wave whose range is whole 256-pixel rows writes them itself; with 64-pixel
// ranges the workgroup is one row and LF_EPI_TAIL merges the four waves (small launches).  lf_tapbwd16_ok admits nothing else.
#include "lf_conv_dev.h"
#include "lf_conv_epi.h"

namespace {

constexpr int B16_TILE = 1024;
template <int EPIC> struct B16Cfg {
    static constexpr bool ST_ADD = (EPIC & LF_EPI_ADD) != 0;
    static constexpr bool AUX_IS_X = (EPIC & LF_EPI_MASKBN) != 0;                            // the recomputed-BN operand is x itself
    static constexpr bool ST_AUX = (EPIC & LF_EPI_STATS_XHAT) != 0 && !AUX_IS_X;            // a tensor of its own
    static constexpr bool SUMS = (EPIC & LF_EPI_STATS_XHAT) != 0;
    static constexpr int T_ADD = 6, T_AUX = ST_AUX ? 6 + (ST_ADD ? 1 : 0) : 4;
    static constexpr int NTILE = 6 + (ST_ADD ? 1 : 0) + (ST_AUX ? 1 : 0);                    // = DMA instructions per stage
    static constexpr int STAGES = NTILE == 6 ? 3 : 2;                                        // two workgroups per CU: <= 80 KB each
    static constexpr int STAGE = NTILE * B16_TILE, WAVE_LDS = STAGES * STAGE;
    static_assert(WG_WAVES * WAVE_LDS + 1024 <= 80 * 1024, "two workgroups per CU");
    static_assert(WAVE_LDS >= 13 * 64 * 4, "the ring also stages the wave's weight-gradient sums");
};

typedef __attribute__((address_space(3))) float* lds_f32_p;
typedef __attribute__((address_space(3))) f32x4* lds_f32x4_p;
typedef __attribute__((address_space(3))) unsigned char* lds_u8_p;

template <bool PRO, int EPIC>
__global__ __launch_bounds__(256, 2) void tapbwd16_kernel(const LfTapGeom g, const LfWgradArgs wa, const LfTapArgs a, const long pps,
                                                          const int write_bias, const int wave_rows) {
    using Cfg = B16Cfg<EPIC>;
    constexpr int NTAPS = 3, NT = 1, epi = EPIC;
    constexpr bool S16 = false, HOISTV = true;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int pl = lane & 15, kq = lane >> 4;
    const long npix_l = (long)g.N * g.Hl * g.Wl;
    const unsigned npix = (unsigned)npix_l, bx = blockIdx.x;
    const int cob = 0;
    const long sub = (long)blockIdx.x * WG_WAVES + wave;
    const long p_begin = sub * pps;
    long p_end = p_begin + pps;
    if (p_end > npix_l) p_end = npix_l;
    const int niter = p_end > p_begin ? (int)((p_end - p_begin + 15) / 16) : 0;
    f32x4 acc[NTAPS];
#pragma unroll
    for (int t = 0; t < NTAPS; ++t) acc[t] = zero4();
    float bsum = 0.f;
    const unsigned tbytes = (unsigned)min((long)g.N * g.Hs * g.Ws * g.s_pix * 4, (long)LF_OOB);      // every tensor has x's geometry
    const i32x4s rx = make_rsrc_words(wa.x, tbytes), rg = make_rsrc_words(wa.g, tbytes),
                 radd = make_rsrc_words(a.add_src, Cfg::ST_ADD ? tbytes : 0u), raux = make_rsrc_words(a.aux, Cfg::ST_AUX ? tbytes : 0u);
    lds_u8_p const ring = (lds_u8_p)lf_tap_lds + wave * Cfg::WAVE_LDS;
    const unsigned lds0 = (unsigned)(size_t)ring;
    const int tdh0 = g.tdh[0], tdh1 = g.tdh[1], tdh2 = g.tdh[2], tdw0 = g.tdw[0], tdw1 = g.tdw[1], tdw2 = g.tdw[2];
    // load cursor: (image, row, column) of the next 16-pixel group (wave-uniform; Wl % 64 == 0: a group lies in one row)
    long p_ld = p_begin;
    int pj_, pi_, pn_;
    row1_coords(g, niter ? (unsigned)p_begin : 0u, pn_, pi_, pj_);
    int cj = pj_, ci = pi_, cn = pn_;                         // compute cursor: the group being multiplied and stored
    const int px = lane >> 2, chunk = lane & 3;
    int slot_ld = 0;
    auto issue = [&]() __attribute__((always_inline)) {
        const bool ok = p_ld < p_end;
        const int j = pj_ + px;
        const unsigned dst = lds0 + (unsigned)(slot_ld * Cfg::STAGE);
#pragma unroll
        for (int t = 0; t < NTAPS; ++t) {
            const int dh = t == 0 ? tdh0 : t == 1 ? tdh1 : tdh2, dw = t == 0 ? tdw0 : t == 1 ? tdw1 : tdw2;
            const int sy = pi_ + dh, sx = j + dw;
            const bool in = ok && sy >= 0 && sy < g.Hs && sx >= 0 && sx < g.Ws;
            const unsigned o = in ? (unsigned)((((pn_ * g.Hs + sy) * g.Ws + sx) * g.s_pix + g.s_choff + chunk * 4) * 4) : LF_OOB;
            lds_dma16(rg, dst + (unsigned)(t * B16_TILE), o, 0u);
            lds_dma16(rx, dst + (unsigned)((3 + t) * B16_TILE), o, 0u);
        }
        if constexpr (Cfg::ST_ADD || Cfg::ST_AUX) {
            const unsigned o = ok ? (unsigned)((((pn_ * g.Hs + pi_) * g.Ws + j) * g.s_pix + g.s_choff + chunk * 4) * 4) : LF_OOB;
            if constexpr (Cfg::ST_ADD) lds_dma16(radd, dst + (unsigned)(Cfg::T_ADD * B16_TILE), o, 0u);
            if constexpr (Cfg::ST_AUX) lds_dma16(raux, dst + (unsigned)(Cfg::T_AUX * B16_TILE), o, 0u);
        }
        slot_ld = slot_ld == Cfg::STAGES - 1 ? 0 : slot_ld + 1;
        p_ld += 16;
        pj_ += 16;
        if (pj_ >= g.Wl) { pj_ = 0; if (++pi_ >= g.Hl) { pi_ = 0; ++pn_; } }
    };
    // everything the compiler counts is loaded, and has arrived, before the first DMA: the packed data-gradient weights
    // [tap][4][16][4] (tapgemm_lean_kernel's operand: lane (output channel pl, source channels 4 s4 + kq)), the prologue's and the
    // epilogue's per-channel vectors
    f32x4 w3[NTAPS];
    {
        const __amdgpu_buffer_rsrc_t rwl = make_rsrc(a.wp, (unsigned)(NTAPS * 16 * 16 * 4));
#pragma unroll
        for (int t = 0; t < NTAPS; ++t) w3[t] = ldb4(rwl, (unsigned)(kq * 16 + pl) * 16u, (unsigned)(t * 16 * 64));
    }
    float psc = 1.f, psh = 0.f;
    if constexpr (PRO) { psc = wa.pro_sc[pl]; psh = wa.pro_sh[pl]; }
#undef LF_EPI_ACC
#define LF_EPI_ACC(n, m) dacc
#undef LF_EPI_LDADD
#define LF_EPI_LDADD(o) (*(lds_f32x4_p)(epi_lane + Cfg::T_ADD * B16_TILE))
#undef LF_EPI_LDMSK
#define LF_EPI_LDMSK(o) (*(lds_f32x4_p)(epi_lane + 4 * B16_TILE))
#undef LF_EPI_LDAUX
#define LF_EPI_LDAUX(o) (*(lds_f32x4_p)(epi_lane + Cfg::T_AUX * B16_TILE))
#undef LF_EPI_HOIST_ALL
#define LF_EPI_HOIST_ALL true
#undef LF_EPI_ROW1
#define LF_EPI_ROW1 true      /* no per-tile Dropout2d factor: a launch with a.dm is declined (its load would be a counted load in the loop) */
    LF_EPI_HEAD
    (void)r_add; (void)r_msk; (void)r_aux;                    // (the loads they serve elsewhere read the stage here)
    if constexpr ((EPIC & LF_EPI_MASKBN) != 0) asm volatile("" ::"v"(hv[0][0]), "v"(hv[0][1]) : "memory");
    asm volatile("s_waitcnt vmcnt(0)" ::"v"(w3[0]), "v"(w3[1]), "v"(w3[2]), "v"(psc), "v"(psh) : "memory");
#pragma unroll
    for (int q = 0; q < Cfg::STAGES - 1; ++q) issue();
    int slot_c = 0;
    f32x4 row1 = zero4(), row2 = zero4();                     // the running 256-pixel statistics row of a wave that owns whole rows
    for (int it = 0; it < niter; ++it) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        issue();
        wait_vm_lgkm0<Cfg::NTILE * (Cfg::STAGES - 1)>();
        lds_u8_p const st = ring + slot_c * Cfg::STAGE;
        slot_c = slot_c == Cfg::STAGES - 1 ? 0 : slot_c + 1;
        lds_u8_p const epi_lane = st + pl * 64 + kq * 16;     // the accumulator's lane layout: pixel pl, channels 4 kq .. 4 kq + 3
        // ---- weight gradient: tapwgrad16_f32_kernel's fragments and instruction order
        {
            lds_f32_p const frag = (lds_f32_p)(st + kq * 64 + pl * 4);
            float gv[4], xv[NTAPS][4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                gv[u] = frag[(1 * B16_TILE + u * 256) / 4];
#pragma unroll
                for (int t = 0; t < NTAPS; ++t) xv[t][u] = frag[((3 + t) * B16_TILE + u * 256) / 4];
            }
            if constexpr (PRO) {
#pragma unroll
                for (int t = 0; t < NTAPS; ++t) {
                    const int dh = t == 0 ? tdh0 : t == 1 ? tdh1 : tdh2, dw = t == 0 ? tdw0 : t == 1 ? tdw1 : tdw2;
                    const bool rowok = (unsigned)(ci + dh) < (unsigned)g.Hs;
                    const int c0 = cj + dw;
                    const bool edge = c0 < 0 || c0 + 15 >= g.Ws;
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        float v = fmaxf(xv[t][u] * psc + psh, 0.f);
                        if (edge) v = (unsigned)(c0 + 4 * u + kq) < (unsigned)g.Ws ? v : 0.f;
                        xv[t][u] = rowok ? v : 0.f;
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
#pragma unroll
                for (int t = 0; t < NTAPS; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[t][u], gv[u], acc[t], 0, 0, 0);
                bsum += gv[u];
            }
        }
        // ---- data gradient: tapgemm_lean_kernel's arithmetic (one 16-product chain per tap, summed in tap order)
        f32x4 dacc;
#pragma unroll
        for (int t = 0; t < NTAPS; ++t) {
            const f32x4 x3 = *(lds_f32x4_p)(epi_lane + t * B16_TILE);
            f32x4 part;
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) part = __builtin_amdgcn_mfma_f32_16x16x4f32(w3[t][s4], x3[s4], s4 ? part : zero4(), 0, 0, 0);
            dacc = t ? dacc + part : part;
        }
        {
            const int pn[1] = {cn}, pi[1] = {ci}, pj[1] = {cj + pl};
            const bool pv[1] = {true};                        // (a range ends on a group boundary: npix % 16 == 0)
            LF_EPI_TILE(0)
        }
        if constexpr (Cfg::SUMS) {
            // a wave that owns whole 256-pixel rows.  tapgemm_lean_kernel's association, so that the rows are its rows bit for bit: the
            // lane sums of 64 pixels (one of its waves) -> sum16, the four 64-pixel totals added in order; the row leaves with its last group
            if (wave_rows && ((it & 3) == 3 || it == niter - 1)) {
                f32x4 q1, q2;
                q1.x = sum16(s1[0].x); q1.y = sum16(s1[0].y); q1.z = sum16(s1[0].z); q1.w = sum16(s1[0].w);
                q2.x = sum16(s2[0].x); q2.y = sum16(s2[0].y); q2.z = sum16(s2[0].z); q2.w = sum16(s2[0].w);
                const bool first = (it & 15) < 4;
                row1 = first ? q1 : row1 + q1;
                row2 = first ? q2 : row2 + q2;
                s1[0] = zero4(); s2[0] = zero4();
                if (((it & 15) == 15 || it == niter - 1) && pl == 0) {
                    const long row = (p_begin >> 8) + (it >> 4);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        a.stats[(long)(kq * 4 + e) * a.stats_ld + row] = row1[e];
                        a.stats[(long)(g.Cd + kq * 4 + e) * a.stats_ld + row] = row2[e];
                    }
                }
            }
        }
        cj += 16;
        if (cj >= g.Wl) { cj = 0; if (++ci >= g.Hl) { ci = 0; ++cn; } }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // the trailing (dead) stages: nothing may land in LDS after this
    if (!wave_rows) {
        const int pn[1] = {0};                                // (named by the tail's ROW1 form, which is compiled out)
        LF_EPI_TAIL
    }
#undef LF_EPI_ACC
#define LF_EPI_ACC(n, m) acc[n][m]
#undef LF_EPI_LDADD
#define LF_EPI_LDADD(o) epi_ld<S16>(r_add, o)
#undef LF_EPI_LDMSK
#define LF_EPI_LDMSK(o) epi_ld<S16>(r_msk, o)
#undef LF_EPI_LDAUX
#define LF_EPI_LDAUX(o) epi_ld<S16>(r_aux, o)
#undef LF_EPI_HOIST_ALL
#define LF_EPI_HOIST_ALL false
#undef LF_EPI_ROW1
#define LF_EPI_ROW1 false
    // the four waves' weight-gradient sums, staged in each wave's own (now dead) ring: [12 accumulator registers + bias][lane]
    float* const red = reinterpret_cast<float*>(lf_tap_lds);
    constexpr int RW = Cfg::WAVE_LDS / 4;
    if (wave > 0) {
#pragma unroll
        for (int t = 0; t < NTAPS; ++t)
#pragma unroll
            for (int e = 0; e < 4; ++e) red[wave * RW + (t * 4 + e) * 64 + lane] = acc[t][e];
    }
    red[wave * RW + 12 * 64 + lane] = bsum;
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int t = 0; t < NTAPS; ++t) {
            float* out = wa.partial + ((long)blockIdx.x * NTAPS + t) * g.Cs * g.Cd;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float v = acc[t][e];
#pragma unroll
                for (int w = 1; w < WG_WAVES; ++w) v += red[w * RW + (t * 4 + e) * 64 + lane];
                out[(long)(4 * kq + e) * g.Cd + pl] = v;          // row = x-channel 4*kq+e, col = g-channel pl
            }
        }
        if (write_bias && wa.bias_partial) {
            float v = red[12 * 64 + lane] + red[RW + 12 * 64 + lane] + red[2 * RW + 12 * 64 + lane] + red[3 * RW + 12 * 64 + lane];
            v += __shfl_xor(v, 16, 64);
            v += __shfl_xor(v, 32, 64);
            if (kq == 0) wa.bias_partial[(long)blockIdx.x * g.Cd + pl] = v;
        }
    }
}

std::atomic<int> g_bwd16_mode{1};             // lf_tapbwd16_set: 0 off, 1 the shipped routing, 2 * m the forms of bit mask m (A/B runs)
// forms (pro, epi) the network's launches take: every compiled form (DESIGN.md section 4 has the per-form step times)
enum { B16_MASK = 1, B16_MASKBN = 2, B16_EPI3 = 4, B16_ADD = 8 };
constexpr int g_bwd16_routed = B16_MASK | B16_MASKBN | B16_EPI3 | B16_ADD;

int form_of(int pro, int epi) {
    if (pro == LF_PRO_NONE && epi == LF_EPI_MASK) return B16_MASK;
    if (pro == LF_PRO_BNRELU && epi == (LF_EPI_MASKBN | LF_EPI_STATS_XHAT)) return B16_MASKBN;
    if (pro == LF_PRO_NONE && epi == (LF_EPI_ADD | LF_EPI_MASK | LF_EPI_STATS_XHAT)) return B16_EPI3;
    if (pro == LF_PRO_NONE && epi == LF_EPI_ADD) return B16_ADD;
    return 0;
}
template <typename F>
auto with_form(int form, F&& f) {
    switch (form) {
        case B16_MASK: return f(tapbwd16_kernel<false, LF_EPI_MASK>, B16Cfg<LF_EPI_MASK>{});
        case B16_MASKBN: return f(tapbwd16_kernel<true, LF_EPI_MASKBN | LF_EPI_STATS_XHAT>, B16Cfg<LF_EPI_MASKBN | LF_EPI_STATS_XHAT>{});
        case B16_EPI3: return f(tapbwd16_kernel<false, LF_EPI_ADD | LF_EPI_MASK | LF_EPI_STATS_XHAT>, B16Cfg<LF_EPI_ADD | LF_EPI_MASK | LF_EPI_STATS_XHAT>{});
        default: return f(tapbwd16_kernel<false, LF_EPI_ADD>, B16Cfg<LF_EPI_ADD>{});
    }
}

}  // namespace

void lf_tapbwd16_set(int mode) { g_bwd16_mode = mode < 0 ? 0 : mode; }
bool lf_tapbwd16_routed(int pro, int epi) {
    const int mode = g_bwd16_mode.load();
    const int forms = mode == 0 ? 0 : mode == 1 ? g_bwd16_routed : mode >> 1;
    return (forms & form_of(pro, epi)) != 0;
}

bool lf_tapbwd16_ok(const LfTapGeom& gf, const LfTapGeom& gd, const LfWgradArgs& w, const LfTapArgs& a, int pro, int epi) {
    const int form = form_of(pro, epi);
    if (!form) return false;
    // one geometry for both halves: stride 1, 3 taps about the pixel itself, dense 16-channel tensors of the logical size
    const LfTapGeom& g = gf;
    bool same = gf.N == gd.N && gf.Hl == gd.Hl && gf.Wl == gd.Wl && gf.Hs == gd.Hs && gf.Ws == gd.Ws && gf.s_pix == gd.s_pix && gf.s_choff == gd.s_choff &&
                gf.ssh == gd.ssh && gf.ssw == gd.ssw && gf.Hd == gd.Hd && gf.Wd == gd.Wd && gf.d_pix == gd.d_pix && gf.d_choff == gd.d_choff &&
                gf.dsh == gd.dsh && gf.dsw == gd.dsw && gf.dah == gd.dah && gf.daw == gd.daw && gf.Cs == gd.Cs && gf.Cd == gd.Cd && gf.ntaps == gd.ntaps;
    for (int t = 0; same && t < 3 && t < gf.ntaps; ++t) same = gf.tdh[t] == gd.tdh[t] && gf.tdw[t] == gd.tdw[t];
    if (!same) return false;
    if (!(g.Cs == 16 && g.Cd == 16 && g.ntaps == 3 && g.ssh == 1 && g.ssw == 1 && g.dsh == 1 && g.dsw == 1 && g.dah == 0 && g.daw == 0 &&
          g.Hs == g.Hl && g.Hd == g.Hl && g.Ws == g.Wl && g.Wd == g.Wl && g.s_pix == 16 && g.d_pix == 16 && g.s_choff == 0 && g.d_choff == 0 &&
          g.tdh[1] == 0 && g.tdw[1] == 0))
        return false;
    if (g.N < 1 || g.Hl < 1 || g.Wl < 64 || g.Wl % 64 != 0) return false;
    const long npix = (long)g.N * g.Hl * g.Wl;
    if (npix * 64 >= (long)LF_OOB) return false;                                    // 32-bit byte offsets, the out-of-range offset beyond the tensor
    if (lf_tapgemm_bf16_lds() < 3) return false;                                    // the LDS rings are switched off
    if (w.s16 || a.s16 || a.wp16 || w.dbg || a.dbg || a.bias || a.dm) return false;
    if (!w.x || !w.g || !w.partial || !w.bias_partial || !a.wp || !a.dst || a.src != w.g) return false;
    if (a.dst == w.x || a.dst == w.g) return false;
    if ((pro == LF_PRO_BNRELU) != (w.pro_sc != nullptr) || (w.pro_sc != nullptr) != (w.pro_sh != nullptr)) return false;
    if ((epi & LF_EPI_MASK) && a.mask_src != w.x) return false;
    if ((epi & LF_EPI_MASKBN) && (a.aux != w.x || !a.msc || !a.msh)) return false;
    if ((epi & LF_EPI_ADD) && (!a.add_src || a.add_src == a.dst)) return false;
    if ((epi & LF_EPI_STATS_XHAT) && (!a.aux || a.aux == a.dst || !a.stats)) return false;
    if (epi & LF_EPI_STATS_XHAT) {
        // who writes a 256-pixel statistics row: the wave that owns it, or the four 64-pixel waves of a workgroup together
        const long pps = lf_tapwgrad_wave_pixels(g);
        if (!(pps % 256 == 0 || pps == 64 || (lf_tapwgrad_splits(g) == 1 && npix <= 256))) return false;
        if (a.stats_ld < lf_tapgemm_stat_rows(g)) return false;
    }
    return with_form(form, [&](auto kern, auto cfg) {
        return allow_big_lds(reinterpret_cast<const void*>(kern), 128 * 1024);
    });
}

int lf_tapbwd16_launch(const LfTapGeom& gf, const LfTapGeom& gd, const LfWgradArgs& w, const LfTapArgs& a, int pro, int epi, hipStream_t st) {
    LF_REQUIRE(lf_tapbwd16_ok(gf, gd, w, a, pro, epi), "tapbwd16: the fused kernel does not take this launch (pro %d, epi %d, %d x %d x %d x %d -> %d)",
               pro, epi, gf.N, gf.Hl, gf.Wl, gf.Cs, gf.Cd);
    const long pps = lf_tapwgrad_wave_pixels(gf);
    const int gx = lf_tapwgrad_splits(gf);
    const int wave_rows = pps % 256 == 0;
    with_form(form_of(pro, epi), [&](auto kern, auto cfg) {
        hipLaunchKernelGGL(kern, dim3(gx), dim3(256), (size_t)WG_WAVES * decltype(cfg)::WAVE_LDS, st, gf, w, a, pps, 1, wave_rows);
        return true;
    });
    LF_CHECK_LAUNCH("tapbwd16");
    return 0;
}
