// The epilogue the tap-GEMM kernels of lf_conv.hip, lf_conv_pair.hip, lf_conv_bf16.hip and lf_bwd16.hip share (bias, ReLU, masks, residual, BatchNorm sums), as
// macros expanded inside the kernel body: they use the kernel's own names (g, a, epi, npix, bx, cob, wave, pl, kq, pn / pi / pj /
// pv, acc, and the constants NT, EPIC, S16, HOISTV).  Internal: included after lf_conv_dev.h by those four files and by
// lf_conv_stream.h (the stream tile body the first two share) only.
//
// Protocol of the LF_EPI_* parameters.  The values defined in this header are the DEFAULTS, and they hold at every point of a file
// outside a kernel that differs: such a kernel #undef's and redefines a parameter directly before the lines that expand the
// epilogue and restores this header's value directly after them, inside its own body.  A restore that is forgotten changes every
// kernel behind it in the file without a diagnostic, so a redefinition and its restore are kept within sight of each other.
// The kernels that redefine:
//   lf_conv.hip       tapgemm_kernel         LF_EPI_ONE_TILE, LF_EPI_TID, LF_EPI_ROW1
//                     tapgemm_thin_kernel    LF_EPI_LDADD (expands LF_EPI_HEAD / LF_EPI_TILE(0) / LF_EPI_TAIL: one pixel tile per wave)
//                     tapgemm_split_kernel   LF_EPI_GROUPS (around the whole kernel), LF_EPI_PIVOT
//   lf_conv_stream.h  stream_tile            LF_EPI_GROUPS, LF_EPI_ROW1, LF_EPI_ACC, LF_EPI_FIRST, LF_EPI_ROW_OK -- the tile body of
//                                            tapstream_kernel (lf_conv.hip) and tappair_kernel (lf_conv_pair.hip): the stream
//                                            family's only redefinitions
//   lf_conv_pair.hip  tappair128_kernel      LF_EPI_GROUPS, LF_EPI_TID, LF_EPI_ROW1, LF_EPI_TILE_OF (in pair128_phase)
//   lf_conv_bf16.hip  tapgemm_bf16_kernel, tapgemm_bf16_ring_kernel   LF_EPI_PIVOT
//                     tapgemm_bf16_thin_kernel   LF_EPI_LDADD (expands LF_EPI_HEAD / LF_EPI_TILE(0) / LF_EPI_TAIL, as tapgemm_thin_kernel)
//   lf_bwd16.hip      tapbwd16_kernel        LF_EPI_ACC, LF_EPI_ROW1, LF_EPI_LDADD, LF_EPI_LDMSK, LF_EPI_LDAUX, LF_EPI_HOIST_ALL
// tapgemm_lean_kernel and tapgemm_bf16_lean_kernel expand the defaults; the whole-line and wave-private bf16 kernels have epilogues
// of their own and expand nothing from here.
#pragma once

#define LF_EPI_GROUPS 1      /* 4-wave groups per workgroup; the 512-thread split kernel redefines it */
#define LF_EPI_ONE_TILE false  /* tapgemm_kernel: true for the per-lane-row form of the three-tensor epilogue (one register short) */
#define LF_EPI_TID threadIdx.x  /* tapgemm_kernel: its per-tile laundered copy */
#define LF_EPI_ROW1 false      /* tapgemm_kernel: its ROW1 (a wave's 64 pixels in one image row) */
#define LF_EPI_PIVOT true      /* BN forward sums about a pivot (below); the run-time-flag forms of the 128-register split kernel and of the LDS-ring \
                                  kernels (cold paths: no network launch) have no registers for it and sum about 0 -- same row format */
#define LF_EPI_ACC(n, m) acc[n][m]   /* the finished sum of channel tile n, pixel tile m (tapstream_kernel: its one live pixel tile) */
#define LF_EPI_FIRST(m) ((m) == 0)   /* the pixel tile whose first pixel is the pivot of the BN forward sums */
#define LF_EPI_ROW_OK(tg) true       /* 4-wave group tg owns a tile of the launch (tapstream_kernel: the last pair of tiles may be half empty) */
/* the 256-pixel tile (= statistics row) of 4-wave group tg: the groups of a workgroup own consecutive tiles (tappair128_kernel: ONE
 * tile, its two groups produce the two 64-channel halves) */
#define LF_EPI_TILE_OF(tg) (bx * (unsigned)LF_EPI_GROUPS + (unsigned)(tg))
/* the lane's four elements of the residual / mask / BN operand at element offset o (tapbwd16_kernel: its LDS-staged tiles) */
#define LF_EPI_LDADD(o) epi_ld<S16>(r_add, o)
#define LF_EPI_LDMSK(o) epi_ld<S16>(r_msk, o)
#define LF_EPI_LDAUX(o) epi_ld<S16>(r_aux, o)
#define LF_EPI_HOIST_ALL false       /* tapbwd16_kernel: the MASKBN vectors held in registers beside the BN-backward sums too */
/* The epilogue in three parts, so that a kernel can run the per-pixel-tile part one tile at a time (stream_tile); LF_TAPGEMM_EPILOGUE
 * below is the three in a row, the form every other kernel expands. */
#define LF_EPI_HEAD \
    /* Pixel-tile outer, channel-tile inner: the loads of one operand tensor issued back to back cover one pixel's     \
     * contiguous channel run, so every cache line is touched once while it is hot (the channel-tile-outer order        \
     * revisited each line NT times with the whole grid's working set in between: 4x the HBM reads with bf16 tensors). \
     * The channel tiles of a pixel tile go in chunks of NC = 2 (one 128-byte line of fp32): with all NT tiles' operand \
     * loads in flight at once the three-tensor epilogues (ADD + MASK + BN-backward sums) needed 270+ registers and     \
     * spilled 13-29 of them to scratch.  NOBIAS: data-gradient epilogues (compiled-in flags) carry no bias vector. */  \
    const bool stats = (epi & (LF_EPI_STATS_SQ | LF_EPI_STATS_XHAT)) != 0; \
    constexpr bool NOBIAS = EPIC >= 0 && !(EPIC & LF_EPI_BIAS) && (EPIC & (LF_EPI_MASK | LF_EPI_ADD | LF_EPI_MASKBN | LF_EPI_STATS_XHAT)) != 0; \
    constexpr int NC = (NT % 2 == 0 && !LF_EPI_ONE_TILE) ? 2 : 1; \
    /* MASKBN + STATS_XHAT: the mask's two per-channel vectors are re-read (L1) instead of held -- 32 registers, the difference \
     * between two and three waves per SIMD for that variant */ \
    constexpr bool HOISTM = HOISTV && (LF_EPI_HOIST_ALL || !(EPIC >= 0 && (EPIC & LF_EPI_MASKBN) && (EPIC & LF_EPI_STATS_XHAT))); \
    const __amdgpu_buffer_rsrc_t r_dst = make_rsrc(a.dst, 0xffffffffu), r_add = make_rsrc(a.add_src, 0xffffffffu), \
                                 r_msk = make_rsrc(a.mask_src, 0xffffffffu), r_aux = make_rsrc(a.aux, 0xffffffffu), \
                                 r_bias = make_rsrc(a.bias, 0xffffffffu), r_msc = make_rsrc(a.msc, 0xffffffffu), \
                                 r_msh = make_rsrc(a.msh, 0xffffffffu), r_dm = make_rsrc(a.dm, 0xffffffffu); \
    /* BatchNorm FORWARD statistics (STATS_SQ) are accumulated about a PIVOT: per channel the value of the wave's first pixel   \
     * (lane 0 of the 16-lane row, broadcast by DPP): sum (v - piv), sum (v - piv)^2.  With |v - piv| ~ sigma neither sum loses the  \
     * digits that sum v^2 loses when |mean| >> sigma -- E[v^2] - mean^2 from fp32 partials kept 2^-24 (mean / sigma)^2 of the    \
     * variance: 2.3e-4 on a parameter gradient at 50 sigma, where nn.BatchNorm2d has no such term (round 6).  A wave turns its   \
     * sums into (sum v, M2 = sum (v - mean_wave)^2) of its 64 pixels, the workgroup's four waves are merged with Chan's formula    \
     * (differences of wave means, never squares of sums), and the partial row of a 256-pixel tile is [sum v][M2 about the tile's  \
     * own mean]; the finalise kernel merges the tiles in fp64 (LfStatPart::tile_pix). */ \
    f32x4 s1[NT], s2[NT], bs[NOBIAS ? 1 : NT], hv[HOISTV ? NT : 1][2], piv[LF_EPI_PIVOT ? NT : 1]; \
_Pragma("unroll") \
    for (int n = 0; n < NT; ++n) { \
        const int co = cob + n * 16 + kq * 4; \
        s1[n] = zero4(); s2[n] = zero4(); piv[LF_EPI_PIVOT ? n : 0] = zero4(); \
        if constexpr (!NOBIAS) bs[n] = a.bias ? ldb4(r_bias, co * 4u, 0u) : zero4(); \
        if (HOISTV) { \
            if (HOISTM && (epi & LF_EPI_MASKBN)) { hv[n][0] = ldb4(r_msc, co * 4u, 0u); hv[n][1] = ldb4(r_msh, co * 4u, 0u); } \
        } \
    }
/* one 16-pixel tile m: operand loads, bias / residual / masks / ReLU, the stores and the per-lane statistics */
#define LF_EPI_TILE(m) \
    { \
        const unsigned dbase = (unsigned)(((pn[m] * g.Hd + pi[m] * g.dsh + g.dah) * g.Wd + pj[m] * g.dsw + g.daw) * g.d_pix + g.d_choff + cob + kq * 4); \
_Pragma("unroll") \
        for (int n0 = 0; n0 < NT; n0 += NC) { \
        f32x4 la[NC], lm[NC], lx[NC], ld[NC]; \
_Pragma("unroll") \
        for (int j = 0; j < NC; ++j) { \
            const int n = n0 + j; \
            if (epi & LF_EPI_ADD) la[j] = LF_EPI_LDADD(dbase + n * 16); \
            if (epi & LF_EPI_MASK) lm[j] = LF_EPI_LDMSK(dbase + n * 16); \
            if (epi & (LF_EPI_MASKBN | LF_EPI_STATS_XHAT)) lx[j] = LF_EPI_LDAUX(dbase + n * 16); \
            if ((epi & LF_EPI_STATS_XHAT) && a.dm && !LF_EPI_ROW1) ld[j] = ldb4(r_dm, (unsigned)(pn[m] * g.Cd + cob + n * 16 + kq * 4) * 4u, 0u); \
        } \
_Pragma("unroll") \
        for (int j = 0; j < NC; ++j) { \
            const int n = n0 + j; \
            f32x4 v = LF_EPI_ACC(n, m); \
            if constexpr (!NOBIAS) v += bs[n]; \
            if (epi & LF_EPI_ADD) v += la[j]; \
            if (epi & LF_EPI_MASK) v = keep_pos(v, lm[j]); \
            const int co = cob + n * 16 + kq * 4;   /* per-channel vectors: L1-resident, re-read instead of held in registers */ \
            if (epi & LF_EPI_MASKBN) v = keep_pos(v, lx[j] * (HOISTM ? hv[HOISTV ? n : 0][0] : ldb4(r_msc, co * 4u, 0u)) + (HOISTM ? hv[HOISTV ? n : 0][1] : ldb4(r_msh, co * 4u, 0u))); \
            if (epi & LF_EPI_RELU) v = S16 ? relu_keep_nan(v) : max0(v); \
            if (S16) v = round_bf16(v);   /* statistics are taken from the values as stored */ \
            if (pv[m]) epi_st<S16>(r_dst, dbase + n * 16, v); \
            if (!pv[m]) v = zero4(); \
            if (epi & LF_EPI_STATS_SQ) { \
                if (LF_EPI_PIVOT && LF_EPI_FIRST(m)) piv[LF_EPI_PIVOT ? n : 0] = bcast16(v); \
                f32x4 dv = LF_EPI_PIVOT ? v - piv[LF_EPI_PIVOT ? n : 0] : v; \
                if (!pv[m]) dv = zero4(); \
                s1[n] += dv; s2[n] += dv * dv; \
            } \
            if (epi & LF_EPI_STATS_XHAT) { \
                const f32x4 gm = (a.dm && !LF_EPI_ROW1) ? v * ld[j] : v; \
                s1[n] += gm; s2[n] += gm * lx[j];      /* RAW second sum: the finalise kernel applies x^ = t * rstd - mean * rstd in fp64 */ \
            } \
        } \
        } \
    }
/* once per 256-pixel tile: the wave's sums -> one partial row (DPP row sums, LDS staging, Chan merge of the four waves) */
#define LF_EPI_TAIL \
    if (LF_EPI_ROW1 && (epi & LF_EPI_STATS_XHAT) && a.dm) { \
        /* a wave's pixels lie in ONE image: the Dropout2d factor of (image, channel) scales the wave's sums once */ \
_Pragma("unroll") \
        for (int n = 0; n < NT; ++n) { \
            const f32x4 dmv = ldb4(r_dm, (unsigned)(pn[0] * g.Cd + cob + n * 16 + kq * 4) * 4u, 0u); \
            s1[n] *= dmv; s2[n] *= dmv; \
        } \
    } \
    if (stats) { \
        /* one partial row per 256-pixel tile: 4-wave group EG of the workgroup (EG = 0 in the 256-thread kernels) */ \
        const int EW = wave & 3, EG = wave >> 2; \
        __shared__ float sred[LF_EPI_GROUPS][WG_WAVES][NT][4][8]; \
_Pragma("unroll") \
        for (int n = 0; n < NT; ++n) { \
            f32x4 r1, r2; \
            r1.x = sum16(s1[n].x); r1.y = sum16(s1[n].y); r1.z = sum16(s1[n].z); r1.w = sum16(s1[n].w); \
            r2.x = sum16(s2[n].x); r2.y = sum16(s2[n].y); r2.z = sum16(s2[n].z); r2.w = sum16(s2[n].w); \
            if (epi & LF_EPI_STATS_SQ) {      /* pivot sums -> (sum v, M2 about the wave's own mean) of the wave's nw valid pixels */ \
                const unsigned lf_t0 = (LF_EPI_TILE_OF(EG) * (unsigned)WG_WAVES + (unsigned)EW) * 64u; \
                const float nw = lf_t0 < npix ? (float)min(npix - lf_t0, 64u) : 0.f; \
                const float rn = nw > 0.f ? 1.f / nw : 0.f; \
                r2 = r2 - r1 * r1 * rn; \
                r2.x = fmaxf(r2.x, 0.f); r2.y = fmaxf(r2.y, 0.f); r2.z = fmaxf(r2.z, 0.f); r2.w = fmaxf(r2.w, 0.f); \
                if (LF_EPI_PIVOT) r1 = r1 + piv[LF_EPI_PIVOT ? n : 0] * nw; \
            } \
            if (pl == 0) { \
                float* d = sred[EG][EW][n][kq]; \
                d[0] = r1.x; d[1] = r1.y; d[2] = r1.z; d[3] = r1.w; d[4] = r2.x; d[5] = r2.y; d[6] = r2.z; d[7] = r2.w; \
            } \
        } \
        __syncthreads(); \
        if ((LF_EPI_TID & 255) < NT * 4 * 8 && LF_EPI_ROW_OK(LF_EPI_TID >> 8)) { \
            const int tg = LF_EPI_TID >> 8, tt = LF_EPI_TID & 255; \
            const int j = tt & 7, q = (tt >> 3) & 3, n = tt >> 5; \
            float v = sred[tg][0][n][q][j] + sred[tg][1][n][q][j] + sred[tg][2][n][q][j] + sred[tg][3][n][q][j]; \
            if ((epi & LF_EPI_STATS_SQ) && j >= 4) {      /* Chan: M2 = sum_w M2_w + sum_w n_w (mean_w - mean)^2 */ \
                const unsigned lf_tb = LF_EPI_TILE_OF(tg) * (unsigned)(WG_WAVES * 64); \
                float nwv[4], sw[4], nt = 0.f, st = 0.f; \
_Pragma("unroll") \
                for (int w = 0; w < 4; ++w) { \
                    const unsigned t0w = lf_tb + (unsigned)w * 64u; \
                    nwv[w] = t0w < npix ? (float)min(npix - t0w, 64u) : 0.f; \
                    sw[w] = sred[tg][w][n][q][j - 4]; \
                    nt += nwv[w]; st += sw[w]; \
                } \
                const float mg = nt > 0.f ? st / nt : 0.f; \
_Pragma("unroll") \
                for (int w = 0; w < 4; ++w) \
                    if (nwv[w] > 0.f) { const float dmw = sw[w] / nwv[w] - mg; v += nwv[w] * dmw * dmw; } \
            } \
            const int co = cob + n * 16 + q * 4 + (j & 3); \
            a.stats[((long)(j >> 2) * g.Cd + co) * a.stats_ld + (long)LF_EPI_TILE_OF(tg)] = v;      /* channel-major rows */ \
        } \
    }
#define LF_TAPGEMM_EPILOGUE \
    __builtin_amdgcn_s_setprio(3);   /* ahead of the partner wave's MFMA stream: the sooner this wave retires, the sooner its slot refills */ \
    LF_EPI_HEAD \
_Pragma("unroll") \
    for (int m = 0; m < MT; ++m) LF_EPI_TILE(m) \
    LF_EPI_TAIL
