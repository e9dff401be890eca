// Tap-GEMM convolution kernels for gfx950 on bf16 tensors (precision mode "bf16": bf16 elements in HBM, bf16 MFMA 16x16x32, fp32
// accumulate), and their router.  See lf_conv.h for the contract and lf_conv.hip for the fp32 kernels and lf_tapgemm_launch, which
// calls lf_tapgemm_bf16_route (at the end of this file) for every launch with packed bf16 weights.
//
// Kernels in this file:
//   tapgemm_bf16_kernel       operands streamed into registers (operand prologue, ragged widths)
//   tapgemm_bf16_ring_kernel  every tap table but the 3-tap convolutions': persistent LDS-DMA ring
//   tapgemm_bf16_wl_kernel    the 3-tap convolutions at 64 / 128 channels: memory touched in whole 128-byte lines
//                             (LDS-DMA operand ring, weights in registers, LDS-transposed stores)
//   tapgemm_bf16_wv_kernel    the 3-tap convolutions at 64 channels: a wave owns its pixels and all 64 output channels
//   tapgemm_bf16_lean_kernel  16 -> 16 channels (two taps per K = 32 MFMA)
//   tapgemm_bf16_thin_kernel  one 16-pixel tile per wave, for launches that cannot fill the device: one frame (the frozen detector)
// The streaming, ring and lean kernels expand the epilogue they share with the fp32 kernels (LF_TAPGEMM_EPILOGUE, lf_conv_epi.h), the
// thin kernel its three parts (one pixel tile);
// the whole-line and wave-private kernels have their own (same arithmetic, output and operand tensors through LDS tiles).
// The device and launch helpers shared with lf_conv.hip and lf_wgrad.hip are in lf_conv_dev.h, the LDS-DMA helpers in lf_ldsdma.h.
#include "lf_conv_dev.h"
#include "lf_conv_epi.h"

namespace {

// ---------------------------------------------------------------------------------------
// bf16 matrix-core kernel, operands streamed into registers (precision mode "bf16": bf16 tensors in HBM, fp32 accumulate; the
// launches the LDS kernels below do not take: operand prologue, ragged widths, tap tables with few pixels).
// v_mfma_f32_16x16x32_bf16: a lane supplies 8 consecutive k of its row / column (k-block kq = l>>4 of the 32-channel step), C/D
// layout as the fp32 form -- so the tap table, the pixel mapping and the whole epilogue are shared with tapgemm_kernel.  Per
// 32-channel step a lane loads ONE dwordx4 of its pixel (8 bf16 channels: the operand as it is), or, with the BN+ReLU prologue,
// widens it, applies the prologue and the validity mask in fp32 and converts back with v_cvt_pk_bf16_f32 (round to nearest even);
// 16 MFMAs (one per 16x16 tile) per step.  Weights are pre-packed bf16 [tap][ceil(Cs/32)*4][Cd][8], zero-padded to whole
// 32-channel steps, so the partial last step of a 16- or 48-channel contraction multiplies (valid, clamped) pixel data by zeros.
// At the bf16 rate (16 cycles per MFMA) the loop is bound by the operand path, not by the matrix cores.
// (Through round 5 the kernel also took fp32 tensors -- precision mode "bf16_mfma": removed, no BASELINE configuration used it.)
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ bf16x8 cvt_bf16x8(f32x4 lo, f32x4 hi) {
    bf16x8 r;
    r[0] = (__bf16)lo.x; r[1] = (__bf16)lo.y; r[2] = (__bf16)lo.z; r[3] = (__bf16)lo.w;
    r[4] = (__bf16)hi.x; r[5] = (__bf16)hi.y; r[6] = (__bf16)hi.z; r[7] = (__bf16)hi.w;
    return r;
}

// EPIC >= 0: epilogue flags compiled in (as in tapgemm_kernel).  FAST (no prologue, whole 32-channel steps): a padding position
// holds the out-of-range offset and reads as zero bits, the channel step is a scalar offset -- no per-step VALU work at all on
// bf16 tensors, where the 16 MFMAs of a step take 256 cycles and every VALU instruction beside them ~13.
template <int NT, int PROC, int EPIC = -1, bool FAST = false>
__global__ __launch_bounds__(256, 2) void tapgemm_bf16_kernel(const LfTapGeom g, const LfTapArgs a, const int pro, const int epi_rt) {
    static_assert(!FAST || PROC == 0, "FAST: the out-of-range zero must be the operand itself");
    const int epi = EPIC >= 0 ? EPIC : epi_rt;
    constexpr bool HOISTV = true, S16 = true;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int pl = lane & 15, kq = lane >> 4;
    const unsigned npix = (unsigned)(g.N * g.Hl * g.Wl);
    const int cob = blockIdx.y * NT * 16;
    const unsigned bx = xcd_swizzle(blockIdx.x);
    const unsigned tile0 = (bx * WG_WAVES + wave) * (MT * 16);

    int pn[MT], pi[MT], pj[MT];
    bool pv[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        const unsigned p = tile0 + m * 16 + pl;
        pv[m] = p < npix;
        const unsigned q = pv[m] ? p : 0u;
        const unsigned r = q / (unsigned)g.Wl;
        pj[m] = (int)(q - r * (unsigned)g.Wl);
        pn[m] = (int)(r / (unsigned)g.Hl);
        pi[m] = (int)(r - (unsigned)pn[m] * (unsigned)g.Hl);
    }
    f32x4 acc[NT][MT];
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int m = 0; m < MT; ++m) acc[n][m] = zero4();

    // one dwordx4 per tile is the whole 8-channel operand (xl holds raw bf16 bits)
    struct Step { u32x4 w[NT]; f32x4 xl[MT]; f32x4 sc0, sc1, sh0, sh1; unsigned ok; };
    __shared__ uint4 tab_off[WG_WAVES][LF_MAX_TAPS][64];
    __shared__ unsigned tab_ok[WG_WAVES][LF_MAX_TAPS][64];
    const int ncb = (g.Cs + 31) >> 5;                       // 32-channel steps per tap
    const int nsteps = g.ntaps * ncb;
    // FAST with a partial last step (16 or 48 source channels): the table has one row per (tap, step) instead of one per tap -- the
    // launcher admits nsteps <= LF_MAX_TAPS -- and a lane whose 8 channels lie at or beyond Cs holds the out-of-range offset: it
    // reads the buffer bound's zeros, not the memory behind the pixel's channels (the next pixel, another tensor's slice: their
    // Inf / NaN against the zero-padded weights would be NaN in every output channel).  Whole steps: one row per tap, as before.
    const bool part = FAST && (g.Cs & 31) != 0;
    const int nrows = part ? nsteps : g.ntaps;
    for (int r = 0; r < nrows; ++r) {
        const int t = part ? r / ncb : r, c0 = (part ? r - t * ncb : 0) * 32 + kq * 8;
        const int dh = g.tdh[t], dw = g.tdw[t];
        unsigned o[MT], okb = 0;
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const int sy = pi[m] * g.ssh + dh, sx = pj[m] * g.ssw + dw;
            const bool in = pv[m] && sy >= 0 && sy < g.Hs && sx >= 0 && sx < g.Ws;
            const int syc = min(max(sy, 0), g.Hs - 1), sxc = min(max(sx, 0), g.Ws - 1);
            o[m] = (unsigned)(((pn[m] * g.Hs + syc) * g.Ws + sxc) * g.s_pix + g.s_choff);
            if constexpr (FAST) o[m] = (in && c0 < g.Cs) ? (o[m] + c0) * 2u : LF_OOB;      // bytes, this lane's 8 channels
            okb |= (in ? 1u : 0u) << m;
        }
        tab_off[wave][r][lane] = make_uint4(o[0], o[1], o[2], o[3]);
        tab_ok[wave][r][lane] = okb;
    }
    const __amdgpu_buffer_rsrc_t rw = make_rsrc(a.wp16, 0xffffffffu),
                                 rx = make_rsrc(a.src, FAST ? (unsigned)min((long)g.N * g.Hs * g.Ws * g.s_pix * 2, (long)LF_OOB) : 0xffffffffu),
                                 rsc = make_rsrc(a.pro_sc, 0xffffffffu), rsh = make_rsrc(a.pro_sh, 0xffffffffu);
    const unsigned wlane = (unsigned)(kq * g.Cd + cob + pl) * 16u;      // bytes (8 bf16 per lane and tile)
    const int wstep = g.Cd * 32;                            // bf16 elements per 32-channel step
    const int ntaps = g.ntaps;
    const int wlast = (nsteps - 1) * wstep;
    int t_ld = 0, cb_ld = 0, wofs = 0;
    auto issue = [&](Step& S) {
        const bool live = t_ld < ntaps;
        const int tc = live ? (part ? t_ld * ncb + cb_ld : t_ld) : nrows - 1;      // (scalar) a table ROW: per (tap, step) if part, else per tap; a dead step takes the last one
        const uint4 o = tab_off[wave][tc][lane];
        const unsigned okb = tab_ok[wave][tc][lane];
#pragma unroll
        for (int n = 0; n < NT; ++n) S.w[n] = __builtin_bit_cast(u32x4, ldb4(rw, wlane + n * 256, (unsigned)wofs * 2u));
        const int c8 = min(cb_ld * 32 + kq * 8, g.Cs - 8);  // a partial last step re-reads valid channels (weights are 0)
        if constexpr (FAST) {
            const unsigned dead = live ? 0u : LF_OOB;        // a dead step (odd step count) reads zeros
            const unsigned cs = part ? 0u : (unsigned)cb_ld * 64u;      // (a per-step row holds its channel offset)
            S.xl[0] = ldb4(rx, o.x | dead, cs); S.xl[1] = ldb4(rx, o.y | dead, cs);
            S.xl[2] = ldb4(rx, o.z | dead, cs); S.xl[3] = ldb4(rx, o.w | dead, cs);
        } else {                                             // buffer-addressed (see ldb4): bf16 elements, 16 bytes = 8 channels
            S.xl[0] = ldb4(rx, (o.x + c8) * 2u, 0u);
            S.xl[1] = ldb4(rx, (o.y + c8) * 2u, 0u);
            S.xl[2] = ldb4(rx, (o.z + c8) * 2u, 0u);
            S.xl[3] = ldb4(rx, (o.w + c8) * 2u, 0u);
        }
        if constexpr (PROC == LF_PRO_BNRELU) {
            S.sc0 = ldb4(rsc, c8 * 4u, 0u); S.sc1 = ldb4(rsc, c8 * 4u + 16u, 0u);
            S.sh0 = ldb4(rsh, c8 * 4u, 0u); S.sh1 = ldb4(rsh, c8 * 4u + 16u, 0u);
        }
        S.ok = live ? okb : 0u;
        const int cbn = cb_ld + 1;
        const bool wrap = cbn == ncb;
        wofs = min(wofs + wstep, wlast);                    // a dead step re-reads the last live weights
        cb_ld = live ? (wrap ? 0 : cbn) : cb_ld;
        t_ld = (live && wrap) ? t_ld + 1 : t_ld;
    };
    auto mma = [&](const Step& S) {
        bf16x8 xb[MT];
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const bool in = FAST || ((S.ok >> m) & 1u);
            if constexpr (PROC != LF_PRO_BNRELU) {       // raw bf16 bits: mask and use as they are
                u32x4 r = __builtin_bit_cast(u32x4, S.xl[m]);
                r.x = in ? r.x : 0u; r.y = in ? r.y : 0u; r.z = in ? r.z : 0u; r.w = in ? r.w : 0u;
                xb[m] = __builtin_bit_cast(bf16x8, r);
                continue;
            }
            f32x4 lo, hi;
            {
                const u32x4 r = __builtin_bit_cast(u32x4, S.xl[m]);
                lo.x = __uint_as_float(r.x << 16); lo.y = __uint_as_float(r.x & 0xffff0000u);
                lo.z = __uint_as_float(r.y << 16); lo.w = __uint_as_float(r.y & 0xffff0000u);
                hi.x = __uint_as_float(r.z << 16); hi.y = __uint_as_float(r.z & 0xffff0000u);
                hi.z = __uint_as_float(r.w << 16); hi.w = __uint_as_float(r.w & 0xffff0000u);
            }
            if constexpr (PROC == LF_PRO_BNRELU) { lo = max0(lo * S.sc0 + S.sh0); hi = max0(hi * S.sc1 + S.sh1); }
            lo.x = in ? lo.x : 0.f; lo.y = in ? lo.y : 0.f; lo.z = in ? lo.z : 0.f; lo.w = in ? lo.w : 0.f;
            hi.x = in ? hi.x : 0.f; hi.y = in ? hi.y : 0.f; hi.z = in ? hi.z : 0.f; hi.w = in ? hi.w : 0.f;
            xb[m] = cvt_bf16x8(lo, hi);
        }
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            const bf16x8 wb = __builtin_bit_cast(bf16x8, S.w[n]);
#pragma unroll
            for (int m = 0; m < MT; ++m)
                acc[n][m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wb, xb[m], acc[n][m], 0, 0, 0);
        }
    };
    static_assert(MT == 4, "tab_off packs 4 pixel tiles");
    Step A, B;
    issue(A);
    const int npairs = (nsteps + 1) >> 1;
    for (int pr = 0; pr < npairs; ++pr) {
        issue(B);
        mma(A);
        issue(A);
        mma(B);
    }
#undef LF_EPI_PIVOT
#define LF_EPI_PIVOT (EPIC >= 0 || NT < 4)      /* (the 64-channel-slab run-time-flag forms have no registers for the pivot: 282-810 spilled) */
    LF_TAPGEMM_EPILOGUE
#undef LF_EPI_PIVOT
#define LF_EPI_PIVOT true
}

// ---------------------------------------------------------------------------------------
// bf16 tensors through LDS (round 4): the launches of precision mode "bf16" without an operand prologue.  Two kernels,
// tapgemm_bf16_ring_kernel (any tap table; 32-channel K-steps) and tapgemm_bf16_wl_kernel (the 3-tap convolutions, whole
// 128-byte lines), share the machinery below: operands travel by `buffer_load_dwordx4 ... lds` (LDS-DMA: no register is held
// while the load is in flight) into a ring of LDS stages; the ring is ordered by hand --
//     s_waitcnt vmcnt(N) lgkmcnt(0)   my DMA of this step has landed (N instructions of younger steps may be in flight) and my
//                                     fragment reads of the step before have retired
//     s_barrier                       ... everyone's
//     issue the step that is R - 1 ahead into the stage the previous step occupied; read fragments; MFMAs
// -- with the bare s_barrier, because __syncthreads() carries a release fence that drains vmcnt to 0, i.e. the whole ring, every
// step.  The lgkmcnt(0) is not optional: hipcc moves a step's last MFMAs, and the waits for their operands, behind the next
// barrier, and a DMA instruction whose pixels are all padding returns its zeros without a memory round trip and overtakes those
// reads (wrong tiles in one launch of three at dilation 8 and row width 80 before the wait was there).
// ---------------------------------------------------------------------------------------
constexpr int LB_STAGES = 3;
constexpr int LB_X_BYTES = WG_WAVES * 64 * 64;          // 16 KB
constexpr int LB_W_BYTES = 4 * 64 * 16;                 // 4 KB
constexpr int LB_STAGE_BYTES = LB_X_BYTES + LB_W_BYTES;

// (lds_dma16, make_rsrc_words, wait_vm_lgkm0: lf_ldsdma.h)

// ---------------------------------------------------------------------------------------
// tapgemm_bf16_ring_kernel: LDS-staged bf16 tap-GEMM for ANY tap table (the 9-tap stride-2 convolution, the transposed-convolution
// phases, their gradients; the 3-tap convolutions go to tapgemm_bf16_wl_kernel), 64-output-channel slabs, 32-channel K-steps.
//
// Stage (20 KB) = X [wave 4][pixel 64][slot 4][16 B] + W [k-block 4][cout 64][16 B], 3 stages: two workgroups per CU.
//  * X: DMA instruction m of wave w carries pixels w*64 + m*16 + (lane >> 2), 16 bytes (8 channels) per lane, lane-linear in LDS
//    (that is what LDS-DMA does); a pixel's four 16-byte slots are XOR-swizzled by (pixel >> 2) & 3 -- applied to the SOURCE channel
//    block of the lane -- so that the fragment read of 8 consecutive lanes touches 8 different bank groups.  A padding tap
//    position carries the out-of-range offset: the DMA writes zeros.
//  * W: the packed bf16 weights [tap][k-block][Cd][8] make a (tap, 32-channel) step's 64-channel slab four 1 KB runs: one DMA
//    instruction per wave, fragment reads contiguous.
//  * PERSISTENT: a workgroup walks its work items (pixel tile x output-channel slab) and its load cursor runs two K-steps ahead
//    of the compute cursor ACROSS item boundaries: the first operands of the next item land while this item's epilogue stores
//    (the one-tile form of this kernel spent 2.7 of its 13 us building a per-lane tap table and 2.8 in the epilogue with the
//    memory pipe idle: profiles/r4_bf16_phases_one_tile.txt).
//  * No tap table: the launcher admits geometries whose 16-pixel groups lie in one image row (Wl % 16 == 0), so a DMA
//    instruction's 16 pixels share (image, row) -- wave-uniform, scalar registers: ONE division pair per wave and item -- and a
//    lane's byte offset is a scalar base plus a per-lane constant, with the column test (one unsigned compare) selecting the
//    out-of-range offset for padding.
// K order = tapgemm_bf16_kernel's: results bit-identical (tools/bf16_ab.py).  (A form owning all 128 output channels per
// workgroup -- X through the ring once per tap -- and the one-tile form are in DESIGN.md section 9.)
// ---------------------------------------------------------------------------------------
struct RingGroups { int n[4], i[4], j[4]; bool ok[4]; };
// the four consecutive 16-pixel groups from group index G0 on: (image, row, first column), all wave-uniform
__device__ __forceinline__ void groups_at(unsigned G0, int Hl, unsigned GR, unsigned ngroups, RingGroups& o) {
    const unsigned Gc = G0 < ngroups ? G0 : 0u;
    const unsigned R = Gc / GR;
    int jg = __builtin_amdgcn_readfirstlane((int)(Gc - R * GR));
    int n = __builtin_amdgcn_readfirstlane((int)(R / (unsigned)Hl));
    int i = __builtin_amdgcn_readfirstlane((int)R) - n * Hl;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        o.ok[m] = G0 + m < ngroups;
        // a group past the last pixel takes the position of group 0 (tapgemm_bf16_kernel's `q = pv ? p : 0`): nothing of it is stored or
        // summed, but the epilogues still LOAD its operand tensors -- past the tensor's end otherwise, and 0 * (a NaN found there) is a
        // NaN in the BN-backward sum of the tile (tests/test_convchain_shapes_gpu.py: 800 pixels, three and an eighth tiles)
        o.n[m] = o.ok[m] ? n : 0; o.i[m] = o.ok[m] ? i : 0; o.j[m] = o.ok[m] ? jg * 16 : 0;
        if (++jg == (int)GR) { jg = 0; if (++i == Hl) { i = 0; ++n; } }
    }
}
// ... of wave `wave` of the 256-pixel tile `tile`
__device__ __forceinline__ void ring_groups(unsigned tile, int wave, int Hl, unsigned GR, unsigned ngroups, RingGroups& o) {
    groups_at((tile * WG_WAVES + (unsigned)wave) * 4u, Hl, GR, ngroups, o);
}

// DBG: per-wave stamps, 16 x uint64 per wave: start, hardware id, then (K loop done, epilogue stores retired) per item, 7 items
template <int EPIC, bool DBG = false>
__global__ __launch_bounds__(256, 2) void tapgemm_bf16_ring_kernel(const LfTapGeom g, const LfTapArgs a, const int pro, const int epi_rt) {
    constexpr bool S16 = true, HOISTV = true;
    unsigned long long* dbgp = nullptr;
    int dbgk = 0;
    if constexpr (DBG) {
        dbgp = a.dbg + ((unsigned long long)blockIdx.x * WG_WAVES + (threadIdx.x >> 6)) * 16;
        if ((threadIdx.x & 63) == 0) {
            unsigned hwid, xcc;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
            dbgp[0] = __builtin_amdgcn_s_memrealtime();
            dbgp[1] = (unsigned long long)hwid | ((unsigned long long)xcc << 32);
        }
    }
    constexpr int STAGE = LB_STAGE_BYTES;
    const int epi = EPIC >= 0 ? EPIC : epi_rt;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int pl = lane & 15, kq = lane >> 4;
    const unsigned npix = (unsigned)(g.N * g.Hl * g.Wl), ngroups = npix >> 4, GR = (unsigned)g.Wl >> 4;
    const unsigned ntiles = (npix + PIX_PER_WG - 1) / PIX_PER_WG;
    const int slsh = g.Cd > 64 ? 1 : 0;                           // output-channel slabs per pixel tile: 1 or 2
    const unsigned nitems = ntiles << slsh;
    // work items first, first + stride, ... inside this XCD's contiguous range (see tapgemm_kernel)
    unsigned it_first = blockIdx.x, it_stride = gridDim.x, it_end = nitems;
    if ((gridDim.x & 7u) == 0 && (nitems & 7u) == 0) {
        const unsigned per = nitems >> 3;
        it_first = (blockIdx.x & 7u) * per + (blockIdx.x >> 3); it_stride = gridDim.x >> 3; it_end = (blockIdx.x & 7u) * per + per;
    }
    // tap offsets: tap t in lane t (read back with v_readlane: no dependent scalar loads in the issue path)
    int tapv = 0;
#pragma unroll
    for (int t = 0; t < LF_MAX_TAPS; ++t)
        if (lane == t) tapv = (g.tdh[t] & 0xffff) | (g.tdw[t] << 16);

    const int ncb = g.Cs >> 5;
    const int nsteps = g.ntaps * ncb;
    const i32x4s rx = make_rsrc_words(a.src, (unsigned)min((long)g.N * g.Hs * g.Ws * g.s_pix * 2, (long)LF_OOB)),
                 rw = make_rsrc_words(a.wp16, 0xffffffffu);
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)lf_tap_lds;
    unsigned char* const stages = lf_tap_lds;
    const int wstep = g.Cd * 64;                               // bytes per 32-channel step (4 k-blocks x Cd x 16)
    const int spix2 = g.s_pix * 2;
    // per-lane constants of the DMA mapping: instruction m, this lane -> pixel (group m) + (lane >> 2), channel block
    // (lane & 3) ^ ((lane >> 4) & 3) of the 32-channel step
    const int dq = lane >> 2, dkq = (lane & 3) ^ ((lane >> 4) & 3);
    const unsigned lane_x = (unsigned)((dq * g.ssw * g.s_pix + g.s_choff + dkq * 8) * 2);
    const int lane_dx = dq * g.ssw;
    const unsigned lane_w = (unsigned)((wave * g.Cd + lane) * 16);

    // ---- load cursor (wave-uniform): item, tap, channel block, ring stage; the item's four groups as (pixel index of the
    // row position without the tap, row, column) and a validity mask
    unsigned it_ld = it_first;
    int t_ld = 0, cb_ld = 0, st_ld = 0, wofs = 0, cob_ld = 0;
    int lrow[4], liy[4], lsx[4];
    unsigned lok = 0;
    auto cursor_item = [&]() {
        lok = 0;
        if (it_ld < it_end) {
            RingGroups G;
            ring_groups(it_ld >> slsh, wave, g.Hl, GR, ngroups, G);
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                liy[m] = G.i[m] * g.ssh; lsx[m] = G.j[m] * g.ssw;
                lrow[m] = (G.n[m] * g.Hs + liy[m]) * g.Ws + lsx[m];
                lok |= G.ok[m] ? 1u << m : 0u;
            }
            cob_ld = (int)(it_ld & (unsigned)slsh) * 64;
        } else {
#pragma unroll
            for (int m = 0; m < 4; ++m) { liy[m] = 0; lsx[m] = 0; lrow[m] = 0; }
        }
    };
    cursor_item();
    auto issue = [&]() {                                     // DMA of the cursor's step into stage st_ld
        const unsigned st = lds0 + (unsigned)(st_ld * STAGE);
        const int tv = __builtin_amdgcn_readlane(tapv, t_ld);
        const int dh = (int)(short)(tv & 0xffff), dw = tv >> 16;
        const int tapoff = dh * g.Ws + dw;
        const unsigned xs = st + (unsigned)wave * 4096u;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int sy = liy[m] + dh;
            const bool yok = ((lok >> m) & 1u) && sy >= 0 && sy < g.Hs;
            const unsigned base = (unsigned)((lrow[m] + tapoff) * spix2 + cb_ld * 64);
            const bool in = yok && (unsigned)(lsx[m] + dw + lane_dx) < (unsigned)g.Ws;
            lds_dma16(rx, xs + (unsigned)m * 1024u, in ? base + lane_x : LF_OOB, 0u);
        }
        lds_dma16(rw, st + (unsigned)(LB_X_BYTES + wave * 1024), lane_w + (unsigned)(cob_ld * 16), (unsigned)wofs);
        // advance; past the last item the X part writes zeros (out-of-range offsets) into a stage nobody reads
        st_ld = st_ld == LB_STAGES - 1 ? 0 : st_ld + 1;
        wofs += wstep;
        if (++cb_ld == ncb) {
            cb_ld = 0;
            if (++t_ld == g.ntaps) { t_ld = 0; wofs = 0; it_ld += it_stride; cursor_item(); }
        }
    };
    issue();
    issue();
    // fragment addresses (bytes inside a stage)
    const unsigned xfrag = (unsigned)(wave * 4096 + pl * 64 + ((kq ^ (pl >> 2)) & 3) * 16);       // + m * 1024
    const unsigned wfrag = (unsigned)(LB_X_BYTES + (kq * 64 + pl) * 16);                           // + n * 256
    int st_c = 0;
    for (unsigned it = it_first; it < it_end; it += it_stride) {
        constexpr int NT = 4;
        f32x4 acc[NT][MT];
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int m = 0; m < MT; ++m) acc[n][m] = zero4();
        for (int s = 0; s < nsteps; ++s) {
            // my DMA of this step has landed (the instructions of the next step may still be in flight) ...
            asm volatile("s_waitcnt vmcnt(5) lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();        // ... and everyone's; everyone is past the fragment reads of the step before
            asm volatile("" ::: "memory");
            issue();                             // two steps ahead -> the stage the previous step occupied
            const unsigned char* st = stages + st_c * STAGE;
            st_c = st_c == LB_STAGES - 1 ? 0 : st_c + 1;
            bf16x8 xb[MT];
#pragma unroll
            for (int m = 0; m < MT; ++m) xb[m] = *reinterpret_cast<const bf16x8*>(st + xfrag + m * 1024);
            bf16x8 wb[NT];
#pragma unroll
            for (int n = 0; n < NT; ++n) wb[n] = *reinterpret_cast<const bf16x8*>(st + wfrag + n * 256);
#pragma unroll
            for (int n = 0; n < NT; ++n)
#pragma unroll
                for (int m = 0; m < MT; ++m)
                    acc[n][m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wb[n], xb[m], acc[n][m], 0, 0, 0);
        }
        if constexpr (DBG) {
            asm volatile("" ::"v"(acc[0][0][0]));
            if (lane == 0 && dbgk < 7) dbgp[2 + 2 * dbgk] = __builtin_amdgcn_s_memrealtime();
        }
        // ---- epilogue of this item (the accumulator layout of tapgemm_bf16_kernel: tile m = group m, pixel m*16 + pl)
        const unsigned bx = it >> slsh;
        int pn[MT], pi[MT], pj[MT];
        bool pv[MT];
        {
            RingGroups G;
            ring_groups(bx, wave, g.Hl, GR, ngroups, G);
#pragma unroll
            for (int m = 0; m < MT; ++m) { pn[m] = G.n[m]; pi[m] = G.i[m]; pj[m] = G.j[m] + pl; pv[m] = G.ok[m]; }
        }
        const int cob = (int)(it & (unsigned)slsh) * 64;
#undef LF_EPI_PIVOT
#define LF_EPI_PIVOT (EPIC >= 0)
        LF_TAPGEMM_EPILOGUE
#undef LF_EPI_PIVOT
#define LF_EPI_PIVOT true
        __builtin_amdgcn_s_setprio(0);
        if constexpr (DBG) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (lane == 0 && dbgk < 7) dbgp[3 + 2 * dbgk] = __builtin_amdgcn_s_memrealtime();
            ++dbgk;
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // the two trailing (dead) steps: nothing may land in LDS after this
    __builtin_amdgcn_s_barrier();
}

// ---------------------------------------------------------------------------------------
// tapgemm_bf16_wl_kernel ("whole lines"): the 3-tap bf16 convolutions of non_bottleneck_1d (Cs = Cd = 64 or 128, stride 1).
//
// tools/l2_stream.hip measures what bounds every bf16 kernel above (profiles/r4_l2_stream.txt): an instruction whose 64 lanes
// touch 16 cache lines moves 16 lines' worth of L1 time whatever it uses of them.  The MFMA operand layout -- a lane = 16 bytes of
// pixel l & 15 -- makes a register load take 64 bytes of each of 16 lines (3 taps of a 52 MB tensor: 26.9 us, 5.9 TB/s; the same
// bytes as whole lines: 12.5 us, 12.5 TB/s), and the accumulator layout makes the epilogue store 8 bytes per lane, 32 of each
// line (+17 us for 52 MB against +7 us as whole lines).  All of the above kernels sit at that ~44 us; this one touches memory
// in whole 128-byte lines only:
//  * X: LDS-DMA instructions of 8 pixels x 128 bytes (lane -> pixel l >> 3, 16-byte chunk l & 7) into a ring of K-steps of
//    64 pixels x 64 channels (8 KB); the waves read MFMA fragments from it (chunk XOR (pixel >> 1) & 7 on the SOURCE side
//    makes the ds_read_b128 lane groups conflict-free);
//  * output: the epilogue writes bf16 quads into an LDS tile (16-byte chunks XOR pixel), barrier, then every wave stores
//    1 KB instructions of 4 pixels x 256 bytes (8 x 128 at 64 channels);
//  * W: NOT in LDS and not in the ring -- the workgroup's 64 pixels are shared by its four waves, each owning a quarter of the
//    output channels (wave tile 64 pixels x Cd/4), so a wave's weights are 3 taps x Cs x Cd/4 = 24 KB at 128 channels: 96
//    REGISTERS per lane, loaded once per persistent workgroup, statically indexed by the fully unrolled K loop.  The LDS
//    is ring (4 to 8 stages of 8 KB, by variant) + output tile + the epilogue's operand tiles (WlCfg below) = at most 80 KB: two
//    workgroups per CU, each with its ring's depth - 1 K-steps in flight.
// Work item = 256 pixels (the BN-statistics row of the other kernels) as four 64-pixel sub-tiles; the ring runs across
// sub-tiles and items.  K order = tapgemm_bf16_kernel's (tap, then channel): results bit-identical.
// ---------------------------------------------------------------------------------------
constexpr int WL_STAGE = 64 * 128;
// Epilogue operand tensors (the data gradient's ReLU-mask source, residual gradient, BN-backward operand) come in whole lines too: by
// LDS-DMA into tiles of the output tile's layout, issued behind the first K-step of the sub-tile they belong to and read by the
// epilogue in the accumulator layout (8 bytes per lane from LDS instead of 32 of every 128-byte line from L2: +40 us per tensor and
// launch at 80 x 160 x 64 images before).  The residual lands IN the output tile (each lane overwrites what it read); the other
// two have their own tiles, which come out of the ring's depth: 2 x 80 KB per CU.
template <int CB, int EPIC, int PROC = 0> struct WlCfg {
    static constexpr int NT = CB / 2, KS = CB / 2, NSTEP = 3 * KS, CD = CB * 32, PIXB = CD * 2;
    static constexpr int OUT_BYTES = 64 * PIXB;
    static constexpr bool ST_ADD = EPIC >= 0 && (EPIC & LF_EPI_ADD) != 0, ST_MSK = EPIC >= 0 && (EPIC & LF_EPI_MASK) != 0,
                          ST_AUX = EPIC >= 0 && (EPIC & (LF_EPI_MASKBN | LF_EPI_STATS_XHAT)) != 0 &&
                                   !(CB == 4 && (EPIC & LF_EPI_MASKBN) != 0);          // (that variant has no registers left for it: 7 spilled)
    static constexpr int NBUF = (ST_MSK ? 1 : 0) + (ST_AUX ? 1 : 0);                  // tiles beside the output tile
    static constexpr int NI = OUT_BYTES / 1024 / WG_WAVES;                            // 1 KB instructions per wave and tile
    static constexpr int NAUXI = ((ST_ADD ? 1 : 0) + NBUF) * NI;                      // staging instructions per wave and sub-tile
    static constexpr int MAXST = CB == 4 ? 6 : 8;
    static constexpr int FIT = (80 * 1024 - OUT_BYTES * (1 + NBUF)) / WL_STAGE;
    static constexpr int STAGES = FIT < MAXST ? FIT : MAXST;
    static constexpr int TILES_END = STAGES * WL_STAGE + OUT_BYTES * (1 + NBUF);        // the prologue's scale / shift vectors live here
    static constexpr size_t LDS = (size_t)TILES_END + (PROC ? 2 * CD * 4 : 0);
    static_assert(STAGES >= 3, "ring too shallow");
};

// PROC = 1 (the block's third convolution: its operand is relu(bn1(t2)), never stored): behind its own vmcnt wait and in front of
// the step's barrier every wave transforms the 16 pixels x 64 channels IT brought in, in place in the stage (fp32 math on the
// widened values, tapgemm_bf16_kernel's expressions: results bit-identical), so the four waves that read the fragments do not
// each redo it; padding pixels (zeros from the DMA) are kept zero by the same column / row test that issued them.
template <int CB, int EPIC, int PROC = 0>
__global__ __launch_bounds__(256, 2) void tapgemm_bf16_wl_kernel(const LfTapGeom g, const LfTapArgs a, const int pro, const int epi_rt) {
    typedef WlCfg<CB, EPIC, PROC> C;
    constexpr int NT = C::NT, KS = C::KS, NSTEP = C::NSTEP, S = C::STAGES, CD = C::CD, PIXB = C::PIXB, NCH = PIXB / 16;
    constexpr bool S16 = true;
    const int epi = EPIC >= 0 ? EPIC : epi_rt;
    constexpr bool NOBIAS = EPIC >= 0 && !(EPIC & LF_EPI_BIAS) && (EPIC & (LF_EPI_MASK | LF_EPI_ADD | LF_EPI_MASKBN | LF_EPI_STATS_XHAT)) != 0;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int pl = lane & 15, kq = lane >> 4;
    const int cobw = wave * 16 * NT;                        // this wave's output channels
    const unsigned npix = (unsigned)(g.N * g.Hl * g.Wl), ngroups = npix >> 4, GR = (unsigned)g.Wl >> 4;
    const unsigned nitems = (npix + PIX_PER_WG - 1) / PIX_PER_WG;
    const XcdRange itr = xcd_range(nitems);
    const unsigned it_first = itr.first, it_stride = itr.stride, it_end = itr.end;
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)lf_tap_lds;
    unsigned char* const ring = lf_tap_lds;
    unsigned char* const otile = lf_tap_lds + S * WL_STAGE;
    unsigned char* const mtile = otile + C::OUT_BYTES;                                 // mask source (when staged)
    unsigned char* const xtile = otile + C::OUT_BYTES * (C::ST_MSK ? 2 : 1);          // BN-backward operand (when staged)

    // ---- this wave's weights -> registers: [tap][32-channel k-block][16-channel output tile], the MFMA A operand
    bf16x8 wr[3][CB][NT];
    {
        const __amdgpu_buffer_rsrc_t rw = make_rsrc(a.wp16, 0xffffffffu);
#pragma unroll
        for (int t = 0; t < 3; ++t)
#pragma unroll
            for (int kb = 0; kb < CB; ++kb)
#pragma unroll
                for (int n = 0; n < NT; ++n)
                    wr[t][kb][n] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(
                        rw, (int)((((t * CB + kb) * 4 + kq) * CD + cobw + n * 16 + pl) * 16), 0, 0));
    }
    // tap t's offsets in lane t, read back with v_readlane (a select chain over three values indexed by the run-time tap becomes an
    // indexed array in scratch memory -- and the kernel-argument struct with it)
    int tapv = 0;
#pragma unroll
    for (int t = 0; t < 3; ++t)
        if (lane == t) tapv = (g.tdh[t] & 0xffff) | (g.tdw[t] << 16);
    const i32x4s rx = make_rsrc_words(a.src, (unsigned)min((long)g.N * g.Hs * g.Ws * g.s_pix * 2, (long)LF_OOB));
    const int spix2 = g.s_pix * 2;
    // DMA mapping: this wave carries group `wave` of the sub-tile (pixels wave*16 ..+15) as two instructions jj of 8 pixels;
    // lane -> pixel jj*8 + (lane >> 3), LDS slot lane & 7 = chunk XOR ((pixel >> 1) & 7)
    const int dpx = lane >> 3;
    unsigned lane_x[2];
    int lane_dx[2];
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
        const int chunk = (lane & 7) ^ ((jj * 4 + (lane >> 4)) & 7);
        lane_x[jj] = (unsigned)(((jj * 8 + dpx) * g.s_pix + g.s_choff) * 2 + chunk * 16);
        lane_dx[jj] = jj * 8 + dpx;
    }
    // ---- load cursor (wave-uniform): item, sub-tile, step; this wave's group of the cursor's sub-tile
    unsigned it_ld = it_first;
    int sub_ld = 0, s_ld = 0, st_ld = 0;
    int lrow = 0, liy = 0, lsx = 0;
    bool lok = false;
    auto cursor_sub = [&]() __attribute__((always_inline)) {
        lok = false;
        if (it_ld < it_end) {
            const unsigned G = (it_ld * 4u + (unsigned)sub_ld) * 4u + (unsigned)wave;
            lok = G < ngroups;
            const unsigned Gc = lok ? G : 0u;
            const unsigned R = Gc / GR;
            const int jg = __builtin_amdgcn_readfirstlane((int)(Gc - R * GR));
            const int n = __builtin_amdgcn_readfirstlane((int)(R / (unsigned)g.Hl));
            const int i = __builtin_amdgcn_readfirstlane((int)R) - n * g.Hl;
            liy = i; lsx = jg * 16;
            lrow = (n * g.Hs + i) * g.Ws + lsx;
        }
    };
    cursor_sub();
    auto issue = [&]() __attribute__((always_inline)) {
        const int t = KS == 1 ? s_ld : s_ld >> 1, ks = KS == 1 ? 0 : s_ld & 1;
        const int tv = __builtin_amdgcn_readlane(tapv, t);
        const int dh = (int)(short)(tv & 0xffff), dw = tv >> 16;
        const int sy = liy + dh;
        const bool yok = lok && sy >= 0 && sy < g.Hs;
        const unsigned base = (unsigned)((lrow + dh * g.Ws + dw) * spix2 + ks * 128);
        const unsigned dst = lds0 + (unsigned)(st_ld * WL_STAGE + wave * 2048);
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            const bool in = yok && (unsigned)(lsx + dw + lane_dx[jj]) < (unsigned)g.Ws;
            lds_dma16(rx, dst + (unsigned)jj * 1024u, in ? base + lane_x[jj] : LF_OOB, 0u);
        }
        st_ld = st_ld == S - 1 ? 0 : st_ld + 1;
        if (++s_ld == NSTEP) {
            s_ld = 0;
            if (++sub_ld == 4) { sub_ld = 0; it_ld += it_stride; }
            cursor_sub();
        }
    };
#pragma unroll
    for (int i = 0; i < S - 1; ++i) issue();

    float* const ptab = reinterpret_cast<float*>(lf_tap_lds + C::TILES_END);           // [2][CD]: scale, shift
    if constexpr (PROC == LF_PRO_BNRELU) {
        for (int c = threadIdx.x; c < CD; c += 256) { ptab[c] = a.pro_sc[c]; ptab[CD + c] = a.pro_sh[c]; }
        __syncthreads();
    }
    // ---- staging of the epilogue's operand tensors: wave w carries group w of the sub-tile (NI instructions of 1 KB per tensor);
    // instruction ii = w * NI + k is bytes ii*1024 .. +1023 of the pixel-major tile: lane -> pixel p, 16-byte slot = chunk XOR p
    // (resources bounded by the tensor: the out-of-range offset of a group beyond it reads zeros)
    const unsigned dbytes = (unsigned)min((long)g.N * g.Hd * g.Wd * g.d_pix * 2, (long)LF_OOB);
    const i32x4s ra_add = make_rsrc_words(a.add_src, dbytes), ra_msk = make_rsrc_words(a.mask_src, dbytes), ra_aux = make_rsrc_words(a.aux, dbytes);
    auto stage_tensors = [&](const RingGroups& G) __attribute__((always_inline)) {
        if constexpr (C::NAUXI > 0) {
            const int gn = wave == 0 ? G.n[0] : wave == 1 ? G.n[1] : wave == 2 ? G.n[2] : G.n[3];
            const int gi = wave == 0 ? G.i[0] : wave == 1 ? G.i[1] : wave == 2 ? G.i[2] : G.i[3];
            const int gj = wave == 0 ? G.j[0] : wave == 1 ? G.j[1] : wave == 2 ? G.j[2] : G.j[3];
            const bool gok = wave == 0 ? G.ok[0] : wave == 1 ? G.ok[1] : wave == 2 ? G.ok[2] : G.ok[3];
            const unsigned base = (unsigned)(((gn * g.Hd + gi) * g.Wd + gj) * g.d_pix * 2);
            const unsigned dst0 = lds0 + (unsigned)(S * WL_STAGE + wave * C::NI * 1024);
#pragma unroll
            for (int k = 0; k < C::NI; ++k) {
                const int ii = wave * C::NI + k;
                const int p = (ii * 1024) / PIXB + (lane * 16) / PIXB, slot = ((lane * 16) % PIXB) / 16;
                const unsigned st_lane = (unsigned)((((p & 15) * g.d_pix + g.d_choff) * 2) + ((slot ^ p) & (NCH - 1)) * 16);
                const unsigned vo = gok ? base + st_lane : LF_OOB;                // (a whole group beyond the tensor: zeros)
                if constexpr (C::ST_ADD) lds_dma16(ra_add, dst0 + (unsigned)(k * 1024), vo, 0u);
                if constexpr (C::ST_MSK) lds_dma16(ra_msk, dst0 + (unsigned)(C::OUT_BYTES + k * 1024), vo, 0u);
                if constexpr (C::ST_AUX) lds_dma16(ra_aux, dst0 + (unsigned)(C::OUT_BYTES * (C::ST_MSK ? 2 : 1) + k * 1024), vo, 0u);
            }
        }
    };

    // epilogue constants
    const __amdgpu_buffer_rsrc_t r_dst = make_rsrc(a.dst, 0xffffffffu), r_add = make_rsrc(a.add_src, 0xffffffffu),
                                 r_msk = make_rsrc(a.mask_src, 0xffffffffu), r_aux = make_rsrc(a.aux, 0xffffffffu),
                                 r_bias = make_rsrc(a.bias, 0xffffffffu), r_msc = make_rsrc(a.msc, 0xffffffffu),
                                 r_msh = make_rsrc(a.msh, 0xffffffffu), r_dm = make_rsrc(a.dm, 0xffffffffu);
    // fragment read addresses inside a stage: pixel m*16 + pl (128 B rows), chunk kb*4 + kq XOR (pl >> 1) & 7
    const unsigned xf0 = (unsigned)(pl * 128 + (((0 + kq) ^ (pl >> 1)) & 7) * 16), xf1 = (unsigned)(pl * 128 + (((4 + kq) ^ (pl >> 1)) & 7) * 16);
    const bool stats = (epi & (LF_EPI_STATS_SQ | LF_EPI_STATS_XHAT)) != 0;
    int st_c = 0;
    for (unsigned bx = it_first; bx < it_end; bx += it_stride) {
        constexpr bool PIVOT = EPIC >= 0;    // the pivot of the BN forward sums (see LF_TAPGEMM_EPILOGUE); the run-time-flag form sums about 0
        f32x4 s1[NT], s2[NT], piv[PIVOT ? NT : 1];
#pragma unroll
        for (int n = 0; n < NT; ++n) { s1[n] = zero4(); s2[n] = zero4(); piv[PIVOT ? n : 0] = zero4(); }
        for (int sub = 0; sub < 4; ++sub) {
            f32x4 acc[NT][MT];
#pragma unroll
            for (int n = 0; n < NT; ++n)
#pragma unroll
                for (int m = 0; m < MT; ++m) acc[n][m] = zero4();
            RingGroups G;
            groups_at((bx * 4u + (unsigned)sub) * 4u, g.Hl, GR, ngroups, G);
#pragma unroll
            for (int s = 0; s < NSTEP; ++s) {
                // my DMA of this step has landed: exactly S - 2 younger ring steps of 2 instructions may be in flight -- plus, behind
                // step 0, this sub-tile's staging instructions while the step's own DMA is older than they are (steps 1 .. S-1; the
                // count must not EXCEED the younger instructions, or the wait passes early) ...
                // ... and MY fragment reads of the step before have retired (lgkmcnt): hipcc moves that step's last MFMAs -- and the
                // waits for their operands -- behind the barrier, and the stage is restaged right behind it: a DMA instruction whose 8
                // pixels are all padding returns its zeros without a memory round trip and overtook those reads (wrong tiles in 1 of
                // 3 launches at dilation 8, row width 80)
                if (s >= 1 && s <= S - 1) wait_vm_lgkm0<2 * (S - 2) + C::NAUXI>();
                else wait_vm_lgkm0<2 * (S - 2)>();
                const int t = KS == 1 ? s : s >> 1, ks = KS == 1 ? 0 : s & 1;          // (compile-time after unrolling: wr is indexed statically)
                if constexpr (PROC == LF_PRO_BNRELU) {
                    // my part of this step's stage has landed: relu(bn(x)) on it, in place (the other waves read it behind the barrier)
                    unsigned char* mine = ring + st_c * WL_STAGE + wave * 2048;
                    const int tv = __builtin_amdgcn_readlane(tapv, t);
                    const int dh = (int)(short)(tv & 0xffff), dw = tv >> 16;
                    const int gi = wave == 0 ? G.i[0] : wave == 1 ? G.i[1] : wave == 2 ? G.i[2] : G.i[3];
                    const int gj = wave == 0 ? G.j[0] : wave == 1 ? G.j[1] : wave == 2 ? G.j[2] : G.j[3];
                    const bool gok = wave == 0 ? G.ok[0] : wave == 1 ? G.ok[1] : wave == 2 ? G.ok[2] : G.ok[3];
                    const int sy = gi + dh;
                    const bool yok = gok && sy >= 0 && sy < g.Hs;
#pragma unroll
                    for (int jj = 0; jj < 2; ++jj) {
                        const bool in = yok && (unsigned)(gj + dw + lane_dx[jj]) < (unsigned)g.Ws;
                        const int c0 = ks * 64 + (((lane & 7) ^ ((jj * 4 + (lane >> 4)) & 7)) * 8);      // this lane's 8 channels
                        u32x4v r = *reinterpret_cast<const u32x4v*>(mine + jj * 1024 + lane * 16);
                        const f32x4 sc0 = *reinterpret_cast<const f32x4*>(ptab + c0), sc1 = *reinterpret_cast<const f32x4*>(ptab + c0 + 4),
                                    sh0 = *reinterpret_cast<const f32x4*>(ptab + CD + c0), sh1 = *reinterpret_cast<const f32x4*>(ptab + CD + c0 + 4);
                        f32x4 lo, hv;
                        lo.x = __uint_as_float(r[0] << 16); lo.y = __uint_as_float(r[0] & 0xffff0000u);
                        lo.z = __uint_as_float(r[1] << 16); lo.w = __uint_as_float(r[1] & 0xffff0000u);
                        hv.x = __uint_as_float(r[2] << 16); hv.y = __uint_as_float(r[2] & 0xffff0000u);
                        hv.z = __uint_as_float(r[3] << 16); hv.w = __uint_as_float(r[3] & 0xffff0000u);
                        lo = max0(lo * sc0 + sh0); hv = max0(hv * sc1 + sh1);
                        lo.x = in ? lo.x : 0.f; lo.y = in ? lo.y : 0.f; lo.z = in ? lo.z : 0.f; lo.w = in ? lo.w : 0.f;
                        hv.x = in ? hv.x : 0.f; hv.y = in ? hv.y : 0.f; hv.z = in ? hv.z : 0.f; hv.w = in ? hv.w : 0.f;
                        *reinterpret_cast<bf16x8*>(mine + jj * 1024 + lane * 16) = cvt_bf16x8(lo, hv);
                    }
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");       // my writes are in the stage
                }
                __builtin_amdgcn_s_barrier();        // ... and everyone's; everyone is past the fragment reads of the step before
                asm volatile("" ::: "memory");
                issue();                             // S - 1 steps ahead -> the stage the previous step occupied
                if (s == 0) stage_tensors(G);        // (everyone is past the previous sub-tile's reads of the tiles: the barrier above)
                const unsigned char* st = ring + st_c * WL_STAGE;
                st_c = st_c == S - 1 ? 0 : st_c + 1;
#pragma unroll
                for (int kb = 0; kb < 2; ++kb) {
                    bf16x8 xb[MT];
#pragma unroll
                    for (int m = 0; m < MT; ++m) xb[m] = *reinterpret_cast<const bf16x8*>(st + (kb ? xf1 : xf0) + m * 2048);
#pragma unroll
                    for (int n = 0; n < NT; ++n)
#pragma unroll
                        for (int m = 0; m < MT; ++m)
                            acc[n][m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wr[t][ks * 2 + kb][n], xb[m], acc[n][m], 0, 0, 0);
                }
            }
            // ---- epilogue of the sub-tile: accumulator tile (n, m) = channels cobw + n*16 + kq*4 .. +3 of pixel m*16 + pl
            if constexpr (C::NAUXI > 0) {            // the staged tensors have landed: mine (the ring steps issued since are younger) ...
                wait_vm_lgkm0<2 * (NSTEP - 1)>();
                __builtin_amdgcn_s_barrier();        // ... and everyone's
                asm volatile("" ::: "memory");
            }
            // (128 channels, MASKBN + BN-backward sums: the mask's per-channel vectors are re-read from L1 per use -- held, they are the
            // 9 registers that variant would spill beside its 96 weight registers)
            constexpr bool HOISTM = !(CB == 4 && EPIC >= 0 && (EPIC & LF_EPI_MASKBN) != 0 && (EPIC & LF_EPI_STATS_XHAT) != 0);
            f32x4 bs[NOBIAS ? 1 : NT], hsc[HOISTM ? NT : 1], hsh[HOISTM ? NT : 1];
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                const unsigned co = (unsigned)(cobw + n * 16 + kq * 4);
                if constexpr (!NOBIAS) bs[n] = a.bias ? ldb4(r_bias, co * 4u, 0u) : zero4();
                if constexpr (HOISTM) { if (epi & LF_EPI_MASKBN) { hsc[n] = ldb4(r_msc, co * 4u, 0u); hsh[n] = ldb4(r_msh, co * 4u, 0u); } }
            }
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                const unsigned dbase = (unsigned)(((G.n[m] * g.Hd + G.i[m]) * g.Wd + G.j[m] + pl) * g.d_pix + g.d_choff + cobw + kq * 4);
                f32x4 la[NT], lm[NT], lx[NT], ld[NT];
                auto tile_ld = [&](const unsigned char* tile, int n) __attribute__((always_inline)) {      // this lane's 4 channels of (m, n)
                    const int p = m * 16 + pl, chunk = (cobw + n * 16 + kq * 4) >> 3;
                    const uint2 q = *reinterpret_cast<const uint2*>(tile + p * PIXB + ((chunk ^ p) & (NCH - 1)) * 16 + (kq & 1) * 8);
                    f32x4 v;
                    v.x = __uint_as_float(q.x << 16); v.y = __uint_as_float(q.x & 0xffff0000u);
                    v.z = __uint_as_float(q.y << 16); v.w = __uint_as_float(q.y & 0xffff0000u);
                    return v;
                };
#pragma unroll
                for (int n = 0; n < NT; ++n) {
                    if (epi & LF_EPI_ADD) la[n] = C::ST_ADD ? tile_ld(otile, n) : epi_ld<S16>(r_add, dbase + n * 16);
                    if (epi & LF_EPI_MASK) lm[n] = C::ST_MSK ? tile_ld(mtile, n) : epi_ld<S16>(r_msk, dbase + n * 16);
                    if (epi & (LF_EPI_MASKBN | LF_EPI_STATS_XHAT)) lx[n] = C::ST_AUX ? tile_ld(xtile, n) : epi_ld<S16>(r_aux, dbase + n * 16);
                    if ((epi & LF_EPI_STATS_XHAT) && a.dm) ld[n] = ldb4(r_dm, (unsigned)(G.n[m] * g.Cd + cobw + n * 16 + kq * 4) * 4u, 0u);
                }
#pragma unroll
                for (int n = 0; n < NT; ++n) {
                    f32x4 v = acc[n][m];
                    if constexpr (!NOBIAS) v += bs[n];
                    if (epi & LF_EPI_ADD) v += la[n];
                    if (epi & LF_EPI_MASK) v = keep_pos(v, lm[n]);
                    if (epi & LF_EPI_MASKBN) {
                        const unsigned co = (unsigned)(cobw + n * 16 + kq * 4);
                        v = keep_pos(v, lx[n] * (HOISTM ? hsc[HOISTM ? n : 0] : ldb4(r_msc, co * 4u, 0u)) + (HOISTM ? hsh[HOISTM ? n : 0] : ldb4(r_msh, co * 4u, 0u)));
                    }
                    if (epi & LF_EPI_RELU) v = max0(v);
                    lf_bf16x4 b;
                    b[0] = (lf_bf16)v.x; b[1] = (lf_bf16)v.y; b[2] = (lf_bf16)v.z; b[3] = (lf_bf16)v.w;
                    // output tile: pixel p = m*16 + pl, 16-byte chunk (channel / 8) XOR p, half kq & 1
                    const int p = m * 16 + pl, chunk = (cobw + n * 16 + kq * 4) >> 3;
                    *reinterpret_cast<lf_bf16x4*>(otile + p * PIXB + ((chunk ^ p) & (NCH - 1)) * 16 + (kq & 1) * 8) = b;
                    if (stats) {
                        v.x = (float)b[0]; v.y = (float)b[1]; v.z = (float)b[2]; v.w = (float)b[3];     // statistics of the values as stored
                        if (!G.ok[m]) v = zero4();
                        if (epi & LF_EPI_STATS_SQ) {
                            if (PIVOT && sub == 0 && m == 0) piv[PIVOT ? n : 0] = bcast16(v);      // the item's first pixel (this wave owns all 256 of its channels)
                            f32x4 dv = PIVOT ? v - piv[PIVOT ? n : 0] : v;
                            if (!G.ok[m]) dv = zero4();
                            s1[n] += dv; s2[n] += dv * dv;
                        }
                        if (epi & LF_EPI_STATS_XHAT) {
                            const f32x4 gm = a.dm ? v * ld[n] : v;
                            s1[n] += gm; s2[n] += gm * lx[n];
                        }
                    }
                }
                if constexpr (!HOISTM) __builtin_amdgcn_sched_barrier(0);      // one pixel tile's operands at a time
            }
            __syncthreads();                          // the output tile is complete
            // whole-line stores: instruction ii of the tile = bytes ii*1024 .. +1023 of the (pixel-major) tile
            constexpr int NI = C::OUT_BYTES / 1024 / WG_WAVES;
#pragma unroll
            for (int k = 0; k < NI; ++k) {
                const int ii = wave * NI + k;
                const int p = (ii * 1024) / PIXB + (lane * 16) / PIXB;            // pixel of the sub-tile
                const int slot = ((lane * 16) % PIXB) / 16;
                const int grp = (ii * 1024 / PIXB) >> 4;                          // uniform: an instruction's pixels lie in one group
                const int gn = grp == 0 ? G.n[0] : grp == 1 ? G.n[1] : grp == 2 ? G.n[2] : G.n[3];
                const int gi = grp == 0 ? G.i[0] : grp == 1 ? G.i[1] : grp == 2 ? G.i[2] : G.i[3];
                const int gj = grp == 0 ? G.j[0] : grp == 1 ? G.j[1] : grp == 2 ? G.j[2] : G.j[3];
                const bool gok = grp == 0 ? G.ok[0] : grp == 1 ? G.ok[1] : grp == 2 ? G.ok[2] : G.ok[3];
                if (gok) {
                    const u32x4v v = *reinterpret_cast<const u32x4v*>(otile + ii * 1024 + lane * 16);
                    const unsigned off = (unsigned)((((gn * g.Hd + gi) * g.Wd + gj + (p & 15)) * g.d_pix + g.d_choff) * 2 + ((slot ^ p) & (NCH - 1)) * 16);
                    __builtin_amdgcn_raw_buffer_store_b128(v, r_dst, (int)off, 0, 0);
                }
            }
            // (the next sub-tile's first barrier orders these reads of the output tile before its next writes)
        }
        if (stats) {
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                f32x4 r1, r2;
                r1.x = sum16(s1[n].x); r1.y = sum16(s1[n].y); r1.z = sum16(s1[n].z); r1.w = sum16(s1[n].w);
                r2.x = sum16(s2[n].x); r2.y = sum16(s2[n].y); r2.z = sum16(s2[n].z); r2.w = sum16(s2[n].w);
                if (epi & LF_EPI_STATS_SQ) {      // pivot sums -> (sum v, M2 about the item's own mean) of the item's valid pixels
                    const unsigned t0 = bx * (unsigned)PIX_PER_WG;
                    const float ni = t0 < npix ? (float)min(npix - t0, (unsigned)PIX_PER_WG) : 0.f;
                    const float rn = ni > 0.f ? 1.f / ni : 0.f;
                    r2 = r2 - r1 * r1 * rn;
                    r2.x = fmaxf(r2.x, 0.f); r2.y = fmaxf(r2.y, 0.f); r2.z = fmaxf(r2.z, 0.f); r2.w = fmaxf(r2.w, 0.f);
                    if (PIVOT) r1 = r1 + piv[PIVOT ? n : 0] * ni;
                }
                if (pl == 0) {            // channel-major rows: [2][Cd][stats_ld] (32-bit indices: 2 * Cd * stats_ld floats is far below 2^31)
                    float* d = a.stats + (unsigned)((cobw + n * 16 + kq * 4) * a.stats_ld) + bx;
                    const unsigned half = (unsigned)(g.Cd * a.stats_ld);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        d[(unsigned)(e * a.stats_ld)] = r1[e];
                        d[half + (unsigned)(e * a.stats_ld)] = r2[e];
                    }
                }
            }
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // the trailing (dead) steps: nothing may land in LDS after this
    __builtin_amdgcn_s_barrier();
}

// ---------------------------------------------------------------------------------------
// tapgemm_bf16_wv_kernel ("wave-private", round 6): the 3-tap bf16 convolutions of non_bottleneck_1d at 64 channels.
//
// At 64 channels the whole-line kernel above shares a 64-pixel sub-tile between its four waves (each owns 16 output channels):
// 24 MFMAs per wave between five workgroup barriers, and the launch sits at 4.0 TB/s of tensor bytes where the same kernel at 128
// channels has twice the work per barrier.  But at 64 channels ALL the weights of the convolution are 3 taps x 64 x 64 x 2 B =
// 24 KB = 96 registers per lane -- what a wave of the 128-channel form holds for its quarter of the output channels.  So here a
// wave owns its pixels AND every output channel: wave tile = 32 pixels x 64 channels (8 accumulator tiles), the weights live in
// its registers for the workgroup's life, its operands arrive by LDS-DMA in a PRIVATE ring (stage = one tap of its 32 pixels = 4 KB,
// 4 instructions of 8 pixels x 128 B: whole lines), its output leaves through a private 4 KB tile as whole-line stores -- and no
// instruction of the K loop or the epilogue waits for another wave: the only barriers are the two that merge the four waves'
// BatchNorm partial sums into the 256-pixel statistics row, in the launches that take statistics.
//   ring order (per wave):   s_waitcnt vmcnt(N) lgkmcnt(0)      my DMA of this step has landed; my fragment reads of the step before
//                                                               have retired (their stage is restaged next)
//                            issue the step R - 1 ahead; read fragments; 16 MFMAs
// N counts the vector-memory instructions YOUNGER than the awaited DMA: 4 (R - 2) ring instructions, the item's staging
// instructions behind its first step, and -- vmcnt retires loads AND stores in issue order on gfx9-family hardware -- the four
// whole-line stores of the previous item's epilogue in front of an item's first step (all four are always issued: a group beyond
// the tensor stores to the out-of-range offset, which the buffer unit drops).
// Work: a workgroup walks 256-pixel tiles (the statistics rows of the other kernels) inside its XCD's range; wave w takes pixels
// w*64 .. w*64+63 of the tile as two items of 32.  K order = tapgemm_bf16_kernel's (tap, then channel): results bit-identical.
// Measured on one box (tools/bf16_ab.py, config 3's 64 x 80 x 160 x 64 launches, whole-line kernel -> this one): forward 52.1 -> 41.6 us,
// data gradient + mask 65.0 -> 60.3 / 66.7 -> 58.1.  The BN+ReLU operand prologue (the block's third convolution) was built here
// too -- the wave transforming the stage it brought in, in place, behind its own vmcnt wait -- and is SLOWER than the streaming
// kernel's register form (102.9 vs 88.3 us: the transform sits between the wave's DMA wait and its fragment reads, three times per
// pixel, with one partner wave to hide it): removed, those launches stay on tapgemm_bf16_kernel.
// ---------------------------------------------------------------------------------------
constexpr int WV_PX = 32, WV_STAGE = WV_PX * 128;
template <int EPIC> struct WvCfg {
    static constexpr bool ST_ADD = EPIC >= 0 && (EPIC & LF_EPI_ADD) != 0, ST_MSK = EPIC >= 0 && (EPIC & LF_EPI_MASK) != 0,
                          ST_AUX = EPIC >= 0 && (EPIC & (LF_EPI_MASKBN | LF_EPI_STATS_XHAT)) != 0;
    static constexpr int NBUF = (ST_MSK ? 1 : 0) + (ST_AUX ? 1 : 0);                  // tiles beside the output tile
    static constexpr int R = NBUF == 1 ? 3 : 4;                                       // ring stages (one extra tile: 3 keeps two workgroups per CU)
    static constexpr int NAUXI = ((ST_ADD ? 1 : 0) + NBUF) * 4;                       // staging instructions per item
    static constexpr int WAVE_LDS = (R + 1 + NBUF) * WV_STAGE;
    static constexpr size_t LDS = (size_t)WG_WAVES * WAVE_LDS;
};

// (two workgroups per CU by LDS except with two staged operand tiles or run-time flags: those get the whole register file)
template <int EPIC>
__global__ __launch_bounds__(256, (EPIC >= 0 && WvCfg<EPIC>::NBUF < 2) ? 2 : 1) void tapgemm_bf16_wv_kernel(const LfTapGeom g, const LfTapArgs a, const int pro, const int epi_rt) {
    typedef WvCfg<EPIC> C;
    constexpr int NT = 4, MW = 2, R = C::R, CD = 64;
    constexpr bool S16 = true;
    const int epi = EPIC >= 0 ? EPIC : epi_rt;
    constexpr bool NOBIAS = EPIC >= 0 && !(EPIC & LF_EPI_BIAS) && (EPIC & (LF_EPI_MASK | LF_EPI_ADD | LF_EPI_MASKBN | LF_EPI_STATS_XHAT)) != 0;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int pl = lane & 15, kq = lane >> 4;
    const unsigned npix = (unsigned)(g.N * g.Hl * g.Wl), ngroups = npix >> 4, GR = (unsigned)g.Wl >> 4;
    const unsigned ntiles = (npix + PIX_PER_WG - 1) / PIX_PER_WG;
    const XcdRange itr = xcd_range(ntiles);
    const unsigned it_first = itr.first, it_stride = itr.stride, it_end = itr.end;
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)lf_tap_lds + (unsigned)(wave * C::WAVE_LDS);
    unsigned char* const ring = lf_tap_lds + wave * C::WAVE_LDS;
    unsigned char* const otile = ring + R * WV_STAGE;
    unsigned char* const mtile = otile + WV_STAGE;                                     // mask source (when staged)
    unsigned char* const xtile = otile + WV_STAGE * (C::ST_MSK ? 2 : 1);              // BN-backward operand (when staged)

    // ---- all the weights -> registers: [tap][32-channel k-block][16-channel output tile], the MFMA A operand
    bf16x8 wr[3][2][NT];
    {
        const __amdgpu_buffer_rsrc_t rw = make_rsrc(a.wp16, 0xffffffffu);
#pragma unroll
        for (int t = 0; t < 3; ++t)
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int n = 0; n < NT; ++n)
                    wr[t][kb][n] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(
                        rw, (int)((((t * 2 + kb) * 4 + kq) * CD + n * 16 + pl) * 16), 0, 0));
    }
    int tapv = 0;            // tap t's offsets in lane t (v_readlane: see tapgemm_bf16_wl_kernel)
#pragma unroll
    for (int t = 0; t < 3; ++t)
        if (lane == t) tapv = (g.tdh[t] & 0xffff) | (g.tdw[t] << 16);
    const i32x4s rx = make_rsrc_words(a.src, (unsigned)min((long)g.N * g.Hs * g.Ws * g.s_pix * 2, (long)LF_OOB));
    const int spix2 = g.s_pix * 2;
    // DMA mapping: instruction q of a step carries pixels q*8 .. q*8+7 of the item (group q >> 1): lane -> pixel q*8 + (lane >> 3),
    // LDS slot lane & 7 = chunk XOR ((pixel >> 1) & 7) -- which depends on q & 1 only
    const int dpx = lane >> 3;
    unsigned lane_x[2];
    int lane_dx[2];
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
        const int chunk = (lane & 7) ^ ((jj * 4 + (lane >> 4)) & 7);
        lane_x[jj] = (unsigned)(((jj * 8 + dpx) * g.s_pix + g.s_choff) * 2 + chunk * 16);
        lane_dx[jj] = jj * 8 + dpx;
    }
    // the two 16-pixel groups of item (tile, h) of this wave: (image, row, first column), wave-uniform
    struct Item { int n[2], i[2], j[2]; bool ok[2]; };
    auto item_at = [&](unsigned tile, int h, Item& o) __attribute__((always_inline)) {
        const unsigned G0 = tile * 16u + (unsigned)(wave * 4 + h * 2);
        const unsigned Gc = G0 < ngroups ? G0 : 0u;
        const unsigned Rw = Gc / GR;
        int jg = __builtin_amdgcn_readfirstlane((int)(Gc - Rw * GR));
        int n = __builtin_amdgcn_readfirstlane((int)(Rw / (unsigned)g.Hl));
        int i = __builtin_amdgcn_readfirstlane((int)Rw) - n * g.Hl;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            o.ok[q] = G0 + q < ngroups;
            o.n[q] = n; o.i[q] = i; o.j[q] = jg * 16;
            if (++jg == (int)GR) { jg = 0; if (++i == g.Hl) { i = 0; ++n; } }
        }
    };
    // ---- load cursor (wave-uniform): tile, half, tap, ring stage; its item's groups as (pixel index without the tap, row, column)
    unsigned tile_ld = it_first;
    int h_ld = 0, t_ld = 0, st_ld = 0;
    int lrow[2] = {0, 0}, liy[2] = {0, 0}, lsx[2] = {0, 0};
    bool lok[2] = {false, false};
    auto cursor_item = [&]() __attribute__((always_inline)) {
        lok[0] = false; lok[1] = false;
        if (tile_ld < it_end) {
            Item I;
            item_at(tile_ld, h_ld, I);
#pragma unroll
            for (int q = 0; q < 2; ++q) { lok[q] = I.ok[q]; liy[q] = I.i[q]; lsx[q] = I.j[q]; lrow[q] = (I.n[q] * g.Hs + I.i[q]) * g.Ws + I.j[q]; }
        }
    };
    cursor_item();
    auto issue = [&]() __attribute__((always_inline)) {
        const int tv = __builtin_amdgcn_readlane(tapv, t_ld);
        const int dh = (int)(short)(tv & 0xffff), dw = tv >> 16;
        const unsigned dst = lds0 + (unsigned)(st_ld * WV_STAGE);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int gq = q >> 1, jj = q & 1;
            const int sy = liy[gq] + dh;
            const bool yok = lok[gq] && sy >= 0 && sy < g.Hs;
            const unsigned base = (unsigned)((lrow[gq] + dh * g.Ws + dw) * spix2);
            const bool in = yok && (unsigned)(lsx[gq] + dw + lane_dx[jj]) < (unsigned)g.Ws;
            lds_dma16(rx, dst + (unsigned)q * 1024u, in ? base + lane_x[jj] : LF_OOB, 0u);
        }
        st_ld = st_ld == R - 1 ? 0 : st_ld + 1;
        if (++t_ld == 3) {
            t_ld = 0;
            if (++h_ld == 2) { h_ld = 0; tile_ld += it_stride; }
            cursor_item();
        }
    };
#pragma unroll
    for (int i = 0; i < R - 1; ++i) issue();

    // ---- staging of the epilogue's operand tensors (whole lines, the output tile's layout): instruction ii = pixels ii*8 .. +7 of
    // the item: lane -> pixel p = ii*8 + (lane >> 3), 16-byte slot lane & 7 = chunk XOR (p & 7)
    const unsigned dbytes = (unsigned)min((long)g.N * g.Hd * g.Wd * g.d_pix * 2, (long)LF_OOB);
    const i32x4s ra_add = make_rsrc_words(a.add_src, dbytes), ra_msk = make_rsrc_words(a.mask_src, dbytes), ra_aux = make_rsrc_words(a.aux, dbytes);
    auto tile_lane_off = [&](int ii) __attribute__((always_inline)) {          // byte offset of this lane's chunk inside its group's 16 pixels
        const int p = ii * 8 + (lane >> 3);
        return (unsigned)((((p & 15) * g.d_pix + g.d_choff) * 2) + (((lane & 7) ^ p) & 7) * 16);
    };
    auto stage_tensors = [&](const Item& I) __attribute__((always_inline)) {
        if constexpr (C::NAUXI > 0) {
            const unsigned dst0 = lds0 + (unsigned)(R * WV_STAGE);
#pragma unroll
            for (int ii = 0; ii < 4; ++ii) {
                const int gq = ii >> 1;
                const unsigned base = (unsigned)(((I.n[gq] * g.Hd + I.i[gq]) * g.Wd + I.j[gq]) * g.d_pix * 2);
                const unsigned vo = I.ok[gq] ? base + tile_lane_off(ii) : LF_OOB;      // (a group beyond the tensor: zeros)
                if constexpr (C::ST_ADD) lds_dma16(ra_add, dst0 + (unsigned)(ii * 1024), vo, 0u);
                if constexpr (C::ST_MSK) lds_dma16(ra_msk, dst0 + (unsigned)(WV_STAGE + ii * 1024), vo, 0u);
                if constexpr (C::ST_AUX) lds_dma16(ra_aux, dst0 + (unsigned)(WV_STAGE * (C::ST_MSK ? 2 : 1) + ii * 1024), vo, 0u);
            }
        }
    };

    // epilogue constants (destination bounded by the tensor: the store of a group beyond it goes to the out-of-range offset and is dropped)
    const __amdgpu_buffer_rsrc_t r_dst = make_rsrc(a.dst, dbytes), r_add = make_rsrc(a.add_src, 0xffffffffu),
                                 r_msk = make_rsrc(a.mask_src, 0xffffffffu), r_aux = make_rsrc(a.aux, 0xffffffffu),
                                 r_bias = make_rsrc(a.bias, 0xffffffffu), r_msc = make_rsrc(a.msc, 0xffffffffu),
                                 r_msh = make_rsrc(a.msh, 0xffffffffu), r_dm = make_rsrc(a.dm, 0xffffffffu);
    // fragment read addresses inside a stage: pixel m*16 + pl (128 B rows), chunk kb*4 + kq XOR (pl >> 1) & 7
    const unsigned xf0 = (unsigned)(pl * 128 + (((0 + kq) ^ (pl >> 1)) & 7) * 16), xf1 = (unsigned)(pl * 128 + (((4 + kq) ^ (pl >> 1)) & 7) * 16);
    const bool stats = (epi & (LF_EPI_STATS_SQ | LF_EPI_STATS_XHAT)) != 0;
    int st_c = 0;
    bool first_item = true;          // no stores in flight in front of the very first step
    for (unsigned bx = it_first; bx < it_end; bx += it_stride) {
        constexpr bool PIVOT = EPIC >= 0;    // the pivot of the BN forward sums (see LF_TAPGEMM_EPILOGUE); the run-time-flag form sums about 0
        f32x4 s1[NT], s2[NT], piv[PIVOT ? NT : 1];
#pragma unroll
        for (int n = 0; n < NT; ++n) { s1[n] = zero4(); s2[n] = zero4(); piv[PIVOT ? n : 0] = zero4(); }
        for (int h = 0; h < 2; ++h) {
            f32x4 acc[NT][MW];
#pragma unroll
            for (int n = 0; n < NT; ++n)
#pragma unroll
                for (int m = 0; m < MW; ++m) acc[n][m] = zero4();
            Item I;
            item_at(bx, h, I);
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                // my DMA of this step has landed; my fragment reads of the step before have retired (header: what N counts)
                if (t == 0) {
                    if (first_item) wait_vm_lgkm0<4 * (R - 2)>();
                    else wait_vm_lgkm0<4 * (R - 2) + 4>();
                } else wait_vm_lgkm0<4 * (R - 2) + C::NAUXI>();
                issue();                             // R - 1 steps ahead -> the stage the previous step occupied
                if (t == 0) stage_tensors(I);
                const unsigned char* st = ring + st_c * WV_STAGE;
                st_c = st_c == R - 1 ? 0 : st_c + 1;
#pragma unroll
                for (int kb = 0; kb < 2; ++kb) {
                    bf16x8 xb[MW];
#pragma unroll
                    for (int m = 0; m < MW; ++m) xb[m] = *reinterpret_cast<const bf16x8*>(st + (kb ? xf1 : xf0) + m * 2048);
#pragma unroll
                    for (int n = 0; n < NT; ++n)
#pragma unroll
                        for (int m = 0; m < MW; ++m)
                            acc[n][m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wr[t][kb][n], xb[m], acc[n][m], 0, 0, 0);
                }
            }
            first_item = false;
            // ---- epilogue of the item: accumulator tile (n, m) = channels n*16 + kq*4 .. +3 of pixel m*16 + pl
            if constexpr (C::NAUXI > 0) wait_vm_lgkm0<8>();      // the staged tensors have landed (the two ring steps issued since are younger)
            constexpr bool HOISTM = !(EPIC >= 0 && (EPIC & LF_EPI_MASKBN) != 0 && (EPIC & LF_EPI_STATS_XHAT) != 0);
            f32x4 bs[NOBIAS ? 1 : NT], hsc[HOISTM ? NT : 1], hsh[HOISTM ? NT : 1];
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                const unsigned co = (unsigned)(n * 16 + kq * 4);
                if constexpr (!NOBIAS) bs[n] = a.bias ? ldb4(r_bias, co * 4u, 0u) : zero4();
                if constexpr (HOISTM) { if (epi & LF_EPI_MASKBN) { hsc[n] = ldb4(r_msc, co * 4u, 0u); hsh[n] = ldb4(r_msh, co * 4u, 0u); } }
            }
#pragma unroll
            for (int m = 0; m < MW; ++m) {
                const unsigned dbase = (unsigned)(((I.n[m] * g.Hd + I.i[m]) * g.Wd + I.j[m] + pl) * g.d_pix + g.d_choff + kq * 4);
                auto tile_ld = [&](const unsigned char* tile, int n) __attribute__((always_inline)) {      // this lane's 4 channels of (m, n)
                    const int p = m * 16 + pl, chunk = (n * 16 + kq * 4) >> 3;
                    const uint2 q = *reinterpret_cast<const uint2*>(tile + p * 128 + ((chunk ^ p) & 7) * 16 + (kq & 1) * 8);
                    f32x4 v;
                    v.x = __uint_as_float(q.x << 16); v.y = __uint_as_float(q.x & 0xffff0000u);
                    v.z = __uint_as_float(q.y << 16); v.w = __uint_as_float(q.y & 0xffff0000u);
                    return v;
                };
                // (two channel tiles at a time: with all four tiles' operands live beside the 96 weight registers the three-operand
                // epilogues spilled 10-31 registers)
#pragma unroll
                for (int n0 = 0; n0 < NT; n0 += 2) {
                f32x4 la[NT], lm[NT], lx[NT];
#pragma unroll
                for (int n = n0; n < n0 + 2; ++n) {
                    if (epi & LF_EPI_ADD) la[n] = C::ST_ADD ? tile_ld(otile, n) : epi_ld<S16>(r_add, dbase + n * 16);
                    if (epi & LF_EPI_MASK) lm[n] = C::ST_MSK ? tile_ld(mtile, n) : epi_ld<S16>(r_msk, dbase + n * 16);
                    if (epi & (LF_EPI_MASKBN | LF_EPI_STATS_XHAT)) lx[n] = C::ST_AUX ? tile_ld(xtile, n) : epi_ld<S16>(r_aux, dbase + n * 16);
                }
#pragma unroll
                for (int n = n0; n < n0 + 2; ++n) {
                    f32x4 v = acc[n][m];
                    if constexpr (!NOBIAS) v += bs[n];
                    if (epi & LF_EPI_ADD) v += la[n];
                    if (epi & LF_EPI_MASK) v = keep_pos(v, lm[n]);
                    if (epi & LF_EPI_MASKBN) {
                        const unsigned co = (unsigned)(n * 16 + kq * 4);
                        v = keep_pos(v, lx[n] * (HOISTM ? hsc[HOISTM ? n : 0] : ldb4(r_msc, co * 4u, 0u)) + (HOISTM ? hsh[HOISTM ? n : 0] : ldb4(r_msh, co * 4u, 0u)));
                    }
                    if (epi & LF_EPI_RELU) v = max0(v);
                    lf_bf16x4 b;
                    b[0] = (lf_bf16)v.x; b[1] = (lf_bf16)v.y; b[2] = (lf_bf16)v.z; b[3] = (lf_bf16)v.w;
                    // output tile: pixel p = m*16 + pl, 16-byte chunk (channel / 8) XOR p, half kq & 1
                    const int p = m * 16 + pl, chunk = (n * 16 + kq * 4) >> 3;
                    *reinterpret_cast<lf_bf16x4*>(otile + p * 128 + ((chunk ^ p) & 7) * 16 + (kq & 1) * 8) = b;
                    if (stats) {
                        v.x = (float)b[0]; v.y = (float)b[1]; v.z = (float)b[2]; v.w = (float)b[3];     // statistics of the values as stored
                        if (!I.ok[m]) v = zero4();
                        if (epi & LF_EPI_STATS_SQ) {
                            if (PIVOT && h == 0 && m == 0) piv[PIVOT ? n : 0] = bcast16(v);      // this wave's first pixel of the tile
                            f32x4 dv = PIVOT ? v - piv[PIVOT ? n : 0] : v;
                            if (!I.ok[m]) dv = zero4();
                            s1[n] += dv; s2[n] += dv * dv;
                        }
                        if (epi & LF_EPI_STATS_XHAT) {
                            // (the Dropout2d factor of (image, channel): an L1-resident vector, read where it is used instead of held)
                            const f32x4 gm = a.dm ? v * ldb4(r_dm, (unsigned)(I.n[m] * g.Cd + n * 16 + kq * 4) * 4u, 0u) : v;
                            s1[n] += gm; s2[n] += gm * lx[n];
                        }
                    }
                }
                __builtin_amdgcn_sched_barrier(0);      // one chunk's operands at a time
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");        // my quads are in the output tile
            // whole-line stores: instruction ii = pixels ii*8 .. +7 of the item (all four always issued: header)
#pragma unroll
            for (int ii = 0; ii < 4; ++ii) {
                const int gq = ii >> 1;
                const u32x4v v = *reinterpret_cast<const u32x4v*>(otile + ii * 1024 + lane * 16);
                const unsigned base = (unsigned)(((I.n[gq] * g.Hd + I.i[gq]) * g.Wd + I.j[gq]) * g.d_pix * 2);
                __builtin_amdgcn_raw_buffer_store_b128(v, r_dst, (int)(I.ok[gq] ? base + tile_lane_off(ii) : LF_OOB), 0, 0);
            }
            // (the next item's first wait carries lgkmcnt(0): these reads of the output tile retire before its next writes)
        }
        if (stats) {
            // the four waves' sums of this 256-pixel tile -> one partial row (the merge of LF_TAPGEMM_EPILOGUE); staging area = the
            // first 512 bytes of every wave's output tile (free: its stores read it above, the next item writes it 3 steps from now)
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            float (*sred)[4][8] = reinterpret_cast<float (*)[4][8]>(otile);           // [n][kq][8]
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                f32x4 r1, r2;
                r1.x = sum16(s1[n].x); r1.y = sum16(s1[n].y); r1.z = sum16(s1[n].z); r1.w = sum16(s1[n].w);
                r2.x = sum16(s2[n].x); r2.y = sum16(s2[n].y); r2.z = sum16(s2[n].z); r2.w = sum16(s2[n].w);
                if (epi & LF_EPI_STATS_SQ) {      // pivot sums -> (sum v, M2 about the wave's own mean) of the wave's nw valid pixels
                    const unsigned t0 = (bx * (unsigned)WG_WAVES + (unsigned)wave) * 64u;
                    const float nw = t0 < npix ? (float)min(npix - t0, 64u) : 0.f;
                    const float rn = nw > 0.f ? 1.f / nw : 0.f;
                    r2 = r2 - r1 * r1 * rn;
                    r2.x = fmaxf(r2.x, 0.f); r2.y = fmaxf(r2.y, 0.f); r2.z = fmaxf(r2.z, 0.f); r2.w = fmaxf(r2.w, 0.f);
                    if (PIVOT) r1 = r1 + piv[PIVOT ? n : 0] * nw;
                }
                if (pl == 0) {
                    float* d = sred[n][kq];
                    d[0] = r1.x; d[1] = r1.y; d[2] = r1.z; d[3] = r1.w; d[4] = r2.x; d[5] = r2.y; d[6] = r2.z; d[7] = r2.w;
                }
            }
            __syncthreads();
            if (threadIdx.x < NT * 4 * 8) {
                const int tt = threadIdx.x;
                const int j = tt & 7, q = (tt >> 3) & 3, n = tt >> 5;
                auto at = [&](int w, int jj) { return reinterpret_cast<const float (*)[4][8]>(lf_tap_lds + w * C::WAVE_LDS + R * WV_STAGE)[n][q][jj]; };
                float v = at(0, j) + at(1, j) + at(2, j) + at(3, j);
                if ((epi & LF_EPI_STATS_SQ) && j >= 4) {      // Chan: M2 = sum_w M2_w + sum_w n_w (mean_w - mean)^2
                    float nwv[4], sw[4], nt = 0.f, stt = 0.f;
#pragma unroll
                    for (int w = 0; w < 4; ++w) {
                        const unsigned t0w = (bx * (unsigned)WG_WAVES + (unsigned)w) * 64u;
                        nwv[w] = t0w < npix ? (float)min(npix - t0w, 64u) : 0.f;
                        sw[w] = at(w, j - 4);
                        nt += nwv[w]; stt += sw[w];
                    }
                    const float mg = nt > 0.f ? stt / nt : 0.f;
#pragma unroll
                    for (int w = 0; w < 4; ++w)
                        if (nwv[w] > 0.f) { const float dmw = sw[w] / nwv[w] - mg; v += nwv[w] * dmw * dmw; }
                }
                a.stats[((long)(j >> 2) * g.Cd + n * 16 + q * 4 + (j & 3)) * a.stats_ld + bx] = v;      // channel-major rows
            }
            __syncthreads();      // the staging areas are output tiles again
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // the trailing (dead) steps: nothing may land in LDS after this
    __builtin_amdgcn_s_barrier();
}

// ---------------------------------------------------------------------------------------
// tapgemm_bf16_lean_kernel: the 16 -> 16 channel 3-tap convolutions on bf16 tensors (decoder, full-resolution stage: HBM-bound,
// a pixel is 32 bytes).  The general bf16 kernel ran them in its run-time-flag form, one 32-channel K-step per tap with half
// of every operand register zero padding and one step in flight (101 us per launch at 160 x 320 x 64 images, 2.1 TB/s).  Here
//  * one MFMA contracts TWO taps: k-blocks 0-1 of the K = 32 step are tap 2i's 16 channels, k-blocks 2-3 tap 2i+1's -- a lane's
//    16-byte load is half a pixel at the tap its k-block belongs to, an instruction covers 2 x 16 consecutive pixels x 32 B
//    (whole lines); the three taps are 2 MFMAs per 16 x 16 tile, all 8 loads of a wave requested up front;
//  * prologue and epilogue flags compiled in, (image, row) of the 16-pixel groups in scalar registers (Wl % 16 == 0).
// The chain order (tap 0 + tap 1 in one K = 32 dot product, then tap 2) differs from tapgemm_bf16_kernel's three K-steps:
// results agree to fp32 rounding, not bit for bit.
// ---------------------------------------------------------------------------------------
template <int PROC, int EPIC>
__global__ __launch_bounds__(256, 4) void tapgemm_bf16_lean_kernel(const LfTapGeom g, const LfTapArgs a, const int pro_rt, const int epi_rt) {
    constexpr int NT = 1;
    constexpr bool S16 = true, HOISTV = EPIC >= 0;
    const int epi = EPIC >= 0 ? EPIC : epi_rt;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int pl = lane & 15, kq = lane >> 4;
    const unsigned npix = (unsigned)(g.N * g.Hl * g.Wl), ngroups = npix >> 4, GR = (unsigned)g.Wl >> 4;
    const int cob = 0;
    const unsigned bx = xcd_swizzle(blockIdx.x);
    RingGroups G;
    ring_groups(bx, wave, g.Hl, GR, ngroups, G);
    const int hi = kq >> 1, c8 = (kq & 1) * 8;              // which tap of the pair, which half of the pixel
    const __amdgpu_buffer_rsrc_t rw = make_rsrc(a.wp16, 0xffffffffu),
                                 rx = make_rsrc(a.src, (unsigned)min((long)g.N * g.Hs * g.Ws * g.s_pix * 2, (long)LF_OOB));
    // weights: packed [tap][4 k-blocks of 8 channels (2 real, 2 zero)][Cd][8]; MFMA i, lane (pl, kq): tap 2i + hi, k-block kq & 1
    bf16x8 wb[2];
    wb[0] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rw, (int)((((hi ? 1 : 0) * 4 + (kq & 1)) * g.Cd + pl) * 16), 0, 0));
    {
        u32x4v w2 = __builtin_amdgcn_raw_buffer_load_b128(rw, (int)(((2 * 4 + (kq & 1)) * g.Cd + pl) * 16), 0, 0);
        if (hi) { w2[0] = 0u; w2[1] = 0u; w2[2] = 0u; w2[3] = 0u; }       // there is no fourth tap
        wb[1] = __builtin_bit_cast(bf16x8, w2);
    }
    (void)pro_rt;
    u32x4v xr[2][MT];
    bool in[2][MT];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int dh = i == 0 ? (hi ? g.tdh[1] : g.tdh[0]) : g.tdh[2], dw = i == 0 ? (hi ? g.tdw[1] : g.tdw[0]) : g.tdw[2];
        const bool tapok = i == 0 || !hi;
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const int sy = G.i[m] * g.ssh + dh, sx = (G.j[m] + pl) * g.ssw + dw;
            in[i][m] = tapok && G.ok[m] && sy >= 0 && sy < g.Hs && sx >= 0 && sx < g.Ws;
            const unsigned off = (unsigned)((((G.n[m] * g.Hs + sy) * g.Ws + sx) * g.s_pix + g.s_choff + c8) * 2);
            xr[i][m] = __builtin_amdgcn_raw_buffer_load_b128(rx, (int)(in[i][m] ? off : LF_OOB), 0, 0);
        }
    }
    f32x4 sc0, sc1, sh0, sh1;
    if constexpr (PROC == LF_PRO_BNRELU) {
        sc0 = ldg4(a.pro_sc + c8); sc1 = ldg4(a.pro_sc + c8 + 4);
        sh0 = ldg4(a.pro_sh + c8); sh1 = ldg4(a.pro_sh + c8 + 4);
    }
    f32x4 acc[NT][MT];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            bf16x8 xb;
            if constexpr (PROC == LF_PRO_BNRELU) {          // relu(bn(x)) in fp32 on the widened values; padding is zero AFTER the transform
                const u32x4v r = xr[i][m];
                f32x4 lo, hv;
                lo.x = __uint_as_float(r[0] << 16); lo.y = __uint_as_float(r[0] & 0xffff0000u);
                lo.z = __uint_as_float(r[1] << 16); lo.w = __uint_as_float(r[1] & 0xffff0000u);
                hv.x = __uint_as_float(r[2] << 16); hv.y = __uint_as_float(r[2] & 0xffff0000u);
                hv.z = __uint_as_float(r[3] << 16); hv.w = __uint_as_float(r[3] & 0xffff0000u);
                lo = max0(lo * sc0 + sh0); hv = max0(hv * sc1 + sh1);
                const bool ok = in[i][m];
                lo.x = ok ? lo.x : 0.f; lo.y = ok ? lo.y : 0.f; lo.z = ok ? lo.z : 0.f; lo.w = ok ? lo.w : 0.f;
                hv.x = ok ? hv.x : 0.f; hv.y = ok ? hv.y : 0.f; hv.z = ok ? hv.z : 0.f; hv.w = ok ? hv.w : 0.f;
                xb = cvt_bf16x8(lo, hv);
            } else xb = __builtin_bit_cast(bf16x8, xr[i][m]);
            acc[0][m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wb[i], xb, i ? acc[0][m] : zero4(), 0, 0, 0);
        }
    int pn[MT], pi[MT], pj[MT];
    bool pv[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) { pn[m] = G.n[m]; pi[m] = G.i[m]; pj[m] = G.j[m] + pl; pv[m] = G.ok[m]; }
    LF_TAPGEMM_EPILOGUE
}

// ---------------------------------------------------------------------------------------
// tapgemm_bf16_thin_kernel: tapgemm_thin_kernel's tiling (lf_conv.hip) on bf16 tensors and the bf16 matrix cores, for the launches of
// one camera frame -- 8 to 32 workgroups of the kernels above on 256 CUs.  A wave owns ONE 16-pixel tile and NT 16-channel slabs, a
// workgroup 64 consecutive logical pixels, blockIdx.y walks the slab groups, one workgroup per tile: no walk, no workgroup barrier.
// The general LfTapGeom (any tap count, strides, sub-pixel destination offsets, ragged Wl); no operand prologue, no statistics; the
// epilogues the inference schedule issues: bias + ReLU and bias + residual + ReLU (BRES), the shared text (LF_EPI_HEAD / TILE / TAIL).
// Every output element is tapgemm_bf16_kernel's bit for bit (tests/test_thin_bf16_conv_gpu.py), and so the wave-private, whole-line
// and ring kernels': K-steps tap-major then 32-channel step, ONE fp32 MFMA chain per accumulator, a lane supplies the 8 channels
// kq * 8 .. of its pixel in the step, padding is zero bits (the out-of-range offset), an odd step count ends with the streaming
// kernel's dead step (the last live weights against zeros).  K is not split.
// Source channels: whole 32-channel steps, or 16 (DownsamplerBlock(16, 64)'s convolution: one half-filled step per tap) -- there the
// lanes kq = 2, 3, whose channels the pixel does not have, hold the out-of-range offset in every tap-table row: they read the buffer
// bound's zeros, not the next pixel (whose Inf / NaN against the zero-padded weights would be NaN in every output channel).
// A thin wave is alone on its SIMD and a step's MFMAs take NT x 8 passes, so nothing hides a load but the depth of the wave's own
// queue: a ring of R K-steps of operands (4 * (NT + 1) registers per step) is in flight.  The steps a turn of the ring requests
// beyond the K loop carry the out-of-range offset for BOTH operands: returned as zeros without a memory round trip, never used.
// Operand budgets of 80, 120, 160 and 200 registers per lane (R = the even step count a budget holds, at most 18: the longest K
// loop of the network) were measured in the detector, DESIGN.md section 9: within 4 % at one frame and 7 % at eight, the deepest the
// slowest; R = 14 / 10 / 6 at NT = 1 / 2 / 3 (the 120-register build's, fastest at one frame, where NT is 1 and 2) and 4 at NT = 4
// (the 80-register build's, fastest at 8 frames, where NT is 4) ship.
// ---------------------------------------------------------------------------------------
constexpr int thin16_ring(int nt) { return nt == 1 ? 14 : nt == 2 ? 10 : nt == 3 ? 6 : 4; }
__device__ __forceinline__ f32x4 widen_bf16x4(u32x2v q) {
    f32x4 v;
    v.x = __uint_as_float(q[0] << 16); v.y = __uint_as_float(q[0] & 0xffff0000u);
    v.z = __uint_as_float(q[1] << 16); v.w = __uint_as_float(q[1] & 0xffff0000u);
    return v;
}
template <int NT, int EPIC>
__global__ __launch_bounds__(256, 2) void tapgemm_bf16_thin_kernel(const LfTapGeom g, const LfTapArgs a) {
    constexpr int epi = EPIC, R = thin16_ring(NT);
    constexpr bool S16 = true, HOISTV = true;
    static_assert(R % 2 == 0 && (EPIC == LF_EPI_RELU || EPIC == BRES), "the ring holds whole pairs of K-steps");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int pl = lane & 15, kq = lane >> 4;
    const unsigned npix = (unsigned)(g.N * g.Hl * g.Wl);
    const int cob = blockIdx.y * NT * 16;
    const unsigned bx = xcd_swizzle(blockIdx.x);       // (see tapgemm_kernel: XCD-contiguous ranges)
    int pn[1], pi[1], pj[1];
    bool pv[1];
    {
        const unsigned p = (bx * WG_WAVES + wave) * 16 + pl;
        pv[0] = p < npix;
        const unsigned q = pv[0] ? p : 0u;
        const unsigned r = q / (unsigned)g.Wl;
        pj[0] = (int)(q - r * (unsigned)g.Wl);
        pn[0] = (int)(r / (unsigned)g.Hl);
        pi[0] = (int)(r - (unsigned)pn[0] * (unsigned)g.Hl);
    }
    // tapgemm_bf16_kernel's tap table (FAST form), one pixel tile wide: this lane's source byte offset per tap -- its 8 channels of
    // the first 32-channel step --, LF_OOB (reads as zeros) for padding and for channels the pixel does not have (Cs = 16)
    __shared__ unsigned tab[WG_WAVES][LF_MAX_TAPS][64];
    for (int t = 0; t < g.ntaps; ++t) {
        const int sy = pi[0] * g.ssh + g.tdh[t], sx = pj[0] * g.ssw + g.tdw[t];
        const bool in = pv[0] && sy >= 0 && sy < g.Hs && sx >= 0 && sx < g.Ws && kq * 8 < g.Cs;
        const int syc = min(max(sy, 0), g.Hs - 1), sxc = min(max(sx, 0), g.Ws - 1);
        const unsigned o = (unsigned)(((pn[0] * g.Hs + syc) * g.Ws + sxc) * g.s_pix + g.s_choff + kq * 8) * 2u;
        tab[wave][t][lane] = in ? o : LF_OOB;
    }
    // (each lane reads back only what it wrote: no barrier needed)
    f32x4 acc[NT][1];
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[n][0] = zero4();
    // (both ahead of the loop: the round trips of the bias vector and of the residual run under it -- behind it, nothing would hide
    // them; the residual stays as loaded -- widening it here would wait for it in front of the first operand request)
    LF_EPI_HEAD
    u32x2v addv[NT];
    if constexpr ((EPIC & LF_EPI_ADD) != 0) {
        const unsigned db = (unsigned)(((pn[0] * g.Hd + pi[0] * g.dsh + g.dah) * g.Wd + pj[0] * g.dsw + g.daw) * g.d_pix + g.d_choff + cob + kq * 4);
#pragma unroll
        for (int n = 0; n < NT; ++n) addv[n] = __builtin_amdgcn_raw_buffer_load_b64(r_add, (int)((db + n * 16) * 2u), 0, 0);
    }
    {
        struct Step { u32x4v w[NT]; u32x4v x; };
        const int ncb = (g.Cs + 31) >> 5, ntaps = g.ntaps, nsteps = ntaps * ncb;      // 32-channel steps per tap (Cs = 16: one, half filled)
        const int wstep = g.Cd * 64;                                        // bytes per 32-channel step (4 k-blocks x Cd x 16)
        const int npad = (nsteps + 1) & ~1;                                 // an odd step count ends with a dead step
        const __amdgpu_buffer_rsrc_t rx = make_rsrc(a.src, (unsigned)min((long)g.N * g.Hs * g.Ws * g.s_pix * 2, (long)LF_OOB));
        const __amdgpu_buffer_rsrc_t rw = make_rsrc(a.wp16, (unsigned)(nsteps * wstep));
        const unsigned wlane = (unsigned)(kq * g.Cd + cob + pl) * 16u;      // bytes (8 bf16 per lane and slab)
        const int wlast = (nsteps - 1) * wstep;
        int s_ld = 0, t_ld = 0, cb_ld = 0, wofs = 0;
        // the next K-step's operands -> S.  Step nsteps of an odd count: the last live weights against zeros (tapgemm_bf16_kernel's dead
        // step); from npad on -- the ring's turn reaches beyond the loop -- both operands out of range
        auto issue = [&](Step& S) {
            const bool live = t_ld < ntaps;
            const unsigned beyond = s_ld < npad ? 0u : LF_OOB;
            const unsigned o = tab[wave][live ? t_ld : ntaps - 1][lane] | (live ? 0u : LF_OOB);
#pragma unroll
            for (int n = 0; n < NT; ++n) S.w[n] = __builtin_amdgcn_raw_buffer_load_b128(rw, (int)((wlane + n * 256) | beyond), wofs, 0);
            S.x = __builtin_amdgcn_raw_buffer_load_b128(rx, (int)o, cb_ld * 64, 0);
            const int cbn = cb_ld + 1;
            const bool wrap = cbn == ncb;
            wofs = min(wofs + wstep, wlast);
            cb_ld = live ? (wrap ? 0 : cbn) : cb_ld;
            t_ld = (live && wrap) ? t_ld + 1 : t_ld;
            ++s_ld;
        };
        Step ring[R];
#pragma unroll
        for (int p = 0; p < R; ++p) issue(ring[p]);
        // one K-step: NT MFMAs, each continuing its accumulator's chain; refill: the slot's next occupant, R K-steps ahead
        auto step = [&](Step& S, auto refill) {
            const bf16x8 xb = __builtin_bit_cast(bf16x8, S.x);
#pragma unroll
            for (int n = 0; n < NT; ++n)
                acc[n][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, S.w[n]), xb, acc[n][0], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (decltype(refill)::value) issue(S);
            __builtin_amdgcn_sched_barrier(0);
        };
        // whole turns of the ring in a loop without an early exit (see tapgemm_thin_kernel), then the last, partial turn
        int base = 0;
        for (; base + R <= npad; base += R) {
#pragma unroll
            for (int j = 0; j < R; ++j) step(ring[j], std::true_type{});
        }
#pragma unroll
        for (int j = 0; j < R - 2; j += 2) {
            if (base + j >= npad) break;          // (wave-uniform; npad and R are even)
            step(ring[j], std::false_type{});
            step(ring[j + 1], std::false_type{});
        }
    }
#undef LF_EPI_LDADD
#define LF_EPI_LDADD(o) widen_bf16x4(addv[((o) - dbase) >> 4])      /* the residual of channel tile n, loaded ahead of the loop */
    LF_EPI_TILE(0)
#undef LF_EPI_LDADD
#define LF_EPI_LDADD(o) epi_ld<S16>(r_add, o)
    LF_EPI_TAIL
}

int g_bf16_lds = 4;            // tools / A-B runs only: 4 = wave-private (64 ch) / whole-line (128 ch) + 16-channel kernels where they apply, else the ring (shipped);
                               // 3 = the whole-line kernel at 64 channels too (round 5's routing); 2 = the ring
                               // for every launch it takes; 0 = the streaming bf16 kernel only
std::atomic<long> g_part_fast_launches{0};   // launches with Cs % 32 != 0 that took a compiled-in whole-step form (lf_tapgemm_partial_fast_launches)
int g_bf16_no_partial_fast = 0; // kernel-level tests only: launches with Cs % 32 != 0 decline the compiled-in whole-step forms of tapgemm_bf16_kernel
std::atomic<long> g_ring_launches{0};        // launches tapgemm_bf16_ring_kernel took (lf_tapgemm_bf16_ring_launches)
// tapgemm_bf16_thin_kernel (see there).  lf_debug_set_thin_bf16: mode 0 = LfTapArgs::thin and the grid size decide, 2 = every launch the
// kernel is compiled for takes it; nt = 0: the launcher's choice, 1..4: that many slabs per wave where it divides Cd / 16.  Its own
// switch and counter: lf_debug_set_thin / lf_debug_thin_launches (the fp32 kernel's, lf_conv.hip) do not touch bf16 launches.
std::atomic<int> g_thin16_mode{0}, g_thin16_nt{0};
std::atomic<long> g_thin16_launches{0};
std::atomic<int> g_bf16_cap{0};              // kernel-level tests only: > 0 caps grid.x of the resident launches below, so that one workgroup
                                             // walks several items at small shapes; 0 (shipped): launch_resident's own size

}  // namespace

void lf_tapgemm_set_bf16_lds(int v) { g_bf16_lds = v; }
int lf_tapgemm_bf16_lds() { return g_bf16_lds; }
void lf_tapgemm_set_bf16_no_partial_fast(int v) { g_bf16_no_partial_fast = v; }
long lf_tapgemm_partial_fast_launches() { return g_part_fast_launches.load(); }
long lf_tapgemm_bf16_ring_launches() { return g_ring_launches.load(); }
void lf_tapgemm_set_bf16_max_workgroups(int v) { g_bf16_cap = v > 0 ? v : 0; }
void lf_tapgemm_set_thin_bf16(int mode, int nt) { g_thin16_mode = mode == 2 ? 2 : 0; g_thin16_nt = (nt >= 1 && nt <= 4) ? nt : 0; }
long lf_tapgemm_thin_bf16_launches() { return g_thin16_launches.load(); }

namespace {
// tapgemm_bf16_ring_kernel: persistent
template <int EPIV, bool DBGV = false>
void launch_bf16_ring(unsigned nitems, hipStream_t st, const LfTapGeom& g, const LfTapArgs& a, int pro, int epi) {
    launch_resident(tapgemm_bf16_ring_kernel<EPIV, DBGV>, dim3(nitems), 256, (size_t)LB_STAGES * LB_STAGE_BYTES, 0, (unsigned)g_bf16_cap.load(), 0, st, g, a,
                    pro, epi);
    ++g_ring_launches;
}
// false: the runtime refused the kernel's LDS budget on this device (nothing launched: the caller takes the ring / streaming kernel)
template <int CBV, int EPIV, int PROV = 0>
bool launch_bf16_wl(unsigned nitems, hipStream_t st, const LfTapGeom& g, const LfTapArgs& a, int pro, int epi) {
    return launch_resident(tapgemm_bf16_wl_kernel<CBV, EPIV, PROV>, dim3(nitems), 256, WlCfg<CBV, EPIV, PROV>::LDS, BIG_LDS, (unsigned)g_bf16_cap.load(), 0, st, g, a,
                           pro, epi);
}
// tapgemm_bf16_wv_kernel (64 channels): same contract
template <int EPIV>
bool launch_bf16_wv(unsigned ntiles, hipStream_t st, const LfTapGeom& g, const LfTapArgs& a, int pro, int epi) {
    return launch_resident(tapgemm_bf16_wv_kernel<EPIV>, dim3(ntiles), 256, WvCfg<EPIV>::LDS, BIG_LDS, (unsigned)g_bf16_cap.load(), 0, st, g, a, pro, epi);
}

// the streaming tapgemm_bf16_kernel (FAST: its whole-step forms, see there); _rt: the run-time-flag form of an output slab width
template <int NTV, int PROV, int EPIV = -1, bool FAST = false>
void launch_bf16_stream(dim3 grid, hipStream_t st, const LfTapGeom& g, const LfTapArgs& a, int pro, int epi) {
    hipLaunchKernelGGL((tapgemm_bf16_kernel<NTV, PROV, EPIV, FAST>), grid, dim3(256), 0, st, g, a, pro, epi);
}
template <int NTV>
void launch_bf16_stream_rt(dim3 grid, hipStream_t st, const LfTapGeom& g, const LfTapArgs& a, int pro, int epi) {
    if (pro == LF_PRO_BNRELU) launch_bf16_stream<NTV, 1>(grid, st, g, a, pro, epi);
    else launch_bf16_stream<NTV, 0>(grid, st, g, a, pro, epi);
}
// tapgemm_bf16_thin_kernel: one workgroup per 64 pixels and group of nt slabs (lf_tapgemm_thin_pick_nt: shared with the fp32 route)
template <int EPIV>
void launch_bf16_thin(const LfTapGeom& g, const LfTapArgs& a, hipStream_t st) {
    const int nt = lf_tapgemm_thin_pick_nt(g, g_thin16_nt.load());
    const dim3 grid((unsigned)lf_cdiv((long)g.N * g.Hl * g.Wl, WG_WAVES * 16), g.Cd / (16 * nt));
    switch (nt) {
        case 4: hipLaunchKernelGGL((tapgemm_bf16_thin_kernel<4, EPIV>), grid, dim3(256), 0, st, g, a); break;
        case 3: hipLaunchKernelGGL((tapgemm_bf16_thin_kernel<3, EPIV>), grid, dim3(256), 0, st, g, a); break;
        case 2: hipLaunchKernelGGL((tapgemm_bf16_thin_kernel<2, EPIV>), grid, dim3(256), 0, st, g, a); break;
        default: hipLaunchKernelGGL((tapgemm_bf16_thin_kernel<1, EPIV>), grid, dim3(256), 0, st, g, a); break;
    }
    ++g_thin16_launches;
    if (EPIV == BRES) ++g_bres_launches;
}
}  // namespace

// precision mode bf16: bf16 tensors on the bf16 matrix cores (lf_tapgemm_launch's route for the launches with wp16)
int lf_tapgemm_bf16_route(const LfTapGeom& g, const LfTapArgs& a, int pro, int epi, int epis, long npix, int nt, dim3 grid, hipStream_t st) {
    LF_REQUIRE(a.s16, "tapgemm: the bf16 matrix-core kernels take bf16 tensors (s16); bf16 operands on fp32 tensors were removed in round 6");
    LF_REQUIRE(g.Cs >= 8 && g.s_pix >= g.s_choff + 8, "tapgemm bf16: needs at least 8 source channels");
    const bool in_offsets = (long)g.N * g.Hs * g.Ws * g.s_pix * 2 < (long)LF_OOB;    // the bf16 source inside 32-bit byte offsets
    // a launch of an output slab of 32 channels or more (the 64- / 128-channel convolutions, the stride-2 layers, the up-sampler
    // phases) that cannot put one workgroup on every CU: the thin tiling, where the caller asks for it (launch_fp32_route's rule).
    // Whole 32-channel steps, or 16 source channels; everything else runs where it ran
    const int thin_mode = g_thin16_mode.load();
    if ((a.thin || thin_mode == 2) && nt >= 2 && !a.dbg && pro == LF_PRO_NONE && ((epis == LF_EPI_RELU && a.bias) || epis == BRES) &&
        (g.Cs % 32 == 0 || g.Cs == 16) && g.s_pix >= g.s_choff + g.Cs && in_offsets &&
        (thin_mode == 2 || (long)grid.x * grid.y < lf_tapgemm_device_cus())) {
        if (epis == BRES) launch_bf16_thin<BRES>(g, a, st);
        else launch_bf16_thin<LF_EPI_RELU>(g, a, st);
        LF_CHECK_LAUNCH("tapgemm_bf16_thin");
        return 0;
    }
    // the 16 -> 16 channel 3-tap convolutions on bf16 tensors: tapgemm_bf16_lean_kernel
    if (a.s16 && g_bf16_lds >= 3 && !a.dbg && g.Cs == 16 && g.Cd == 16 && g.ntaps == 3 && g.Wl % 16 == 0 && g.s_pix % 8 == 0 && g.s_choff % 8 == 0 && in_offsets) {
        with_epi<true>(epis, [&](auto e) {
            constexpr int E = decltype(e)::value;
            if (pro == LF_PRO_BNRELU) hipLaunchKernelGGL((tapgemm_bf16_lean_kernel<1, E>), grid, dim3(256), 0, st, g, a, pro, epi);
            else hipLaunchKernelGGL((tapgemm_bf16_lean_kernel<0, E>), grid, dim3(256), 0, st, g, a, pro, epi);
        });
        if (epis == BRES) ++g_bres_launches;
        LF_CHECK_LAUNCH("tapgemm_bf16_lean");
        return 0;
    }
    const bool fast16 = nt == 4 && a.s16 && pro != LF_PRO_BNRELU && g.Cs % 32 == 0 && in_offsets;
    // Which kernel (g_bf16_lds = 4, the shipped setting): the 3-tap convolutions of non_bottleneck_1d at 64 / 128 channels ->
    // tapgemm_bf16_wl_kernel (whole lines); every other prologue-free launch at 64-channel output slabs whose 16-pixel groups lie
    // in one image row (the 9-tap stride-2 convolution, the transposed-convolution phases, their gradients) ->
    // tapgemm_bf16_ring_kernel; the rest (operand prologue, ragged widths) -> the streaming tapgemm_bf16_kernel
    // the block's third convolution (BN+ReLU operand prologue), at 128 channels: 83 -> 60 us per launch at config 3's size; at 64
    // channels the in-LDS transform is as long as the whole step (88 -> 91 us): those stay on the streaming kernel
    const bool fast16p = nt == 4 && a.s16 && pro == LF_PRO_BNRELU && epi == LF_EPI_RELU && g.Cs == 128 && in_offsets;
    const bool line3 = g_bf16_lds >= 3 && !a.dbg && g.ntaps == 3 && g.Cs == g.Cd && (g.Cd == 64 || g.Cd == 128) && g.Wl % 16 == 0 &&
                       g.ssh == 1 && g.ssw == 1 && g.dsh == 1 && g.dsw == 1 && g.dah == 0 && g.daw == 0 && g.Hs == g.Hl && g.Ws == g.Wl &&
                       g.Hd == g.Hl && g.Wd == g.Wl && g.s_pix % 8 == 0 && g.s_choff % 8 == 0 && g.d_pix % 8 == 0 && g.d_choff % 8 == 0 &&
                       (long)g.N * g.Hd * g.Wd * g.d_pix * 2 < (long)LF_OOB;
    // 64 channels (g_bf16_lds = 4, shipped): tapgemm_bf16_wv_kernel -- a wave owns its pixels and all 64 output channels; 3 = the
    // whole-line kernel for both channel counts (round 5's routing, kept for A/B runs: tools/bf16_ab.py)
    const bool wv = line3 && g_bf16_lds == 4 && g.Cd == 64 && fast16;
    const bool wl = line3 && (fast16 || fast16p);      // (also what the wave-private kernel declines)
    const unsigned ntiles = (unsigned)lf_cdiv(npix, PIX_PER_WG);
    if (wv) {
        const bool launched = with_epi<true>(epis, [&](auto e) {
            constexpr int E = decltype(e)::value;
            // (ADD + MASK + BN-backward sums: two staged operand tiles leave room for ONE workgroup per CU here -- 123.6 us in config
            // 3's step against 115.8 us on the whole-line kernel, which takes these launches: not compiled, `launched` stays false)
            if constexpr (E == (LF_EPI_ADD | LF_EPI_MASK | LF_EPI_STATS_XHAT)) return false;
            else return launch_bf16_wv<E>(ntiles, st, g, a, pro, epi);
        });
        if (launched) {
            if (epis == BRES) ++g_bres_launches;
            LF_CHECK_LAUNCH("tapgemm_bf16_wv");
            return 0;
        }
    }
    if (wl && fast16p) {        // (128 channels only)
        if (launch_bf16_wl<4, LF_EPI_RELU, 1>(ntiles, st, g, a, pro, epi)) {
            LF_CHECK_LAUNCH("tapgemm_bf16_wl (prologue)");
            return 0;
        }
    } else if (wl) {
        const bool launched = with_epi<true>(epis, [&](auto e) {
            constexpr int E = decltype(e)::value;
            return g.Cs == 128 ? launch_bf16_wl<4, E>(ntiles, st, g, a, pro, epi) : launch_bf16_wl<2, E>(ntiles, st, g, a, pro, epi);
        });
        if (launched) {
            if (epis == BRES) ++g_bres_launches;
            LF_CHECK_LAUNCH("tapgemm_bf16_wl");
            return 0;
        }
    }
    // compiled-in whole-step forms at Cs % 32 != 0 (below): their tap table has one row per (tap, step)
    const bool part_fast = !g_bf16_no_partial_fast && g.ntaps * ((g.Cs + 31) / 32) <= LF_MAX_TAPS;
    const bool ring = fast16 && g_bf16_lds >= 2 && g.Wl % 16 == 0 && g.Cd % 64 == 0;
    const unsigned nitems = ntiles * (unsigned)(g.Cd / 64);
    if (ring && a.dbg) {        // stamps (tools/kbench.py --phases16): the plain convolution only
        LF_REQUIRE(epis == 0, "tapgemm bf16 ring: stamps are compiled into the plain convolution only");
        launch_bf16_ring<0, true>(nitems, st, g, a, pro, epi);
    } else if (ring) {
        with_epi<false>(epis, [&](auto e) { launch_bf16_ring<decltype(e)::value>(nitems, st, g, a, pro, epi); });
    } else if (fast16) {       // the bf16-tensor launches of the network at 64 output channels per workgroup
        with_epi<false>(epis, [&](auto e) { launch_bf16_stream<4, 0, decltype(e)::value, true>(grid, st, g, a, pro, epi); });
    } else if (nt == 4 && a.s16 && pro != LF_PRO_BNRELU && g.Cs == 16 && (epis == (LF_EPI_MASK | LF_EPI_STATS_XHAT) || epis == 0) && part_fast && in_offsets) {
        // 16 source channels into a 64-channel slab (the data gradient of UpsamplerBlock(64, 16): 9 taps, stride 2, with the previous
        // layer's mask + BN-backward sums; 204 us per launch at config 3 on the run-time-flag form): ONE 32-channel step per tap on the
        // compiled-in form.  Lanes kq = 2, 3 -- channels 16..31 of the step, which the pixel does not have -- hold the out-of-range
        // offset and read the buffer bound's zeros against the zero-padded half of the packed weights
        if (epis == 0) launch_bf16_stream<4, 0, 0, true>(grid, st, g, a, pro, epi);
        else launch_bf16_stream<4, 0, LF_EPI_MASK | LF_EPI_STATS_XHAT, true>(grid, st, g, a, pro, epi);
        ++g_part_fast_launches;
    } else if (nt == 3 && a.s16 && pro != LF_PRO_BNRELU && g.Cs == 16 && (epis == LF_EPI_STATS_SQ || epis == LF_EPI_RELU || epis == 0) && part_fast && in_offsets) {
        // ... and the 16 -> 48 channel convolution of DownsamplerBlock(16, 64) (9 taps, stride 2, BN forward sums; 112 us on the run-time-flag form)
        // (RELU: the inference engine's folded form of the same convolution)
        if (epis == 0) launch_bf16_stream<3, 0, 0, true>(grid, st, g, a, pro, epi);
        else if (epis == LF_EPI_RELU) launch_bf16_stream<3, 0, LF_EPI_RELU, true>(grid, st, g, a, pro, epi);
        else launch_bf16_stream<3, 0, LF_EPI_STATS_SQ, true>(grid, st, g, a, pro, epi);
        ++g_part_fast_launches;
    } else if (nt == 4 && a.s16 && pro == LF_PRO_BNRELU && epi == LF_EPI_RELU) {
        launch_bf16_stream<4, 1, LF_EPI_RELU, false>(grid, st, g, a, pro, epi);
    } else if (nt == 1 && a.s16 && pro != LF_PRO_BNRELU && ((g.Cs + 31) / 32 * 32 + g.s_choff <= g.s_pix) && in_offsets &&
               (g.Cs % 32 == 0 || part_fast) &&
               (epis == 0 || epis == LF_EPI_STATS_SQ || epis == LF_EPI_ADD || epis == LF_EPI_RELU)) {
        // 16 output channels from whole 32-channel steps (round 6: the sub-pixel phases of UpsamplerBlock(64, 16) and the data gradient
        // of DownsamplerBlock(16, 64)'s convolution: 8 launches per step on the run-time-flag form before): padding as out-of-range
        // offsets, compiled-in epilogue.  In a partial last step (48 source channels) the lanes of channels 48..63 hold the out-of-range
        // offset too: zeros against the zero-padded weights, not the pixel's next channels (another tensor's slice)
        if (epis == 0) launch_bf16_stream<1, 0, 0, true>(grid, st, g, a, pro, epi);
        else if (epis == LF_EPI_STATS_SQ) launch_bf16_stream<1, 0, LF_EPI_STATS_SQ, true>(grid, st, g, a, pro, epi);
        else if (epis == LF_EPI_RELU) launch_bf16_stream<1, 0, LF_EPI_RELU, true>(grid, st, g, a, pro, epi);   // (inference: folded phases)
        else launch_bf16_stream<1, 0, LF_EPI_ADD, true>(grid, st, g, a, pro, epi);
        if (g.Cs % 32 != 0) ++g_part_fast_launches;
    } else {
        switch (nt) {
            case 4: launch_bf16_stream_rt<4>(grid, st, g, a, pro, epi); break;
            case 3: launch_bf16_stream_rt<3>(grid, st, g, a, pro, epi); break;
            case 2: launch_bf16_stream_rt<2>(grid, st, g, a, pro, epi); break;
            default: launch_bf16_stream_rt<1>(grid, st, g, a, pro, epi); break;
        }
    }
    LF_CHECK_LAUNCH("tapgemm_bf16");
    return 0;
}
