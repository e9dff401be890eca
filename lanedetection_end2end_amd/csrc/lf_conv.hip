// Tap-GEMM convolution kernels for gfx950 (see lf_conv.h for the contract).
//
// Matrix-core mapping (v_mfma_f32_16x16x4_f32, exact fp32, D = A*B + C, wave64):
//   A[i][k]: lane l supplies row i = l&15, k-slot kq = l>>4      -> weights / x-channels
//   B[k][j]: lane l supplies col j = l&15, k-slot kq = l>>4      -> pixels / g-channels
//   D[i][j]: lane l holds rows 4*(l>>4)+e (e = 0..3), col l&15
// Forward/dgrad: rows = output channels, cols = 16 pixels, k = source channels.  Each lane
// loads ONE float4 = 4 consecutive channels (16*cg + 4*kq + s, s = 0..3) of its pixel / of its
// weight row and feeds MFMA step s with element s: the k order is permuted identically on both
// operands, which a contraction does not care about.  A pixel's 16 channels (64 B) are read by 4
// lanes, a 16-pixel tile by one wave instruction; accumulators come out as 4 consecutive output
// channels per lane -> one float4 store per (tile, lane).  No LDS: operands stream from L1/L2
// straight into VGPRs, one (tap, 16-channel) step prefetched ahead of the MFMAs that use it.
// fp32 MFMA runs at the vector rate (157 TF), 1/16 of bf16, so one dwordx4 per operand tile per
// 16 MFMAs (512 cycles) is far below what the load path sustains.
//
// Kernels in this file:
//   tapgemm_kernel            fp32 matrix cores, operands streamed L2 -> VGPR: the 64- / 128-channel launches of the network
//   tapstream_kernel          fp32, the 3-tap convolutions at 64 / 128 channels: weights resident in LDS, pixels streamed past them
//   tapgemm_thin_kernel       tapgemm_kernel re-tiled (one 16-pixel tile per wave) for launches that cannot fill the device: one frame
//   tapgemm_lean_kernel       16-channel layers in fp32 (HBM-bound)
//   tapgemm_split_kernel      precision mode fp32x9: fp32 results from exact 3-way bf16 splits on the bf16 matrix cores
// All five take fp32 tensors; lf_tapgemm_launch, at the end of the file, routes a launch to one of them or, for bf16 tensors, to
// lf_tapgemm_bf16_route.  The kernels on bf16 tensors and that route are in lf_conv_bf16.hip, the weight gradients with their
// split-K reductions in lf_wgrad.hip, the weight-packing and BatchNorm-fold kernels in lf_pack.hip; the device helpers and launch
// helpers shared with lf_conv_bf16.hip and lf_wgrad.hip are in lf_conv_dev.h.
// The tap-GEMM kernels of both files share one epilogue (LF_TAPGEMM_EPILOGUE, lf_conv_epi.h: bias, ReLU, masks, residual, BN sums).
// tapstream_kernel's tile body is stream_tile in lf_conv_stream.h, which the fused forward pair (lf_conv_pair.hip) runs too.
#include "lf_conv_dev.h"
#include "lf_conv_epi.h"
#include "lf_conv_stream.h"

namespace {

constexpr size_t LF_TAP_LDS_PER_TAP = (size_t)WG_WAVES * 64 * (sizeof(uint4) + sizeof(unsigned));

// EPIC >= 0: the epilogue flags are compiled in (the combinations the network uses at 64 output channels per workgroup); the
// epilogue of one wave runs beside its partner's MFMA stream at ~14 cycles per VALU instruction, so the ~1500 instructions of
// the runtime-flag form (EPIC = -1) cost 9 us of a 30 us workgroup life -- and the slot it occupies cannot be refilled.
// (A one-operand-set form at <= 128 registers, four workgroups per CU so that the 4096 waves of a 64-channel launch run as ONE
// round, was measured and dropped: 72 vs 68 us -- three waves per SIMD of this form already overlap rounds.)
// ROW1 (Wl % 64 == 0): a wave's 64 pixels lie in one image row, so (image, row, first column) are wave-uniform and live in
// scalar registers: two divisions instead of eight in the prologue and ~10 vector registers less.
// DBG: per-wave phase stamps (tools/kbench.py --phases); compiled only into the instantiation lf_debug_conv1d_fwd_phases launches
// (the run-time-flag forms -- cold paths: the --clas trunk, kernel-level tests -- hold the union of all epilogue state beside the
// two accumulator sets and are given the whole register file, one wave per SIMD, instead of spilling 14-21 registers)
template <int NT, int PROC, int EPIC = -1, bool ROW1 = false, bool DBG = false>
__global__ __launch_bounds__(256, (EPIC >= 0 || NT < 4) ? 2 : 1) void tapgemm_kernel(const LfTapGeom g, const LfTapArgs a, const int pro, const int epi_rt) {
    const int epi = EPIC >= 0 ? EPIC : epi_rt;
    constexpr bool S16 = false, HOISTV = EPIC >= 0;  // compiled-in flags: the per-channel vectors are loaded once, after the loop
    unsigned long long tstamp[4] = {0ull, 0ull, 0ull, 0ull};
    if constexpr (DBG) tstamp[0] = __builtin_amdgcn_s_memrealtime();
    const unsigned npix = (unsigned)(g.N * g.Hl * g.Wl);       // < 2^31, checked by the launcher
    // Workgroup b runs on XCD b % 8 (observed dispatch order).  Give every XCD a CONTIGUOUS range of pixel
    // tiles so that the halo rows neighbouring tiles share (and both halves of blockIdx.y) meet in one L2.
    // (A persistent loop over tiles and a 3-set operand ring were measured and dropped: at batch 32 every
    // layer is one or two rounds of resident workgroups, and the extra live state cost more than it hid.)
    // Round 3: the grid is sized to the workgroups the chip holds at once (launcher: occupancy x CUs) and a workgroup walks its
    // tiles first, first + stride, ... -- so WHICH workgroup (hence which CU: they are dealt breadth-first) processes the tiles
    // beyond the first round is fixed by construction, one extra tile per CU.  Left to the dispatcher, the 256 second-round
    // workgroups of a 64-channel launch (1024 workgroups, 768 resident) went to whichever CUs retired workgroups first: with the
    // three co-resident workgroups of a CU finishing together, a third of the CUs took three more and the rest none -- 71.5
    // instead of 58.5 us, decided by details as small as dead code behind the epilogue (r3 A/B runs, tools/ab_conv.py).
    const int cob = blockIdx.y * NT * 16;
    const unsigned ntiles = (npix + PIX_PER_WG - 1) / PIX_PER_WG;
    unsigned t_first = blockIdx.x, t_stride = gridDim.x, t_end = ntiles;
    if ((gridDim.x & 7u) == 0 && (ntiles & 7u) == 0) {
        const unsigned per = ntiles >> 3;
        t_first = (blockIdx.x & 7u) * per + (blockIdx.x >> 3); t_stride = gridDim.x >> 3; t_end = (blockIdx.x & 7u) * per + per;
    }
    for (unsigned bx = t_first; bx < t_end; bx += t_stride) {
    // (the thread index is laundered per tile: hoisted out of the tile loop, the per-lane constants derived from it would
    // stay live across the whole body -- 10-20 registers, the difference between three and two waves per SIMD)
    unsigned tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    const int lane = tid & 63, wave = tid >> 6;
    const int pl = lane & 15, kq = lane >> 4;
    const unsigned tile0 = (bx * WG_WAVES + (ROW1 ? __builtin_amdgcn_readfirstlane(wave) : wave)) * (MT * 16);

    int pn[MT], pi[MT], pj[MT];
    bool pv[MT];
    if constexpr (ROW1) {
        const unsigned q = tile0 < npix ? tile0 : 0u;
        const unsigned r = q / (unsigned)g.Wl;
        const int j0 = __builtin_amdgcn_readfirstlane((int)(q - r * (unsigned)g.Wl));
        const int n0 = __builtin_amdgcn_readfirstlane((int)(r / (unsigned)g.Hl));
        const int i0 = __builtin_amdgcn_readfirstlane((int)r) - n0 * g.Hl;
#pragma unroll
        for (int m = 0; m < MT; ++m) { pv[m] = tile0 < npix; pn[m] = n0; pi[m] = i0; pj[m] = j0 + m * 16 + pl; }
    } else {
#pragma unroll
        for (int m = 0; m < MT; ++m) {   // 32-bit divisions: the 64-bit ones expand to ~100 instructions each
            const unsigned p = tile0 + m * 16 + pl;
            pv[m] = p < npix;
            const unsigned q = pv[m] ? p : 0u;
            const unsigned r = q / (unsigned)g.Wl;
            pj[m] = (int)(q - r * (unsigned)g.Wl);
            pn[m] = (int)(r / (unsigned)g.Hl);
            pi[m] = (int)(r - (unsigned)pn[m] * (unsigned)g.Hl);
        }
    }

    // Two accumulator sets (round 4): `acc` holds the running chain of ONE pair of K-steps (32 products per element), `accl`
    // the sum of the finished pairs.  One fp32 fma chain over the whole contraction (K = 192 at 64 channels, 384 at 128) left
    // the logits ~1.25x further from fp64 than oneDNN's fp32 convolution; tools/accum_study.py reproduces that on the CPU with
    // the kernel's summation order emulated (1.31x) and shows where it comes from (the 64-channel layers' K = 192 chain; the
    // folded BatchNorm and the fp32 statistics partials do not matter) and what removes it: 32-term segments summed into a
    // second accumulator -> 0.90x.  The flush is a VALU add per accumulator register and pair, issued between the MFMAs that
    // restart the chain from a zero C operand; the 64 extra registers put every variant at two waves per SIMD.
    f32x4 acc[NT][MT], accl[NT][MT];
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int m = 0; m < MT; ++m) { acc[n][m] = zero4(); accl[n][m] = zero4(); }

    const int ncg = g.Cs >> 4;
    const int nsteps = g.ntaps * ncg;

    {
        // Branch-free main loop.  Per-tap source offsets and validity bits are computed ONCE
        // into an LDS table (one 16-byte row per lane and tap); the loop body is one basic block of two
        // K-steps (128 MFMAs + ~20 loads) with scalar selects for the (tap, channel-group) counters, so the
        // accumulators stay in place and the scheduler is free to sink loads between MFMAs.  Steps past the
        // end (odd step counts) are issued with clamped addresses and a zero mask.
        struct Step { f32x4 w[NT]; f32x4 x[MT]; f32x4 sc, sh; unsigned ok; };
        // (dynamic LDS, 5 KB per tap: the static 9-tap table was 46 KB and capped the CU at 3 workgroups)
        uint4 (*tab_off)[64] = reinterpret_cast<uint4 (*)[64]>(lf_tap_lds) + wave * g.ntaps;
        unsigned (*tab_ok)[64] = reinterpret_cast<unsigned (*)[64]>(lf_tap_lds + (size_t)WG_WAVES * g.ntaps * 64 * sizeof(uint4)) + wave * g.ntaps;
        // PROC == 0: a padding position holds the out-of-range offset LF_OOB, the buffer load returns the zero itself;
        // with the BN+ReLU prologue (transform(0) != 0) the offsets are clamped and the mask is applied after the transform.
        for (int t = 0; t < g.ntaps; ++t) {
            const int dh = g.tdh[t], dw = g.tdw[t];
            unsigned o[MT], okb = 0;
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                const int sy = pi[m] * g.ssh + dh, sx = pj[m] * g.ssw + dw;
                const bool in = pv[m] && sy >= 0 && sy < g.Hs && sx >= 0 && sx < g.Ws;
                const int syc = min(max(sy, 0), g.Hs - 1), sxc = min(max(sx, 0), g.Ws - 1);
                o[m] = (unsigned)(((pn[m] * g.Hs + syc) * g.Ws + sxc) * g.s_pix + g.s_choff + kq * 4) * 4u;
                if (PROC == 0 && !in) o[m] = LF_OOB;
                okb |= (in ? 1u : 0u) << m;
            }
            tab_off[t][lane] = make_uint4(o[0], o[1], o[2], o[3]);
            tab_ok[t][lane] = okb;
        }
        // (each lane reads back only what it wrote: no barrier needed)
        const __amdgpu_buffer_rsrc_t rx = make_rsrc(a.src, (unsigned)min((long)g.N * g.Hs * g.Ws * g.s_pix * 4, (long)LF_OOB));
        const __amdgpu_buffer_rsrc_t rw = make_rsrc(a.wp, 0xffffffffu), rsc = make_rsrc(a.pro_sc, 0xffffffffu), rsh = make_rsrc(a.pro_sh, 0xffffffffu);
        const unsigned wlane = (unsigned)(kq * g.Cd + cob + pl) * 16u;      // bytes
        const int wstep = g.Cd * 64;                       // bytes per 16-channel step
        const int ntaps = g.ntaps;
        const int wlast = (nsteps - 1) * wstep;
        int t_ld = 0, cg_ld = 0, wofs = 0;
        auto issue = [&](Step& S) {
            const bool live = t_ld < ntaps;
            const int tc = live ? t_ld : ntaps - 1;
            uint4 o = tab_off[tc][lane];
            const unsigned okb = tab_ok[tc][lane];
#pragma unroll
            for (int n = 0; n < NT; ++n) S.w[n] = ldb4(rw, wlane + n * 256, (unsigned)wofs);
            const unsigned c16 = (unsigned)cg_ld * 64u;    // bytes
            if constexpr (PROC == 0) {                     // a dead step (odd step count) reads zeros
                const unsigned dead = live ? 0u : LF_OOB;
                o.x |= dead; o.y |= dead; o.z |= dead; o.w |= dead;
            }
            S.x[0] = ldb4(rx, o.x, c16);
            S.x[1] = ldb4(rx, o.y, c16);
            S.x[2] = ldb4(rx, o.z, c16);
            S.x[3] = ldb4(rx, o.w, c16);
            if constexpr (PROC == LF_PRO_BNRELU) { S.sc = ldb4(rsc, (unsigned)kq * 16u, c16); S.sh = ldb4(rsh, (unsigned)kq * 16u, c16); }
            S.ok = live ? okb : 0u;
            // advance (scalar selects, no branches); a dead step re-reads the last live operands
            const int cgn = cg_ld + 1;
            const bool wrap = cgn == ncg;
            wofs = min(wofs + wstep, wlast);                // a dead step re-reads the last live weights
            cg_ld = live ? (wrap ? 0 : cgn) : cg_ld;
            t_ld = (live && wrap) ? t_ld + 1 : t_ld;
        };
        auto finish = [&](Step& S) {
            if constexpr (PROC == LF_PRO_BNRELU) {
#pragma unroll
                for (int m = 0; m < MT; ++m) {
                    f32x4 v = max0(S.x[m] * S.sc + S.sh);
                    const bool in = (S.ok >> m) & 1u;
                    v.x = in ? v.x : 0.f; v.y = in ? v.y : 0.f; v.z = in ? v.z : 0.f; v.w = in ? v.w : 0.f;
                    S.x[m] = v;
                }
            }
        };
        auto mma = [&](const Step& S, int s) {
#pragma unroll
            for (int n = 0; n < NT; ++n)
#pragma unroll
                for (int m = 0; m < MT; ++m)
                    acc[n][m] = __builtin_amdgcn_mfma_f32_16x16x4f32(S.w[n][s], S.x[m][s], acc[n][m], 0, 0, 0);
        };
        // first quarter of a pair: every accumulator is flushed into the long-term set and its chain restarted (C = 0).  The
        // add of tile (n, m) reads what the LAST quarter of the previous pair wrote 16 MFMAs ago -- no dependency stall -- and
        // issues in the shadow of the neighbouring MFMAs.
        // (64-product segments -- the even / odd tiles flushing in turn, two pairs per iteration, half the adds -- were measured:
        // +0.45 % on the step, logits 0.92x instead of 0.85x; the 32-product form stays: DESIGN.md section 9)
        auto mma_restart = [&](const Step& S) {
#pragma unroll
            for (int n = 0; n < NT; ++n)
#pragma unroll
                for (int m = 0; m < MT; ++m) {
                    accl[n][m] += acc[n][m];
                    // (pinned: without the empty asm the IR passes sink all 64 adds behind the next loads, and the restarted
                    // chains then live in a THIRD register set beside the old one -- 256 registers, 13-65 of them spilled)
                    asm volatile("" : "+v"(accl[n][m]));
                    acc[n][m] = __builtin_amdgcn_mfma_f32_16x16x4f32(S.w[n][0], S.x[m][0], zero4(), 0, 0, 0);
                    __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);      // 2 VALU (v_pk_add_f32 x 2) ...
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);      // ... then this tile's MFMA
                }
        };
        static_assert(MT == 4, "tab_off packs 4 pixel tiles");
        if constexpr (DBG) tstamp[1] = __builtin_amdgcn_s_memrealtime();
        Step A, B;
        issue(A);
        finish(A);
        const int npairs = (nsteps + 1) >> 1;
        // (Priority falling with progress makes the two waves of a SIMD finish together instead of ~12 us apart -- measured
        // neutral at 128 channels and 15 % SLOWER at 64, where a third / fourth wave waits for the slot of the first finisher.)
        // Step order, pinned by scheduling fences: first quarter of this step's MFMAs, the next step's loads, two more quarters,
        // then the operand prologue of the next step (BN+ReLU / BatchNorm-backward transform: pure VALU work on the OTHER
        // register set, its loads had 32 MFMAs to land) interleaved with the last quarter -- the prologue's VALU instructions
        // issue in the shadow of MFMAs instead of in front of them.  (Where the loads sit inside the step does not matter at
        // three waves per SIMD: r3 sweep over six positions.)
        for (int pr = 0; pr < npairs; ++pr) {
            mma_restart(A);
            __builtin_amdgcn_sched_barrier(0);
            issue(B);                                   // (behind the first quarter: its eight dead operand registers are reused)
            __builtin_amdgcn_sched_barrier(0);
            mma(A, 1); mma(A, 2);
            __builtin_amdgcn_sched_barrier(0);
            finish(B);
            mma(A, 3);
            __builtin_amdgcn_sched_barrier(0);
            mma(B, 0);
            __builtin_amdgcn_sched_barrier(0);
            issue(A);
            __builtin_amdgcn_sched_barrier(0);
            mma(B, 1); mma(B, 2);
            __builtin_amdgcn_sched_barrier(0);
            finish(A);
            mma(B, 3);
            __builtin_amdgcn_sched_barrier(0);
        }
    }

#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int m = 0; m < MT; ++m) acc[n][m] += accl[n][m];
    if constexpr (!ROW1) {
        // per-lane pixel coordinates are RECOMPUTED for the epilogue (from a laundered thread index, so that the compiler cannot
        // keep the prologue's copies): 16 registers that would otherwise live across the main loop, where two accumulator sets
        // and two operand sets leave no room for them (24-32 registers spilled around the loop in the BatchNorm-backward-sum
        // variants).  The ROW1 form holds them in scalar registers.
        unsigned tid2 = threadIdx.x;
        asm volatile("" : "+v"(tid2));
        const unsigned tile0b = (bx * WG_WAVES + (tid2 >> 6)) * (MT * 16);
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const unsigned p = tile0b + m * 16 + (tid2 & 15u);
            pv[m] = p < npix;
            const unsigned q = pv[m] ? p : 0u;
            const unsigned r = q / (unsigned)g.Wl;
            pj[m] = (int)(q - r * (unsigned)g.Wl);
            pn[m] = (int)(r / (unsigned)g.Hl);
            pi[m] = (int)(r - (unsigned)pn[m] * (unsigned)g.Hl);
        }
    }
    if constexpr (DBG) {   // make the stamp wait for the last MFMA: touch one accumulator
        asm volatile("" ::"v"(acc[0][0][0]));
        tstamp[2] = __builtin_amdgcn_s_memrealtime();
    }
#undef LF_EPI_ONE_TILE
#define LF_EPI_ONE_TILE (!ROW1 && EPIC == (LF_EPI_ADD | LF_EPI_MASK | LF_EPI_STATS_XHAT))
#undef LF_EPI_TID
#define LF_EPI_TID tid
#undef LF_EPI_ROW1
#define LF_EPI_ROW1 ROW1
    LF_TAPGEMM_EPILOGUE
#undef LF_EPI_ONE_TILE
#define LF_EPI_ONE_TILE false
#undef LF_EPI_TID
#define LF_EPI_TID threadIdx.x
#undef LF_EPI_ROW1
#define LF_EPI_ROW1 false
    if (stats && bx + t_stride < t_end) __syncthreads();      // the statistics staging area is reused by the next tile
    __builtin_amdgcn_s_setprio(0);
    }   // tiles of this workgroup
    if constexpr (DBG) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        tstamp[3] = __builtin_amdgcn_s_memrealtime();
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        if (lane == 0 && a.dbg) {
            unsigned long long* d = a.dbg + ((unsigned long long)(blockIdx.y * gridDim.x + blockIdx.x) * WG_WAVES + wave) * 8;
            d[0] = tstamp[0]; d[1] = tstamp[1]; d[2] = tstamp[2]; d[3] = tstamp[3];
            unsigned hwid, xcc;                   // which SIMD the wave ran on (tools/kbench.py --phases pairs the waves up)
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
            d[4] = (unsigned long long)hwid | ((unsigned long long)xcc << 32);
        }
    }
}

// ---------------------------------------------------------------------------------------
// tapstream_kernel: the fp32 3-tap C -> C convolutions and data gradients (C = CS = 64 or 128, Wl % 64 == 0) with the weights
// RESIDENT IN LDS and the pixels streamed past them.  Ownership is tapgemm_kernel's -- a 4-wave group owns a 256-pixel tile, a wave
// 64 pixels x 64 output channels, tiles walked inside the XCD's contiguous range, one statistics row per tile -- but a wave computes
// its 64 pixels as FOUR 16-pixel sub-tiles in turn (16 + 16 accumulator registers instead of 64 + 64) against weights copied once
// per workgroup (48 KB at 64 channels, 96 KB at 128): the tile body is stream_tile (lf_conv_stream.h), shared with tappair_kernel.
// This kernel is the walk around it: X runs through a register ring filled R K-steps ahead with buffer loads, and the ring wraps
// across the workgroup's tiles -- the tail of a tile requests the first K-steps of the next, so they are in flight while this
// tile's last epilogue runs.  A prefetch past the last tile reads the out-of-range offset (zeros; with the operand prologue: pixel
// 0 of the tensor, masked).  Results are tapgemm_kernel's bit for bit (tests/test_fp32_stream_gpu.py).
// G: 4-wave groups per workgroup (128 channels: one 512-thread workgroup per CU, its two groups own tiles 2u and 2u + 1).
template <int CS, int PROC, int EPIC, int G>
__global__ __launch_bounds__(256 * G, G == 1 ? 2 : 1) void tapstream_kernel(const LfTapGeom g, const LfTapArgs a) {
    constexpr int NS = 3 * (CS / 16), R = STREAM_R;
    constexpr bool stats = (EPIC & (LF_EPI_STATS_SQ | LF_EPI_STATS_XHAT)) != 0;
    const unsigned npix = (unsigned)(g.N * g.Hl * g.Wl);
    const int cob = blockIdx.y * 64;
    const unsigned ntiles = (npix + PIX_PER_WG - 1) / PIX_PER_WG, nunits = (ntiles + G - 1) / G;
    const XcdRange u = xcd_range(nunits);      // (see tapgemm_kernel: XCD-contiguous ranges)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int pl = lane & 15, kq = lane >> 4;
    const unsigned wtile = (unsigned)__builtin_amdgcn_readfirstlane(wave);
    f32x4* const wl = reinterpret_cast<f32x4*>(lf_tap_lds);
    float* const pvec = reinterpret_cast<float*>(wl + NS * 256);              // BN+ReLU operand prologue: scale [CS], shift [CS]
    const __amdgpu_buffer_rsrc_t rx = make_rsrc(a.src, (unsigned)min((long)g.N * g.Hs * g.Ws * g.s_pix * 4, (long)LF_OOB));

    // the first R K-steps of X are requested BEFORE the weights are copied: their latency runs under the copy
    f32x4 ring[R];
    StreamWT cur = stream_coords<G>(g, npix, wtile, u.first, u.first < u.end);
#pragma unroll
    for (int p = 0; p < R; ++p) ring[p] = stream_xload<CS, PROC>(g, rx, cur, p, pl, kq);
    stream_copy_weights<CS, 256 * G>(wl, a.wp, cob);
    if constexpr (PROC == LF_PRO_BNRELU) stream_copy_prologue<CS, 256 * G>(pvec, a);
    __syncthreads();

    for (unsigned bx = u.first; bx < u.end; bx += u.stride) {
        const StreamWT nxt = stream_coords<G>(g, npix, wtile, bx + u.stride, bx + u.stride < u.end);
        stream_tile<CS, PROC, EPIC, G, true>(g, a, wl, pvec, bx, ntiles, npix, cob, cur, rx, ring,
                                             [&](int p) { return stream_xload<CS, PROC>(g, rx, nxt, p, pl, kq); });
        if (stats && bx + u.stride < u.end) __syncthreads();      // the statistics staging area is reused by the next tile
        cur = nxt;
    }
}

// ---------------------------------------------------------------------------------------
// tapgemm_thin_kernel: tapgemm_kernel re-tiled for launches whose regular grid (256 pixels x 64 channels per workgroup) cannot
// fill the device -- one camera frame: 8 to 32 workgroups on 256 CUs.  A wave owns ONE 16-pixel tile and NT 16-channel slabs, a
// workgroup 64 consecutive logical pixels, blockIdx.y walks the slab groups, one workgroup per tile (no walk).  The general
// LfTapGeom (any tap count, strides, sub-pixel destination offsets, ragged Wl); no operand prologue, no statistics; the epilogues
// the inference schedules issue: bias + ReLU and bias + residual + ReLU (BRES).
// Every output element is tapgemm_kernel's bit for bit (tests/test_thin_conv_gpu.py): the same MFMA with the same operand roles
// and k-slot permutation, K-steps tap-major then 16-channel group, the chain restarted from a zero C operand at every pair of
// K-steps with accl += acc in front of it and acc + accl at the end, the zero-operand dead step of an odd step count (the last
// live weights against zeros), the shared epilogue text.  K is not split.
// A thin wave is alone on its SIMD, so nothing hides a load but the wave's own MFMAs: a ring of R K-steps of operands (4 * (NT + 1)
// registers per step) is in flight, R = LF_THIN_DEPTH / NT rounded to whole pairs of K-steps -- about the same bytes in flight
// whatever NT, a step's MFMA time growing with NT.  Depths 4, 8 and 16 were measured: 8.  The ring changes
// which registers a step's operands arrive in, not the order of the MFMAs: scheduling fences pin it.
#ifndef LF_THIN_DEPTH
#define LF_THIN_DEPTH 8
#endif
constexpr int thin_ring(int nt) {
    const int r = (LF_THIN_DEPTH / nt + 1) / 2 * 2;
    return r < 2 ? 2 : r;
}
template <int NT, int EPIC>
__global__ __launch_bounds__(256, 2) void tapgemm_thin_kernel(const LfTapGeom g, const LfTapArgs a) {
    constexpr int epi = EPIC, R = thin_ring(NT);
    constexpr bool S16 = false, HOISTV = true;
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
    // tapgemm_kernel's tap table, one pixel tile wide: this lane's source byte offset per tap, LF_OOB (reads as zeros) for padding
    __shared__ unsigned tab[WG_WAVES][LF_MAX_TAPS][64];
    for (int t = 0; t < g.ntaps; ++t) {
        const int sy = pi[0] * g.ssh + g.tdh[t], sx = pj[0] * g.ssw + g.tdw[t];
        const bool in = pv[0] && sy >= 0 && sy < g.Hs && sx >= 0 && sx < g.Ws;
        const int syc = min(max(sy, 0), g.Hs - 1), sxc = min(max(sx, 0), g.Ws - 1);
        const unsigned o = (unsigned)(((pn[0] * g.Hs + syc) * g.Ws + sxc) * g.s_pix + g.s_choff + kq * 4) * 4u;
        tab[wave][t][lane] = in ? o : LF_OOB;
    }
    // (each lane reads back only what it wrote: no barrier needed)
    f32x4 acc[NT][1], accl[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) { acc[n][0] = zero4(); accl[n] = zero4(); }
    // (both ahead of the loop: the round trips of the bias vector and of the residual run under it -- behind it, nothing would hide them)
    LF_EPI_HEAD
    f32x4 addv[NT];
    if constexpr ((EPIC & LF_EPI_ADD) != 0) {
        const unsigned db = (unsigned)(((pn[0] * g.Hd + pi[0] * g.dsh + g.dah) * g.Wd + pj[0] * g.dsw + g.daw) * g.d_pix + g.d_choff + cob + kq * 4);
#pragma unroll
        for (int n = 0; n < NT; ++n) addv[n] = epi_ld<S16>(r_add, db + n * 16);
    }
    {
        struct Step { f32x4 w[NT]; f32x4 x; };
        const __amdgpu_buffer_rsrc_t rx = make_rsrc(a.src, (unsigned)min((long)g.N * g.Hs * g.Ws * g.s_pix * 4, (long)LF_OOB));
        const __amdgpu_buffer_rsrc_t rw = make_rsrc(a.wp, 0xffffffffu);
        const unsigned wlane = (unsigned)(kq * g.Cd + cob + pl) * 16u;      // bytes
        const int ncg = g.Cs >> 4, ntaps = g.ntaps, nsteps = ntaps * ncg;
        const int wstep = g.Cd * 64, wlast = (nsteps - 1) * wstep;          // bytes per 16-channel step
        const int npad = (nsteps + 1) & ~1;                                 // an odd step count ends with a dead step
        int t_ld = 0, cg_ld = 0, wofs = 0;
        // the next K-step's operands -> S; past the last live step: the last live weights against zeros (tapgemm_kernel's dead step)
        auto issue = [&](Step& S) {
            const bool live = t_ld < ntaps;
            const unsigned o = tab[wave][live ? t_ld : ntaps - 1][lane] | (live ? 0u : LF_OOB);
#pragma unroll
            for (int n = 0; n < NT; ++n) S.w[n] = ldb4(rw, wlane + n * 256, (unsigned)wofs);
            S.x = ldb4(rx, o, (unsigned)cg_ld * 64u);
            const int cgn = cg_ld + 1;
            const bool wrap = cgn == ncg;
            wofs = min(wofs + wstep, wlast);
            cg_ld = live ? (wrap ? 0 : cgn) : cg_ld;
            t_ld = (live && wrap) ? t_ld + 1 : t_ld;
        };
        Step ring[R];
#pragma unroll
        for (int p = 0; p < R; ++p) issue(ring[p]);
        // one pair of K-steps = one 32-product chain; refill: each slot's next occupant, R K-steps ahead, behind its last MFMA
        auto pair = [&](Step& A, Step& B, auto refill) {
#pragma unroll
            for (int n = 0; n < NT; ++n) {    // the finished pair's chain joins the long-term sum, the next starts from C = 0
                accl[n] += acc[n][0];
                asm volatile("" : "+v"(accl[n]));
                acc[n][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(A.w[n][0], A.x[0], zero4(), 0, 0, 0);
            }
#pragma unroll
            for (int s = 1; s < 4; ++s)
#pragma unroll
                for (int n = 0; n < NT; ++n) acc[n][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(A.w[n][s], A.x[s], acc[n][0], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (decltype(refill)::value) issue(A);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int n = 0; n < NT; ++n) acc[n][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(B.w[n][s], B.x[s], acc[n][0], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (decltype(refill)::value) issue(B);
            __builtin_amdgcn_sched_barrier(0);
        };
        // whole turns of the ring in a loop without an early exit (one that joins the latch makes the compiler's wait counts at
        // the loop head assume the youngest load of every path: the ring drained once per turn), then the last, partial turn
        int base = 0;
        for (; base + R <= npad; base += R) {
#pragma unroll
            for (int j = 0; j < R; j += 2) pair(ring[j], ring[j + 1], std::true_type{});
        }
#pragma unroll
        for (int j = 0; j < R - 2; j += 2) {
            if (base + j >= npad) break;          // (wave-uniform)
            pair(ring[j], ring[j + 1], std::false_type{});
        }
    }
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[n][0] += accl[n];
#undef LF_EPI_LDADD
#define LF_EPI_LDADD(o) addv[((o) - dbase) >> 4]      /* the residual of channel tile n, loaded ahead of the loop */
    LF_EPI_TILE(0)
#undef LF_EPI_LDADD
#define LF_EPI_LDADD(o) epi_ld<S16>(r_add, o)
    LF_EPI_TAIL
}

// ---------------------------------------------------------------------------------------
// fp32 ON THE bf16 MATRIX CORES ("split" mode, LfTapArgs::split = 9).  gfx950 multiplies bf16 16x faster
// than fp32 (v_mfma_f32_16x16x32_bf16: 16 cycles for K = 32; v_mfma_f32_16x16x4_f32: 8 x 32 cycles for the same K),
// so an fp32 product is formed from bf16 pieces instead: every fp32 operand is split EXACTLY into three bf16 values
//     a = a_h + a_m + a_l,   a_h = bf16(a), a_m = bf16(a - a_h), a_l = bf16(a - a_h - a_m)      (8 + 8 + 8 mantissa bits)
// (both subtractions are exact in fp32, a_l is exact because at most 8 significant bits are left), and
//     a * b = sum_{i,j} a_i * b_j
// where each of the nine bf16 x bf16 products is exact in the fp32 accumulator; all nine are kept: the result is an fp32
// accumulation of exact products, the same contract as the fp32 FMA chain of tapgemm_kernel.  (A 6-term form that dropped
// a_m*b_l, a_l*b_m, a_l*b_l -- < 2^-24 |a b| together -- existed through round 5; no BASELINE configuration used it.)
// Tensors, accumulators, epilogue and statistics are fp32 as in mode 0.
// Cost per 64 x 64 x 32 wave step: 144 MFMAs x 16 cycles = 2304 cycles against 4096 on the fp32 cores.
// The pixel operand is split in registers (v_cvt_pk_bf16_f32 + exact residuals, ~5 VALU ops per element, issued in the
// shadow of the MFMAs); weights are split once per forward by the pack kernel ([tap][K/8][Cd][3][8] bf16) and, being
// 3x the bytes of the fp32 form, staged ONCE per workgroup and step through LDS (double-buffered, one barrier per step)
// instead of once per wave from L1, which would saturate the 64 B/clk L1 path at this MFMA rate.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ void split3(const f32x4 lo, const f32x4 hi, bf16x8& h, bf16x8& m, bf16x8& l) {
    f32x2 p[4] = {{lo.x, lo.y}, {lo.z, lo.w}, {hi.x, hi.y}, {hi.z, hi.w}};
    u32x4 uh, um, ul;
#pragma unroll
    for (int i = 0; i < 4; ++i) uh[i] = split_pair(p[i]);
#pragma unroll
    for (int i = 0; i < 4; ++i) um[i] = split_pair(p[i]);
#pragma unroll
    for (int i = 0; i < 4; ++i)     // what is left has at most 8 significant bits: the third conversion is exact
        ul[i] = __builtin_bit_cast(unsigned, __builtin_convertvector(p[i], bf16x2));
    h = __builtin_bit_cast(bf16x8, uh); m = __builtin_bit_cast(bf16x8, um); l = __builtin_bit_cast(bf16x8, ul);
}

// Workgroup = 512 threads = two 4-wave groups A (waves 0-3) and B (waves 4-7); waves w and w+4 share SIMD w.  A wave's
// step has a VALU part (split the 32 pixel values it loaded, issue the next loads) and a matrix part (144 MFMAs).
// Two waves running the same code in lockstep would both want the VALU, then both the matrix pipe; so B runs HALF A STEP
// behind A, phase-locked by the workgroup barrier: while A multiplies, B splits, and vice versa -- the matrix pipe of every
// SIMD always has exactly one wave streaming back-to-back MFMAs.  Group A also stages the weights: W[s+1] is written to
// the idle LDS buffer during A's split phase (B is reading W[s-1]'s successor W[s] from the other one).
#undef LF_EPI_GROUPS
#define LF_EPI_GROUPS 2
template <int NT, int PROC, int EPIC = -1, bool DBG = false>
__global__ __launch_bounds__(512, 2) void tapgemm_split_kernel(const LfTapGeom g, const LfTapArgs a, const int pro, const int epi_rt) {
    const int epi = EPIC >= 0 ? EPIC : epi_rt;      // compiled-in epilogue flags, as in tapgemm_kernel
    constexpr bool S16 = false, HOISTV = EPIC >= 0;
    constexpr int WAVES = 8;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int pl = lane & 15, kq = lane >> 4;
    const int grp = wave >> 2;
    unsigned long long tstamp[4] = {0ull, 0ull, 0ull, 0ull};
    if constexpr (DBG) tstamp[0] = __builtin_amdgcn_s_memrealtime();
    const unsigned npix = (unsigned)(g.N * g.Hl * g.Wl);
    const int cob = blockIdx.y * NT * 16;
    const unsigned bx = xcd_swizzle(blockIdx.x);
    const unsigned tile0 = (bx * WAVES + wave) * (MT * 16);

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

    struct Raw { f32x4 xl[MT], xh[MT]; f32x4 sc0, sc1, sh0, sh1; unsigned ok; };
    __shared__ uint4 tab_off[WAVES][LF_MAX_TAPS][64];
    __shared__ unsigned tab_ok[WAVES][LF_MAX_TAPS][64];
    __shared__ u32x4 wl[2][3][4][NT * 16];          // [buffer][piece][k-block of 8][output channel]: 16 B rows, conflict-free
    for (int t = 0; t < g.ntaps; ++t) {
        const int dh = g.tdh[t], dw = g.tdw[t];
        unsigned o[MT], okb = 0;
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const int sy = pi[m] * g.ssh + dh, sx = pj[m] * g.ssw + dw;
            const bool in = pv[m] && sy >= 0 && sy < g.Hs && sx >= 0 && sx < g.Ws;
            const int syc = min(max(sy, 0), g.Hs - 1), sxc = min(max(sx, 0), g.Ws - 1);
            o[m] = (unsigned)(((pn[m] * g.Hs + syc) * g.Ws + sxc) * g.s_pix + g.s_choff + kq * 8);
            okb |= (in ? 1u : 0u) << m;
        }
        tab_off[wave][t][lane] = make_uint4(o[0], o[1], o[2], o[3]);
        tab_ok[wave][t][lane] = okb;
    }
    const int ncb = g.Cs >> 5;                               // 32-channel steps per tap (launcher: Cs % 32 == 0)
    const int nsteps = g.ntaps * ncb;
    const int ntaps = g.ntaps;
    // weight staging by group A: thread -> (k-block, output channel) of the workgroup's NT*16-channel slab
    const int tid = threadIdx.x;
    const bool filler = tid < NT * 64;                       // NT = 4: exactly the 256 threads of group A
    const int f_kb = filler ? tid / (NT * 16) : 0, f_co = filler ? tid % (NT * 16) : 0;
    const u32x4* wsrc = reinterpret_cast<const u32x4*>(a.wp16) + ((long)f_kb * g.Cd + cob + f_co) * 3;
    const int wstep = g.Cd * 4 * 3;                          // u32x4 per 32-channel step
    int wstepi = 0;
    u32x4 wreg[3];
    auto wfetch = [&]() {
        const u32x4* p = wsrc + (long)min(wstepi, nsteps - 1) * wstep;
        wreg[0] = p[0]; wreg[1] = p[1]; wreg[2] = p[2];
        ++wstepi;
    };
    auto wstore = [&](int buf) {
        if (filler) { wl[buf][0][f_kb][f_co] = wreg[0]; wl[buf][1][f_kb][f_co] = wreg[1]; wl[buf][2][f_kb][f_co] = wreg[2]; }
    };
    const __amdgpu_buffer_rsrc_t rx = make_rsrc(a.src, 0xffffffffu), rsc = make_rsrc(a.pro_sc, 0xffffffffu),
                                 rsh = make_rsrc(a.pro_sh, 0xffffffffu);
    int t_ld = 0, cb_ld = 0;
    auto issue = [&](Raw& S) {
        const bool live = t_ld < ntaps;
        const int tc = live ? t_ld : ntaps - 1;
        const uint4 o = tab_off[wave][tc][lane];
        const unsigned okb = tab_ok[wave][tc][lane];
        const int c32 = cb_ld * 32;
        const unsigned cs = (unsigned)c32 * 4u;          // scalar byte offset of the channel step (buffer-addressed, see ldb4)
        S.xl[0] = ldb4(rx, o.x * 4u, cs); S.xh[0] = ldb4(rx, o.x * 4u + 16u, cs);
        S.xl[1] = ldb4(rx, o.y * 4u, cs); S.xh[1] = ldb4(rx, o.y * 4u + 16u, cs);
        S.xl[2] = ldb4(rx, o.z * 4u, cs); S.xh[2] = ldb4(rx, o.z * 4u + 16u, cs);
        S.xl[3] = ldb4(rx, o.w * 4u, cs); S.xh[3] = ldb4(rx, o.w * 4u + 16u, cs);
        if constexpr (PROC == LF_PRO_BNRELU) {
            const unsigned c8 = (unsigned)(kq * 8) * 4u;
            S.sc0 = ldb4(rsc, c8, cs); S.sc1 = ldb4(rsc, c8 + 16u, cs);
            S.sh0 = ldb4(rsh, c8, cs); S.sh1 = ldb4(rsh, c8 + 16u, cs);
        }
        S.ok = live ? okb : 0u;
        const int cbn = cb_ld + 1;
        const bool wrap = cbn == ncb;
        cb_ld = live ? (wrap ? 0 : cbn) : cb_ld;
        t_ld = (live && wrap) ? t_ld + 1 : t_ld;
    };
    static_assert(MT == 4, "tab_off packs 4 pixel tiles");
    static_assert(NT == 4, "group A (256 threads) stages a 64-channel weight slab");
    Raw R;
    bf16x8 xb[MT][3];
    if constexpr (DBG) tstamp[1] = __builtin_amdgcn_s_memrealtime();
    if (grp == 0) wfetch();       // W[0]
    issue(R);                     // pixels of step 0
    if (grp == 1) __syncthreads();            // B starts one phase late
    for (int step = 0; step < nsteps; ++step) {
        // ---- VALU phase: split this step's pixels, start the next loads; A publishes W[step]
        if (grp == 0) { wstore(step & 1); wfetch(); }
        if constexpr (PROC == LF_PRO_BNRELU) {
#pragma unroll
            for (int m = 0; m < MT; ++m) { R.xl[m] = max0(R.xl[m] * R.sc0 + R.sh0); R.xh[m] = max0(R.xh[m] * R.sc1 + R.sh1); }
        }
        if (__builtin_amdgcn_ballot_w64(R.ok != 15u) != 0ull) {      // wave-uniform: only tiles that touch the padding mask
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                const bool in = (R.ok >> m) & 1u;
                f32x4 lo = R.xl[m], hi = R.xh[m];
                lo.x = in ? lo.x : 0.f; lo.y = in ? lo.y : 0.f; lo.z = in ? lo.z : 0.f; lo.w = in ? lo.w : 0.f;
                hi.x = in ? hi.x : 0.f; hi.y = in ? hi.y : 0.f; hi.z = in ? hi.z : 0.f; hi.w = in ? hi.w : 0.f;
                R.xl[m] = lo; R.xh[m] = hi;
            }
        }
#pragma unroll
        for (int m = 0; m < MT; ++m) split3(R.xl[m], R.xh[m], xb[m][0], xb[m][1], xb[m][2]);
        issue(R);                 // next step's pixels (clamped / masked past the end) fly during the matrix phase
        // the split must be DONE before the barrier: without the scheduling fence hipcc sinks the whole VALU block
        // below s_barrier (register-only code is free to move), i.e. into this group's own matrix phase
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int pc = 0; pc < 3; ++pc) asm volatile("" ::"v"(xb[m][pc]));
        __builtin_amdgcn_sched_barrier(0);
        __syncthreads();
        __builtin_amdgcn_sched_barrier(0);
        // ---- matrix phase (the partner group is in its VALU phase)
        const int cur = step & 1;
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            const bf16x8 wh = __builtin_bit_cast(bf16x8, wl[cur][0][kq][n * 16 + pl]);
            const bf16x8 wm = __builtin_bit_cast(bf16x8, wl[cur][1][kq][n * 16 + pl]);
            const bf16x8 wo = __builtin_bit_cast(bf16x8, wl[cur][2][kq][n * 16 + pl]);
            // smallest terms first; consecutive MFMAs of one term go to four different accumulators
#pragma unroll
            for (int m = 0; m < MT; ++m) acc[n][m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wo, xb[m][2], acc[n][m], 0, 0, 0);
#pragma unroll
            for (int m = 0; m < MT; ++m) acc[n][m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wo, xb[m][1], acc[n][m], 0, 0, 0);
#pragma unroll
            for (int m = 0; m < MT; ++m) acc[n][m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wm, xb[m][2], acc[n][m], 0, 0, 0);
#pragma unroll
            for (int m = 0; m < MT; ++m) acc[n][m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wo, xb[m][0], acc[n][m], 0, 0, 0);
#pragma unroll
            for (int m = 0; m < MT; ++m) acc[n][m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh, xb[m][2], acc[n][m], 0, 0, 0);
#pragma unroll
            for (int m = 0; m < MT; ++m) acc[n][m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wm, xb[m][1], acc[n][m], 0, 0, 0);
#pragma unroll
            for (int m = 0; m < MT; ++m) acc[n][m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wm, xb[m][0], acc[n][m], 0, 0, 0);
#pragma unroll
            for (int m = 0; m < MT; ++m) acc[n][m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh, xb[m][1], acc[n][m], 0, 0, 0);
#pragma unroll
            for (int m = 0; m < MT; ++m) acc[n][m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh, xb[m][0], acc[n][m], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        __syncthreads();
        __builtin_amdgcn_sched_barrier(0);
    }
    if (grp == 0) __syncthreads();            // A pairs B's extra first barrier (B's last matrix phase)
    if constexpr (DBG) {
        asm volatile("" ::"v"(acc[0][0][0]));
        tstamp[2] = __builtin_amdgcn_s_memrealtime();
    }
#undef LF_EPI_PIVOT
#define LF_EPI_PIVOT (EPIC >= 0)
    LF_TAPGEMM_EPILOGUE
#undef LF_EPI_PIVOT
#define LF_EPI_PIVOT true
    if constexpr (DBG) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        tstamp[3] = __builtin_amdgcn_s_memrealtime();
        if (lane == 0 && a.dbg) {
            unsigned long long* d = a.dbg + ((unsigned long long)(blockIdx.y * gridDim.x + blockIdx.x) * WAVES + wave) * 8;
            d[0] = tstamp[0]; d[1] = tstamp[1]; d[2] = tstamp[2]; d[3] = tstamp[3];
        }
    }
}
#undef LF_EPI_GROUPS
#define LF_EPI_GROUPS 1

// Lean variant for 16-output-channel launches (the 128x256 stage, ~3 % of the FLOPs): these are HBM-bound
// (0.75*C = 12 FLOP/B), so the goal is bytes in flight, not MFMA issue: no operand ring, few registers,
// many waves per SIMD; the compiler is free to hoist the next step's loads.
// A wave of these launches is 48 MFMAs between a prologue and an epilogue of VALU work, 16 waves per SIMD in sequence: the
// index arithmetic IS the kernel.  PROC / EPIC compiled in (EPIC = -1: run-time flags); with Wl % 64 == 0 a wave's 64 pixels lie
// in one image row, so (image, row, first column) are wave-uniform: two divisions instead of eight, scalar row terms.
template <int NT, int PROC = -1, int EPIC = -1>
__global__ __launch_bounds__(256, 4) void tapgemm_lean_kernel(const LfTapGeom g, const LfTapArgs a, const int pro_rt, const int epi_rt) {
    constexpr bool S16 = false, HOISTV = EPIC >= 0;
    const int pro = PROC >= 0 ? PROC : pro_rt, epi = EPIC >= 0 ? EPIC : epi_rt;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int pl = lane & 15, kq = lane >> 4;
    const unsigned npix = (unsigned)(g.N * g.Hl * g.Wl);
    const int cob = blockIdx.y * NT * 16;
    unsigned bx = blockIdx.x;
    if ((gridDim.x & 7u) == 0) bx = (bx & 7u) * (gridDim.x >> 3) + (bx >> 3);
    const unsigned tile0 = (bx * WG_WAVES + __builtin_amdgcn_readfirstlane(wave)) * (MT * 16);
    int pn[MT], pi[MT], pj[MT];
    bool pv[MT];
    const bool onerow = (g.Wl & 63) == 0;
    if (onerow) {
        const unsigned q = tile0 < npix ? tile0 : 0u;                 // wave-uniform
        const unsigned r = q / (unsigned)g.Wl;
        const int j0 = (int)(q - r * (unsigned)g.Wl), n0 = (int)(r / (unsigned)g.Hl), i0 = (int)(r - (unsigned)n0 * (unsigned)g.Hl);
#pragma unroll
        for (int m = 0; m < MT; ++m) { pv[m] = tile0 < npix; pn[m] = n0; pi[m] = i0; pj[m] = j0 + m * 16 + pl; }
    } else {
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
    }
    f32x4 acc[NT][MT];
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int m = 0; m < MT; ++m) acc[n][m] = zero4();
    f32x4 seg[NT][MT];                 // running chain of the general path (see below)
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int m = 0; m < MT; ++m) seg[n][m] = zero4();
    const int ncg = g.Cs >> 4;
    const float* wp = a.wp + (long)(kq * g.Cd + cob + pl) * 4;
    // x: num_records = the tensor, so that LF_OOB reads as 0.0f (padding without masks when there is no prologue)
    const __amdgpu_buffer_rsrc_t rwl = make_rsrc(a.wp, 0xffffffffu),
                                 rxl = make_rsrc(a.src, (unsigned)min((long)g.N * g.Hs * g.Ws * g.s_pix * 4, (long)LF_OOB));
    const unsigned wlane = (unsigned)(kq * g.Cd + cob + pl) * 16u;
    if (g.Cs == 16 && g.ntaps == 3) {
        // the 16 -> 16 channel 1-D convs (24 launches per step): all three taps' operands are requested before the first
        // MFMA -- one memory round trip per wave instead of three (these launches are HBM-bound, a wave is ~0.2 us of MFMAs)
        f32x4 w3[3][NT], x3[3][MT];
        bool in3[3][MT];
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const int dh = g.tdh[t], dw = g.tdw[t];
#pragma unroll
            for (int n = 0; n < NT; ++n) w3[t][n] = ldb4(rwl, wlane + n * 256, (unsigned)(t * g.Cd * 64));
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                const int sy = pi[m] * g.ssh + dh, sx = pj[m] * g.ssw + dw;
                in3[t][m] = pv[m] && sy >= 0 && sy < g.Hs && sx >= 0 && sx < g.Ws;
                const int syc = min(max(sy, 0), g.Hs - 1), sxc = min(max(sx, 0), g.Ws - 1);
                const unsigned off = (unsigned)(((pn[m] * g.Hs + syc) * g.Ws + sxc) * g.s_pix + g.s_choff + kq * 4) * 4u;
                x3[t][m] = ldb4(rxl, (PROC == 0 && !in3[t][m]) ? LF_OOB : off, 0u);
            }
        }
        f32x4 sc = zero4(), sh = zero4();
        if (pro == LF_PRO_BNRELU) { sc = ldg4(a.pro_sc + kq * 4); sh = ldg4(a.pro_sh + kq * 4); }
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            if constexpr (PROC != 0) {
#pragma unroll
                for (int m = 0; m < MT; ++m) {
                    f32x4 v = x3[t][m];
                    if (pro == LF_PRO_BNRELU) v = max0(v * sc + sh);
                    v.x = in3[t][m] ? v.x : 0.f; v.y = in3[t][m] ? v.y : 0.f; v.z = in3[t][m] ? v.z : 0.f; v.w = in3[t][m] ? v.w : 0.f;
                    x3[t][m] = v;
                }
            }
            // one fma chain per TAP (16 products), the three summed afterwards: the summation-error rule of tapgemm_kernel
            // (segments of <= 32 products), here for the layers next to the logits
            f32x4 part[NT][MT];
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
                for (int n = 0; n < NT; ++n)
#pragma unroll
                    for (int m = 0; m < MT; ++m)
                        part[n][m] = __builtin_amdgcn_mfma_f32_16x16x4f32(w3[t][n][s4], x3[t][m][s4], s4 ? part[n][m] : zero4(), 0, 0, 0);
#pragma unroll
            for (int n = 0; n < NT; ++n)
#pragma unroll
                for (int m = 0; m < MT; ++m) acc[n][m] = t ? acc[n][m] + part[n][m] : part[n][m];
        }
    } else
    for (int t = 0; t < g.ntaps; ++t) {
        const int dh = g.tdh[t], dw = g.tdw[t];
        unsigned xo[MT];
        bool in[MT];
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const int sy = pi[m] * g.ssh + dh, sx = pj[m] * g.ssw + dw;
            in[m] = pv[m] && sy >= 0 && sy < g.Hs && sx >= 0 && sx < g.Ws;
            const int syc = min(max(sy, 0), g.Hs - 1), sxc = min(max(sx, 0), g.Ws - 1);
            xo[m] = (unsigned)(((pn[m] * g.Hs + syc) * g.Ws + sxc) * g.s_pix + g.s_choff + kq * 4);
        }
        for (int cg = 0; cg < ncg; ++cg) {
            f32x4 w[NT], x[MT];
#pragma unroll
            for (int n = 0; n < NT; ++n) w[n] = ldg4(wp + n * 64);
            wp += (long)g.Cd * 16;
#pragma unroll
            for (int m = 0; m < MT; ++m) x[m] = ldg4(a.src + xo[m] + cg * 16);
            if (pro == LF_PRO_BNRELU) {
                const f32x4 sc = ldg4(a.pro_sc + cg * 16 + kq * 4), sh = ldg4(a.pro_sh + cg * 16 + kq * 4);
#pragma unroll
                for (int m = 0; m < MT; ++m) x[m] = max0(x[m] * sc + sh);
            }
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                x[m].x = in[m] ? x[m].x : 0.f; x[m].y = in[m] ? x[m].y : 0.f;
                x[m].z = in[m] ? x[m].z : 0.f; x[m].w = in[m] ? x[m].w : 0.f;
            }
            // (a chain restarts every two channel groups = 32 products and is added into acc: tapgemm_kernel's rule)
            if ((cg & 1) == 0) {
#pragma unroll
                for (int n = 0; n < NT; ++n)
#pragma unroll
                    for (int m = 0; m < MT; ++m) { acc[n][m] += seg[n][m]; seg[n][m] = zero4(); }
            }
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int n = 0; n < NT; ++n)
#pragma unroll
                    for (int m = 0; m < MT; ++m)
                        seg[n][m] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[n][s], x[m][s], seg[n][m], 0, 0, 0);
        }
    }
    if (!(g.Cs == 16 && g.ntaps == 3)) {
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int m = 0; m < MT; ++m) acc[n][m] += seg[n][m];
    }
    LF_TAPGEMM_EPILOGUE
}

int g_split_any_size = 0;      // kernel-level tests only: let the split kernel take launches below its shipped size rule

int pick_nt(int Cd) {
    const int tiles = Cd / 16;
    if (tiles % 4 == 0) return 4;
    if (tiles % 3 == 0) return 3;
    if (tiles % 2 == 0) return 2;
    return 1;
}

}  // namespace

// (not in the anonymous namespace: lf_tapgemm_bf16_route counts its launches in the same object, declared in lf_conv.h)
std::atomic<long> g_bres_launches{0};   // compiled-in bias + residual + ReLU launches (lf_tapgemm_bias_residual_launches)

void lf_tapgemm_set_split_any_size(int v) { g_split_any_size = v; }
long lf_tapgemm_bias_residual_launches() { return g_bres_launches.load(); }

// launches the split kernel takes: whole 32-channel K-steps, 64-channel output slabs (NT = 4), whole 512-pixel
// workgroups (its two 4-wave groups each own one 256-pixel statistics row), 16-byte aligned pixels
bool lf_tapgemm_split_ok(const LfTapGeom& g) {
    const long npix = (long)g.N * g.Hl * g.Wl;
    // its 512-pixel workgroups run one per CU: a launch that cannot put one on (most of) the 256 CUs is faster on the fp32
    // cores with their 256-pixel workgroups, two per CU (batch 16: 1412 vs 1484 images/s before this rule)
    const long wgs = npix / (2 * PIX_PER_WG) * (g.Cd / 64);
    return g.Cs % 32 == 0 && g.Cd % 64 == 0 && g.s_pix % 4 == 0 && g.s_choff % 4 == 0 && npix % (2 * PIX_PER_WG) == 0 &&
           (wgs >= 192 || g_split_any_size);
}

int lf_tapgemm_stat_rows(const LfTapGeom& g) {
    const long npix = (long)g.N * g.Hl * g.Wl;
    return lf_cdiv(npix, PIX_PER_WG);
}
int lf_tapgemm_stat_rows_for(const LfTapGeom& g, const LfTapArgs& a) {
    (void)a;
    return lf_cdiv((long)g.N * g.Hl * g.Wl, PIX_PER_WG);
}

namespace {
// hipExtAnyOrderLaunch for the next fp32 launch (set by lf_tapgemm_launch_unordered): the dispatch packet carries no barrier
// bit, so the kernel may start while the PREVIOUS packet of the stream is still running -- its workgroups fill the slots the
// previous kernel's last workgroups leave (the caller guarantees the two are independent).
thread_local unsigned g_launch_flags = 0;
template <typename K>
void launch_tapgemm(K kernel, dim3 grid, size_t lds, hipStream_t st, const LfTapGeom& g, const LfTapArgs& a, int pro, int epi) {
    launch_resident(kernel, grid, 256, lds, 0, 0, g_launch_flags, st, g, a, pro, epi);
}
// tapstream_kernel (see there).  lf_debug_set_fp32_stream: mode 0 = tapgemm_kernel takes every launch, 1 = the shipped routing
// (g_stream_routed: which (channel count, variant) pairs were faster in the step); max_workgroups > 0 caps the grid, so that a
// workgroup walks several tiles at small shapes.  Mode 2 routes every variant the kernel is compiled for (A/B runs, tests).
std::atomic<int> g_stream_mode{1}, g_stream_cap{0};
enum { LF_STREAM_RELU = 1, LF_STREAM_STATS = 2, LF_STREAM_MASK = 4, LF_STREAM_PRO = 8, LF_STREAM_X48 = 16, LF_STREAM_X38 = 32 };   // X48, X38: 64 channels only
constexpr int g_stream_routed[2] = {LF_STREAM_RELU | LF_STREAM_STATS | LF_STREAM_MASK | LF_STREAM_PRO | LF_STREAM_X48 | LF_STREAM_X38,      // 64 channels
                                    0};     // 128 channels: one tile per wave at batch 32 -- the 96 KB copy is never amortised: +2 us alone, +2..5 in the step (with the per-tile epilogue head of stream_tile: level alone, the step not re-measured)
// false: the runtime refused the kernel's LDS budget on this device (nothing launched: the caller takes tapgemm_kernel)
template <int CS, int PROV, int EPIV>
bool launch_tapstream(hipStream_t st, const LfTapGeom& g, const LfTapArgs& a) {
    constexpr int G = CS == 128 ? 2 : 1;
    const size_t lds = (size_t)3 * (CS / 16) * 4096 + (PROV == LF_PRO_BNRELU ? 2 * CS * sizeof(float) : 0);
    const unsigned ntiles = (unsigned)lf_cdiv((long)g.N * g.Hl * g.Wl, PIX_PER_WG);
    return launch_resident(tapstream_kernel<CS, PROV, EPIV, G>, dim3((ntiles + G - 1) / G, CS / 64), 256 * G, lds, BIG_LDS,
                           (unsigned)g_stream_cap.load(), g_launch_flags, st, g, a);
}
template <int CS>
bool route_tapstream(int variant, hipStream_t st, const LfTapGeom& g, const LfTapArgs& a) {
    switch (variant) {
        case LF_STREAM_RELU: return launch_tapstream<CS, 0, LF_EPI_RELU>(st, g, a);
        case LF_STREAM_STATS: return launch_tapstream<CS, 0, LF_EPI_STATS_SQ>(st, g, a);
        case LF_STREAM_MASK: return launch_tapstream<CS, 0, LF_EPI_MASK>(st, g, a);
        case LF_STREAM_PRO: return launch_tapstream<CS, 1, LF_EPI_RELU>(st, g, a);
        case LF_STREAM_X48: if constexpr (CS == 64) return launch_tapstream<CS, 0, LF_EPI_MASKBN | LF_EPI_STATS_XHAT>(st, g, a); else return false;
        case LF_STREAM_X38: if constexpr (CS == 64) return launch_tapstream<CS, 0, LF_EPI_ADD | LF_EPI_MASK | LF_EPI_STATS_XHAT>(st, g, a); else return false;
        default: return false;
    }
}

// tapgemm_thin_kernel (see there).  lf_debug_set_thin: mode 0 = LfTapArgs::thin and the grid size decide, 2 = every launch the
// kernel is compiled for takes it; nt = 0: the launcher's choice, 1..4: that many slabs per wave where it divides Cd / 16.
std::atomic<int> g_thin_mode{0}, g_thin_nt{0};
std::atomic<long> g_thin_launches{0};
int device_cus() { return lf_tapgemm_device_cus(); }
// the forms the thin kernel is compiled for: no prologue, bias + ReLU or bias + residual + ReLU
bool thin_compiled(const LfTapArgs& a, int pro, int epis) {
    return pro == LF_PRO_NONE && ((epis == LF_EPI_RELU && a.bias) || epis == BRES);
}
int thin_pick_nt(const LfTapGeom& g) { return lf_tapgemm_thin_pick_nt(g, g_thin_nt.load()); }
template <int EPIV>
void launch_thin(const LfTapGeom& g, const LfTapArgs& a, hipStream_t st) {
    const int nt = thin_pick_nt(g);
    const dim3 grid((unsigned)lf_cdiv((long)g.N * g.Hl * g.Wl, WG_WAVES * 16), g.Cd / (16 * nt));
    switch (nt) {
        case 4: hipLaunchKernelGGL((tapgemm_thin_kernel<4, EPIV>), grid, dim3(256), 0, st, g, a); break;
        case 3: hipLaunchKernelGGL((tapgemm_thin_kernel<3, EPIV>), grid, dim3(256), 0, st, g, a); break;
        case 2: hipLaunchKernelGGL((tapgemm_thin_kernel<2, EPIV>), grid, dim3(256), 0, st, g, a); break;
        default: hipLaunchKernelGGL((tapgemm_thin_kernel<1, EPIV>), grid, dim3(256), 0, st, g, a); break;
    }
    ++g_thin_launches;
    if (EPIV == BRES) ++g_bres_launches;
}

// precision mode fp32x9: fp32 tensors, the weights packed as three bf16 terms (tapgemm_split_kernel)
int launch_split_route(const LfTapGeom& g, const LfTapArgs& a, int pro, int epi, int epis, long npix, hipStream_t st) {
    LF_REQUIRE(a.split == 9, "tapgemm: split must be 9 (got %d; the 6-term form was removed in round 6)", a.split);
    LfTapArgs b = a;
    b.wp16 = a.wp48;
    const dim3 grid2((unsigned)(npix / (2 * PIX_PER_WG)), g.Cd / 64);     // 512-pixel workgroups (two 4-wave groups)
    if (a.dbg) {       // phase stamps (tools/kbench.py --phases): the plain conv only
        LF_REQUIRE(pro == LF_PRO_NONE && epi == 0, "tapgemm: phase stamps are compiled into the plain convolution only");
        hipLaunchKernelGGL((tapgemm_split_kernel<4, 0, 0, true>), grid2, dim3(512), 0, st, g, b, pro, epi);
    } else {
        with_pro_epi<false>(pro, epi, epis, [&](auto p, auto e) {
            hipLaunchKernelGGL((tapgemm_split_kernel<4, decltype(p)::value, decltype(e)::value>), grid2, dim3(512), 0, st, g, b, pro, epi);
        });
    }
    LF_CHECK_LAUNCH("tapgemm_split");
    return 0;
}

// the run-time-flag tapgemm_kernel of the output slab widths below 64 channels
template <int NTV>
void launch_tapgemm_rt(dim3 grid, size_t tap_lds, hipStream_t st, const LfTapGeom& g, const LfTapArgs& a, int pro, int epi) {
    if (pro == LF_PRO_BNRELU) launch_tapgemm(tapgemm_kernel<NTV, 1>, grid, tap_lds, st, g, a, pro, epi);
    else launch_tapgemm(tapgemm_kernel<NTV, 0>, grid, tap_lds, st, g, a, pro, epi);
}

// precision mode fp32 (and the fp32x9 launches the split kernel does not take): fp32 tensors on the fp32 matrix cores
int launch_fp32_route(const LfTapGeom& g, const LfTapArgs& a, int pro, int epi, int epis, int nt, dim3 grid, hipStream_t st) {
    const size_t tap_lds = LF_TAP_LDS_PER_TAP * g.ntaps;
    if (a.dbg) {           // phase stamps (tools/kbench.py --phases): the plain 64-channel-slab convolution only
        LF_REQUIRE(nt == 4 && pro == LF_PRO_NONE && epi == 0 && !a.wp16, "tapgemm: phase stamps are compiled into the plain fp32 convolution only");
        if ((g.Wl & 63) == 0) hipLaunchKernelGGL((tapgemm_kernel<4, 0, 0, true, true>), grid, dim3(256), tap_lds, st, g, a, pro, epi);
        else hipLaunchKernelGGL((tapgemm_kernel<4, 0, 0, false, true>), grid, dim3(256), tap_lds, st, g, a, pro, epi);
        LF_CHECK_LAUNCH("tapgemm (stamps)");
        return 0;
    }
    // a launch of tapgemm_kernel's (64- / 128-channel slabs, the stride-2 layers, the up-sampler phases) that cannot put one
    // workgroup on every CU: the thin tiling, where the caller asks for it
    const int thin_mode = g_thin_mode.load();
    if ((a.thin || thin_mode == 2) && nt >= 2 && thin_compiled(a, pro, epis) &&
        (thin_mode == 2 || (long)grid.x * grid.y < device_cus())) {
        if (epis == BRES) launch_thin<BRES>(g, a, st);
        else launch_thin<LF_EPI_RELU>(g, a, st);
        LF_CHECK_LAUNCH("tapgemm_thin");
        return 0;
    }
    if (g_stream_mode.load() != 0 && nt == 4 && g.ntaps == 3 && g.Cs == g.Cd && (g.Cs == 64 || g.Cs == 128) && (g.Wl & 63) == 0) {
        // the 3-tap C -> C launches of the non_bottleneck_1d blocks: weights resident in LDS, pixels streamed (tapstream_kernel)
        const int variant = pro == LF_PRO_BNRELU ? (epi == LF_EPI_RELU ? LF_STREAM_PRO : 0)
                          : epis == LF_EPI_RELU ? LF_STREAM_RELU : epis == LF_EPI_STATS_SQ ? LF_STREAM_STATS : epis == LF_EPI_MASK ? LF_STREAM_MASK
                          : epis == (LF_EPI_MASKBN | LF_EPI_STATS_XHAT) ? LF_STREAM_X48 : epis == (LF_EPI_ADD | LF_EPI_MASK | LF_EPI_STATS_XHAT) ? LF_STREAM_X38 : 0;
        if (variant && (g_stream_mode.load() == 2 || (g_stream_routed[g.Cs == 128] & variant)) &&
            (g.Cs == 64 ? route_tapstream<64>(variant, st, g, a) : route_tapstream<128>(variant, st, g, a))) {
            LF_CHECK_LAUNCH("tapstream");
            return 0;
        }
    }
    switch (nt) {
        case 4:
            with_pro_epi<true>(pro, epi, epis, [&](auto p, auto e) {
                constexpr int P = decltype(p)::value, E = decltype(e)::value;
                if ((g.Wl & 63) == 0) launch_tapgemm(tapgemm_kernel<4, P, E, true>, grid, tap_lds, st, g, a, pro, epi);
                else launch_tapgemm(tapgemm_kernel<4, P, E, false>, grid, tap_lds, st, g, a, pro, epi);
                if constexpr (E == BRES) ++g_bres_launches;
            });
            break;
        case 3: launch_tapgemm_rt<3>(grid, tap_lds, st, g, a, pro, epi); break;
        case 2: launch_tapgemm_rt<2>(grid, tap_lds, st, g, a, pro, epi); break;
        default:
            with_pro_epi<true>(pro, epi, epis, [&](auto p, auto e) {
                constexpr int P = decltype(p)::value, E = decltype(e)::value;
                hipLaunchKernelGGL((tapgemm_lean_kernel<1, P, E>), grid, dim3(256), 0, st, g, a, pro, epi);
                if constexpr (E == BRES) ++g_bres_launches;
            });
            break;
    }
    LF_CHECK_LAUNCH("tapgemm");
    return 0;
}
}  // namespace

void lf_tapgemm_set_fp32_stream(int mode, int max_workgroups) { g_stream_mode = mode; g_stream_cap = max_workgroups > 0 ? max_workgroups : 0; }

int lf_tapgemm_device_cus() {
    static std::map<int, int> cache;
    const int dev = current_device();
    std::lock_guard<std::mutex> lock(g_launch_state_mutex);
    auto it = cache.find(dev);
    if (it != cache.end()) return it->second;
    int cus = 0;
    if (dev < 0 || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 1;
    return cache[dev] = cus;
}
// slabs per wave: the largest of 4, 3, 2, 1 dividing Cd / 16 that still gives one workgroup per CU, else 1
int lf_tapgemm_thin_pick_nt(const LfTapGeom& g, int forced) {
    const int slabs = g.Cd / 16;
    if (forced >= 1 && forced <= 4 && slabs % forced == 0) return forced;
    const long tiles = lf_cdiv((long)g.N * g.Hl * g.Wl, WG_WAVES * 16);
    for (int nt = 4; nt > 1; --nt)
        if (slabs % nt == 0 && tiles * (slabs / nt) >= lf_tapgemm_device_cus()) return nt;
    return 1;
}

void lf_tapgemm_set_thin(int mode, int nt) { g_thin_mode = mode == 2 ? 2 : 0; g_thin_nt = (nt >= 1 && nt <= 4) ? nt : 0; }
long lf_tapgemm_thin_launches() { return g_thin_launches.load(); }

int lf_tapgemm_launch_unordered(const LfTapGeom& g, const LfTapArgs& a, int pro, int epi, hipStream_t st) {
    g_launch_flags = hipExtAnyOrderLaunch;
    const int rc = lf_tapgemm_launch(g, a, pro, epi, st);
    g_launch_flags = 0;
    return rc;
}

int lf_tapgemm_launch(const LfTapGeom& g, const LfTapArgs& a, int pro, int epi, hipStream_t st) {
    LF_REQUIRE(g.Cs % 16 == 0 && g.Cd % 16 == 0, "tapgemm: channels must be multiples of 16 (Cs=%d Cd=%d)", g.Cs, g.Cd);
    LF_REQUIRE(g.s_pix % 4 == 0 && g.s_choff % 4 == 0 && g.d_pix % 4 == 0 && g.d_choff % 4 == 0, "tapgemm: unaligned channel layout");
    LF_REQUIRE(g.ntaps >= 1 && g.ntaps <= LF_MAX_TAPS, "tapgemm: bad tap count %d", g.ntaps);
    const long npix = (long)g.N * g.Hl * g.Wl;
    LF_REQUIRE(npix < (1L << 30), "tapgemm: too many pixels (%ld)", npix);
    const int nt = pick_nt(g.Cd);
    const dim3 grid(lf_cdiv(npix, PIX_PER_WG), g.Cd / (16 * nt));
    LF_REQUIRE((long)g.N * g.Hs * g.Ws * g.s_pix * 4 < (long)LF_OOB, "tapgemm: source tensor too large for 32-bit byte offsets");
    LF_REQUIRE((long)g.N * g.Hd * g.Wd * g.d_pix * 4 < (long)LF_OOB, "tapgemm: destination tensor too large for 32-bit byte offsets");
    const int epis = (epi == (LF_EPI_ADD | LF_EPI_RELU) && a.bias) ? BRES             // (see BRES)
                   : ((epi & (LF_EPI_MASK | LF_EPI_ADD | LF_EPI_MASKBN | LF_EPI_STATS_XHAT)) && a.bias) ? -2 : epi;
    LF_REQUIRE(!a.s16 || a.wp16, "tapgemm: bf16 tensors need the bf16 matrix-core kernel (wp16)");
    if (a.split && a.wp48 && !a.wp16 && lf_tapgemm_split_ok(g)) return launch_split_route(g, a, pro, epi, epis, npix, st);
    LF_REQUIRE(!a.s16 || (g.s_pix % 8 == 0 && g.s_choff % 8 == 0), "tapgemm: bf16 source layout must be 16-byte aligned per pixel");
    if (a.wp16) return lf_tapgemm_bf16_route(g, a, pro, epi, epis, npix, nt, grid, st);
    return launch_fp32_route(g, a, pro, epi, epis, nt, grid, st);
}
