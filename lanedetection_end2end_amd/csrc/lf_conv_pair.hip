// tappair_kernel: the two halves of a non_bottleneck_1d block's 3x1 -> 1x3 forward pair (lf_erfnet.hip, K_NB: cv[0] -> cv[1] and
// cv[2] -> cv[3]; fp32 tensors, C -> C channels) in ONE launch:
//     t = relu(conv_a(pro(x)) + bias_a)        3 taps along H, stored to its own tensor exactly as its own launch stores it
//     y = conv_b(t) + bias_b                   3 taps along W, with the per-tile BatchNorm statistics rows (LF_EPI_STATS_SQ)
// conv_b runs along W and a 4-wave group's tile is 256 consecutive pixels = whole image rows (256 % Wl == 0): every source pixel of
// conv_b lies in the tile the same group has just produced, whatever the dilation -- no halo, no recomputation, no workgroup ever
// waits for another.  t has to be written anyway (the backward pass reads it as a ReLU mask and as a weight-gradient operand), so
// it is the exchange medium itself: every wave drains its stores (vmcnt(0)), the workgroup passes a barrier (workgroup-scope
// release / acquire: the waves of a workgroup share one L1), and only then is t read back.  No operand of conv_b is requested
// before that barrier; nothing waits on another workgroup.
//
// Per-element arithmetic is that of the two launches it replaces (tapstream_kernel / tapgemm_kernel, lf_conv.hip): the same K
// order, the same 32-product segments flushed into the second accumulator set, the same epilogue text (lf_conv_epi.h), the same
// tile ownership and hence the same statistics rows: t, y and the rows are bit-identical (tests/test_fwd_pair_gpu.py).
//
// This file holds what is the pair's own: the two kernels' outer loops, the hand-over, pair128_phase, routing and launch.
//
// 64 channels: the stream tile body (stream_tile, lf_conv_stream.h: the one tapstream_kernel runs) twice per tile.  Both
// convolutions' weights stay resident in LDS (2 x 48 KB), which leaves room for one workgroup per CU: 512 threads, its two
// 4-wave groups own tiles 2u and 2u + 1 -- the same two waves per SIMD as two 256-thread tapstream workgroups.  Tile-major
// (conv_a, barrier, conv_b, next tile): t in flight between its store and its read is one tile per group, 4 MB per XCD at batch
// 32, half of what the phase-major order would hold against a 4 MB L2.  The X ring is filled afresh behind the barrier (conv_b)
// and, for the next tile's conv_a, during the tail of conv_b.
#include "lf_conv_stream.h"

namespace {

// lf_tappair_ok admits dense stride-1 CS -> CS tensors of the logical size only: with those fields written as constants the two
// geometries share (N, H, W) and differ in their three tap offsets -- the index arithmetic folds and the scalar registers hold six
// tap offsets instead of two whole descriptors (which spilled 40 of them).  The shared fields are set here; the tap offsets stay one
// line in each kernel (set in here too, tappair128_kernel's register allocation moves).
template <int CS>
__device__ __forceinline__ void pair_geoms(const LfTapGeom& ga_in, LfTapGeom& ga, LfTapGeom& gb) {
    ga.N = ga_in.N; ga.Hl = ga.Hs = ga.Hd = ga_in.Hl; ga.Wl = ga.Ws = ga.Wd = ga_in.Wl;
    ga.s_pix = ga.d_pix = ga.Cs = ga.Cd = CS; ga.s_choff = ga.d_choff = 0; ga.ntaps = 3;
    ga.ssh = ga.ssw = ga.dsh = ga.dsw = 1; ga.dah = ga.daw = 0;
    gb = ga;
}

// ga / aa: conv_a (along H, LF_EPI_RELU, PROC its operand prologue), gb / ab: conv_b (along W, LF_EPI_STATS_SQ); ab.src == aa.dst.
// G 4-wave groups per workgroup, group q of unit u owns tile u * G + q; units are walked as tapstream_kernel walks them.
template <int CS, int PROC, int G>
__global__ __launch_bounds__(256 * G, 1) void tappair_kernel(const LfTapGeom ga_in, const LfTapArgs aa, const LfTapGeom gb_in, const LfTapArgs ab) {
    constexpr int NS = 3 * (CS / 16), R = STREAM_R;
    LfTapGeom ga, gb;
    pair_geoms<CS>(ga_in, ga, gb);
#pragma unroll
    for (int t = 0; t < 3; ++t) { ga.tdh[t] = ga_in.tdh[t]; ga.tdw[t] = 0; gb.tdh[t] = 0; gb.tdw[t] = gb_in.tdw[t]; }
    const unsigned npix = (unsigned)(ga.N * ga.Hl * ga.Wl);
    const int cob = 0;
    const unsigned ntiles = (npix + PIX_PER_WG - 1) / PIX_PER_WG, nunits = (ntiles + G - 1) / G;
    const XcdRange u = xcd_range(nunits);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int pl = lane & 15, kq = lane >> 4;
    const unsigned wtile = (unsigned)__builtin_amdgcn_readfirstlane(wave);
    f32x4* const wla = reinterpret_cast<f32x4*>(lf_tap_lds);
    f32x4* const wlb = wla + NS * 256;
    float* const pvec = reinterpret_cast<float*>(wlb + NS * 256);             // BN+ReLU operand prologue of conv_a
    const __amdgpu_buffer_rsrc_t rxa = make_rsrc(aa.src, (unsigned)min((long)ga.N * ga.Hs * ga.Ws * ga.s_pix * 4, (long)LF_OOB));
    const __amdgpu_buffer_rsrc_t rxb = make_rsrc(ab.src, (unsigned)min((long)gb.N * gb.Hs * gb.Ws * gb.s_pix * 4, (long)LF_OOB));

    // the first R K-steps of conv_a's X are requested BEFORE the weights are copied: their latency runs under the copy
    // (the logical grids of the two convolutions are one, lf_tappair_ok: a wave's coordinates serve both)
    f32x4 ring[R];
    StreamWT cur = stream_coords<G>(ga, npix, wtile, u.first, u.first < u.end);
#pragma unroll
    for (int p = 0; p < R; ++p) ring[p] = stream_xload<CS, PROC>(ga, rxa, cur, p, pl, kq);
    stream_copy_weights<CS, 256 * G>(wla, aa.wp, cob);
    stream_copy_weights<CS, 256 * G>(wlb, ab.wp, cob);
    if constexpr (PROC == LF_PRO_BNRELU) stream_copy_prologue<CS, 256 * G>(pvec, aa);
    __syncthreads();

    for (unsigned bx = u.first; bx < u.end; bx += u.stride) {
        const StreamWT nxt = stream_coords<G>(ga, npix, wtile, bx + u.stride, bx + u.stride < u.end);
        stream_tile<CS, PROC, LF_EPI_RELU, G, false>(ga, aa, wla, pvec, bx, ntiles, npix, cob, cur, rxa, ring, [](int) { return zero4(); });
        // the hand-over: my stores of t have left, then everybody's have -- only now may any wave of the workgroup read t.  (It also
        // separates the previous tile's reads of the statistics staging area from this tile's writes.)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        // the X ring is filled afresh behind the barrier (conv_b) and, for the next tile's conv_a, during the tail of conv_b
#pragma unroll
        for (int p = 0; p < R; ++p) ring[p] = stream_xload<CS, 0>(gb, rxb, cur, p, pl, kq);
        stream_tile<CS, 0, LF_EPI_STATS_SQ, G, true>(gb, ab, wlb, pvec, bx, ntiles, npix, cob, cur, rxb, ring,
                                                      [&](int p) { return stream_xload<CS, PROC>(ga, rxa, nxt, p, pl, kq); });
        cur = nxt;
    }
}

// ---------------------------------------------------------------------------------------
// 128 channels: conv_b contracts over all 128 channels of t, so both 64-output-channel halves of a tile must come from one
// workgroup: 512 threads, 4-wave group q produces channels [64 q, 64 q + 64) of the tile, for both convolutions.  The weights
// (192 KB per convolution) do not fit LDS: operands are streamed L1 / L2 -> VGPR as tapgemm_kernel streams them, whose tile body
// (ROW1 form: tap table in LDS, two operand sets, two accumulator sets, the compiled-in epilogue) this is, twice per tile.  One
// workgroup per CU = the two waves per SIMD of tapgemm_kernel's two 256-thread workgroups.
//
// pair128_phase is a DELIBERATE COPY of tapgemm_kernel's ROW1 tile body (lf_conv.hip), not a shared function: called from both
// kernels as one __forceinline__ template, the body moved the register allocation of every tapgemm_kernel instantiation (228 ->
// 216-232 VGPRs, <3,0,-1> from 31 to 150 spilled SGPRs) and gave tappair128_kernel 308 bytes of scratch.  Any edit to either copy
// must be mirrored in the other (tests/test_fwd_pair_gpu.py compares them bit for bit).
constexpr size_t PAIR128_LDS = (size_t)2 * WG_WAVES * 3 * 64 * (sizeof(uint4) + sizeof(unsigned));      // tap tables of 8 waves

template <int PROC, int EPIC>
__device__ __forceinline__ void pair128_phase(const LfTapGeom& g, const LfTapArgs& a, const unsigned bx, const unsigned npix) {
    constexpr int NT = 4, NTAPS = 3;
    constexpr int epi = EPIC;
    constexpr bool S16 = false, HOISTV = true;
    unsigned tid = threadIdx.x;      // (laundered per phase, as tapgemm_kernel launders it per tile)
    asm volatile("" : "+v"(tid));
    const int lane = tid & 63, wave = tid >> 6;
    const int pl = lane & 15, kq = lane >> 4;
    const int cob = __builtin_amdgcn_readfirstlane(wave >> 2) * 64;
    const unsigned tile0 = (bx * WG_WAVES + (unsigned)(__builtin_amdgcn_readfirstlane(wave) & 3)) * (MT * 16);
    int pn[MT], pi[MT], pj[MT];
    bool pv[MT];
    {
        const unsigned q = tile0 < npix ? tile0 : 0u;
        const unsigned r = q / (unsigned)g.Wl;
        const int j0 = __builtin_amdgcn_readfirstlane((int)(q - r * (unsigned)g.Wl));
        const int n0 = __builtin_amdgcn_readfirstlane((int)(r / (unsigned)g.Hl));
        const int i0 = __builtin_amdgcn_readfirstlane((int)r) - n0 * g.Hl;
#pragma unroll
        for (int m = 0; m < MT; ++m) { pv[m] = tile0 < npix; pn[m] = n0; pi[m] = i0; pj[m] = j0 + m * 16 + pl; }
    }
    f32x4 acc[NT][MT], accl[NT][MT];
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int m = 0; m < MT; ++m) { acc[n][m] = zero4(); accl[n][m] = zero4(); }
    const int ncg = g.Cs >> 4;
    const int nsteps = NTAPS * ncg;
    {
        struct Step { f32x4 w[NT]; f32x4 x[MT]; f32x4 sc, sh; unsigned ok; };
        uint4 (*tab_off)[64] = reinterpret_cast<uint4 (*)[64]>(lf_tap_lds) + wave * NTAPS;
        unsigned (*tab_ok)[64] = reinterpret_cast<unsigned (*)[64]>(lf_tap_lds + (size_t)2 * WG_WAVES * NTAPS * 64 * sizeof(uint4)) + wave * NTAPS;
        for (int t = 0; t < NTAPS; ++t) {
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
        const int wlast = (nsteps - 1) * wstep;
        int t_ld = 0, cg_ld = 0, wofs = 0;
        auto issue = [&](Step& S) {
            const bool live = t_ld < NTAPS;
            const int tc = live ? t_ld : NTAPS - 1;
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
        // first quarter of a pair of K-steps: every accumulator is flushed into the long-term set and its chain restarted (C = 0)
        auto mma_restart = [&](const Step& S) {
#pragma unroll
            for (int n = 0; n < NT; ++n)
#pragma unroll
                for (int m = 0; m < MT; ++m) {
                    accl[n][m] += acc[n][m];
                    asm volatile("" : "+v"(accl[n][m]));      // (pinned: see tapgemm_kernel)
                    acc[n][m] = __builtin_amdgcn_mfma_f32_16x16x4f32(S.w[n][0], S.x[m][0], zero4(), 0, 0, 0);
                    __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                }
        };
        static_assert(MT == 4, "tab_off packs 4 pixel tiles");
        Step A, B;
        issue(A);
        finish(A);
        const int npairs = (nsteps + 1) >> 1;
        for (int pr = 0; pr < npairs; ++pr) {      // (step order and fences: tapgemm_kernel's)
            mma_restart(A);
            __builtin_amdgcn_sched_barrier(0);
            issue(B);
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
#undef LF_EPI_GROUPS
#define LF_EPI_GROUPS 2
#undef LF_EPI_TID
#define LF_EPI_TID tid
#undef LF_EPI_ROW1
#define LF_EPI_ROW1 true
#undef LF_EPI_TILE_OF
#define LF_EPI_TILE_OF(tg) (bx)
    LF_TAPGEMM_EPILOGUE
#undef LF_EPI_GROUPS
#define LF_EPI_GROUPS 1
#undef LF_EPI_TID
#define LF_EPI_TID threadIdx.x
#undef LF_EPI_ROW1
#define LF_EPI_ROW1 false
#undef LF_EPI_TILE_OF
#define LF_EPI_TILE_OF(tg) (bx * (unsigned)LF_EPI_GROUPS + (unsigned)(tg))
    __builtin_amdgcn_s_setprio(0);
}

template <int PROC>
__global__ __launch_bounds__(512, 1) void tappair128_kernel(const LfTapGeom ga_in, const LfTapArgs aa, const LfTapGeom gb_in, const LfTapArgs ab) {
    LfTapGeom ga, gb;
    pair_geoms<128>(ga_in, ga, gb);
#pragma unroll
    for (int t = 0; t < 3; ++t) { ga.tdh[t] = ga_in.tdh[t]; ga.tdw[t] = 0; gb.tdh[t] = 0; gb.tdw[t] = gb_in.tdw[t]; }
    const unsigned npix = (unsigned)(ga.N * ga.Hl * ga.Wl);
    const unsigned ntiles = (npix + PIX_PER_WG - 1) / PIX_PER_WG;
    unsigned t_first = blockIdx.x, t_stride = gridDim.x, t_end = ntiles;      // (xcd_range written out: with the call the kernel's text moves)
    if ((gridDim.x & 7u) == 0 && (ntiles & 7u) == 0) {
        const unsigned per = ntiles >> 3;
        t_first = (blockIdx.x & 7u) * per + (blockIdx.x >> 3); t_stride = gridDim.x >> 3; t_end = (blockIdx.x & 7u) * per + per;
    }
    for (unsigned bx = t_first; bx < t_end; bx += t_stride) {
        pair128_phase<PROC, LF_EPI_RELU>(ga, aa, bx, npix);
        // the hand-over (see tappair_kernel); it also separates the previous tile's reads of the statistics staging area from this
        // tile's writes
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        pair128_phase<0, LF_EPI_STATS_SQ>(gb, ab, bx, npix);
    }
}

// lf_debug_set_fwd_pair: mode 0 = the two launches, 1 = the shipped routing (g_pair_routed: the forms that lowered the step), 2 =
// every compiled form; max_workgroups > 0 caps the grid, so that one workgroup walks several tiles at small shapes
std::atomic<int> g_pair_mode{1}, g_pair_cap{0};
enum { PAIR_PLAIN = 1, PAIR_PRO = 2 };      // conv_a without / with the BN+ReLU operand prologue
constexpr int g_pair_compiled[2] = {PAIR_PLAIN | PAIR_PRO, PAIR_PLAIN | PAIR_PRO};      // [64 channels, 128 channels]
constexpr int g_pair_routed[2] = {PAIR_PLAIN | PAIR_PRO, PAIR_PLAIN | PAIR_PRO};

int pair_form(int pro) { return pro == LF_PRO_BNRELU ? PAIR_PRO : PAIR_PLAIN; }

template <int CS, int PROC, int G>
bool launch_tappair(const LfTapGeom& ga, const LfTapArgs& aa, const LfTapGeom& gb, const LfTapArgs& ab, hipStream_t st) {
    const size_t lds = (size_t)2 * 3 * (CS / 16) * 4096 + (PROC == LF_PRO_BNRELU ? 2 * CS * sizeof(float) : 0);
    const unsigned ntiles = (unsigned)lf_cdiv((long)ga.N * ga.Hl * ga.Wl, PIX_PER_WG);
    return launch_resident(tappair_kernel<CS, PROC, G>, dim3((ntiles + G - 1) / G), 256 * G, lds, BIG_LDS, (unsigned)g_pair_cap.load(), 0u,
                           st, ga, aa, gb, ab);
}

}  // namespace

void lf_tappair_set(int mode, int max_workgroups) { g_pair_mode = mode < 0 ? 0 : mode; g_pair_cap = max_workgroups > 0 ? max_workgroups : 0; }

bool lf_tappair_routed(int C, int pro) {
    if (C != 64 && C != 128) return false;
    const int mode = g_pair_mode.load();
    // 4 * m (A/B runs in the step): exactly the compiled forms of bit mask m = (64 channels) | (128 channels) << 2
    const int forms = mode == 0 ? 0 : mode == 1 ? g_pair_routed[C == 128] : mode >= 4 ? ((mode >> 2) >> (C == 128 ? 2 : 0)) & 3 : 3;
    return (forms & g_pair_compiled[C == 128] & pair_form(pro)) != 0;
}

bool lf_tappair_ok(const LfTapGeom& ga, const LfTapGeom& gb, const LfTapArgs& aa, const LfTapArgs& ab, int pro, int epi_a, int epi_b) {
    const int C = ga.Cs;
    if (!(C == 64 || C == 128) || !(g_pair_compiled[C == 128] & pair_form(pro))) return false;
    if (epi_a != LF_EPI_RELU || epi_b != LF_EPI_STATS_SQ || !(pro == LF_PRO_NONE || pro == LF_PRO_BNRELU)) return false;      // (training: the statistics epilogue)
    // fp32 tensors in precision mode 0
    if (aa.s16 || ab.s16 || aa.wp16 || ab.wp16 || aa.split || ab.split || aa.dbg || ab.dbg) return false;
    // two dense stride-1 C -> C convolutions over one logical grid, conv_b reading the tensor conv_a writes
    for (const LfTapGeom* g : {&ga, &gb})
        if (!(g->Cs == C && g->Cd == C && g->ntaps == 3 && g->ssh == 1 && g->ssw == 1 && g->dsh == 1 && g->dsw == 1 && g->dah == 0 && g->daw == 0 &&
              g->Hs == g->Hl && g->Hd == g->Hl && g->Ws == g->Wl && g->Wd == g->Wl && g->s_pix == C && g->d_pix == C && g->s_choff == 0 && g->d_choff == 0))
            return false;
    if (ga.N != gb.N || ga.Hl != gb.Hl || ga.Wl != gb.Wl || ga.N < 1 || ga.Hl < 1) return false;
    // conv_a along H, conv_b along W, each 3 taps about the pixel itself
    for (int t = 0; t < 3; ++t)
        if (ga.tdw[t] != 0 || gb.tdh[t] != 0) return false;
    if (ga.tdh[1] != 0 || gb.tdw[1] != 0) return false;
    // a 256-pixel tile is whole image rows, a wave's 64 pixels lie in one row
    if (ga.Wl < 64 || ga.Wl % 64 != 0 || 256 % ga.Wl != 0) return false;
    const long npix = (long)ga.N * ga.Hl * ga.Wl;
    if (npix >= (1L << 30) || npix * C * 4 >= (long)LF_OOB) return false;      // 32-bit byte offsets, the out-of-range offset beyond the tensors
    if (!aa.src || !aa.dst || !aa.wp || !ab.wp || !ab.dst || ab.src != aa.dst || aa.dst == aa.src || ab.dst == aa.dst || ab.dst == aa.src) return false;
    if ((pro == LF_PRO_BNRELU) != (aa.pro_sc != nullptr) || (aa.pro_sc != nullptr) != (aa.pro_sh != nullptr)) return false;
    if (!ab.stats || ab.stats_ld < lf_tapgemm_stat_rows(gb)) return false;
    if (C == 128) return true;
    return allow_big_lds(pro == LF_PRO_BNRELU ? reinterpret_cast<const void*>(tappair_kernel<64, 1, 2>) : reinterpret_cast<const void*>(tappair_kernel<64, 0, 2>), BIG_LDS);
}

int lf_tappair_launch(const LfTapGeom& ga, const LfTapGeom& gb, const LfTapArgs& aa, const LfTapArgs& ab, int pro, hipStream_t st) {
    LF_REQUIRE(lf_tappair_ok(ga, gb, aa, ab, pro, LF_EPI_RELU, LF_EPI_STATS_SQ), "tappair: the fused kernel does not take this pair (pro %d, %d x %d x %d x %d)",
               pro, ga.N, ga.Hl, ga.Wl, ga.Cs);
    bool launched;
    if (ga.Cs == 128) {
        const dim3 grid((unsigned)lf_cdiv((long)ga.N * ga.Hl * ga.Wl, PIX_PER_WG));
        const unsigned cap = (unsigned)g_pair_cap.load();
        launched = pro == LF_PRO_BNRELU ? launch_resident(tappair128_kernel<1>, grid, 512, PAIR128_LDS, 0, cap, 0u, st, ga, aa, gb, ab)
                                        : launch_resident(tappair128_kernel<0>, grid, 512, PAIR128_LDS, 0, cap, 0u, st, ga, aa, gb, ab);
    } else
        launched = pro == LF_PRO_BNRELU ? launch_tappair<64, 1, 2>(ga, aa, gb, ab, st) : launch_tappair<64, 0, 2>(ga, aa, gb, ab, st);
    LF_REQUIRE(launched, "tappair: the LDS attribute lf_tappair_ok obtained was refused at launch");
    LF_CHECK_LAUNCH("tappair");
    return 0;
}
