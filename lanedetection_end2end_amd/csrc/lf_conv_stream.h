// The fp32 stream tile body: one 3-tap C -> C convolution (C = CS = 64 or 128, Wl % 64 == 0) over one 256-pixel tile per 4-wave
// group, the weights RESIDENT IN LDS and the pixels streamed past them through a register ring.  tapstream_kernel (lf_conv.hip)
// runs it once per tile, tappair_kernel (lf_conv_pair.hip) twice -- conv_a, then conv_b on what conv_a stored.  Internal: included
// by those two files only, everything in an anonymous namespace.
//
// A wave computes its 64 pixels x 64 output channels as FOUR 16-pixel sub-tiles in turn (16 + 16 accumulator registers): per K-step
// one dwordx4 X load per lane, four lane-contiguous ds_read_b128 of the weights ([K-step][channel tile][lane] float4) and 16 MFMAs.
// Results are tapgemm_kernel's bit for bit (tests/test_fp32_stream_gpu.py, tests/test_fwd_pair_gpu.py): the same K order, the same
// 32-product segments flushed into accl, the same epilogue text (LF_EPI_HEAD / LF_EPI_TILE / LF_EPI_TAIL) over the sub-tiles in the
// order 0, 1, 2, 3.  K order, segment rule and epilogue parameters of the stream family exist HERE and nowhere else.
#pragma once
#include "lf_conv_dev.h"
#include "lf_conv_epi.h"

namespace {

constexpr int STREAM_R = 8;       // K-steps of X in flight per wave (the ring)

struct StreamWT { int n0, i0, j0; bool v; };      // a wave's 64 pixels lie in one image row: (image, row, first column), wave-uniform

// wave wtile (of the workgroup's 4 G) of unit u: tile u * G + wtile / 4, wave wtile % 4 of it -- pixels from (u * 4G + wtile) * 64;
// !live (a unit past the workgroup's range): every load of it reads zeros / is masked.  (npix and wtile by reference, as the
// kernels' lambdas captured them: passed by value, tappair_kernel's register allocation moves)
template <int G>
__device__ __forceinline__ StreamWT stream_coords(const LfTapGeom& g, const unsigned& npix, const unsigned& wtile, unsigned u, bool live) {
    const unsigned tile0 = (u * (unsigned)(4 * G) + wtile) * 64u;
    StreamWT c;
    c.v = live && tile0 < npix;
    row1_coords(g, c.v ? tile0 : 0u, c.n0, c.i0, c.j0);
    return c;
}
// byte offset of this lane's four source channels of (sub-tile, tap) -- tapgemm_kernel's tap table, computed where it is used
template <int PROC>
__device__ __forceinline__ unsigned stream_xoff(const LfTapGeom& g, const StreamWT& c, int sub, int t, int pl, int kq, bool& in) {
    const int sy = c.i0 * g.ssh + g.tdh[t], sx = (c.j0 + sub * 16 + pl) * g.ssw + g.tdw[t];
    in = c.v && sy >= 0 && sy < g.Hs && sx >= 0 && sx < g.Ws;
    const int syc = min(max(sy, 0), g.Hs - 1), sxc = min(max(sx, 0), g.Ws - 1);
    const unsigned o = (unsigned)(((c.n0 * g.Hs + syc) * g.Ws + sxc) * g.s_pix + g.s_choff + kq * 4) * 4u;
    return (PROC == 0 && !in) ? LF_OOB : o;
}
// position p of a tile's K sequence: sub-tile p / NS, then tap-major, then 16-channel groups
template <int CS, int PROC>
__device__ __forceinline__ f32x4 stream_xload(const LfTapGeom& g, __amdgpu_buffer_rsrc_t rx, const StreamWT& c, int p, int pl, int kq) {
    constexpr int NCG = CS / 16, NS = 3 * NCG;
    const int k = p % NS;
    bool in;
    const unsigned o = stream_xoff<PROC>(g, c, p / NS, k / NCG, pl, kq, in);
    return ldb4(rx, o, (unsigned)(k % NCG) * 64u);
}
// the workgroup's 64-output-channel slice of the packed weights [tap][CS/4][Cd][4] -> LDS [K-step][channel tile n][kq][pl] float4
template <int CS, int THREADS>
__device__ __forceinline__ void stream_copy_weights(f32x4* wl, const float* wp, int cob) {
    constexpr int NS = 3 * (CS / 16);
    const __amdgpu_buffer_rsrc_t rw = make_rsrc(wp, (unsigned)(3 * CS * CS * 4));
    for (int idx = threadIdx.x; idx < NS * 256; idx += THREADS) {
        const int col = idx & 63, row = idx >> 6;                          // row = tap * (CS / 4) + 4 * channel group + kq
        wl[((row >> 2) * 4 + (col >> 4)) * 64 + (row & 3) * 16 + (col & 15)] = ldb4(rw, (unsigned)(row * CS + cob + col) * 16u, 0u);
    }
}
// the BN+ReLU operand prologue -> LDS: scale [CS], shift [CS]
template <int CS, int THREADS>
__device__ __forceinline__ void stream_copy_prologue(float* pvec, const LfTapArgs& a) {
    const __amdgpu_buffer_rsrc_t rsc = make_rsrc(a.pro_sc, CS * 4u), rsh = make_rsrc(a.pro_sh, CS * 4u);
    for (int i = threadIdx.x; i < 2 * CS; i += THREADS)
        pvec[i] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(i < CS ? rsc : rsh, (i < CS ? i : i - CS) * 4, 0, 0));
}

// One convolution over one tile per 4-wave group (unit bx: tiles bx * G ..).  ring holds the first STREAM_R K-steps of X on entry
// and wraps across the sub-tiles, so the operands of the next sub-tile are in flight while this one's epilogue runs, and the stores
// of a tile leave in four pieces spread over its life instead of in one burst at its end.  TAIL: the last STREAM_R slots are
// refilled from tail(p), p = 0 .. STREAM_R - 1 (what the caller wants in flight behind this tile: its next tile's first K-steps),
// else they are left alone.  The epilogue head runs per tile, as in tapgemm_kernel: sums and pivot start from zero here.
template <int CS, int PROC, int EPIC, int G, bool TAIL, typename Tail>
__device__ __forceinline__ void stream_tile(const LfTapGeom& g, const LfTapArgs& a, const f32x4* wl, const float* pvec, const unsigned bx,
                                            const unsigned ntiles, const unsigned npix, const int cob, const StreamWT& cur,
                                            const __amdgpu_buffer_rsrc_t rx, f32x4 (&ring)[STREAM_R], Tail&& tail) {
    constexpr int NT = 4, NCG = CS / 16, NS = 3 * NCG, R = STREAM_R;
    constexpr int epi = EPIC;
    constexpr bool S16 = false, HOISTV = true;
    static_assert((4 * NS) % R == 0 && R <= NS && NS % 2 == 0, "ring positions and K-step pairs must be compile-time");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int pl = lane & 15, kq = lane >> 4;
    f32x4 wn[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) wn[n] = wl[n * 64 + lane];
#undef LF_EPI_GROUPS
#define LF_EPI_GROUPS G
#undef LF_EPI_ROW1
#define LF_EPI_ROW1 true
#undef LF_EPI_ACC
#define LF_EPI_ACC(n, m) acc[n]
#undef LF_EPI_FIRST
#define LF_EPI_FIRST(m) (sub == 0)
#undef LF_EPI_ROW_OK
#define LF_EPI_ROW_OK(tg) (bx * (unsigned)G + (unsigned)(tg) < ntiles)
    LF_EPI_HEAD
    const int pn[1] = {cur.n0}, pi[1] = {cur.i0};
    const bool pv[1] = {cur.v};
#pragma unroll
    for (int sub = 0; sub < 4; ++sub) {
        f32x4 acc[NT], accl[NT];
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            const int p = sub * NS + k, cg = k % NCG;
            f32x4 w[NT];
#pragma unroll
            for (int n = 0; n < NT; ++n) w[n] = wn[n];
#pragma unroll
            for (int n = 0; n < NT; ++n) wn[n] = wl[(((k + 1) % NS) * 4 + n) * 64 + lane];    // the next K-step's weights
            f32x4 x = ring[p % R];
            if constexpr (PROC == LF_PRO_BNRELU) {
                bool in;
                (void)stream_xoff<PROC>(g, cur, sub, k / NCG, pl, kq, in);
                const f32x4 sc = *reinterpret_cast<const f32x4*>(pvec + cg * 16 + kq * 4);
                const f32x4 sh = *reinterpret_cast<const f32x4*>(pvec + CS + cg * 16 + kq * 4);
                f32x4 v = max0(x * sc + sh);
                v.x = in ? v.x : 0.f; v.y = in ? v.y : 0.f; v.z = in ? v.z : 0.f; v.w = in ? v.w : 0.f;
                x = v;
            }
            if (k % 2 == 0) {       // a pair of K-steps = one 32-product chain: flush the finished one, restart from C = 0
#pragma unroll
                for (int n = 0; n < NT; ++n) {
                    if (k == 0) accl[n] = zero4();
                    else { accl[n] += acc[n]; asm volatile("" : "+v"(accl[n])); }
                    acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[n][0], x[0], zero4(), 0, 0, 0);
                }
            }
#pragma unroll
            for (int s = (k % 2 == 0) ? 1 : 0; s < 4; ++s)
#pragma unroll
                for (int n = 0; n < NT; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[n][s], x[s], acc[n], 0, 0, 0);
            // this ring slot's next occupant, R K-steps ahead: this tile's, or what the caller wants in flight behind this tile
            if (p + R < 4 * NS) ring[p % R] = stream_xload<CS, PROC>(g, rx, cur, p + R, pl, kq);
            else if constexpr (TAIL) ring[p % R] = tail(p + R - 4 * NS);
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[n] += accl[n];
        const int pj[1] = {cur.j0 + sub * 16 + pl};
        LF_EPI_TILE(0)
    }
    LF_EPI_TAIL
#undef LF_EPI_GROUPS
#define LF_EPI_GROUPS 1
#undef LF_EPI_ROW1
#define LF_EPI_ROW1 false
#undef LF_EPI_ACC
#define LF_EPI_ACC(n, m) acc[n][m]
#undef LF_EPI_FIRST
#define LF_EPI_FIRST(m) ((m) == 0)
#undef LF_EPI_ROW_OK
#define LF_EPI_ROW_OK(tg) true
}

}  // namespace
