// Weight-gradient kernels of the tap-GEMM convolutions for gfx950 (see lf_conv.h for the contract; the forward and data-gradient
// kernels are in lf_conv.hip and lf_conv_bf16.hip, the device helpers shared with them in lf_conv_dev.h, the read-once kernel in lf_wgrad_ro.hip).
//
// Matrix-core mapping (v_mfma_f32_16x16x4_f32, exact fp32, D = A*B + C, wave64):
//   A[i][k]: lane l supplies row i = l&15, k-slot kq = l>>4      -> weights / x-channels
//   B[k][j]: lane l supplies col j = l&15, k-slot kq = l>>4      -> pixels / g-channels
//   D[i][j]: lane l holds rows 4*(l>>4)+e (e = 0..3), col l&15
//
// Kernels in this file:
//   tapwgrad_kernel / tapwgrad16_kernel / tapwgrad16_tr_kernel   weight gradients, split-K over pixels
//   tapwgrad16_f32_kernel     the 16 x 16 channel weight gradient on fp32 tensors through a per-wave LDS-DMA ring
//   the split-K reductions (one per weight gradient, or batched per backward pass).
#include "lf_conv_dev.h"

// ---------------------------------------------------------------------------------------
// weight gradient: dW[t][ci][co] = sum_p pro(X[spix(p,t)][ci]) * G[dpix(p)][co]
// rows = x-channels, cols = g-channels, k = 4 pixels per MFMA (k-slot kq <-> pixel p0+kq).
// Vector mode (channels % 64 == 0): a lane's float4 = channels 4*pl..4*pl+3 of its pixel feeds
// FOUR MFMA tiles (tile r = channels {4*i + r}); so 2 dwordx4 loads feed 16 MFMAs.
// ---------------------------------------------------------------------------------------
namespace {

// storage-typed loads of the weight-gradient kernels (S16: x and g hold bf16 elements, widened exactly to fp32)
// (buffer-addressed, element offsets: see ldb4)
template <bool S16>
__device__ __forceinline__ f32x4 wg_ld4(__amdgpu_buffer_rsrc_t r, unsigned off) { return epi_ld<S16>(r, off); }
template <bool S16>
__device__ __forceinline__ float wg_ld1(__amdgpu_buffer_rsrc_t r, unsigned off, unsigned soff = 0u) {
    if constexpr (S16) return __uint_as_float((unsigned)__builtin_amdgcn_raw_buffer_load_b16(r, (int)(off * 2u), (int)(soff * 2u), 0) << 16);
    else return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, (int)(off * 4u), (int)(soff * 4u), 0));
}
__device__ __forceinline__ uint2 wg_ldraw(__amdgpu_buffer_rsrc_t r, unsigned off) {      // 4 bf16 elements, raw
    return __builtin_bit_cast(uint2, __builtin_amdgcn_raw_buffer_load_b64(r, (int)(off * 2u), 0, 0));
}

typedef short s16x4 __attribute__((ext_vector_type(4)));

// BFM (bf16 tensors, 64-channel blocks on both sides): the four K=4 fp32 MFMAs of an iteration's four pixel
// sub-steps become ONE v_mfma_f32_16x16x16_bf16 per tile -- a lane's four pixels (p+kq, +4, +8, +12) are exactly its
// four k of the K=16 step -- with the operands assembled from the raw 8-byte loads by v_perm_b32 (no widening).
// PROT: 0 / 1 = the BN+ReLU prologue flag compiled in (the fp32 64-channel-block launches of the network), -1 = run-time
// (Round 6 built a PAIRED form -- 8-wave workgroups running the two jobs (tap, x-block, g-block 0 / 1) that read the same X stream side
// by side, one barrier per loop trip so that the partner's load finds the line in the CU's L1 -- to test whether the job form's
// re-reads bound the kernel: FETCH_SIZE fell 25 % (283 vs 376 MB per launch) and the launch did NOT get faster (64.2 vs 63.0 us, the
// step +0.13 ms); neither do operands from HBM instead of the Infinity Cache cost anything (profiles/r6_wgrad_traffic.txt).  The kernel
// is bound by issue / the matrix pipes; the form was removed (git: commit 45fe98c has it).)
template <bool XV, bool GV, int XT, int GT, int U, bool S16, bool BFM = false, int PROT = -1, bool DBG = false>
__global__ __launch_bounds__(256, 2) void tapwgrad_kernel(const LfTapGeom g, const LfWgradArgs a, const int pro_rt,
                                                      const long pps, const int write_bias, const int gxs) {
    constexpr int XTiles = XV ? 4 : XT, GTiles = GV ? 4 : GT;
    const int pro = PROT >= 0 ? (PROT ? LF_PRO_BNRELU : LF_PRO_NONE) : pro_rt;
    constexpr int XB = XTiles * 16, GB = GTiles * 16;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int pl = lane & 15, kq = lane >> 4;
    unsigned long long tstamp[4] = {0ull, 0ull, 0ull, 0ull};
    if constexpr (DBG) tstamp[0] = __builtin_amdgcn_s_memrealtime();
    // 1-D grid of gx * ntaps * (channel-block pairs) workgroups.  Workgroup L runs on XCD L % 8 (observed): each
    // XCD gets a contiguous run of the (pixel-split, channel-block, tap) order with the tap fastest, so all jobs of
    // one pixel range -- which read the same G rows and overlapping X rows -- follow each other through ONE L2
    // instead of streaming both tensors from HBM once per tap (FETCH_SIZE 177 MB -> see profiles/).
    const int ncob = g.Cd / GB;
    const unsigned ord = xcd_swizzle(blockIdx.x);
    const unsigned nz = (unsigned)((g.Cs / XB) * ncob);
    const int t = (int)(ord % (unsigned)g.ntaps);
    const int bz = (int)((ord / (unsigned)g.ntaps) % nz);                 // channel-block pair: next fastest
    const unsigned bxs = ord / ((unsigned)g.ntaps * nz);                  // pixel-split index: slowest
    (void)gxs;
    const int cib = bz / ncob, cob = bz % ncob;
    // Loop state is WAVE-UNIFORM (scalar registers): a wave walks its pixel range in groups of 4U consecutive pixels of one
    // image row; lane (pl, kq) takes pixel kq + 4u of the group.  A VALU instruction issued beside the partner wave's MFMA
    // stream costs ~13 cycles, so the per-lane address / mask arithmetic of the first version (~150 instructions per 64 MFMAs)
    // was as long as the matrix work itself.
    const long npix = (long)g.N * g.Hl * g.Wl;
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    const long sub = (long)bxs * WG_WAVES + wave_u;
    const long p_begin = sub * pps;
    long p_end = p_begin + pps;
    if (p_end > npix) p_end = npix;
    const int niter = p_end > p_begin ? (int)((p_end - p_begin) / (4 * U)) : 0;     // pps and npix are multiples of 4U

    f32x4 acc[XTiles][GTiles];
#pragma unroll
    for (int r = 0; r < XTiles; ++r)
#pragma unroll
        for (int q = 0; q < GTiles; ++q) acc[r][q] = zero4();
    float bsum[GTiles];
#pragma unroll
    for (int q = 0; q < GTiles; ++q) bsum[q] = 0.f;

    int pj, pi, pn;                       // (column, row, image) of the current group's first pixel
    {
        const unsigned q = niter ? (unsigned)p_begin : 0u;
        const unsigned r = q / (unsigned)g.Wl;
        pj = (int)(q - r * (unsigned)g.Wl);
        pn = (int)(r / (unsigned)g.Hl);
        pi = (int)(r - (unsigned)pn * (unsigned)g.Hl);
        // (the divisions run on the vector ALU: pin the uniform results to scalar registers)
        pj = __builtin_amdgcn_readfirstlane(pj); pi = __builtin_amdgcn_readfirstlane(pi); pn = __builtin_amdgcn_readfirstlane(pn);
    }
    const int dh = g.tdh[t], dw = g.tdw[t];
    const int xch = g.s_choff + cib * XB + (XV ? 4 * pl : pl);
    const int gch = g.d_choff + cob * GB + (GV ? 4 * pl : pl);
    // x: num_records = the tensor, so that the out-of-range offset LF_OOB reads as zero (the conv's padding); the launcher
    // keeps tensors below LF_OOB bytes
    const __amdgpu_buffer_rsrc_t rx = make_rsrc(a.x, (unsigned)((long)g.N * g.Hs * g.Ws * g.s_pix << (S16 ? 1 : 2))),
                                 rg = make_rsrc(a.g, (unsigned)((long)g.N * g.Hd * g.Wd * g.d_pix << (S16 ? 1 : 2)));
    f32x4 psc, psh;
    float psc1[XTiles], psh1[XTiles];
    if (pro == LF_PRO_BNRELU) {
        if constexpr (XV) { psc = ldg4(a.pro_sc + cib * XB + 4 * pl); psh = ldg4(a.pro_sh + cib * XB + 4 * pl); }
        else {
#pragma unroll
            for (int r = 0; r < XTiles; ++r) { psc1[r] = a.pro_sc[cib * XB + r * 16 + pl]; psh1[r] = a.pro_sh[cib * XB + r * 16 + pl]; }
        }
    }

    // per-lane constants (element offsets inside a group) and the group strides
    const unsigned gvoff = (unsigned)(kq * g.dsw * g.d_pix + gch), gstep = (unsigned)(4 * g.dsw * g.d_pix);
    const unsigned xvoff = (unsigned)(kq * g.ssw * g.s_pix + xch), xstep = (unsigned)(4 * g.ssw * g.s_pix);
    constexpr unsigned ESH = S16 ? 1 : 2;          // element -> byte shift
    // One iteration = U k-steps = one group (the launcher guarantees Wl % (4U) == 0 and pps % (4U) == 0).  INTERIOR groups
    // (every tap position inside the image -- decided on scalars) load from a scalar base + per-lane constant; the others
    // compute per-lane offsets, and a tap position outside the image gets the out-of-range offset LF_OOB, which the buffer load
    // returns as 0.0f: no masks on the values.  Only with the BN+ReLU prologue (transform(0) != 0) the offsets are clamped
    // and the mask bits applied after the transform.
    // Loads are double-buffered in two named register sets: the next group's 2U loads are in flight during 16*U MFMAs.
    static_assert(!BFM || (S16 && XV && GV && U == 4), "BFM needs bf16 tensors, vector mode, U = 4");
    struct WStep {
        uint2 xr[BFM ? U : 1], gr[BFM ? U : 1];             // BFM: raw bf16 quads
        f32x4 x4[XV ? U : 1], g4[GV ? U : 1];
        float xs[XV ? 1 : U][XTiles], gs[GV ? 1 : U][GTiles];
        unsigned xmask;                                     // used with the prologue only
    };
    constexpr unsigned OOBE = LF_OOB >> ESH;                // in elements
    auto ldx = [&](WStep& S, int u, unsigned voff, unsigned soff) __attribute__((always_inline)) {      // element offsets
        if constexpr (BFM) S.xr[u] = __builtin_bit_cast(uint2, __builtin_amdgcn_raw_buffer_load_b64(rx, (int)(voff << 1), (int)(soff << 1), 0));
        else if constexpr (XV) {
            if constexpr (S16) S.x4[u] = epi_ld<true>(rx, voff, soff);
            else S.x4[u] = ldb4(rx, voff << 2, soff << 2);
        } else {
#pragma unroll
            for (int r = 0; r < XTiles; ++r) S.xs[u][r] = wg_ld1<S16>(rx, voff + r * 16, soff);
        }
    };
    auto wload = [&](WStep& S) __attribute__((always_inline)) {
        const unsigned gso = (unsigned)(((pn * g.Hd + pi * g.dsh + g.dah) * g.Wd + pj * g.dsw + g.daw) * g.d_pix);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const unsigned so = gso + u * gstep;
            if constexpr (BFM) S.gr[u] = __builtin_bit_cast(uint2, __builtin_amdgcn_raw_buffer_load_b64(rg, (int)(gvoff << 1), (int)(so << 1), 0));
            else if constexpr (GV) {
                if constexpr (S16) S.g4[u] = epi_ld<true>(rg, gvoff, so);
                else S.g4[u] = ldb4(rg, gvoff << 2, so << 2);
            } else {
#pragma unroll
                for (int q = 0; q < GTiles; ++q) S.gs[u][q] = wg_ld1<S16>(rg, gvoff + q * 16, so);
            }
        }
        const int sy = pi * g.ssh + dh;
        const bool yin = sy >= 0 && sy < g.Hs;
        const int sx0 = pj * g.ssw + dw, sxl = sx0 + (4 * U - 1) * g.ssw;
        if (yin && sx0 >= 0 && sxl < g.Ws) {
            const unsigned xso = (unsigned)(((pn * g.Hs + sy) * g.Ws + sx0) * g.s_pix);
#pragma unroll
            for (int u = 0; u < U; ++u) ldx(S, u, xvoff, xso + u * xstep);
            S.xmask = 0xfu;
        } else {
            const int syc = min(max(sy, 0), g.Hs - 1);
            const unsigned xso = (unsigned)((pn * g.Hs + syc) * g.Ws * g.s_pix);
            unsigned xm = 0;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int sx = sx0 + (kq + 4 * u) * g.ssw;
                const bool in = yin && sx >= 0 && sx < g.Ws;
                xm |= (in ? 1u : 0u) << u;
                const unsigned oc = (unsigned)(min(max(sx, 0), g.Ws - 1) * g.s_pix + xch);
                ldx(S, u, (in || pro == LF_PRO_BNRELU) ? oc : OOBE, xso);
            }
            S.xmask = xm;
        }
    };
    auto advance = [&]() __attribute__((always_inline)) {
        pj += 4 * U;
        if (pj >= g.Wl) { pj -= g.Wl; if (++pi >= g.Hl) { pi = 0; ++pn; } }
    };
    const bool need_bias = write_bias && a.bias_partial && t == 0 && cib == 0;      // workgroup-uniform
    // BIAS / PRO are compile-time in the loop body: left as scalar conditions the compiler if-converts them into v_cndmask
    // selects over BOTH sides -- the VALU work the scalar loop state was meant to remove.
    auto compute = [&](const WStep& S, auto BIAS_c, auto PRO_c) __attribute__((always_inline)) {
        constexpr bool BIAS = decltype(BIAS_c)::value, PRO = decltype(PRO_c)::value;
        if constexpr (BFM) {
            uint2 xq[U], gq[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const bool xin = !PRO || ((S.xmask >> u) & 1u);
                uint2 xx = S.xr[u], gg = S.gr[u];
                if constexpr (PRO) {          // relu(bn(x)) in fp32 on the widened quad, rounded back
                    f32x4 t4;
                    t4.x = __uint_as_float(xx.x << 16); t4.y = __uint_as_float(xx.x & 0xffff0000u);
                    t4.z = __uint_as_float(xx.y << 16); t4.w = __uint_as_float(xx.y & 0xffff0000u);
                    t4 = max0(t4 * psc + psh);
                    lf_bf16x4 b;
                    b[0] = (lf_bf16)t4.x; b[1] = (lf_bf16)t4.y; b[2] = (lf_bf16)t4.z; b[3] = (lf_bf16)t4.w;
                    xx = __builtin_bit_cast(uint2, b);
                }
                xq[u].x = xin ? xx.x : 0u; xq[u].y = xin ? xx.y : 0u;
                gq[u] = gg;
            }
            // tile e of the x side = channels {4*row + e}: element e of every pixel's quad -> k = 4*kq + u
            s16x4 xa[4], gb[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const unsigned sel = (e & 1) ? 0x07060302u : 0x05040100u;
                uint2 ax, bx;
                if (e < 2) {
                    ax.x = __builtin_amdgcn_perm(xq[1].x, xq[0].x, sel); ax.y = __builtin_amdgcn_perm(xq[3].x, xq[2].x, sel);
                    bx.x = __builtin_amdgcn_perm(gq[1].x, gq[0].x, sel); bx.y = __builtin_amdgcn_perm(gq[3].x, gq[2].x, sel);
                } else {
                    ax.x = __builtin_amdgcn_perm(xq[1].y, xq[0].y, sel); ax.y = __builtin_amdgcn_perm(xq[3].y, xq[2].y, sel);
                    bx.x = __builtin_amdgcn_perm(gq[1].y, gq[0].y, sel); bx.y = __builtin_amdgcn_perm(gq[3].y, gq[2].y, sel);
                }
                xa[e] = __builtin_bit_cast(s16x4, ax);
                gb[e] = __builtin_bit_cast(s16x4, bx);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    acc[r][q] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(xa[r], gb[q], acc[r][q], 0, 0, 0);
            if constexpr (BIAS) {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    bsum[0] += __uint_as_float(gq[u].x << 16); bsum[1] += __uint_as_float(gq[u].x & 0xffff0000u);
                    bsum[2] += __uint_as_float(gq[u].y << 16); bsum[3] += __uint_as_float(gq[u].y & 0xffff0000u);
                }
            }
            return;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            float xv[XTiles], gv[GTiles];
            if constexpr (GV) { gv[0] = S.g4[u].x; gv[1] = S.g4[u].y; gv[2] = S.g4[u].z; gv[3] = S.g4[u].w; }
            else {
#pragma unroll
                for (int q = 0; q < GTiles; ++q) gv[q] = S.gs[u][q];
            }
            if constexpr (XV) {
                f32x4 t4 = S.x4[u];
                if constexpr (PRO) t4 = max0(t4 * psc + psh);
                xv[0] = t4.x; xv[1] = t4.y; xv[2] = t4.z; xv[3] = t4.w;
            } else {
#pragma unroll
                for (int r = 0; r < XTiles; ++r) {
                    float t1 = S.xs[u][r];
                    if constexpr (PRO) t1 = fmaxf(t1 * psc1[r] + psh1[r], 0.f);
                    xv[r] = t1;
                }
            }
            if constexpr (PRO) {
                const bool xin = (S.xmask >> u) & 1u;
#pragma unroll
                for (int r = 0; r < XTiles; ++r) xv[r] = xin ? xv[r] : 0.f;
            }
#pragma unroll
            for (int r = 0; r < XTiles; ++r)
#pragma unroll
                for (int q = 0; q < GTiles; ++q)
                    acc[r][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[r], gv[q], acc[r][q], 0, 0, 0);
            if constexpr (BIAS) {
#pragma unroll
                for (int q = 0; q < GTiles; ++q) bsum[q] += gv[q];
            }
        }
    };

    // (A third operand set -- loads two groups ahead -- spills: the three inlined loop bodies push the accumulators to scratch,
    // 185 us instead of 62.)
    WStep A, B;
    auto run = [&](auto BIAS_c, auto PRO_c) __attribute__((always_inline)) {
        auto step = [&](const WStep& S) __attribute__((always_inline)) { compute(S, BIAS_c, PRO_c); };
        wload(A);
        advance();
        if constexpr (DBG) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); tstamp[1] = __builtin_amdgcn_s_memrealtime(); }
        // Structured loop: pairs of groups (A then B), an odd last group peeled -- one loop body whose accumulators stay in place
        // (the first form, a for(;;) with two exits and conditional prefetches, made hipcc rename the 64 accumulator registers
        // from MFMA to MFMA and copy them at every join: 256 registers, 10 of them spilled in the prologue variant).
        // The prefetch behind the last group reads the next wave's first group -- or, past the tensors, zeros from the bounded
        // buffer resources -- and is never used.  Priority falls with progress (quarters): the waves of a SIMD finish together.
        const int npairs = niter >> 1, qp = npairs >> 2;
#pragma nounroll
        for (int ph = 0; ph < 4; ++ph) {
            switch (ph) {
                case 0: __builtin_amdgcn_s_setprio(3); break;
                case 1: __builtin_amdgcn_s_setprio(2); break;
                case 2: __builtin_amdgcn_s_setprio(1); break;
                default: __builtin_amdgcn_s_setprio(0); break;
            }
            const int n = ph < 3 ? qp : npairs - 3 * qp;
            for (int i = 0; i < n; ++i) {
                wload(B); advance();
                step(A);
                wload(A); advance();
                step(B);
            }
        }
        if (niter & 1) step(A);
    };
    if (niter > 0) {
        if constexpr (PROT >= 0) {
            if (need_bias) run(std::true_type{}, std::integral_constant<bool, PROT == 1>{});
            else run(std::false_type{}, std::integral_constant<bool, PROT == 1>{});
        } else {
            const bool prologue = pro == LF_PRO_BNRELU;
            if (need_bias) { if (prologue) run(std::true_type{}, std::true_type{}); else run(std::true_type{}, std::false_type{}); }
            else { if (prologue) run(std::false_type{}, std::true_type{}); else run(std::false_type{}, std::false_type{}); }
        }
    }
    if constexpr (DBG) { asm volatile("" ::"v"(acc[0][0][0])); tstamp[2] = __builtin_amdgcn_s_memrealtime(); }
    // ---- reduce the 4 waves of the workgroup through LDS, wave 0 writes one partial row
    __builtin_amdgcn_s_setprio(3);
    __shared__ float red[WG_WAVES - 1][XTiles * GTiles * 4][64];
    __shared__ float bred[WG_WAVES][GTiles][64];
    if (wave > 0) {
#pragma unroll
        for (int r = 0; r < XTiles; ++r)
#pragma unroll
            for (int q = 0; q < GTiles; ++q)
#pragma unroll
                for (int e = 0; e < 4; ++e) red[wave - 1][(r * GTiles + q) * 4 + e][lane] = acc[r][q][e];
    }
#pragma unroll
    for (int q = 0; q < GTiles; ++q) bred[wave][q][lane] = bsum[q];
    __syncthreads();
    if (wave == 0) {
        // this workgroup's slab of the partial tensor: < 2^32 bytes (Cs * Cd <= 128 x 128), buffer-addressed
        const __amdgpu_buffer_rsrc_t ro = make_rsrc(a.partial + ((long)bxs * g.ntaps + t) * g.Cs * g.Cd, 0xffffffffu);
#pragma unroll
        for (int r = 0; r < XTiles; ++r)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int i = 4 * kq + e;                                  // row of tile (r,q)
                const int ci = cib * XB + (XV ? 4 * i + r : r * 16 + i);
                float v[GTiles];
#pragma unroll
                for (int q = 0; q < GTiles; ++q) {
                    v[q] = acc[r][q][e];
#pragma unroll
                    for (int w = 0; w < WG_WAVES - 1; ++w) v[q] += red[w][(r * GTiles + q) * 4 + e][lane];
                }
                if constexpr (GV) {          // columns 4*pl .. 4*pl+3 of row ci: one 16-byte store
                    f32x4 v4 = {v[0], v[1], v[2], v[3]};
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4v, v4), ro, (ci * g.Cd + cob * GB + 4 * pl) * 4, 0, 0);
                } else {
#pragma unroll
                    for (int q = 0; q < GTiles; ++q)
                        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v[q]), ro, (ci * g.Cd + cob * GB + q * 16 + pl) * 4, 0, 0);
                }
            }
        if (write_bias && a.bias_partial && t == 0 && cib == 0) {
            // column sums of G over this workgroup's pixels: lanes with equal pl (4 k-slots) x 4 waves
#pragma unroll
            for (int q = 0; q < GTiles; ++q) {
                float v = 0.f;
#pragma unroll
                for (int w = 0; w < WG_WAVES; ++w) v += bred[w][q][lane];
                v += __shfl_xor(v, 16, 64);
                v += __shfl_xor(v, 32, 64);
                if (kq == 0) {
                    const int co = cob * GB + (GV ? 4 * pl + q : q * 16 + pl);
                    a.bias_partial[(long)bxs * g.Cd + co] = v;
                }
            }
        }
    }
    if constexpr (DBG) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        tstamp[3] = __builtin_amdgcn_s_memrealtime();
        if (lane == 0 && a.dbg) {
            unsigned long long* d = a.dbg + ((unsigned long long)blockIdx.x * WG_WAVES + wave) * 8;
            unsigned hwid, xcc;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
            d[0] = tstamp[0]; d[1] = tstamp[1]; d[2] = tstamp[2]; d[3] = tstamp[3];
            d[4] = (unsigned long long)hwid | ((unsigned long long)xcc << 32);
        }
    }
}

// 16 x 16 channel weight gradient with ALL taps in one wave (the 128x256 stage): one pass over G and X
// instead of one per tap -- these launches are HBM-bound, the per-tap split tripled their traffic.
template <int NTAPS, bool S16>
__global__ __launch_bounds__(256) void tapwgrad16_kernel(const LfTapGeom g, const LfWgradArgs a, const int pro,
                                                        const long pps, const int write_bias) {
    constexpr int U = 4;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int pl = lane & 15, kq = lane >> 4;
    const long npix = (long)g.N * g.Hl * g.Wl;
    const long sub = (long)blockIdx.x * WG_WAVES + wave;
    const long p_begin = sub * pps;
    long p_end = p_begin + pps;
    if (p_end > npix) p_end = npix;
    f32x4 acc[NTAPS];
#pragma unroll
    for (int t = 0; t < NTAPS; ++t) acc[t] = zero4();
    float bsum = 0.f;
    float psc = 1.f, psh = 0.f;
    if (pro == LF_PRO_BNRELU) { psc = a.pro_sc[pl]; psh = a.pro_sh[pl]; }
    int tdh[NTAPS], tdw[NTAPS];
#pragma unroll
    for (int t = 0; t < NTAPS; ++t) { tdh[t] = g.tdh[t]; tdw[t] = g.tdw[t]; }
    long p = p_begin + kq;
    int pj, pi, pn;
    {
        const unsigned q = p < npix ? (unsigned)p : 0u;
        const unsigned r = q / (unsigned)g.Wl;
        pj = (int)(q - r * (unsigned)g.Wl);
        pn = (int)(r / (unsigned)g.Hl);
        pi = (int)(r - (unsigned)pn * (unsigned)g.Hl);
    }
    const unsigned gstep = (unsigned)(4 * g.dsw * g.d_pix);
    const __amdgpu_buffer_rsrc_t rx = make_rsrc(a.x, 0xffffffffu), rg = make_rsrc(a.g, 0xffffffffu);
    while (p - kq < p_end) {                        // wave-uniform; 16 pixels of one row per iteration
        const unsigned gofs = (unsigned)(((pn * g.Hd + pi * g.dsh + g.dah) * g.Wd + pj * g.dsw + g.daw) * g.d_pix + g.d_choff + pl);
        float gv[U], xv[NTAPS][U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool v = (p + 4 * u) < p_end;
            const float t0 = wg_ld1<S16>(rg, v ? gofs + u * gstep : gofs);
            gv[u] = v ? t0 : 0.f;
        }
#pragma unroll
        for (int t = 0; t < NTAPS; ++t) {
            const int sy = pi * g.ssh + tdh[t];
            const bool yin = sy >= 0 && sy < g.Hs;
            const unsigned xrow = (unsigned)((pn * g.Hs + min(max(sy, 0), g.Hs - 1)) * g.Ws * g.s_pix + g.s_choff + pl);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int sx = (pj + 4 * u) * g.ssw + tdw[t];
                const bool in = yin && sx >= 0 && sx < g.Ws && (p + 4 * u) < p_end;
                float x0 = wg_ld1<S16>(rx, xrow + (unsigned)(min(max(sx, 0), g.Ws - 1) * g.s_pix));
                if (pro == LF_PRO_BNRELU) x0 = fmaxf(x0 * psc + psh, 0.f);
                xv[t][u] = in ? x0 : 0.f;
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int t = 0; t < NTAPS; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[t][u], gv[u], acc[t], 0, 0, 0);
            bsum += gv[u];
        }
        p += 4 * U;
        pj += 4 * U;
        if (pj >= g.Wl) { pj -= g.Wl; if (++pi >= g.Hl) { pi = 0; ++pn; } }
    }
    __shared__ float red[WG_WAVES - 1][NTAPS * 4][64];
    __shared__ float bred[WG_WAVES][64];
    if (wave > 0) {
#pragma unroll
        for (int t = 0; t < NTAPS; ++t)
#pragma unroll
            for (int e = 0; e < 4; ++e) red[wave - 1][t * 4 + e][lane] = acc[t][e];
    }
    bred[wave][lane] = bsum;
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int t = 0; t < NTAPS; ++t) {
            float* out = a.partial + ((long)blockIdx.x * NTAPS + t) * g.Cs * g.Cd;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float v = acc[t][e];
#pragma unroll
                for (int w = 0; w < WG_WAVES - 1; ++w) v += red[w][t * 4 + e][lane];
                out[(long)(4 * kq + e) * g.Cd + pl] = v;          // row = x-channel 4*kq+e, col = g-channel pl
            }
        }
        if (write_bias && a.bias_partial) {
            float v = bred[0][lane] + bred[1][lane] + bred[2][lane] + bred[3][lane];
            v += __shfl_xor(v, 16, 64);
            v += __shfl_xor(v, 32, 64);
            if (kq == 0) a.bias_partial[(long)blockIdx.x * g.Cd + pl] = v;
        }
    }
}

// 16 x 16 channel weight gradient on bf16 tensors (no operand prologue): the kernel above fetches ONE bf16 per lane and
// instruction (2-byte buffer loads, 16 of them per 16 pixels: 135 us per launch at 160 x 320 x 64 images, where the 210 MB
// it reads take 40).  Here every wave owns a private LDS ring (no barrier in the loop):
//  * LDS-DMA copies 32 pixels x 32 bytes of G and of X at each of the three tap positions, lane-linear (1 KB = whole lines of the
//    NHWC tensors; a padding tap position carries the out-of-range offset and lands as zeros), three stages in flight;
//  * the image [pixel][16 channels] is exactly the [k][n] block ds_read_b64_tr_b16 transposes: lane (channel l & 15, k-group
//    l >> 4) receives pixels 4 (l >> 4) .. +3 of its channel -- the A / B operand of v_mfma_f32_16x16x16_bf16 with K = 16 pixels:
//    per 16 pixels one transposing read per operand, one MFMA per tap.
// Split over pixel ranges and reduced through LDS at the end like tapwgrad16_kernel (same partial layout).
// PRO (round 5): the BN + ReLU operand prologue of the block's third convolution on the transposed operand (a lane holds four pixels
// of ONE channel: scale / shift are two registers; padding re-zeroed after the transform) -- those two launches per step fell back
// to the 2-byte-load kernel before (137 us at 160 x 320 x 64 images).
constexpr int W16_STAGE = 4 * 1024, W16_STAGES = 4;
template <bool PRO>
__global__ __launch_bounds__(256) void tapwgrad16_tr_kernel(const LfTapGeom g, const LfWgradArgs a, const long pps, const int write_bias) {
    constexpr int NTAPS = 3;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int pl = lane & 15, kq = lane >> 4;
    const long npix = (long)g.N * g.Hl * g.Wl;
    const long sub = (long)blockIdx.x * WG_WAVES + wave;
    const long p_begin = sub * pps;
    long p_end = p_begin + pps;
    if (p_end > npix) p_end = npix;
    const int niter = p_end > p_begin ? (int)((p_end - p_begin + 31) / 32) : 0;
    f32x4 acc[NTAPS];
#pragma unroll
    for (int t = 0; t < NTAPS; ++t) acc[t] = zero4();
    float bsum = 0.f;
    const i32x4s rx = make_rsrc_words(a.x, (unsigned)min((long)g.N * g.Hs * g.Ws * g.s_pix * 2, (long)LF_OOB)),
                 rg = make_rsrc_words(a.g, (unsigned)min((long)g.N * g.Hd * g.Wd * g.d_pix * 2, (long)LF_OOB));
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)lf_tap_lds + (unsigned)(wave * W16_STAGES * W16_STAGE);
    const unsigned char* const ring = lf_tap_lds + wave * W16_STAGES * W16_STAGE;
    const int tdh0 = g.tdh[0], tdh1 = g.tdh[1], tdh2 = g.tdh[2], tdw0 = g.tdw[0], tdw1 = g.tdw[1], tdw2 = g.tdw[2];
    // load cursor: (image, row, column) of the next 16-pixel group (wave-uniform; Wl % 16 == 0: a group lies in one row)
    long p_ld = p_begin;
    int pj, pi, pn;
    row1_coords(g, niter ? (unsigned)p_begin : 0u, pn, pi, pj);
    const int px = (lane >> 1) & 15, half = lane & 1;         // lanes 0-31: first group of the stage, 32-63: second
    int st_ld = 0;
    auto issue = [&]() __attribute__((always_inline)) {
        // the two groups of this stage
        int gn[2], gi[2], gj[2];
        bool gok[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            gok[q] = p_ld < p_end;
            gn[q] = pn; gi[q] = pi; gj[q] = pj;
            p_ld += 16;
            pj += 16;
            if (pj >= g.Wl) { pj = 0; if (++pi >= g.Hl) { pi = 0; ++pn; } }
        }
        const bool hi = lane >= 32;
        const int n = hi ? gn[1] : gn[0], i = hi ? gi[1] : gi[0], j = (hi ? gj[1] : gj[0]) + px;
        const bool ok = hi ? gok[1] : gok[0];
        const unsigned dst = lds0 + (unsigned)(st_ld * W16_STAGE);
        const unsigned go = (unsigned)((((n * g.Hd + i * g.dsh + g.dah) * g.Wd + j * g.dsw + g.daw) * g.d_pix + g.d_choff + half * 8) * 2);
        lds_dma16(rg, dst, ok ? go : LF_OOB, 0u);
#pragma unroll
        for (int t = 0; t < NTAPS; ++t) {
            const int dh = t == 0 ? tdh0 : t == 1 ? tdh1 : tdh2, dw = t == 0 ? tdw0 : t == 1 ? tdw1 : tdw2;
            const int sy = i * g.ssh + dh, sx = j * g.ssw + dw;
            const bool in = ok && sy >= 0 && sy < g.Hs && sx >= 0 && sx < g.Ws;
            const unsigned xo = (unsigned)((((n * g.Hs + sy) * g.Ws + sx) * g.s_pix + g.s_choff + half * 8) * 2);
            lds_dma16(rx, dst + (unsigned)((1 + t) * 1024), in ? xo : LF_OOB, 0u);
        }
        st_ld = st_ld == W16_STAGES - 1 ? 0 : st_ld + 1;
    };
#pragma unroll
    for (int q = 0; q < W16_STAGES - 1; ++q) issue();
    typedef short s16x4 __attribute__((ext_vector_type(4)));
    typedef short s16x2 __attribute__((ext_vector_type(2)));
    typedef s16x4 __attribute__((address_space(3))) * lds_s16x4_p;
    float psc = 1.f, psh = 0.f;
    if constexpr (PRO) {
        psc = a.pro_sc[pl]; psh = a.pro_sh[pl];
        asm volatile("" ::"v"(psc), "v"(psh) : "memory");      // loaded before the loop's hand-counted vmcnt waits (see lf_wgrad_ro.hip)
    }
    // compute cursor (PRO: the padding tests of the group being multiplied): row and first column of its 16-pixel halves
    int cj = 0, ci = 0;
    {
        const unsigned q = niter ? (unsigned)p_begin : 0u;
        const unsigned r = q / (unsigned)g.Wl;
        cj = __builtin_amdgcn_readfirstlane((int)(q - r * (unsigned)g.Wl));
        ci = __builtin_amdgcn_readfirstlane((int)(r % (unsigned)g.Hl));
    }
    int st_c = 0;
    for (int it = 0; it < niter; ++it) {
        // my DMA of this stage has landed (two younger stages of 4 instructions may be in flight); my reads of the stage that is
        // restaged next have retired.  The ring is private to the wave: no barrier.
        asm volatile("s_waitcnt vmcnt(8) lgkmcnt(0)" ::: "memory");
        issue();
        const unsigned char* st = ring + st_c * W16_STAGE;
        st_c = st_c == W16_STAGES - 1 ? 0 : st_c + 1;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const s16x4 gv = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_p)(st + q * 512 + lane * 8));
#pragma unroll
            for (int t = 0; t < NTAPS; ++t) {
                s16x4 xv = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_p)(st + (1 + t) * 1024 + q * 512 + lane * 8));
                if constexpr (PRO) {
                    const int dh = t == 0 ? tdh0 : t == 1 ? tdh1 : tdh2, dw = t == 0 ? tdw0 : t == 1 ? tdw1 : tdw2;
                    const int sy = ci * g.ssh + dh, c0 = cj * g.ssw + dw;            // the half's first pixel at this tap
                    if ((unsigned)sy >= (unsigned)g.Hs) { const s16x4 z = {0, 0, 0, 0}; xv = z; }
                    else {
                        const uint2 u = __builtin_bit_cast(uint2, xv);
                        const f32x2 sc2 = {psc, psc}, sh2 = {psh, psh};
                        f32x2 lo = {__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u)}, hi = {__uint_as_float(u.y << 16), __uint_as_float(u.y & 0xffff0000u)};
                        lo = __builtin_elementwise_fma(lo, sc2, sh2);
                        hi = __builtin_elementwise_fma(hi, sc2, sh2);
                        const s16x2 z2 = {0, 0};
                        s16x2 a2 = __builtin_elementwise_max(__builtin_bit_cast(s16x2, __builtin_convertvector(lo, bf16x2)), z2);
                        s16x2 c2 = __builtin_elementwise_max(__builtin_bit_cast(s16x2, __builtin_convertvector(hi, bf16x2)), z2);
                        if (c0 < 0 || c0 + 15 * g.ssw >= g.Ws) {                    // edge half (wave-uniform test)
                            const int col = c0 + 4 * kq * g.ssw;
                            a2.x = (unsigned)(col) < (unsigned)g.Ws ? a2.x : (short)0; a2.y = (unsigned)(col + g.ssw) < (unsigned)g.Ws ? a2.y : (short)0;
                            c2.x = (unsigned)(col + 2 * g.ssw) < (unsigned)g.Ws ? c2.x : (short)0; c2.y = (unsigned)(col + 3 * g.ssw) < (unsigned)g.Ws ? c2.y : (short)0;
                        }
                        const s16x4 o = {a2.x, a2.y, c2.x, c2.y};
                        xv = o;
                    }
                }
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(xv, gv, acc[t], 0, 0, 0);
            }
            if constexpr (PRO) { cj += 16; if (cj >= g.Wl) { cj = 0; if (++ci >= g.Hl) ci = 0; } }
            bsum += __uint_as_float((unsigned)(unsigned short)gv.x << 16) + __uint_as_float((unsigned)(unsigned short)gv.y << 16) +
                    __uint_as_float((unsigned)(unsigned short)gv.z << 16) + __uint_as_float((unsigned)(unsigned short)gv.w << 16);
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // the trailing (dead) stages: nothing may land in LDS after this
    __shared__ float red[WG_WAVES - 1][NTAPS * 4][64];
    __shared__ float bred[WG_WAVES][64];
    if (wave > 0) {
#pragma unroll
        for (int t = 0; t < NTAPS; ++t)
#pragma unroll
            for (int e = 0; e < 4; ++e) red[wave - 1][t * 4 + e][lane] = acc[t][e];
    }
    bred[wave][lane] = bsum;
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int t = 0; t < NTAPS; ++t) {
            float* out = a.partial + ((long)blockIdx.x * NTAPS + t) * g.Cs * g.Cd;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float v = acc[t][e];
#pragma unroll
                for (int w = 0; w < WG_WAVES - 1; ++w) v += red[w][t * 4 + e][lane];
                out[(long)(4 * kq + e) * g.Cd + pl] = v;          // row = x-channel 4*kq+e, col = g-channel pl
            }
        }
        if (write_bias && a.bias_partial) {
            float v = bred[0][lane] + bred[1][lane] + bred[2][lane] + bred[3][lane];
            v += __shfl_xor(v, 16, 64);
            v += __shfl_xor(v, 32, 64);
            if (kq == 0) a.bias_partial[(long)blockIdx.x * g.Cd + pl] = v;
        }
    }
}

// 16 x 16 channel weight gradient on fp32 tensors through LDS (round 5): tapwgrad16_kernel fetches ONE float per lane and instruction
// -- 16 vector-memory instructions of 256 bytes per 16 pixels; the launch sits on the address units at 43.6 us where its 134 MB take
// 24.  Same ring as the bf16 kernel above, per wave and without a barrier: LDS-DMA copies 16 pixels x 64 bytes of G and of X at
// each of the three tap positions as ONE 1 KB instruction each (lane-linear: pixel l >> 2, 16-byte chunk l & 3; a padding position
// carries the out-of-range offset and lands as zeros), and the MFMA operands -- lane (channel l & 15, pixel slot l >> 4) -- are
// plain ds_read_b32 of 256 contiguous bytes (conflict-free, 2 LDS cycles).  K = 4 pixels per v_mfma_f32_16x16x4_f32, 16 pixels
// per stage.  PRO: BN + ReLU on x in registers (one channel per lane), padding re-zeroed after the transform.
constexpr int W16F_STAGE = 4 * 1024, W16F_STAGES = 4;
template <bool PRO>
__global__ __launch_bounds__(256) void tapwgrad16_f32_kernel(const LfTapGeom g, const LfWgradArgs a, const long pps, const int write_bias) {
    constexpr int NTAPS = 3;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int pl = lane & 15, kq = lane >> 4;
    const long npix = (long)g.N * g.Hl * g.Wl;
    const long sub = (long)blockIdx.x * WG_WAVES + wave;
    const long p_begin = sub * pps;
    long p_end = p_begin + pps;
    if (p_end > npix) p_end = npix;
    const int niter = p_end > p_begin ? (int)((p_end - p_begin + 15) / 16) : 0;
    f32x4 acc[NTAPS];
#pragma unroll
    for (int t = 0; t < NTAPS; ++t) acc[t] = zero4();
    float bsum = 0.f;
    const i32x4s rx = make_rsrc_words(a.x, (unsigned)min((long)g.N * g.Hs * g.Ws * g.s_pix * 4, (long)LF_OOB)),
                 rg = make_rsrc_words(a.g, (unsigned)min((long)g.N * g.Hd * g.Wd * g.d_pix * 4, (long)LF_OOB));
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)lf_tap_lds + (unsigned)(wave * W16F_STAGES * W16F_STAGE);
    typedef __attribute__((address_space(3))) float* lds_f32_p;
    lds_f32_p const frag = (lds_f32_p)((__attribute__((address_space(3))) unsigned char*)lf_tap_lds + wave * W16F_STAGES * W16F_STAGE + kq * 64 + pl * 4);
    const int tdh0 = g.tdh[0], tdh1 = g.tdh[1], tdh2 = g.tdh[2], tdw0 = g.tdw[0], tdw1 = g.tdw[1], tdw2 = g.tdw[2];
    // load cursor: (image, row, column) of the next 16-pixel group (wave-uniform; Wl % 16 == 0: a group lies in one row)
    long p_ld = p_begin;
    int pj, pi, pn;
    row1_coords(g, niter ? (unsigned)p_begin : 0u, pn, pi, pj);
    int cj = pj, ci = pi;                                     // compute cursor (PRO: the padding tests)
    const int px = lane >> 2, chunk = lane & 3;
    auto issue = [&](const int slot) __attribute__((always_inline)) {
        const bool ok = p_ld < p_end;
        const int j = pj + px;
        const unsigned dst = lds0 + (unsigned)(slot * W16F_STAGE);
        const unsigned go = (unsigned)((((pn * g.Hd + pi * g.dsh + g.dah) * g.Wd + j * g.dsw + g.daw) * g.d_pix + g.d_choff + chunk * 4) * 4);
        lds_dma16(rg, dst, ok ? go : LF_OOB, 0u);
#pragma unroll
        for (int t = 0; t < NTAPS; ++t) {
            const int dh = t == 0 ? tdh0 : t == 1 ? tdh1 : tdh2, dw = t == 0 ? tdw0 : t == 1 ? tdw1 : tdw2;
            const int sy = pi * g.ssh + dh, sx = j * g.ssw + dw;
            const bool in = ok && sy >= 0 && sy < g.Hs && sx >= 0 && sx < g.Ws;
            const unsigned xo = (unsigned)((((pn * g.Hs + sy) * g.Ws + sx) * g.s_pix + g.s_choff + chunk * 4) * 4);
            lds_dma16(rx, dst + (unsigned)((1 + t) * 1024), in ? xo : LF_OOB, 0u);
        }
        p_ld += 16;
        pj += 16;
        if (pj >= g.Wl) { pj = 0; if (++pi >= g.Hl) { pi = 0; ++pn; } }
    };
    float psc = 1.f, psh = 0.f;
    if constexpr (PRO) {
        psc = a.pro_sc[pl]; psh = a.pro_sh[pl];
        asm volatile("" ::"v"(psc), "v"(psh) : "memory");      // returned before the hand-counted vmcnt waits of the loop
    }
#pragma unroll
    for (int q = 0; q < W16F_STAGES - 1; ++q) issue(q);
    for (int it0 = 0; it0 < niter; it0 += W16F_STAGES) {
#pragma unroll
        for (int sl = 0; sl < W16F_STAGES; ++sl) {
            if (it0 + sl >= niter) break;
            // my DMA of this stage has landed (two younger stages of 4 instructions may be in flight); my reads of the stage that is
            // restaged next have retired.  The ring is private to the wave: no barrier.
            asm volatile("s_waitcnt vmcnt(8) lgkmcnt(0)" ::: "memory");
            issue((sl + W16F_STAGES - 1) % W16F_STAGES);
            float gv[4], xv[NTAPS][4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                gv[u] = frag[(sl * W16F_STAGE + u * 256) / 4];
#pragma unroll
                for (int t = 0; t < NTAPS; ++t) xv[t][u] = frag[(sl * W16F_STAGE + (1 + t) * 1024 + u * 256) / 4];
            }
            if constexpr (PRO) {
#pragma unroll
                for (int t = 0; t < NTAPS; ++t) {
                    const int dh = t == 0 ? tdh0 : t == 1 ? tdh1 : tdh2, dw = t == 0 ? tdw0 : t == 1 ? tdw1 : tdw2;
                    const bool rowok = (unsigned)(ci * g.ssh + dh) < (unsigned)g.Hs;
                    const int c0 = cj * g.ssw + dw;
                    const bool edge = c0 < 0 || c0 + 15 * g.ssw >= g.Ws;
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        float v = fmaxf(xv[t][u] * psc + psh, 0.f);
                        if (edge) v = (unsigned)(c0 + (4 * u + kq) * g.ssw) < (unsigned)g.Ws ? v : 0.f;
                        xv[t][u] = rowok ? v : 0.f;
                    }
                }
                cj += 16;
                if (cj >= g.Wl) { cj = 0; if (++ci >= g.Hl) ci = 0; }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
#pragma unroll
                for (int t = 0; t < NTAPS; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[t][u], gv[u], acc[t], 0, 0, 0);
                bsum += gv[u];
            }
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // the trailing (dead) stages: nothing may land in LDS after this
    __shared__ float red[WG_WAVES - 1][NTAPS * 4][64];
    __shared__ float bred[WG_WAVES][64];
    if (wave > 0) {
#pragma unroll
        for (int t = 0; t < NTAPS; ++t)
#pragma unroll
            for (int e = 0; e < 4; ++e) red[wave - 1][t * 4 + e][lane] = acc[t][e];
    }
    bred[wave][lane] = bsum;
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int t = 0; t < NTAPS; ++t) {
            float* out = a.partial + ((long)blockIdx.x * NTAPS + t) * g.Cs * g.Cd;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float v = acc[t][e];
#pragma unroll
                for (int w = 0; w < WG_WAVES - 1; ++w) v += red[w][t * 4 + e][lane];
                out[(long)(4 * kq + e) * g.Cd + pl] = v;          // row = x-channel 4*kq+e, col = g-channel pl
            }
        }
        if (write_bias && a.bias_partial) {
            float v = bred[0][lane] + bred[1][lane] + bred[2][lane] + bred[3][lane];
            v += __shfl_xor(v, 16, 64);
            v += __shfl_xor(v, 32, 64);
            if (kq == 0) a.bias_partial[(long)blockIdx.x * g.Cd + pl] = v;
        }
    }
}

struct WgradCfg { int xv, gv, xt, gt, gx, u; long pps; };

WgradCfg wgrad_cfg(const LfTapGeom& g) {
    WgradCfg c;
    c.xv = (g.Cs % 64 == 0);
    c.gv = (g.Cd % 64 == 0);
    c.xt = c.xv ? 4 : g.Cs / 16;
    c.gt = c.gv ? 4 : g.Cd / 16;
    const int xb = c.xt * 16, gb = c.gt * 16;
    const bool small16 = (g.Cs == 16 && g.Cd == 16 && g.ntaps == 3 && g.Wl % 16 == 0);   // all taps in one wave
    const int jobs = small16 ? 1 : g.ntaps * (g.Cs / xb) * (g.Cd / gb);
    const long npix = (long)g.N * g.Hl * g.Wl;
    int gx = (small16 ? 4096 : 2048) / (jobs * WG_WAVES);   // 2 waves/SIMD (254 VGPRs) over 256 CUs; 8 for the lean 16x16 kernel
    if (gx < 1) gx = 1;
    const long maxgx = (npix + 64 * WG_WAVES - 1) / (64 * WG_WAVES);   // at least 64 pixels per wave
    if (gx > maxgx) gx = (int)maxgx;
    if (gx < 1) gx = 1;
    if (!small16) {   // make gx * jobs a multiple of 8 so the kernel's per-XCD ordering applies
        int mlt = 8;
        for (int d = 2; d <= 8; d *= 2) if (jobs % d == 0) mlt = 8 / d;
        if (gx >= mlt) gx = gx / mlt * mlt;
    }
    c.u = (g.Wl % 16 == 0) ? 4 : 1;           // k-steps per loop iteration (16 pixels of one row; 8-pixel iterations at 3 waves/SIMD spill: 1.7x slower)
    const int gran = 4 * c.u;
    long pps = (npix + (long)gx * WG_WAVES - 1) / ((long)gx * WG_WAVES);
    pps = (pps + gran - 1) / gran * gran;
    c.gx = (int)((npix + pps * WG_WAVES - 1) / (pps * WG_WAVES));
    c.pps = pps;
    return c;
}

// tapwgrad_kernel for one (vector mode, channel tiles) choice of wgrad_cfg: picks the storage type, the pixel unroll and -- where
// both operands are in vector mode (VV) -- the bf16-MFMA form on bf16 tensors and the compiled-in prologue choice on fp32 ones.
// (VV also compiles the two forms without either, which no launch takes: dropping them is a change of the device code)
template <bool XV, bool GV, int XT, int GT>
void launch_wgrad(const LfTapGeom& g, const LfWgradArgs& a, int pro, const WgradCfg& c, dim3 grid, int wb, hipStream_t st) {
    constexpr bool VV = XV && GV;
    auto go = [&](auto kern) { hipLaunchKernelGGL(kern, grid, dim3(256), 0, st, g, a, pro, c.pps, wb, c.gx); };
    if (a.s16 && c.u == 4 && VV) go(tapwgrad_kernel<XV, GV, XT, GT, 4, true, VV>);
    else if (a.s16 && c.u == 4) go(tapwgrad_kernel<XV, GV, XT, GT, 4, true>);
    else if (a.s16) go(tapwgrad_kernel<XV, GV, XT, GT, 1, true>);
    else if (c.u == 4 && VV) {
        if constexpr (VV) {
            if (pro == LF_PRO_BNRELU) go(tapwgrad_kernel<XV, GV, XT, GT, 4, false, false, 1>);
            else go(tapwgrad_kernel<XV, GV, XT, GT, 4, false, false, 0>);
        }
    } else if (c.u == 4) go(tapwgrad_kernel<XV, GV, XT, GT, 4, false>);
    else go(tapwgrad_kernel<XV, GV, XT, GT, 1, false>);
}

}  // namespace

int lf_tapwgrad_splits(const LfTapGeom& g) { return wgrad_cfg(g).gx; }
long lf_tapwgrad_wave_pixels(const LfTapGeom& g) { return wgrad_cfg(g).pps; }
int lf_tapwgrad_splits_bound(const LfTapGeom& g, int s16) {
    const int a = lf_tapwgrad_splits(g), c = s16 ? lf_tapwgrad_ro_rows_bound(g) : 0;
    return a > c ? a : c;
}
int lf_tapwgrad_splits_for(const LfTapGeom& g, const LfWgradArgs& a, int pro) {
    if (lf_tapwgrad_ro_ok(g, a.s16) && !a.dbg) return lf_tapwgrad_ro_rows(g);
    (void)pro;
    return wgrad_cfg(g).gx;
}

int lf_tapwgrad_launch(const LfTapGeom& g, const LfWgradArgs& a, int pro, hipStream_t st) {
    LF_REQUIRE(g.Cs % 16 == 0 && g.Cd % 16 == 0, "tapwgrad: channels must be multiples of 16");
    LF_REQUIRE(g.Wl % 4 == 0, "tapwgrad: logical width %d must be a multiple of 4", g.Wl);
    LF_REQUIRE((long)g.N * g.Hs * g.Ws * g.s_pix < (long)(LF_OOB >> 2) && (long)g.N * g.Hd * g.Wd * g.d_pix < (long)(LF_OOB >> 2),
               "tapwgrad: tensor too large for 32-bit byte offsets");
    if (lf_tapwgrad_ro_ok(g, a.s16) && !a.dbg) return lf_tapwgrad_ro_launch(g, a, pro, st);     // bf16 tensors, 3 taps, 64 / 128 channels
    const int wb = a.bias_partial != nullptr;
    const WgradCfg c = wgrad_cfg(g);
    const int xb = c.xt * 16, gb = c.gt * 16;
    if (g.Cs == 16 && g.Cd == 16 && g.ntaps == 3 && g.Wl % 16 == 0) {
        // both LDS-ring forms need 16-byte-aligned pixels of both tensors inside 32-bit byte offsets, and the LDS attribute
        const bool ring_ok = lf_tapgemm_bf16_lds() >= 3 && g.s_pix % 8 == 0 && g.s_choff % 8 == 0 && g.d_pix % 8 == 0 && g.d_choff % 8 == 0 &&
                             (long)g.N * g.Hs * g.Ws * g.s_pix * (a.s16 ? 2 : 4) < (long)LF_OOB && (long)g.N * g.Hd * g.Wd * g.d_pix * (a.s16 ? 2 : 4) < (long)LF_OOB;
        const size_t ring_lds = (size_t)WG_WAVES * W16_STAGES * W16_STAGE;
        static_assert(W16F_STAGES * W16F_STAGE == W16_STAGES * W16_STAGE, "the two 16-channel rings share their LDS budget");
        const bool pr = pro == LF_PRO_BNRELU;
        auto ring = [&](auto kern) {
            if (!allow_big_lds(reinterpret_cast<const void*>(kern), 128 * 1024)) return false;
            hipLaunchKernelGGL(kern, dim3(c.gx), dim3(256), ring_lds, st, g, a, c.pps, wb);
            return true;
        };
        bool launched = false;
        if (ring_ok && a.s16) launched = pr ? ring(tapwgrad16_tr_kernel<true>) : ring(tapwgrad16_tr_kernel<false>);
        else if (ring_ok) launched = pr ? ring(tapwgrad16_f32_kernel<true>) : ring(tapwgrad16_f32_kernel<false>);
        if (!launched) {           // (attribute refused, unaligned channel layout): the one-element-per-lane kernel
            if (a.s16) hipLaunchKernelGGL((tapwgrad16_kernel<3, true>), dim3(c.gx), dim3(256), 0, st, g, a, pro, c.pps, wb);
            else hipLaunchKernelGGL((tapwgrad16_kernel<3, false>), dim3(c.gx), dim3(256), 0, st, g, a, pro, c.pps, wb);
        }
        LF_CHECK_LAUNCH("tapwgrad16");
        return 0;
    }
    dim3 grid(c.gx * g.ntaps * (g.Cs / xb) * (g.Cd / gb));
    if (a.dbg) {           // phase stamps (tools/kbench.py --phases --wgrad): the fp32 64-channel-block kernel without prologue only
        LF_REQUIRE(c.xv && c.gv && c.u == 4 && !a.s16 && pro == LF_PRO_NONE, "tapwgrad: phase stamps are compiled into the plain fp32 kernel only");
        hipLaunchKernelGGL((tapwgrad_kernel<true, true, 4, 4, 4, false, false, 0, true>), grid, dim3(256), 0, st, g, a, pro, c.pps, wb, c.gx);
        LF_CHECK_LAUNCH("tapwgrad (stamps)");
        return 0;
    }
    if (c.xv && c.gv) launch_wgrad<true, true, 4, 4>(g, a, pro, c, grid, wb, st);
    else if (c.xv && c.gt == 1) launch_wgrad<true, false, 4, 1>(g, a, pro, c, grid, wb, st);
    else if (c.xv && c.gt == 3) launch_wgrad<true, false, 4, 3>(g, a, pro, c, grid, wb, st);
    else if (!c.xv && c.xt == 1 && c.gv) launch_wgrad<false, true, 1, 4>(g, a, pro, c, grid, wb, st);
    else if (!c.xv && c.xt == 1 && c.gt == 1) launch_wgrad<false, false, 1, 1>(g, a, pro, c, grid, wb, st);
    else if (!c.xv && c.xt == 1 && c.gt == 3) launch_wgrad<false, false, 1, 3>(g, a, pro, c, grid, wb, st);
    else if (!c.xv && c.xt == 3 && c.gt == 1) launch_wgrad<false, false, 3, 1>(g, a, pro, c, grid, wb, st);
    else if (!c.xv && c.xt == 3 && c.gv) launch_wgrad<false, true, 3, 4>(g, a, pro, c, grid, wb, st);
    else return lf_fail("tapwgrad: unsupported channel combination Cs=%d Cd=%d", g.Cs, g.Cd);
    LF_CHECK_LAUNCH("tapwgrad");
    return 0;
}

// ---------------------------------------------------------------------------------------
// split-K reduction + scatter into the PyTorch parameter-gradient layout; bias rows
// ---------------------------------------------------------------------------------------
namespace {

__global__ __launch_bounds__(1024) void wgrad_reduce_kernel(const float* __restrict__ partial, int splits, int ntaps,
                                                           int Cs, int Cd, float* __restrict__ grad, long sk, long sn,
                                                           TapIdx ti, int wblocks, const float* __restrict__ brows,
                                                           int nbrows, float* __restrict__ bgrad, int baccum) {
    constexpr int SG = 16;                                       // 64 outputs x 16 split groups per block
    __shared__ float sw[SG][64];
    const int og = threadIdx.x & 63, sg = threadIdx.x >> 6;
    if ((int)blockIdx.x >= wblocks) {   // trailing blocks: bias gradient = column sums of the bias partial rows
        const int c = (blockIdx.x - wblocks) * 64 + og;
        float s = 0.f;
        if (c < Cd)
            for (int r = sg; r < nbrows; r += SG) s += brows[(long)r * Cd + c];
        sw[sg][og] = s;
        __syncthreads();
        if (sg == 0 && c < Cd) {
            float v = 0.f;
#pragma unroll
            for (int k = 0; k < SG; ++k) v += sw[k][og];
            bgrad[c] = baccum ? bgrad[c] + v : v;
        }
        return;
    }
    const long per = (long)ntaps * Cs * Cd;
    for (long base = (long)blockIdx.x * 64; base < per; base += (long)wblocks * 64) {
        const long i = base + og;
        float s0 = 0.f, s1 = 0.f;
        if (i < per) {
            int r = sg;
            for (; r + SG < splits; r += 2 * SG) { s0 += partial[(long)r * per + i]; s1 += partial[(long)(r + SG) * per + i]; }
            for (; r < splits; r += SG) s0 += partial[(long)r * per + i];
        }
        sw[sg][og] = s0 + s1;
        __syncthreads();
        if (sg == 0 && i < per) {
            float v = 0.f;
#pragma unroll
            for (int k = 0; k < SG; ++k) v += sw[k][og];          // fixed order: deterministic
            const int n = (int)(i % Cd);
            const long r2 = i / Cd;
            const int k2 = (int)(r2 % Cs), t = (int)(r2 / Cs);
            grad[k2 * sk + n * sn + ti.v[t]] = v;
        }
        __syncthreads();
    }
}

struct ReduceBatch { LfReduceJob j[LF_REDUCE_BATCH]; int blk0[LF_REDUCE_BATCH + 1]; };

// One workgroup = 64 outputs x 4 split groups; a thread sums every 4th partial row in four independent chains, the
// groups are combined through LDS in a fixed order (deterministic; not the summation order of wgrad_reduce_kernel).
// The workgroups of a job come first for its ntaps*Cs*Cd outputs, then one per 64 bias columns.
__global__ __launch_bounds__(256) void wgrad_reduce_batch_kernel(const ReduceBatch B) {
    __shared__ float sw[4][64];
    int jb = 0;
    while (jb + 1 < LF_REDUCE_BATCH && (int)blockIdx.x >= B.blk0[jb + 1]) ++jb;      // uniform scan, <= 32 entries
    const LfReduceJob& J = B.j[jb];
    const int blk = blockIdx.x - B.blk0[jb];
    const int og = threadIdx.x & 63, sg = threadIdx.x >> 6;
    const long per = (long)J.ntaps * J.Cs * J.Cd;
    const int wblocks = (int)((per + 63) / 64);
    const float* __restrict__ rows;
    long width, i;
    int nrows;
    if (blk < wblocks) { rows = J.partial; width = per; i = (long)blk * 64 + og; nrows = J.splits; }
    else { rows = J.bias_rows; width = J.Cd; i = (long)(blk - wblocks) * 64 + og; nrows = J.n_bias_rows; }
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    if (i < width) {
        int r = sg;
        for (; r + 12 < nrows; r += 16) {
            s0 += rows[(long)r * width + i]; s1 += rows[(long)(r + 4) * width + i];
            s2 += rows[(long)(r + 8) * width + i]; s3 += rows[(long)(r + 12) * width + i];
        }
        for (; r < nrows; r += 4) s0 += rows[(long)r * width + i];
    }
    sw[sg][og] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    if (sg == 0 && i < width) {
        const float v = (sw[0][og] + sw[1][og]) + (sw[2][og] + sw[3][og]);
        if (blk < wblocks) {
            const int n = (int)(i % J.Cd);
            const long r2 = i / J.Cd;
            const int k2 = (int)(r2 % J.Cs), t = (int)(r2 / J.Cs);
            J.grad[k2 * J.sk + n * J.sn + J.tapidx[t]] = v;
        } else {
            J.bias_grad[i] = v;
        }
    }
}

__global__ __launch_bounds__(256) void rows_reduce_kernel(const float* __restrict__ rows, int nrows, int C,
                                                         float* __restrict__ dst, int accumulate) {
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), rg = threadIdx.x >> 6;
    __shared__ float sb[4][64];
    float s0 = 0.f, s1 = 0.f;
    if (c < C) {
        int r = rg;
        for (; r + 4 < nrows; r += 8) { s0 += rows[(long)r * C + c]; s1 += rows[(long)(r + 4) * C + c]; }
        for (; r < nrows; r += 4) s0 += rows[(long)r * C + c];
    }
    sb[rg][threadIdx.x & 63] = s0 + s1;
    __syncthreads();
    if (rg == 0 && c < C) {
        const float v = (sb[0][threadIdx.x] + sb[1][threadIdx.x]) + (sb[2][threadIdx.x] + sb[3][threadIdx.x]);
        dst[c] = accumulate ? dst[c] + v : v;
    }
}
}  // namespace

int lf_wgrad_reduce_launch(const float* partial, int splits, int ntaps, int Cs, int Cd, float* grad, long sk, long sn,
                           const int* tapidx_host, const float* bias_rows, int n_bias_rows, float* bias_grad,
                           int bias_accumulate, hipStream_t st) {
    TapIdx ti;
    for (int i = 0; i < LF_MAX_TAPS; ++i) ti.v[i] = i < ntaps ? tapidx_host[i] : 0;
    const long per = (long)ntaps * Cs * Cd;
    int wblocks = lf_cdiv(per, 64);
    if (wblocks > 4096) wblocks = 4096;
    const int bblocks = (bias_rows && bias_grad) ? lf_cdiv(Cd, 64) : 0;
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(wblocks + bblocks), dim3(1024), 0, st, partial, splits, ntaps, Cs, Cd, grad,
                       sk, sn, ti, wblocks, bias_rows, n_bias_rows, bias_grad, bias_accumulate);
    LF_CHECK_LAUNCH("wgrad_reduce");
    return 0;
}

int lf_wgrad_reduce_batch_launch(const LfReduceJob* jobs_host, int njobs, hipStream_t st) {
    for (int j0 = 0; j0 < njobs; j0 += LF_REDUCE_BATCH) {
        const int n = njobs - j0 < LF_REDUCE_BATCH ? njobs - j0 : LF_REDUCE_BATCH;
        ReduceBatch B;
        memset(&B, 0, sizeof(B));
        int blocks = 0;
        for (int i = 0; i < LF_REDUCE_BATCH; ++i) {
            B.blk0[i] = blocks;
            if (i >= n) continue;
            const LfReduceJob& J = jobs_host[j0 + i];
            B.j[i] = J;
            blocks += lf_cdiv((long)J.ntaps * J.Cs * J.Cd, 64) + ((J.bias_rows && J.bias_grad) ? lf_cdiv(J.Cd, 64) : 0);
        }
        B.blk0[LF_REDUCE_BATCH] = blocks;
        hipLaunchKernelGGL(wgrad_reduce_batch_kernel, dim3(blocks), dim3(256), 0, st, B);
        LF_CHECK_LAUNCH("wgrad_reduce_batch");
    }
    return 0;
}

int lf_rows_reduce_launch(const float* rows, int nrows, int C, float* dst, int accumulate, hipStream_t st) {
    hipLaunchKernelGGL(rows_reduce_kernel, dim3(lf_cdiv(C, 64)), dim3(256), 0, st, rows, nrows, C, dst, accumulate);
    LF_CHECK_LAUNCH("rows_reduce");
    return 0;
}
