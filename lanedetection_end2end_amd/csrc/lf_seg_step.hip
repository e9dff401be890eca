// ---------------------------------------------------------------------------------------
// Segmentation-mode step criterion (lf_seg_step): what a step of Net.forward(end_to_end=False) does behind the backbone --
// criterion_seg(output_net, gt) with its gradient, the arg-max lane maps and their fit (BP/main.py:306-318, BEV/main.py:241-244,
// BP/Networks/LSQ_layer.py:279-314) -- in one read of the logits, one read of the target and one write of the gradient.
//   seg_label_kernel    per-class pixel counts of the target as integers: the loss normaliser sum w[t] is exact and has no order;
//   seg_step_kernel     VEC consecutive pixels of a row per thread: max, first arg-max, logsumexp, w[t] (lse - z_t) and the gradient
//                       w[t] / sum w (softmax - onehot) in ce_fwd_kernel's / ce_bwd_kernel's fp32 arithmetic; on rows >= zero_rows a
//                       pixel whose arg-max is class l + 1 <= L adds (l + 1)^2 y^j and (l + 1)^2 x y^j to lane l's fp64 moments, as
//                       Moments<ORDER>::add does for a map valued l + 1 there.  The lane is picked by predicated adds, never by an
//                       index into the accumulators; the grid of a masked row and of a pixel of no lane is not read;
//   seg_finish_kernel   adds the workgroups' loss and moment partials from their fixed slots in a fixed order, gives flagged lanes the
//                       moments of lane (0, 0) ("prevent singular matrix"), solves, writes out / meters, re-zeroes the counts.
// No floating-point atomics, no workgroup waits for another.
// ---------------------------------------------------------------------------------------
#include "lf_common.h"
#include "lf_solve.h"

namespace {

constexpr int SG_THREADS = 256;
constexpr int SG_MAXC = CE_MAXC;    // the class cap of lf_ce2d_fwd (lf_common.h)
constexpr int SG_MAXL = 4;
constexpr int SG_MAXCHUNKS = 128;   // workgroups per image at most
constexpr int SG_COUNT_BYTES = 128; // SG_MAXC class counts + the out-of-range count, uint64, at the head of the workspace

// workgroups per image: about 4096 pixels each
inline int seg_chunks(int H, int W) {
    const long c = ((long)H * W + 4095) / 4096;
    return (int)(c < 1 ? 1 : (c > SG_MAXCHUNKS ? SG_MAXCHUNKS : c));
}
constexpr int seg_nmom(int order) { return 3 * order + 2; }

__global__ __launch_bounds__(SG_THREADS) void seg_label_kernel(const int64_t* __restrict__ tgt, long total, int C,
                                                              unsigned long long* __restrict__ counts) {
    unsigned cnt[SG_MAXC + 1] = {};
    for (long i = (long)blockIdx.x * SG_THREADS + threadIdx.x; i < total; i += (long)gridDim.x * SG_THREADS) {
        const int64_t t = tgt[i];
        const bool ok = t >= 0 && t < C;
#pragma unroll
        for (int c = 0; c < SG_MAXC; ++c) cnt[c] += (ok && t == c) ? 1u : 0u;
        cnt[SG_MAXC] += ok ? 0u : 1u;
    }
#pragma unroll
    for (int c = 0; c <= SG_MAXC; ++c) {
        unsigned v = cnt[c];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if ((threadIdx.x & 63) == 0 && v != 0u) atomicAdd(counts + c, (unsigned long long)v);      // integers: exact in any order
    }
}

// sum w[t] over the labelled pixels from the class counts, classes ascending: the same bits in every workgroup and in the finish
__device__ __forceinline__ double seg_weight_sum(const float* __restrict__ wts, const unsigned long long* __restrict__ counts, int C) {
    double den = 0.0;
#pragma unroll
    for (int c = 0; c < SG_MAXC; ++c)
        if (c < C) den = fma((double)wts[c], (double)counts[c], den);
    return den;
}

struct SegArgs {
    const float* z;
    const int64_t* tgt;
    const float* wts;
    const float* grid;
    long gbs;
    int C, L, H, W, zero_rows, CH;
    long per;                   // units of VEC pixels per workgroup: ceil(units / CH)
    float y_off;
    float* grad;
    float* maps;
    const unsigned long long* counts;
    double* lossp;              // (N, CH)
    double* momp;               // (N, L, CH, 3 * order + 2): wls_solve_kernel's layout with CH chunks
};

// ORDER < 0: cross entropy only.  LMAX: lanes compiled in (2 or 4); a.L <= LMAX of them are live.  VEC = 4 wants W % 4 == 0 and
// 16-byte aligned tensors.
template <int ORDER, int LMAX, int VEC>
__global__ __launch_bounds__(SG_THREADS) void seg_step_kernel(const SegArgs a) {
    constexpr bool FIT = ORDER >= 0;
    constexpr int NM = FIT ? 2 * ORDER + 1 : 1, NQ = FIT ? ORDER + 1 : 0, NMOM = NM + NQ;
    constexpr int NRED = 1 + (FIT ? LMAX * NMOM : 0);
    __shared__ double red[SG_THREADS / LF_WAVE][NRED];
    const int n = blockIdx.y, chunk = blockIdx.x, C = a.C, L = a.L;
    const long P = (long)a.H * a.W;
    // the class weights in LDS (zero past C), and from them and the label counts the normaliser: classes ascending, the same bits
    // in every workgroup and in the finish (a class past C adds +0)
    __shared__ float wsh[SG_MAXC];
    if (threadIdx.x < SG_MAXC) wsh[threadIdx.x] = (int)threadIdx.x < C ? a.wts[threadIdx.x] : 0.f;
    __syncthreads();
    double den = 0.0;
#pragma unroll
    for (int c = 0; c < SG_MAXC; ++c) den = fma((double)wsh[c], (double)a.counts[c], den);
    const float scale = 1.f / (float)den;
    const float* z = a.z + (long)n * C * P;
    const int64_t* tg = a.tgt + (long)n * P;
    float* g = a.grad ? a.grad + (long)n * C * P : nullptr;
    const float* grid = FIT ? a.grid + (long)n * a.gbs : nullptr;
    float* maps = FIT && a.maps ? a.maps + (long)n * L * P : nullptr;
    const long first = (long)a.zero_rows * a.W;
    const unsigned P32 = (unsigned)P;
    const long units = P / VEC;
    const long u0 = a.per * chunk, u1 = u0 + a.per < units ? u0 + a.per : units;
    double num = 0.0;
    double mom[LMAX][NMOM];
#pragma unroll
    for (int l = 0; l < LMAX; ++l)
#pragma unroll
        for (int j = 0; j < NMOM; ++j) mom[l][j] = 0.0;
    for (long u = u0 + threadIdx.x; u < u1; u += SG_THREADS) {
        const long p = u * VEC;
        // (offsets inside one image fit 32 bits -- the entry point checks -- so a class plane costs one scalar, not a pointer pair)
        const unsigned p32 = (unsigned)p;
        float v[SG_MAXC][VEC];
#pragma unroll
        for (int c = 0; c < SG_MAXC; ++c)
            if (c < C) load_px<VEC>(z + ((unsigned)c * P32 + p32), v[c]);
        int64_t t64[VEC];
        if constexpr (VEC == 4) {
            const longlong2 t0 = *reinterpret_cast<const longlong2*>(tg + p);
            const longlong2 t1 = *reinterpret_cast<const longlong2*>(tg + p + 2);
            t64[0] = t0.x; t64[1] = t0.y; t64[2] = t1.x; t64[3] = t1.y;
        } else {
            t64[0] = tg[p];
        }
        const bool live = FIT && p >= first;          // (a unit of four pixels lies in one row)
        int lane_of[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            // first maximum, NaN counts as maximal: seg_maps_kernel's arg-max; the max of the logsumexp is ce_fwd_kernel's fmaxf chain
            float best = v[0][e], mx = v[0][e];
            int am = 0;
#pragma unroll
            for (int c = 1; c < SG_MAXC; ++c)
                if (c < C) {
                    const float x = v[c][e];
                    if (x > best || (x != x && best == best)) { best = x; am = c; }
                    mx = fmaxf(mx, x);
                }
            const bool okt = t64[e] >= 0 && t64[e] < C;    // a label outside [0, C) carries weight 0 (and was counted by the label pass)
            const int t = okt ? (int)t64[e] : 0;
            float zt = 0.f, se = 0.f;
#pragma unroll
            for (int c = 0; c < SG_MAXC; ++c)
                if (c < C) {
                    zt = (c == t) ? v[c][e] : zt;
                    v[c][e] = expf(v[c][e] - mx);
                    se += v[c][e];
                }
            const float w = okt ? wsh[t] : 0.f;
            num += (double)(w * (mx + logf(se) - zt));
            const float ws = w * scale, ise = 1.f / se;
#pragma unroll
            for (int c = 0; c < SG_MAXC; ++c)
                if (c < C) v[c][e] = ws * (v[c][e] * ise - (c == t ? 1.f : 0.f));
            lane_of[e] = (live && am >= 1 && am <= L) ? am : 0;
        }
        if (g) {
#pragma unroll
            for (int c = 0; c < SG_MAXC; ++c)
                if (c < C) store_px<VEC>(g + ((unsigned)c * P32 + p32), v[c]);
        }
        if constexpr (FIT) {
            bool any = false;
#pragma unroll
            for (int e = 0; e < VEC; ++e) any = any || lane_of[e] != 0;
            if (any) {
                float gxy[2 * VEC];
                if constexpr (VEC == 4) {
                    const float4 g0 = *reinterpret_cast<const float4*>(grid + 2 * p);
                    const float4 g1 = *reinterpret_cast<const float4*>(grid + 2 * p + 4);
                    gxy[0] = g0.x; gxy[1] = g0.y; gxy[2] = g0.z; gxy[3] = g0.w;
                    gxy[4] = g1.x; gxy[5] = g1.y; gxy[6] = g1.z; gxy[7] = g1.w;
                } else {
                    gxy[0] = grid[2 * p];
                    gxy[1] = grid[2 * p + 1];
                }
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    if (lane_of[e] == 0) continue;
                    const double x = (double)gxy[2 * e], y = (double)(a.y_off - gxy[2 * e + 1]);
                    // (the lane's selector is a 0 / 1 factor in a register: sixteen compare masks held across the loop spill scalars)
                    double sel[LMAX];
#pragma unroll
                    for (int l = 0; l < LMAX; ++l) sel[l] = (lane_of[e] == l + 1) ? 1.0 : 0.0;
                    double tt = (double)(lane_of[e] * lane_of[e]);
#pragma unroll
                    for (int j = 0; j < NM; ++j) {
#pragma unroll
                        for (int l = 0; l < LMAX; ++l) {
                            const double tl = tt * sel[l];
                            mom[l][j] += tl;
                            if (j < NQ) mom[l][NM + j] = fma(tl, x, mom[l][NM + j]);
                        }
                        tt *= y;
                    }
                }
            }
            if (maps) {
#pragma unroll
                for (int l = 0; l < LMAX; ++l)
                    if (l < L) {
                        float m[VEC];
#pragma unroll
                        for (int e = 0; e < VEC; ++e) m[e] = (lane_of[e] == l + 1) ? (float)(l + 1) : 0.f;
                        store_px<VEC>(maps + ((unsigned)l * P32 + p32), m);
                    }
            }
        }
    }
    // the workgroup's sums into its own slots: a butterfly per wave, then the four waves in ascending order
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    {
        const double s = lf_wave_sum(num);
        if (lane == 0) red[wave][0] = s;
    }
    if constexpr (FIT) {
#pragma unroll
        for (int l = 0; l < LMAX; ++l)
#pragma unroll
            for (int j = 0; j < NMOM; ++j) {
                const double s = lf_wave_sum(mom[l][j]);
                if (lane == 0) red[wave][1 + l * NMOM + j] = s;
            }
    }
    __syncthreads();
    if (threadIdx.x < NRED) {
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < SG_THREADS / LF_WAVE; ++w) s += red[w][threadIdx.x];
        if (threadIdx.x == 0) {
            a.lossp[(long)n * a.CH + chunk] = s;
        } else if constexpr (FIT) {
            const int l = ((int)threadIdx.x - 1) / NMOM, j = ((int)threadIdx.x - 1) % NMOM;
            if (l < L) a.momp[(((long)n * L + l) * a.CH + chunk) * NMOM + j] = s;
        }
    }
}

struct SegFinish {
    const double* lossp;
    const double* momp;
    unsigned long long* counts;
    const float* wts;
    const float* flags;         // (N, L) fp32 or NULL
    int N, C, L, CH, solver;
    double reg;
    double* beta;
    int32_t* status;
    double* out;
    double* meters;
};

// workgroup 0: the loss; workgroups 1..: one thread per (image, lane), wls_solve_kernel's solve (lf_solve_moments) without the Z^-1 output
template <int ORDER>
__global__ __launch_bounds__(LF_WAVE) void seg_finish_kernel(const SegFinish f) {
    if (blockIdx.x == 0) {
        const long slots = (long)f.N * f.CH;
        double s = 0.0;
        for (long i = threadIdx.x; i < slots; i += LF_WAVE) s += f.lossp[i];
        s = lf_wave_sum(s);
        if (threadIdx.x == 0) {
            const double den = seg_weight_sum(f.wts, f.counts, f.C);
            const double loss = s / den;
            f.out[0] = loss; f.out[1] = s; f.out[2] = den; f.out[3] = (double)f.counts[SG_MAXC];
            if (f.meters) { f.meters[0] += loss * f.N; f.meters[1] += f.N; }
            for (int c = 0; c <= SG_MAXC; ++c) f.counts[c] = 0ull;       // the next call's label pass starts from zero
        }
        return;
    }
    if constexpr (ORDER >= 0) {
        constexpr int D = ORDER + 1, NMOM = 3 * ORDER + 2;
        const int nk = ((int)blockIdx.x - 1) * LF_WAVE + (int)threadIdx.x;
        if (nk >= f.N * f.L) return;
        // "prevent singular matrix" (BP/Networks/LSQ_layer.py:308-311): a flagged lane fits map [0, 0]
        const int src = (f.flags && f.flags[nk] != 0.f) ? 0 : nk;
        double mom[NMOM];
#pragma unroll
        for (int j = 0; j < NMOM; ++j) mom[j] = 0.0;
        for (int c = 0; c < f.CH; ++c)
#pragma unroll
            for (int j = 0; j < NMOM; ++j) mom[j] += f.momp[((long)src * f.CH + c) * NMOM + j];
        double b[D], Zi[D][D];
        const int st = lf_solve_moments<ORDER>(mom, f.reg, f.solver, b, Zi);
#pragma unroll
        for (int i = 0; i < D; ++i) f.beta[(long)nk * D + i] = b[i];
        f.status[nk] = st;
    }
}

// with maps AND flags: a flagged lane's map is map [0, 0] (lf_seg_maps); lane (0, 0) itself is left as it is
__global__ __launch_bounds__(SG_THREADS) void seg_flag_maps_kernel(float* __restrict__ maps, const float* __restrict__ flags, long P) {
    const int nk = blockIdx.y;
    if (nk == 0 || flags[nk] == 0.f) return;
    const float* src = maps;
    float* dst = maps + (long)nk * P;
    for (long i = (long)blockIdx.x * SG_THREADS + threadIdx.x; i < P; i += (long)gridDim.x * SG_THREADS) dst[i] = src[i];
}

// grad *= upstream, in place; every workgroup reads the scalar first and leaves at once when it is exactly 1
__global__ __launch_bounds__(SG_THREADS) void seg_scale_kernel(float* __restrict__ g, long n, int vec, const float* __restrict__ up) {
    const float u = up[0];
    if (u == 1.0f) return;
    const long n4 = vec ? n / 4 : 0;
    const long i0 = (long)blockIdx.x * SG_THREADS + threadIdx.x, step = (long)gridDim.x * SG_THREADS;
    for (long i = i0; i < n4; i += step) {
        float4 t = reinterpret_cast<float4*>(g)[i];
        t.x *= u; t.y *= u; t.z *= u; t.w *= u;
        reinterpret_cast<float4*>(g)[i] = t;
    }
    for (long i = 4 * n4 + i0; i < n; i += step) g[i] *= u;
}

inline bool seg_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

template <int ORDER, int LMAX>
void seg_step_launch(const SegArgs& a, int N, int vec, hipStream_t st) {
    const dim3 grid(a.CH, N);
    if (vec == 4) hipLaunchKernelGGL((seg_step_kernel<ORDER, LMAX, 4>), grid, dim3(SG_THREADS), 0, st, a);
    else hipLaunchKernelGGL((seg_step_kernel<ORDER, LMAX, 1>), grid, dim3(SG_THREADS), 0, st, a);
}

}  // namespace

extern "C" size_t lf_seg_step_workspace_bytes(int N, int C, int L, int H, int W, int order) {
    if (N <= 0 || H <= 0 || W <= 0) return 0;
    (void)C;
    const size_t ch = (size_t)seg_chunks(H, W);
    size_t bytes = SG_COUNT_BYTES + (size_t)N * ch * sizeof(double);
    if (L > 0 && order >= 0) bytes += (size_t)N * L * ch * seg_nmom(order) * sizeof(double);
    return bytes;
}

extern "C" int lf_seg_step(const float* logits, const int64_t* target, const float* weights, const float* grid_xy,
                           long grid_batch_stride, const float* gt_line, int N, int C, int L, int H, int W, int zero_rows, int order,
                           double reg, double y_offset, int solver, float* grad_logits, float* maps, double* beta, int32_t* status,
                           double* out, double* meters, void* workspace, void* stream) {
    LF_REQUIRE(logits && target && weights && out && workspace, "lf_seg_step: null pointer");
    LF_REQUIRE(N > 0 && N <= 65535 && H > 0 && W > 0, "lf_seg_step: bad shape (N=%d H=%d W=%d)", N, H, W);
    LF_REQUIRE(C >= 1 && C <= SG_MAXC, "lf_seg_step: C=%d not in 1..%d", C, SG_MAXC);
    LF_REQUIRE((long)H * W * SG_MAXC < (1L << 30), "lf_seg_step: H*W = %ld beyond the 32-bit plane offsets", (long)H * W);
    const bool fit = grid_xy != nullptr;
    if (fit) {
        LF_REQUIRE(beta && status, "lf_seg_step: the fit writes beta and status");
        LF_REQUIRE(L >= 1 && L <= SG_MAXL, "lf_seg_step: L=%d not in 1..%d", L, SG_MAXL);
        LF_REQUIRE(order >= 0 && order <= 3, "lf_seg_step: order %d not in 0..3", order);
        LF_REQUIRE(zero_rows >= 0 && zero_rows <= H, "lf_seg_step: zero_rows %d not in 0..%d", zero_rows, H);
        LF_REQUIRE(solver == LF_SOLVE_LU || solver == LF_SOLVE_CHOLESKY, "lf_seg_step: bad solver %d", solver);
        LF_REQUIRE(grid_batch_stride == 0 || grid_batch_stride >= 2L * H * W, "lf_seg_step: grid_batch_stride %ld below 2*H*W",
                   grid_batch_stride);
    } else {
        LF_REQUIRE(!maps && !gt_line, "lf_seg_step: maps and gt_line belong to the fit (grid_xy is NULL)");
    }
    hipStream_t st = (hipStream_t)stream;
    const long P = (long)H * W, total = (long)N * P;
    const int CH = seg_chunks(H, W);
    unsigned long long* counts = (unsigned long long*)workspace;
    double* lossp = (double*)((char*)workspace + SG_COUNT_BYTES);
    double* momp = lossp + (size_t)N * CH;

    int lblocks = lf_cdiv(total, SG_THREADS * 4);
    if (lblocks > 1024) lblocks = 1024;
    hipLaunchKernelGGL(seg_label_kernel, dim3(lblocks), dim3(SG_THREADS), 0, st, target, total, C, counts);
    LF_CHECK_LAUNCH("seg_label");

    SegArgs a;
    memset(&a, 0, sizeof(a));
    a.z = logits; a.tgt = target; a.wts = weights; a.grid = grid_xy; a.gbs = grid_batch_stride;
    a.C = C; a.L = fit ? L : 0; a.H = H; a.W = W; a.zero_rows = zero_rows; a.CH = CH; a.y_off = (float)y_offset;
    a.grad = grad_logits; a.maps = maps; a.counts = counts; a.lossp = lossp; a.momp = momp;
    const bool vec = W % 4 == 0 && seg_aligned16(logits) && seg_aligned16(target) && (!grad_logits || seg_aligned16(grad_logits)) &&
                     (!fit || (seg_aligned16(grid_xy) && grid_batch_stride % 4 == 0)) && (!maps || seg_aligned16(maps));
    const int v = vec ? 4 : 1;
    a.per = (P / v + CH - 1) / CH;
    const int key = fit ? order * 2 + (L > 2 ? 1 : 0) : -1;
    switch (key) {
        case -1: seg_step_launch<-1, 1>(a, N, v, st); break;
        case 0: seg_step_launch<0, 2>(a, N, v, st); break;
        case 1: seg_step_launch<0, 4>(a, N, v, st); break;
        case 2: seg_step_launch<1, 2>(a, N, v, st); break;
        case 3: seg_step_launch<1, 4>(a, N, v, st); break;
        case 4: seg_step_launch<2, 2>(a, N, v, st); break;
        case 5: seg_step_launch<2, 4>(a, N, v, st); break;
        case 6: seg_step_launch<3, 2>(a, N, v, st); break;
        default: seg_step_launch<3, 4>(a, N, v, st); break;
    }
    LF_CHECK_LAUNCH("seg_step");

    SegFinish f;
    memset(&f, 0, sizeof(f));
    f.lossp = lossp; f.momp = momp; f.counts = counts; f.wts = weights; f.flags = fit ? gt_line : nullptr;
    f.N = N; f.C = C; f.L = a.L; f.CH = CH; f.solver = solver; f.reg = reg;
    f.beta = beta; f.status = status; f.out = out; f.meters = meters;
    const dim3 fgrid(1 + (fit ? lf_cdiv((long)N * L, LF_WAVE) : 0));
    switch (fit ? order : -1) {
        case -1: hipLaunchKernelGGL(seg_finish_kernel<-1>, fgrid, dim3(LF_WAVE), 0, st, f); break;
        case 0: hipLaunchKernelGGL(seg_finish_kernel<0>, fgrid, dim3(LF_WAVE), 0, st, f); break;
        case 1: hipLaunchKernelGGL(seg_finish_kernel<1>, fgrid, dim3(LF_WAVE), 0, st, f); break;
        case 2: hipLaunchKernelGGL(seg_finish_kernel<2>, fgrid, dim3(LF_WAVE), 0, st, f); break;
        default: hipLaunchKernelGGL(seg_finish_kernel<3>, fgrid, dim3(LF_WAVE), 0, st, f); break;
    }
    LF_CHECK_LAUNCH("seg_finish");
    if (maps && gt_line) {
        int cb = lf_cdiv(P, SG_THREADS * 4);
        if (cb > 256) cb = 256;
        hipLaunchKernelGGL(seg_flag_maps_kernel, dim3(cb, N * L), dim3(SG_THREADS), 0, st, maps, gt_line, P);
        LF_CHECK_LAUNCH("seg_flag_maps");
    }
    return 0;
}

extern "C" int lf_seg_step_bwd(float* grad_logits, long n, const float* upstream, void* stream) {
    LF_REQUIRE(grad_logits && upstream && n > 0, "lf_seg_step_bwd: bad arguments");
    int blocks = lf_cdiv(n, SG_THREADS * 4);
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(seg_scale_kernel, dim3(blocks), dim3(SG_THREADS), 0, (hipStream_t)stream, grad_logits, n,
                       seg_aligned16(grad_logits) ? 1 : 0, upstream);
    LF_CHECK_LAUNCH("seg_step_bwd");
    return 0;
}
