// Fitting head for gfx950: fused activation + row mask + weighted-least-squares
// normal equations (streaming fp64 moment accumulation), in-register solve, analytic
// backward.
//
// Reference behaviour (no code shared): BEV/Networks/LSQ_layer.py:103-167,310-325,
// BP/Networks/LSQ_layer.py:85-154, BP/Networks/gels.py.   Math: SURVEY.md 2.2.
//
// Design (DESIGN.md "WLS layer"): the normal matrix of a polynomial fit is Hankel, so the
// whole (N,P,d+1) design-matrix / bmm chain of the reference collapses to 3d+2 moments
//   m_j = sum_i s_i y_i^j (j = 0..2d),  q_j = sum_i s_i x_i y_i^j (j = 0..d),  s_i = act(o_i)^2
// per (image, lane).  One pass over the logits (4 B/pixel) + the shared L2-resident grid;
// masked rows are never read.  Accumulation is fp64 (the reference's fp32 bmm over 131k
// pixels is the source of its 5e-5..1e-4 noise floor); HBM-bound.
#include "lf_common.h"
#include "lf_solve.h"
#include "lf_types.h"

#include <type_traits>

namespace {

constexpr int WLS_THREADS = 256;
constexpr int WLS_CHUNKS = 16;   // row-chunks per (image, lane): N*K*16 workgroups >> 256 CUs at N*K = 64

__device__ __forceinline__ float act_fwd(float o, int kind) {
    switch (kind) {
        case LF_ACT_SQUARE: return o * o;
        case LF_ACT_ABS: return fabsf(o);
        case LF_ACT_RELU: return fmaxf(o, 0.f);
        case LF_ACT_SIGMOID: return 1.f / (1.f + expf(-o));
        case LF_ACT_SOFTPLUS: return o > 20.f ? o : log1pf(expf(o));
        default: return o;
    }
}
__device__ __forceinline__ float act_bwd(float o, int kind) {
    switch (kind) {
        case LF_ACT_SQUARE: return 2.f * o;
        case LF_ACT_ABS: return o > 0.f ? 1.f : (o < 0.f ? -1.f : 0.f);
        case LF_ACT_RELU: return o > 0.f ? 1.f : 0.f;
        case LF_ACT_SIGMOID: { float s = 1.f / (1.f + expf(-o)); return s * (1.f - s); }
        case LF_ACT_SOFTPLUS: return o > 20.f ? 1.f : 1.f / (1.f + expf(-o));
        default: return 1.f;
    }
}

template <int ORDER>
struct Moments {
    static constexpr int NM = 2 * ORDER + 1, NQ = ORDER + 1, N = NM + NQ;
    double v[N] = {};
    // one pixel: weight w (after activation), grid x', grid y', y = y_offset - y' in fp32 as the reference does
    __device__ __forceinline__ void add(float w, float gx, float gy, float y_off) {
        const double s = (double)w * (double)w;
        const double y = (double)(y_off - gy);
        const double x = (double)gx;
        double t = s;
#pragma unroll
        for (int j = 0; j < NM; ++j) {
            v[j] += t;
            if (j < NQ) v[NM + j] = fma(t, x, v[NM + j]);
            t *= y;
        }
    }
};

// Workgroup sum of N per-thread values -> out[0..N): a butterfly per wave, then thread j < N adds the waves in ascending order.
// The whole workgroup calls it (it holds a barrier); a second call in one kernel needs a __syncthreads() first: same LDS rows.
template <int N>
__device__ __forceinline__ void block_store_sums(const double (&v)[N], double* __restrict__ out) {
    __shared__ double red[WLS_THREADS / LF_WAVE][N];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const double s = lf_wave_sum(v[j]);
        if (lane == 0) red[wave][j] = s;
    }
    __syncthreads();
    if (threadIdx.x < N) {
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < WLS_THREADS / LF_WAVE; ++w) s += red[w][threadIdx.x];
        out[threadIdx.x] = s;
    }
}

// ---------------------------------------------------------------------------------------
// Where the fit's grid comes from: a table in memory, or a homography (BEV/Networks/LSQ_layer.py:84-87
// ProjectiveGridGenerator.forward): theta (3,3) shared or (N,3,3) per image, the base coordinates from two host-made tables
// xs (W) / ys (H).
//   (a, b, c) = theta [px, py, 1],  gx = a / c,  gy = b / c          (fp32, one fixed contraction: every kernel here agrees bit for bit)
// ---------------------------------------------------------------------------------------
struct Theta { float t[9]; };
__device__ __forceinline__ Theta theta_load(const float* __restrict__ theta, long theta_bs, int n) {
    Theta h;
#pragma unroll
    for (int i = 0; i < 9; ++i) h.t[i] = theta[(long)n * theta_bs + i];
    return h;
}
__device__ __forceinline__ void theta_point(const Theta& h, float px, float py, float& gx, float& gy, float& c) {
    const float a = fmaf(py, h.t[1], fmaf(px, h.t[0], h.t[2]));
    const float b = fmaf(py, h.t[4], fmaf(px, h.t[3], h.t[5]));
    c = fmaf(py, h.t[7], fmaf(px, h.t[6], h.t[8]));
    gx = a / c;
    gy = b / c;
}

// One pixel's grid point; (c, px, py) are filled by GridTheta only.
struct GridPoint { float gx, gy, c, px, py; };

// Both sources: Args is what the host passes, the constructor binds image n, load() reads what the unit of VEC pixels at p needs
// and point() gives pixel e of that unit.
struct GridTable {
    static constexpr bool kTheta = false;
    struct Args { const float* grid; long bs; };         // (N | 1, H*W, 2) fp32, batch stride 0 when shared
    template <int VEC> struct Unit { float xy[2 * VEC]; };
    const float* g;
    __device__ GridTable(const Args& a, int n) : g(a.grid + (long)n * a.bs) {}
    template <int VEC>
    __device__ __forceinline__ void load(long p, int, Unit<VEC>& u) const {
        if constexpr (VEC == 4) {
            const float4 g0 = *reinterpret_cast<const float4*>(g + 2 * p);
            const float4 g1 = *reinterpret_cast<const float4*>(g + 2 * p + 4);
            u.xy[0] = g0.x; u.xy[1] = g0.y; u.xy[2] = g0.z; u.xy[3] = g0.w;
            u.xy[4] = g1.x; u.xy[5] = g1.y; u.xy[6] = g1.z; u.xy[7] = g1.w;
        } else {
            u.xy[0] = g[2 * p];
            u.xy[1] = g[2 * p + 1];
        }
    }
    template <int VEC>
    __device__ __forceinline__ void point(const Unit<VEC>& u, int e, GridPoint& q) const {
        q.gx = u.xy[2 * e];
        q.gy = u.xy[2 * e + 1];
    }
};
struct GridTheta {                                       // the 8 B/pixel grid read is gone
    static constexpr bool kTheta = true;
    struct Args { const float* theta; long bs; const float* xs; const float* ys; };
    template <int VEC> struct Unit { float px[VEC], py; };
    Theta h;
    const float* xs;
    const float* ys;
    __device__ GridTheta(const Args& a, int n) : h(theta_load(a.theta, a.bs, n)), xs(a.xs), ys(a.ys) {}
    template <int VEC>
    __device__ __forceinline__ void load(long p, int W, Unit<VEC>& u) const {
        const int i = (int)(p / W), j = (int)(p - (long)i * W);
        u.py = ys[i];
        load_px<VEC>(xs + j, u.px);
    }
    template <int VEC>
    __device__ __forceinline__ void point(const Unit<VEC>& u, int e, GridPoint& q) const {
        q.px = u.px[e];
        q.py = u.py;
        theta_point(h, q.px, q.py, q.gx, q.gy, q.c);
    }
};

// Pass 1: per (chunk, image*lane) partial moments; optionally writes the masked weight map.  The first unmasked pixel is
// zero_rows * W: masked rows are never read (nor their grid points evaluated: a pole of theta there stays harmless).
template <int ORDER, int VEC, typename Src>
__global__ __launch_bounds__(WLS_THREADS) void wls_moments_kernel(
    const float* __restrict__ logits, const typename Src::Args grid, int K, int H, int W, int zero_rows, float y_off, int act_kind,
    float* __restrict__ masked, double* __restrict__ partials) {
    using M = Moments<ORDER>;
    const int nk = blockIdx.y, chunk = blockIdx.x;
    const long P = (long)H * W;
    const float* o = logits + (long)nk * P;
    const Src src(grid, nk / K);
    float* mo = masked ? masked + (long)nk * P : nullptr;
    const long first = (long)zero_rows * W;             // first unmasked pixel
    const long units = (P - first) / VEC;
    const long u0 = units * chunk / WLS_CHUNKS, u1 = units * (chunk + 1) / WLS_CHUNKS;
    M acc;
    for (long u = u0 + threadIdx.x; u < u1; u += WLS_THREADS) {
        const long p = first + u * VEC;
        float w[VEC];
        typename Src::template Unit<VEC> unit;
        load_px<VEC>(o + p, w);
        src.load(p, W, unit);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            GridPoint q;
            w[e] = act_fwd(w[e], act_kind);
            src.point(unit, e, q);
            acc.add(w[e], q.gx, q.gy, y_off);
        }
        if (mo) store_px<VEC>(mo + p, w);
    }
    if (mo) {   // masked rows are zeros (index_fill), written without reading the logits
        const long zu = first / VEC, z0 = zu * chunk / WLS_CHUNKS, z1 = zu * (chunk + 1) / WLS_CHUNKS;
        const float zero[VEC] = {};
        for (long u = z0 + threadIdx.x; u < z1; u += WLS_THREADS) store_px<VEC>(mo + u * VEC, zero);
    }
    block_store_sums(acc.v, partials + ((long)nk * WLS_CHUNKS + chunk) * M::N);
}

// Pass 2: one thread per (image, lane): deterministic sum of the chunk partials, build the
// Hankel normal matrix, invert, beta = Z^-1 X.
template <int ORDER>
__global__ void wls_solve_kernel(const double* __restrict__ partials, int NK, double reg, int solver,
                                 double* __restrict__ beta, double* __restrict__ zinv, int32_t* __restrict__ status) {
    using M = Moments<ORDER>;
    constexpr int D = ORDER + 1;
    const int nk = blockIdx.x * blockDim.x + threadIdx.x;
    if (nk >= NK) return;
    double mom[M::N];
#pragma unroll
    for (int j = 0; j < M::N; ++j) mom[j] = 0.0;
    for (int c = 0; c < WLS_CHUNKS; ++c)
#pragma unroll
        for (int j = 0; j < M::N; ++j) mom[j] += partials[((long)nk * WLS_CHUNKS + c) * M::N + j];
    double b[D], Zi[D][D];
    const int st = lf_solve_moments<ORDER>(mom, reg, solver, b, Zi);     // (the GELS flavour's caller passes reg = 0: gels.py has none)
#pragma unroll
    for (int i = 0; i < D; ++i) {
#pragma unroll
        for (int j = 0; j < D; ++j) zinv[((long)nk * D + i) * D + j] = Zi[i][j];
        beta[(long)nk * D + i] = b[i];
    }
    status[nk] = st;
}

// The backward, with v = Z^-1 gbeta, q = Y.v, r = x - Y.beta, s = w^2, y = y_off - gy, per pixel and lane:
//   dL/dlogit = 2 w q r act'(o),   dL/dgx = s q,   dL/dgy = -sum_k s (r v_k - q beta_k) (d - k) y^(d-k-1)
//   dL/dtheta_0 = sum (dgx / c) p,  dL/dtheta_1 = sum (dgy / c) p,  dL/dtheta_2 = sum -((dgx gx + dgy gy) / c) p,   p = [px, py, 1]
// The nine theta sums run in fp64 as per-workgroup partials in a caller-owned workspace, added in a fixed order by a second small
// launch: no atomics, two runs are bit-identical.  Masked rows are neither read nor evaluated (a pole there stays harmless).

// The per-pixel terms of one lane: returns grad_logits, and (dL/dgx, dL/dgy) of that lane.
template <int D>
__device__ __forceinline__ float fit_pixel_bwd(const double (&b)[D], const double (&v)[D], float ov, float gx, float gy, float y_off,
                                               int act_kind, double& dgx, double& dgy) {
    const double y = (double)(y_off - gy);
    double yv = v[0], yb = b[0];
#pragma unroll
    for (int i = 1; i < D; ++i) { yv = fma(yv, y, v[i]); yb = fma(yb, y, b[i]); }   // Horner, highest power first
    const double w = (double)act_fwd(ov, act_kind);
    const double r = (double)gx - yb, s = w * w;
    double dy = 0.0;                                      // sum_k (r v_k - q beta_k) (d - k) y^(d-k-1), Horner
#pragma unroll
    for (int k = 0; k < D - 1; ++k) dy = fma(dy, y, (double)(D - 1 - k) * (r * v[k] - yv * b[k]));
    dgx = s * yv;
    dgy = -s * dy;
    return (float)(2.0 * w * yv * r * (double)act_bwd(ov, act_kind));
}

// beta and v = Z^-1 gbeta of lane nk (Z^-1 is symmetric, so Z^-T g = Z^-1 g)
template <int D>
__device__ __forceinline__ void fit_lane_consts(const double* __restrict__ beta, const double* __restrict__ zinv,
                                                const double* __restrict__ gbeta, long nk, double (&b)[D], double (&v)[D]) {
#pragma unroll
    for (int i = 0; i < D; ++i) {
        b[i] = beta[nk * D + i];
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < D; ++j) s = fma(zinv[(nk * D + i) * D + j], gbeta[nk * D + j], s);
        v[i] = s;
    }
}

constexpr int TH_CHUNKS = 64;    // workgroups per (image, lane) of the backward launches = partial rows per (image, lane)

// nine fp64 sums of one thread: rows (dgx / c, dgy / c, -(dgx gx + dgy gy) / c) times (px, py, 1)
struct ThetaAcc {
    double v[9] = {};
    __device__ __forceinline__ void add(double dgx, double dgy, float gx, float gy, float c, float px, float py) {
        const double ic = 1.0 / (double)c;
        const double t0 = dgx * ic, t1 = dgy * ic, t2 = -(dgx * (double)gx + dgy * (double)gy) * ic;
        const double x = (double)px, y = (double)py;
        v[0] = fma(t0, x, v[0]); v[1] = fma(t0, y, v[1]); v[2] += t0;
        v[3] = fma(t1, x, v[3]); v[4] = fma(t1, y, v[4]); v[5] += t1;
        v[6] = fma(t2, x, v[6]); v[7] = fma(t2, y, v[7]); v[8] += t2;
    }
};

// d/d logits of sum_k <grad_beta_k, beta_k>, elementwise over the whole map (masked rows are written as zeros); with GridTheta
// also the nine theta sums of this workgroup's pixels -> partials[(nk, blockIdx.x)].
template <int ORDER, int VEC, typename Src>
__global__ __launch_bounds__(WLS_THREADS) void wls_bwd_kernel(
    const float* __restrict__ logits, const typename Src::Args grid, int K, int H, int W, int zero_rows, float y_off, int act_kind,
    const double* __restrict__ beta, const double* __restrict__ zinv, const double* __restrict__ gbeta, float* __restrict__ gout,
    double* __restrict__ partials) {
    constexpr int D = ORDER + 1;
    const int nk = blockIdx.y;
    const long P = (long)H * W;
    const float* o = logits + (long)nk * P;
    float* go = gout + (long)nk * P;
    const Src src(grid, nk / K);
    double b[D], v[D];
    fit_lane_consts<D>(beta, zinv, gbeta, nk, b, v);
    const long first = (long)zero_rows * W;
    ThetaAcc acc;
    auto one = [&](float ov, const typename Src::template Unit<VEC>& unit, int e) -> float {
        GridPoint q;
        double dgx, dgy;
        src.point(unit, e, q);
        const float g = fit_pixel_bwd<D>(b, v, ov, q.gx, q.gy, y_off, act_kind, dgx, dgy);
        if constexpr (Src::kTheta) acc.add(dgx, dgy, q.gx, q.gy, q.c, q.px, q.py);
        return g;
    };
    const long units = P / VEC;
    for (long u = (long)blockIdx.x * WLS_THREADS + threadIdx.x; u < units; u += (long)gridDim.x * WLS_THREADS) {
        const long p = u * VEC;
        float r[VEC] = {};
        if (p >= first) {
            float ov[VEC];
            typename Src::template Unit<VEC> unit;
            src.load(p, W, unit);
            load_px<VEC>(o + p, ov);
#pragma unroll
            for (int e = 0; e < VEC; ++e) r[e] = one(ov[e], unit, e);
        }
        store_px<VEC>(go + p, r);
    }
    if constexpr (Src::kTheta) block_store_sums(acc.v, partials + ((long)nk * gridDim.x + blockIdx.x) * 9);
}

// ---- host side: one dispatcher per compile-time choice, one launcher per pass ---------------------------------------------

// the run-time order (0..3, checked by the caller) as a compile-time constant: f(std::integral_constant<int, ORDER>)
template <typename F>
int with_order(int order, F&& f) {
    switch (order) {
        case 0: return f(std::integral_constant<int, 0>{});
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        default: return f(std::integral_constant<int, 3>{});
    }
}
inline int fit_vec(int W) { return W % 4 == 0 ? 4 : 1; }
template <typename F>
int with_vec(int W, F&& f) {
    return fit_vec(W) == 4 ? f(std::integral_constant<int, 4>{}) : f(std::integral_constant<int, 1>{});
}
// workgroups per (image, lane) of the elementwise backward = partial rows of the theta sums
inline int fit_bwd_chunks(int H, int W) {
    const int gx = lf_cdiv((long)H * W / fit_vec(W), WLS_THREADS);
    return gx > TH_CHUNKS ? TH_CHUNKS : gx;
}

// What the fit entry points share; `name` (the entry point) leads the message.
int fit_check(const char* name, int N, int K, int H, int W, int zero_rows, int order, int act_kind) {
    LF_REQUIRE(N > 0 && K > 0 && H > 0 && W > 0, "%s: bad shape %d %d %d %d", name, N, K, H, W);
    LF_REQUIRE(zero_rows >= 0 && zero_rows < H, "%s: zero_rows %d out of [0,%d)", name, zero_rows, H);
    LF_REQUIRE(order >= 0 && order <= 3, "%s: order %d not in 0..3", name, order);
    LF_REQUIRE(act_kind >= 0 && act_kind <= LF_ACT_NONE, "%s: bad activation %d", name, act_kind);
    return 0;
}
// ... and the entry points that take a homography
int theta_check(const char* name, const float* theta, long theta_bs, const float* xs, const float* ys, int N, int H, int W) {
    LF_REQUIRE(theta && xs && ys, "%s: null pointer", name);
    LF_REQUIRE(theta_bs == 0 || theta_bs == 9, "%s: theta_batch_stride %ld is neither 0 nor 9", name, theta_bs);
    LF_REQUIRE(N > 0 && H > 0 && W > 0, "%s: bad shape %d %d %d", name, N, H, W);
    LF_REQUIRE(((size_t)xs & 15) == 0, "%s: the x table is read as vectors: misaligned", name);
    return 0;
}

template <int ORDER>
int wls_solve_launch(const double* partials, int NK, double reg, int solver, double* beta, double* zinv, int32_t* status,
                     hipStream_t st) {
    hipLaunchKernelGGL((wls_solve_kernel<ORDER>), dim3(lf_cdiv(NK, 64)), dim3(64), 0, st, partials, NK, reg, solver, beta, zinv,
                       status);
    LF_CHECK_LAUNCH("wls_solve");
    return 0;
}

template <int ORDER, typename Src>
int wls_fwd_launch(const float* logits, const typename Src::Args grid, int N, int K, int H, int W, int zr, double reg, double y_off,
                   int act, int solver, double* beta, double* zinv, float* masked, double* partials, int32_t* status,
                   hipStream_t st) {
    with_vec(W, [&](auto V) {
        hipLaunchKernelGGL((wls_moments_kernel<ORDER, V(), Src>), dim3(WLS_CHUNKS, N * K), dim3(WLS_THREADS), 0, st, logits, grid, K,
                           H, W, zr, (float)y_off, act, masked, partials);
        return 0;
    });
    LF_CHECK_LAUNCH(Src::kTheta ? "wls_moments_theta" : "wls_moments");
    return wls_solve_launch<ORDER>(partials, N * K, reg, solver, beta, zinv, status, st);
}

// theta_partials: GridTheta only, fit_bwd_chunks(H, W) rows of nine per (image, lane)
template <int ORDER, typename Src>
int wls_bwd_launch(const float* logits, const typename Src::Args grid, int N, int K, int H, int W, int zr, double y_off, int act,
                   const double* beta, const double* zinv, const double* gbeta, float* gout, double* theta_partials,
                   hipStream_t st) {
    with_vec(W, [&](auto V) {
        hipLaunchKernelGGL((wls_bwd_kernel<ORDER, V(), Src>), dim3(fit_bwd_chunks(H, W), N * K), dim3(WLS_THREADS), 0, st, logits,
                           grid, K, H, W, zr, (float)y_off, act, beta, zinv, gbeta, gout, theta_partials);
        return 0;
    });
    LF_CHECK_LAUNCH(Src::kTheta ? "wls_bwd_theta" : "wls_bwd");
    return 0;
}

}  // namespace

// ---------------------------------------------------------------------------------------
// GELS: least squares of an explicit design matrix through the normal equations + Cholesky
// (BP/Networks/gels.py:9-25).  A (N,P,D) fp32, b (N,P) fp32, D <= 4.
// ---------------------------------------------------------------------------------------
namespace {

template <int D>
__global__ __launch_bounds__(WLS_THREADS) void gels_moments_kernel(const float* __restrict__ A, const float* __restrict__ b,
                                                                  long P, double* __restrict__ partials) {
    constexpr int NS = D * (D + 1) / 2 + D;
    const int n = blockIdx.y, chunk = blockIdx.x;
    const long p0 = P * chunk / WLS_CHUNKS, p1 = P * (chunk + 1) / WLS_CHUNKS;
    double acc[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) acc[i] = 0.0;
    for (long p = p0 + threadIdx.x; p < p1; p += WLS_THREADS) {
        double a[D];
#pragma unroll
        for (int j = 0; j < D; ++j) a[j] = (double)A[((long)n * P + p) * D + j];
        const double bv = (double)b[(long)n * P + p];
        int k = 0;
#pragma unroll
        for (int i = 0; i < D; ++i)
#pragma unroll
            for (int j = i; j < D; ++j) { acc[k] = fma(a[i], a[j], acc[k]); ++k; }
#pragma unroll
        for (int i = 0; i < D; ++i) acc[D * (D + 1) / 2 + i] = fma(a[i], bv, acc[D * (D + 1) / 2 + i]);
    }
    block_store_sums(acc, partials + ((long)n * WLS_CHUNKS + chunk) * NS);
}

template <int D>
__global__ void gels_solve_kernel(const double* __restrict__ partials, int N, float* __restrict__ x,
                                  double* __restrict__ zinv, int32_t* __restrict__ status) {
    constexpr int NS = D * (D + 1) / 2 + D;
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    double m[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) m[j] = 0.0;
    for (int c = 0; c < WLS_CHUNKS; ++c)
#pragma unroll
        for (int j = 0; j < NS; ++j) m[j] += partials[((long)n * WLS_CHUNKS + c) * NS + j];
    double Z[D][D], Zi[D][D], X[D];
    int k = 0;
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = i; j < D; ++j) { Z[i][j] = m[k]; Z[j][i] = m[k]; ++k; }
#pragma unroll
    for (int i = 0; i < D; ++i) X[i] = m[D * (D + 1) / 2 + i];
    const int st = invert_chol<D>(Z, Zi);
#pragma unroll
    for (int i = 0; i < D; ++i) {
        double v = 0.0;
#pragma unroll
        for (int j = 0; j < D; ++j) { v = fma(Zi[i][j], X[j], v); zinv[((long)n * D + i) * D + j] = Zi[i][j]; }
        x[(long)n * D + i] = (float)v;
    }
    status[n] = st;
}

template <int D>
__global__ __launch_bounds__(WLS_THREADS) void gels_bwd_kernel(const float* __restrict__ A, const float* __restrict__ b,
                                                              const float* __restrict__ x, const double* __restrict__ zinv,
                                                              const float* __restrict__ gout, long P,
                                                              float* __restrict__ gA, float* __restrict__ gb) {
    const int n = blockIdx.y;
    double xs[D], z[D];
#pragma unroll
    for (int i = 0; i < D; ++i) {
        xs[i] = (double)x[(long)n * D + i];
        double v = 0.0;
#pragma unroll
        for (int j = 0; j < D; ++j) v = fma(zinv[((long)n * D + i) * D + j], (double)gout[(long)n * D + j], v);
        z[i] = v;
    }
    for (long p = (long)blockIdx.x * WLS_THREADS + threadIdx.x; p < P; p += (long)gridDim.x * WLS_THREADS) {
        double a[D], ax = 0.0, az = 0.0;
#pragma unroll
        for (int j = 0; j < D; ++j) { a[j] = (double)A[((long)n * P + p) * D + j]; ax = fma(a[j], xs[j], ax); az = fma(a[j], z[j], az); }
        const double bv = (double)b[(long)n * P + p];
#pragma unroll
        for (int j = 0; j < D; ++j) gA[((long)n * P + p) * D + j] = (float)(-(ax * z[j] + az * xs[j]) + bv * z[j]);
        gb[(long)n * P + p] = (float)az;
    }
}

}  // namespace

extern "C" size_t lf_gels_workspace_bytes(int N, int D) { return (size_t)N * WLS_CHUNKS * (D * (D + 1) / 2 + D) * sizeof(double); }

extern "C" int lf_gels_fwd(const float* A, const float* b, int N, long P, int D, float* x, double* zinv, void* partials,
                           int32_t* status, void* stream) {
    LF_REQUIRE(A && b && x && zinv && partials && status, "lf_gels_fwd: null pointer");
    LF_REQUIRE(D >= 1 && D <= 4 && N > 0 && P > 0, "lf_gels_fwd: bad shape N=%d P=%ld D=%d", N, P, D);
    hipStream_t st = (hipStream_t)stream;
    dim3 g1(WLS_CHUNKS, N);
    double* pp = (double*)partials;
#define LF_GELS(DD)                                                                                              \
    hipLaunchKernelGGL(gels_moments_kernel<DD>, g1, dim3(WLS_THREADS), 0, st, A, b, P, pp);                      \
    hipLaunchKernelGGL(gels_solve_kernel<DD>, dim3(lf_cdiv(N, 64)), dim3(64), 0, st, pp, N, x, zinv, status)
    switch (D) {
        case 1: LF_GELS(1); break;
        case 2: LF_GELS(2); break;
        case 3: LF_GELS(3); break;
        default: LF_GELS(4); break;
    }
#undef LF_GELS
    LF_CHECK_LAUNCH("gels_fwd");
    return 0;
}

extern "C" int lf_gels_bwd(const float* A, const float* b, const float* x, const double* zinv, const float* grad_out, int N,
                           long P, int D, float* grad_A, float* grad_b, void* stream) {
    LF_REQUIRE(A && b && x && zinv && grad_out && grad_A && grad_b, "lf_gels_bwd: null pointer");
    LF_REQUIRE(D >= 1 && D <= 4 && N > 0 && P > 0, "lf_gels_bwd: bad shape");
    hipStream_t st = (hipStream_t)stream;
    int gx = lf_cdiv(P, WLS_THREADS);
    if (gx > 256) gx = 256;
    dim3 g1(gx, N);
    switch (D) {
        case 1: hipLaunchKernelGGL(gels_bwd_kernel<1>, g1, dim3(WLS_THREADS), 0, st, A, b, x, zinv, grad_out, P, grad_A, grad_b); break;
        case 2: hipLaunchKernelGGL(gels_bwd_kernel<2>, g1, dim3(WLS_THREADS), 0, st, A, b, x, zinv, grad_out, P, grad_A, grad_b); break;
        case 3: hipLaunchKernelGGL(gels_bwd_kernel<3>, g1, dim3(WLS_THREADS), 0, st, A, b, x, zinv, grad_out, P, grad_A, grad_b); break;
        default: hipLaunchKernelGGL(gels_bwd_kernel<4>, g1, dim3(WLS_THREADS), 0, st, A, b, x, zinv, grad_out, P, grad_A, grad_b); break;
    }
    LF_CHECK_LAUNCH("gels_bwd");
    return 0;
}

extern "C" size_t lf_wls_workspace_bytes(int N, int K, int order) {
    return (size_t)N * K * WLS_CHUNKS * (3 * order + 2) * sizeof(double);
}

extern "C" int lf_wls_fwd(const float* logits, const float* grid_xy, long grid_batch_stride, int N, int K, int H,
                          int W, int zero_rows, int order, double reg, double y_offset, int act_kind, int solver,
                          double* beta, double* zinv, float* masked, void* partials, int32_t* status, void* stream) {
    LF_REQUIRE(logits && grid_xy && beta && zinv && partials && status, "lf_wls_fwd: null pointer");
    if (fit_check("lf_wls_fwd", N, K, H, W, zero_rows, order, act_kind)) return -1;
    return with_order(order, [&](auto O) {
        return wls_fwd_launch<O(), GridTable>(logits, {grid_xy, grid_batch_stride}, N, K, H, W, zero_rows, reg, y_offset, act_kind,
                                              solver, beta, zinv, masked, (double*)partials, status, (hipStream_t)stream);
    });
}

extern "C" int lf_wls_bwd(const float* logits, const float* grid_xy, long grid_batch_stride, int N, int K, int H,
                          int W, int zero_rows, int order, double y_offset, int act_kind, const double* beta,
                          const double* zinv, const double* grad_beta, float* grad_logits, void* stream) {
    LF_REQUIRE(logits && grid_xy && beta && zinv && grad_beta && grad_logits, "lf_wls_bwd: null pointer");
    if (fit_check("lf_wls_bwd", N, K, H, W, zero_rows, order, act_kind)) return -1;
    return with_order(order, [&](auto O) {
        return wls_bwd_launch<O(), GridTable>(logits, {grid_xy, grid_batch_stride}, N, K, H, W, zero_rows, y_offset, act_kind, beta,
                                              zinv, grad_beta, grad_logits, nullptr, (hipStream_t)stream);
    });
}

// ---------------------------------------------------------------------------------------
// Fused head + fit (inference): decoder.output_conv = ConvTranspose2d(16, K, 2, stride 2) (BEV/Networks/ERFNet.py:123,139), the
// activation, the row mask and the moment pass of the fit (BEV/Networks/LSQ_layer.py:310-325) in ONE pass over the last decoder
// layer's 16-channel NHWC tensor: the (N,K,H,W) logits and the masked weight map are never written (the logits only on request),
// and input rows that feed masked output rows only are never read.  One input pixel per lane (64 contiguous bytes of fp32, 32 of
// bf16) -> its 2 x 2 output pixels for HM_LANES fit lanes; products in head_fwd_kernel's order (bias first, channels ascending);
// moments in fp64 through Moments<ORDER>::add into the partials layout wls_solve_kernel reads.
// ---------------------------------------------------------------------------------------
namespace {

constexpr int HM_LANES = 2;      // fit lanes (head channels) per workgroup: 2 * (3 * ORDER + 2) fp64 accumulators per thread
constexpr int HM_MAXK = 8;

template <int ORDER, typename T>
__global__ __launch_bounds__(WLS_THREADS) void head_moments_kernel(
    const T* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b, const float* __restrict__ grid, long grid_bs,
    int K, int h, int wd, int zero_rows, float y_off, int act_kind, float* __restrict__ logits, double* __restrict__ partials) {
    using M = Moments<ORDER>;
    const int groups = (K + HM_LANES - 1) / HM_LANES;
    const int n = blockIdx.y / groups, k0 = (blockIdx.y % groups) * HM_LANES, chunk = blockIdx.x;
    __shared__ float sw[HM_LANES][16][4];
    __shared__ float sb[HM_LANES];
    for (int i = threadIdx.x; i < HM_LANES * 64; i += WLS_THREADS) {
        const int kk = i >> 6, ci = (i >> 2) & 15, ab = i & 3;
        const int k = k0 + kk < K ? k0 + kk : K - 1;              // (a lane group's spare slot repeats lane K - 1 and is not stored)
        sw[kk][ci][ab] = w[(ci * K + k) * 4 + ab];
        if (ci == 0 && ab == 0) sb[kk] = b[k];
    }
    __syncthreads();
    const int W = 2 * wd;
    const long HW = (long)(2 * h) * W;
    const float* g = grid + (long)n * grid_bs;
    const T* xn = x + (long)n * h * wd * 16;
    // first input row that is needed: with logits requested every row, else the first one with an unmasked output row
    const long first = logits ? 0 : (long)(zero_rows / 2) * wd;
    const long units = (long)h * wd - first;
    const long u0 = units * chunk / WLS_CHUNKS, u1 = units * (chunk + 1) / WLS_CHUNKS;
    M acc[HM_LANES];
    for (long u = u0 + threadIdx.x; u < u1; u += WLS_THREADS) {
        const long p = first + u;
        const int i = (int)(p / wd), j = (int)(p - (long)i * wd);
        float xv[16];
        if constexpr (sizeof(T) == 2) {
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                lf_f32x4 v[2];
                lf_ldq<T, 2>(xn + p * 16 + q * 8, v);
#pragma unroll
                for (int e = 0; e < 4; ++e) { xv[q * 8 + e] = v[0][e]; xv[q * 8 + 4 + e] = v[1][e]; }
            }
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const lf_f32x4 v = lf_ldv(xn + p * 16 + q * 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) xv[q * 4 + e] = v[e];
            }
        }
        // the 2 x 64 head weights are read from LDS per pixel (wave-uniform broadcasts): `lz` is an opaque zero that keeps the
        // compiler from hoisting all 128 of them into registers across the loop (260 VGPRs at order 3: one wave per SIMD)
        int lz = 0;
        asm volatile("" : "+s"(lz));
        const bool live0 = 2 * i >= zero_rows, live1 = 2 * i + 1 >= zero_rows;
        const long q0 = (long)(2 * i) * W + 2 * j;                 // output pixel (2i, 2j); (2i+1, 2j) = q0 + W
        float4 ga = make_float4(0.f, 0.f, 0.f, 0.f), gb = ga;
        if (live0) ga = *reinterpret_cast<const float4*>(g + 2 * q0);
        if (live1) gb = *reinterpret_cast<const float4*>(g + 2 * (q0 + W));
#pragma unroll
        for (int kk = 0; kk < HM_LANES; ++kk) {
            float o[4];
#pragma unroll
            for (int ab = 0; ab < 4; ++ab) o[ab] = sb[kk];
            const float (*swk)[4] = sw[kk] + lz;
#pragma unroll
            for (int ci = 0; ci < 16; ++ci)
#pragma unroll
                for (int ab = 0; ab < 4; ++ab) o[ab] = fmaf(xv[ci], swk[ci][ab], o[ab]);
            if (live0) {
                acc[kk].add(act_fwd(o[0], act_kind), ga.x, ga.y, y_off);
                acc[kk].add(act_fwd(o[1], act_kind), ga.z, ga.w, y_off);
            }
            if (live1) {
                acc[kk].add(act_fwd(o[2], act_kind), gb.x, gb.y, y_off);
                acc[kk].add(act_fwd(o[3], act_kind), gb.z, gb.w, y_off);
            }
            if (logits && k0 + kk < K) {
                float* op = logits + ((long)n * K + k0 + kk) * HW + q0;
                *reinterpret_cast<float2*>(op) = make_float2(o[0], o[1]);
                *reinterpret_cast<float2*>(op + W) = make_float2(o[2], o[3]);
            }
        }
    }
#pragma unroll
    for (int kk = 0; kk < HM_LANES; ++kk) {
        if (kk) __syncthreads();  // (the guard below is uniform over the workgroup -- k0 from blockIdx -- as the barrier inside needs)
        if (k0 + kk < K) block_store_sums(acc[kk].v, partials + (((long)n * K + k0 + kk) * WLS_CHUNKS + chunk) * M::N);
    }
}

}  // namespace

// x (N,h,w,16) NHWC fp32 (x_bf16 = 0) or bf16 bit patterns (1); head_w (16,K,2,2), head_b (K) fp32; the fit runs on the
// (N,K,2h,2w) maps the head would write.  Arguments from grid_xy on as lf_wls_fwd; logits_or_null (N,K,2h,2w) fp32.
extern "C" int lf_head_fit(const void* x, int x_bf16, const float* head_w, const float* head_b, const float* grid_xy,
                           long grid_batch_stride, int N, int h, int w, int K, int zero_rows, int order, double reg, double y_offset,
                           int act_kind, int solver, float* logits_or_null, double* beta, double* zinv, void* partials,
                           int32_t* status, void* stream) {
    LF_REQUIRE(x && head_w && head_b && grid_xy && beta && zinv && partials && status, "lf_head_fit: null pointer");
    LF_REQUIRE(N > 0 && h > 0 && w > 0 && K >= 1 && K <= HM_MAXK, "lf_head_fit: bad shape %d %d %d %d", N, K, h, w);
    LF_REQUIRE(zero_rows >= 0 && zero_rows < 2 * h, "lf_head_fit: zero_rows %d out of [0,%d)", zero_rows, 2 * h);
    LF_REQUIRE(order >= 0 && order <= 3, "lf_head_fit: order %d not in 0..3", order);
    LF_REQUIRE(act_kind >= 0 && act_kind <= LF_ACT_NONE, "lf_head_fit: bad activation %d", act_kind);
    LF_REQUIRE(grid_batch_stride % 4 == 0 && ((size_t)grid_xy & 15) == 0 && ((size_t)x & 15) == 0 &&
               (!logits_or_null || ((size_t)logits_or_null & 7) == 0), "lf_head_fit: grid / input / logits are read and written as vectors: misaligned");
    hipStream_t st = (hipStream_t)stream;
    const dim3 g1(WLS_CHUNKS, N * ((K + HM_LANES - 1) / HM_LANES));
    return with_order(order, [&](auto O) {
        if (x_bf16)
            hipLaunchKernelGGL((head_moments_kernel<O(), lf_bf16>), g1, dim3(WLS_THREADS), 0, st, (const lf_bf16*)x, head_w, head_b,
                               grid_xy, grid_batch_stride, K, h, w, zero_rows, (float)y_offset, act_kind, logits_or_null,
                               (double*)partials);
        else
            hipLaunchKernelGGL((head_moments_kernel<O(), float>), g1, dim3(WLS_THREADS), 0, st, (const float*)x, head_w, head_b,
                               grid_xy, grid_batch_stride, K, h, w, zero_rows, (float)y_offset, act_kind, logits_or_null,
                               (double*)partials);
        LF_CHECK_LAUNCH("head_moments");
        return wls_solve_launch<O()>((const double*)partials, N * K, reg, solver, beta, zinv, status, st);
    });
}

// ---------------------------------------------------------------------------------------
// Fused head + arg-max + fit (inference, segmentation mode): decoder.output_conv with C class channels, the arg-max lane maps of
// Net.forward(end_to_end=False) (BEV/Networks/LSQ_layer.py:302-308, BP/Networks/LSQ_layer.py:279-293,308-311) and the moment pass
// of their fit in ONE pass over the last decoder layer's tensor: neither the (N,C,H,W) logits nor the (N,L,H,W) maps are written.
// The result equals lf_head_fwd + lf_seg_maps + lf_wls_fwd BIT FOR BIT (the arg-max is discontinuous: nothing weaker means
// anything), so the summation is wls_moments_kernel<ORDER, 4, GridTable>'s, restated: a unit is 4 consecutive output pixels of one
// row from the first unmasked pixel on, chunk c owns units [units * c / 16, units * (c + 1) / 16), thread t takes every 256th of
// them, each lane's per-thread sums go through block_store_sums into that lane's chunk slot; every lane adds every pixel of its
// thread (a zero weight too), so each fp64 addition happens in the same thread in the same order.  The logits are
// head_fwd_kernel's (bias first, channels ascending, fmaf), the arg-max seg_maps_kernel's (first maximum, NaN maximal).
// ---------------------------------------------------------------------------------------
namespace {

constexpr int SF_MAXC = 5;       // classes: background + up to 4 lanes
constexpr int SF_MAXL = 4;
typedef float sf_f32x2 __attribute__((ext_vector_type(2)));

// the 32 input values of a unit: two adjacent input pixels of row i, 16 channels each (128 contiguous bytes of fp32, 64 of bf16)
template <typename T>
__device__ __forceinline__ void segfit_load(const T* __restrict__ p, float (&xv)[2][16]) {
    if constexpr (sizeof(T) == 2) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            lf_f32x4 v[2];
            lf_ldq<T, 2>(p + q * 8, v);
#pragma unroll
            for (int e = 0; e < 4; ++e) { xv[q >> 1][(q & 1) * 8 + e] = v[0][e]; xv[q >> 1][(q & 1) * 8 + 4 + e] = v[1][e]; }
        }
    } else {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const lf_f32x4 v = lf_ldv(p + q * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) xv[q >> 2][(q & 3) * 4 + e] = v[e];
        }
    }
}

// arg-max class of the unit's 4 output pixels (tap row a): sw [a][c][ci][b] and sb [c] in LDS
__device__ __forceinline__ void segfit_argmax(const float (&xv)[2][16], const float* __restrict__ sw, const float* __restrict__ sb,
                                              int C, int a, int (&am)[4]) {
    float best[4];
    for (int c = 0; c < C; ++c) {
        // the two outputs of an input pixel (b = 0, 1) as one two-wide fma per channel: the same fmaf per element, half the issues
        sf_f32x2 o01 = {sb[c], sb[c]}, o23 = o01;
        const sf_f32x2* wc = reinterpret_cast<const sf_f32x2*>(sw) + (a * SF_MAXC + c) * 16;
#pragma unroll
        for (int ci = 0; ci < 16; ++ci) {
            const sf_f32x2 t = wc[ci];
            o01 = __builtin_elementwise_fma(sf_f32x2{xv[0][ci], xv[0][ci]}, t, o01);
            o23 = __builtin_elementwise_fma(sf_f32x2{xv[1][ci], xv[1][ci]}, t, o23);
        }
        const float o[4] = {o01.x, o01.y, o23.x, o23.y};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float v = o[e];
            const bool up = c == 0 || v > best[e] || (v != v && best[e] == best[e]);      // (selects, not branches)
            best[e] = up ? v : best[e];
            am[e] = up ? c : am[e];
        }
    }
}

// One workgroup: chunk blockIdx.x of image n, lanes [l0, l0 + NL) (blockIdx.y = n * groups + l0 / NL).  flags: gt_line (N,L) or
// NULL; a flagged lane takes map [0, 0]'s value -- image 0's arg-max == 1 -- against image n's grid (lane (0, 0) thereby stays as
// it is).  classes (N,H,W) uint8 or NULL: written by the workgroups of lane group 0, every row.
template <int ORDER, typename T, int NL>
__global__ __launch_bounds__(WLS_THREADS) void segfit_kernel(
    const T* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b, const float* __restrict__ grid, long grid_bs,
    const float* __restrict__ flags, int C, int L, int h, int wd, int zero_rows, float y_off, uint8_t* __restrict__ classes,
    double* __restrict__ partials) {
    using M = Moments<ORDER>;
    const int groups = (L + NL - 1) / NL;
    const int n = blockIdx.y / groups, l0 = (blockIdx.y % groups) * NL, chunk = blockIdx.x;
    __shared__ float sw[2 * SF_MAXC * 16 * 2];
    __shared__ float sb[SF_MAXC];
    for (int i = threadIdx.x; i < C * 64; i += WLS_THREADS) {
        const int c = i >> 6, ci = (i >> 2) & 15, ab = i & 3;
        sw[(((ab >> 1) * SF_MAXC + c) * 16 + ci) * 2 + (ab & 1)] = w[(ci * C + c) * 4 + ab];
        if (ci == 0 && ab == 0) sb[c] = b[c];
    }
    __syncthreads();
    unsigned flagged = 0;                                 // bit k: lane l0 + k borrows map [0, 0]
    if (flags)
        for (int k = 0; k < NL; ++k)
            if (l0 + k < L && flags[n * L + l0 + k] != 0.f) flagged |= 1u << k;
    const bool other = flagged && n != 0;                 // image 0's arg-max is needed next to this image's (uniform)
    const int W = 2 * wd;
    const long P = (long)(2 * h) * W;
    const GridTable src({grid, grid_bs}, n);
    const T* xn = x + (long)n * h * wd * 16;
    uint8_t* cls = (classes && l0 == 0) ? classes + (long)n * P : nullptr;
    const long first = (long)zero_rows * W;               // first unmasked pixel
    const long units = (P - first) / 4;
    const long u0 = units * chunk / WLS_CHUNKS, u1 = units * (chunk + 1) / WLS_CHUNKS;
    M acc[NL];
    for (long u = u0 + threadIdx.x; u < u1; u += WLS_THREADS) {
        const long p = first + u * 4;
        const int r = (int)(p / W), col = (int)(p - (long)r * W);
        const long xo = ((long)(r >> 1) * wd + (col >> 1)) * 16;
        float xv[2][16];
        GridTable::Unit<4> unit;
        segfit_load<T>(xn + xo, xv);
        src.load<4>(p, W, unit);
        int am[4], am0[4];
        segfit_argmax(xv, sw, sb, C, r & 1, am);
        if (other) {
            segfit_load<T>(x + xo, xv);
            segfit_argmax(xv, sw, sb, C, r & 1, am0);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) am0[e] = am[e];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            GridPoint q;
            src.point(unit, e, q);
#pragma unroll
            for (int k = 0; k < NL; ++k) {
                const float own = am[e] == l0 + k + 1 ? (float)(l0 + k + 1) : 0.f;
                const float lent = am0[e] == 1 ? 1.f : 0.f;
                acc[k].add((flagged >> k) & 1 ? lent : own, q.gx, q.gy, y_off);
            }
        }
        if (cls) *reinterpret_cast<uchar4*>(cls + p) = make_uchar4(am[0], am[1], am[2], am[3]);
    }
    if (cls) {   // the class map covers the masked rows too: their pixels are computed for it and stay out of the fit
        const long zu = first / 4, z0 = zu * chunk / WLS_CHUNKS, z1 = zu * (chunk + 1) / WLS_CHUNKS;
        for (long u = z0 + threadIdx.x; u < z1; u += WLS_THREADS) {
            const long p = u * 4;
            const int r = (int)(p / W), col = (int)(p - (long)r * W);
            float xm[2][16];
            int am[4];
            segfit_load<T>(xn + ((long)(r >> 1) * wd + (col >> 1)) * 16, xm);
            segfit_argmax(xm, sw, sb, C, r & 1, am);
            *reinterpret_cast<uchar4*>(cls + p) = make_uchar4(am[0], am[1], am[2], am[3]);
        }
    }
#pragma unroll
    for (int k = 0; k < NL; ++k) {
        if (k) __syncthreads();  // (the guard below is uniform over the workgroup -- l0 from blockIdx -- as the barrier inside needs)
        if (l0 + k < L) block_store_sums(acc[k].v, partials + (((long)n * L + l0 + k) * WLS_CHUNKS + chunk) * M::N);
    }
}

}  // namespace

// x, head_w (16,C,2,2), head_b (C) as lf_head_fit, C <= 5 classes; the fit runs on the L <= 4 arg-max lane maps lf_seg_maps would
// write from the head's logits (gt_line_or_null (N,L) fp32 as there); classes_or_null (N,2h,2w) uint8.  w even.
extern "C" int lf_head_fit_seg(const void* x, int x_bf16, const float* head_w, const float* head_b, const float* grid_xy,
                               long grid_batch_stride, const float* gt_line_or_null, int N, int h, int w, int C, int L, int zero_rows,
                               int order, double reg, double y_offset, int solver, uint8_t* classes_or_null, double* beta,
                               double* zinv, void* partials, int32_t* status, void* stream) {
    LF_REQUIRE(x && head_w && head_b && grid_xy && beta && zinv && partials && status, "lf_head_fit_seg: null pointer");
    LF_REQUIRE(N > 0 && h > 0 && w > 0 && C >= 1 && C <= SF_MAXC && L >= 1 && L <= SF_MAXL,
               "lf_head_fit_seg: bad shape N=%d C=%d L=%d h=%d w=%d (C <= %d, L <= %d)", N, C, L, h, w, SF_MAXC, SF_MAXL);
    LF_REQUIRE(w % 2 == 0, "lf_head_fit_seg: w = %d is odd: a unit of 4 output pixels must lie in one row", w);
    LF_REQUIRE(zero_rows >= 0 && zero_rows < 2 * h, "lf_head_fit_seg: zero_rows %d out of [0,%d)", zero_rows, 2 * h);
    LF_REQUIRE(order >= 0 && order <= 3, "lf_head_fit_seg: order %d not in 0..3", order);
    LF_REQUIRE(grid_batch_stride % 4 == 0 && ((size_t)grid_xy & 15) == 0 && ((size_t)x & 15) == 0 && ((size_t)classes_or_null & 3) == 0,
               "lf_head_fit_seg: grid / input / classes are read and written as vectors: misaligned");
    hipStream_t st = (hipStream_t)stream;
    // all lanes in one workgroup (the head and the arg-max are computed once per pixel) when the images alone fill the device; below
    // that one lane per workgroup: L times as many workgroups, each repeating the (cheap) head
    const bool split = (long)N * WLS_CHUNKS < 256 && L > 1;
    return with_order(order, [&](auto O) {
        auto launch = [&](auto t, auto NLc) {
            using T = decltype(t);
            constexpr int NL = decltype(NLc)::value;
            hipLaunchKernelGGL((segfit_kernel<O(), T, NL>), dim3(WLS_CHUNKS, N * ((L + NL - 1) / NL)), dim3(WLS_THREADS), 0, st,
                               (const T*)x, head_w, head_b, grid_xy, grid_batch_stride, gt_line_or_null, C, L, h, w, zero_rows,
                               (float)y_offset, classes_or_null, (double*)partials);
        };
        auto lanes = [&](auto t) {
            if (split) launch(t, std::integral_constant<int, 1>{});
            else if (L <= 2) launch(t, std::integral_constant<int, 2>{});
            else launch(t, std::integral_constant<int, 4>{});
        };
        if (x_bf16) lanes(lf_bf16{});
        else lanes(float{});
        LF_CHECK_LAUNCH("segfit");
        return wls_solve_launch<O()>((const double*)partials, N * L, reg, solver, beta, zinv, status, st);
    });
}

// ---------------------------------------------------------------------------------------
// Homography through the fit: the grid and its backward as launches of their own, the fit on the inline route (GridTheta), and
// autograd of the fit w.r.t. an explicit grid.
// ---------------------------------------------------------------------------------------
namespace {

// Grid from theta: one thread per pixel; grid (N | 1, H*W, 2).
__global__ __launch_bounds__(WLS_THREADS) void theta_grid_kernel(const float* __restrict__ theta, long theta_bs,
                                                                const float* __restrict__ xs, const float* __restrict__ ys,
                                                                int H, int W, float* __restrict__ grid) {
    const long P = (long)H * W, p = (long)blockIdx.x * WLS_THREADS + threadIdx.x;
    if (p >= P) return;
    const int n = blockIdx.y, i = (int)(p / W), j = (int)(p - (long)i * W);
    const Theta h = theta_load(theta, theta_bs, n);
    float gx, gy, c;
    theta_point(h, xs[j], ys[i], gx, gy, c);
    *reinterpret_cast<float2*>(grid + ((long)n * P + p) * 2) = make_float2(gx, gy);
}

// Backward of theta_grid_kernel: grad_grid (N | 1, H*W, 2) fp32 -> per-chunk partials of the nine sums per image.  A pixel whose
// incoming gradient is exactly (0, 0) -- a masked row -- contributes nothing and is not evaluated.
__global__ __launch_bounds__(WLS_THREADS) void theta_grid_bwd_kernel(const float* __restrict__ theta, long theta_bs,
                                                                    const float* __restrict__ xs, const float* __restrict__ ys,
                                                                    const float* __restrict__ ggrid, int H, int W,
                                                                    double* __restrict__ partials) {
    const long P = (long)H * W;
    const int n = blockIdx.y;
    const Theta h = theta_load(theta, theta_bs, n);
    ThetaAcc acc;
    for (long p = (long)blockIdx.x * WLS_THREADS + threadIdx.x; p < P; p += (long)gridDim.x * WLS_THREADS) {
        const float2 g = *reinterpret_cast<const float2*>(ggrid + ((long)n * P + p) * 2);
        if (g.x == 0.f && g.y == 0.f) continue;
        const int i = (int)(p / W), j = (int)(p - (long)i * W);
        const float px = xs[j], py = ys[i];
        float gx, gy, c;
        theta_point(h, px, py, gx, gy, c);
        acc.add((double)g.x, (double)g.y, gx, gy, c, px, py);
    }
    block_store_sums(acc.v, partials + ((long)n * gridDim.x + blockIdx.x) * 9);
}

// grad_theta[o] = sum of `rows` consecutive partial rows of nine, one wave per output matrix: each lane adds its rows in
// ascending order, then one butterfly.
__global__ __launch_bounds__(LF_WAVE) void theta_finish_kernel(const double* __restrict__ partials, int rows,
                                                              double* __restrict__ grad_theta) {
    const double* p = partials + (long)blockIdx.x * rows * 9;
    double s[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) s[j] = 0.0;
    for (int r = threadIdx.x; r < rows; r += LF_WAVE)
#pragma unroll
        for (int j = 0; j < 9; ++j) s[j] += p[(long)r * 9 + j];
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        const double t = lf_wave_sum(s[j]);
        if (threadIdx.x == 0) grad_theta[(long)blockIdx.x * 9 + j] = t;
    }
}

// d loss / d grid of an explicit grid: the thread that owns a pixel adds the lanes (and, for a shared grid, the images) in
// ascending order in fp64 and writes one float2; masked rows are written as 0.  The lane constants (beta, v) sit in LDS.
template <int ORDER>
__global__ __launch_bounds__(WLS_THREADS) void wls_bwd_grid_kernel(
    const float* __restrict__ logits, const float* __restrict__ grid, long grid_bs, int NK, int H, int W, int zero_rows, float y_off,
    int act_kind, const double* __restrict__ beta, const double* __restrict__ zinv, const double* __restrict__ gbeta,
    float* __restrict__ ggrid) {
    constexpr int D = ORDER + 1;
    extern __shared__ double lane_consts[];              // [NK][2][D]
    const long P = (long)H * W;
    const long nk0 = (long)blockIdx.y * NK;              // NK = lanes summed by one thread: K (per-image grid) or N*K (shared)
    for (int t = threadIdx.x; t < NK; t += WLS_THREADS) {
        double b[D], v[D];
        fit_lane_consts<D>(beta, zinv, gbeta, nk0 + t, b, v);
#pragma unroll
        for (int i = 0; i < D; ++i) { lane_consts[(t * 2) * D + i] = b[i]; lane_consts[(t * 2 + 1) * D + i] = v[i]; }
    }
    __syncthreads();
    const long p = (long)blockIdx.x * WLS_THREADS + threadIdx.x;
    if (p >= P) return;
    float2 out = make_float2(0.f, 0.f);
    if (p >= (long)zero_rows * W) {
        const float2 g = *reinterpret_cast<const float2*>(grid + (long)blockIdx.y * grid_bs + 2 * p);
        double sx = 0.0, sy = 0.0;
        for (int t = 0; t < NK; ++t) {
            double b[D], v[D], dgx, dgy;
#pragma unroll
            for (int i = 0; i < D; ++i) { b[i] = lane_consts[(t * 2) * D + i]; v[i] = lane_consts[(t * 2 + 1) * D + i]; }
            fit_pixel_bwd<D>(b, v, logits[(nk0 + t) * P + p], g.x, g.y, y_off, act_kind, dgx, dgy);
            sx += dgx;
            sy += dgy;
        }
        out = make_float2((float)sx, (float)sy);
    }
    *reinterpret_cast<float2*>(ggrid + ((long)blockIdx.y * P + p) * 2) = out;
}

}  // namespace

// theta (3,3) fp32 (theta_batch_stride 0) or (N,3,3) (9); xs (W), ys (H) fp32 base coordinates; grid out (N | 1, H*W, 2) fp32.
extern "C" int lf_theta_grid(const float* theta, long theta_batch_stride, const float* xs, const float* ys, int N, int H, int W,
                             float* grid_xy, void* stream) {
    if (theta_check("lf_theta_grid", theta, theta_batch_stride, xs, ys, N, H, W)) return -1;
    LF_REQUIRE(grid_xy && ((size_t)grid_xy & 7) == 0, "lf_theta_grid: grid null or misaligned");
    hipLaunchKernelGGL(theta_grid_kernel, dim3(lf_cdiv((long)H * W, WLS_THREADS), theta_batch_stride ? N : 1), dim3(WLS_THREADS), 0,
                       (hipStream_t)stream, theta, theta_batch_stride, xs, ys, H, W, grid_xy);
    LF_CHECK_LAUNCH("theta_grid");
    return 0;
}

extern "C" size_t lf_theta_grid_bwd_workspace_bytes(int N) { return (size_t)N * TH_CHUNKS * 9 * sizeof(double); }

// grad_grid (N | 1, H*W, 2) fp32 (the shape lf_theta_grid wrote) -> grad_theta (N | 1, 3, 3) fp64.
extern "C" int lf_theta_grid_bwd(const float* theta, long theta_batch_stride, const float* xs, const float* ys,
                                 const float* grad_grid, int N, int H, int W, double* grad_theta, void* workspace, void* stream) {
    if (theta_check("lf_theta_grid_bwd", theta, theta_batch_stride, xs, ys, N, H, W)) return -1;
    LF_REQUIRE(grad_grid && grad_theta && workspace && ((size_t)grad_grid & 7) == 0, "lf_theta_grid_bwd: null or misaligned pointer");
    hipStream_t st = (hipStream_t)stream;
    int chunks = lf_cdiv((long)H * W, WLS_THREADS);
    if (chunks > TH_CHUNKS) chunks = TH_CHUNKS;
    const int outs = theta_batch_stride ? N : 1;
    hipLaunchKernelGGL(theta_grid_bwd_kernel, dim3(chunks, outs), dim3(WLS_THREADS), 0, st, theta, theta_batch_stride, xs, ys,
                       grad_grid, H, W, (double*)workspace);
    LF_CHECK_LAUNCH("theta_grid_bwd");
    hipLaunchKernelGGL(theta_finish_kernel, dim3(outs), dim3(LF_WAVE), 0, st, (const double*)workspace, chunks, grad_theta);
    LF_CHECK_LAUNCH("theta_finish");
    return 0;
}

// lf_wls_fwd with the grid computed inline from theta: arguments as lf_wls_fwd with (theta, theta_batch_stride, xs, ys) in the
// place of (grid_xy, grid_batch_stride); partials >= lf_wls_workspace_bytes.
extern "C" int lf_wls_fwd_theta(const float* logits, const float* theta, long theta_batch_stride, const float* xs, const float* ys,
                                int N, int K, int H, int W, int zero_rows, int order, double reg, double y_offset, int act_kind,
                                int solver, double* beta, double* zinv, float* masked, void* partials, int32_t* status,
                                void* stream) {
    if (theta_check("lf_wls_fwd_theta", theta, theta_batch_stride, xs, ys, N, H, W)) return -1;
    LF_REQUIRE(logits && beta && zinv && partials && status, "lf_wls_fwd_theta: null pointer");
    if (fit_check("lf_wls_fwd_theta", N, K, H, W, zero_rows, order, act_kind)) return -1;
    return with_order(order, [&](auto O) {
        return wls_fwd_launch<O(), GridTheta>(logits, {theta, theta_batch_stride, xs, ys}, N, K, H, W, zero_rows, reg, y_offset,
                                              act_kind, solver, beta, zinv, masked, (double*)partials, status, (hipStream_t)stream);
    });
}

extern "C" size_t lf_wls_bwd_theta_workspace_bytes(int N, int K) { return (size_t)N * K * TH_CHUNKS * 9 * sizeof(double); }

// lf_wls_bwd on the inline route: grad_logits as lf_wls_bwd writes it, and grad_theta (N | 1, 3, 3) fp64 in the same pass;
// workspace >= lf_wls_bwd_theta_workspace_bytes(N, K).
extern "C" int lf_wls_bwd_theta(const float* logits, const float* theta, long theta_batch_stride, const float* xs, const float* ys,
                                int N, int K, int H, int W, int zero_rows, int order, double y_offset, int act_kind,
                                const double* beta, const double* zinv, const double* grad_beta, float* grad_logits,
                                double* grad_theta, void* workspace, void* stream) {
    if (theta_check("lf_wls_bwd_theta", theta, theta_batch_stride, xs, ys, N, H, W)) return -1;
    LF_REQUIRE(logits && beta && zinv && grad_beta && grad_logits && grad_theta && workspace, "lf_wls_bwd_theta: null pointer");
    if (fit_check("lf_wls_bwd_theta", N, K, H, W, zero_rows, order, act_kind)) return -1;
    hipStream_t st = (hipStream_t)stream;
    if (with_order(order, [&](auto O) {
            return wls_bwd_launch<O(), GridTheta>(logits, {theta, theta_batch_stride, xs, ys}, N, K, H, W, zero_rows, y_offset, act_kind,
                                                  beta, zinv, grad_beta, grad_logits, (double*)workspace, st);
        }))
        return -1;
    // per-image theta: K lanes x chunks rows each; shared theta: all N*K lanes into one matrix
    const int outs = theta_batch_stride ? N : 1, rows = (theta_batch_stride ? K : N * K) * fit_bwd_chunks(H, W);
    hipLaunchKernelGGL(theta_finish_kernel, dim3(outs), dim3(LF_WAVE), 0, st, (const double*)workspace, rows, grad_theta);
    LF_CHECK_LAUNCH("theta_finish");
    return 0;
}

// d loss / d grid of lf_wls_fwd's explicit grid (arguments as lf_wls_bwd): grad_grid (N, H*W, 2) fp32, or (H*W, 2) summed over
// the images when grid_batch_stride = 0.
extern "C" int lf_wls_bwd_grid(const float* logits, const float* grid_xy, long grid_batch_stride, int N, int K, int H, int W,
                               int zero_rows, int order, double y_offset, int act_kind, const double* beta, const double* zinv,
                               const double* grad_beta, float* grad_grid, void* stream) {
    LF_REQUIRE(logits && grid_xy && beta && zinv && grad_beta && grad_grid, "lf_wls_bwd_grid: null pointer");
    if (fit_check("lf_wls_bwd_grid", N, K, H, W, zero_rows, order, act_kind)) return -1;
    LF_REQUIRE(grid_batch_stride % 2 == 0 && ((size_t)grid_xy & 7) == 0 && ((size_t)grad_grid & 7) == 0,
               "lf_wls_bwd_grid: grid / grad_grid are read and written as float2: misaligned");
    const int NK = grid_batch_stride ? K : N * K;
    const size_t lds = (size_t)NK * 2 * (order + 1) * sizeof(double);
    LF_REQUIRE(lds <= 48 * 1024, "lf_wls_bwd_grid: %d lanes on one grid exceed the LDS table (%zu bytes)", NK, lds);
    hipStream_t st = (hipStream_t)stream;
    const dim3 g1(lf_cdiv((long)H * W, WLS_THREADS), grid_batch_stride ? N : 1);
    with_order(order, [&](auto O) {
        hipLaunchKernelGGL(wls_bwd_grid_kernel<O()>, g1, dim3(WLS_THREADS), lds, st, logits, grid_xy, grid_batch_stride, NK, H, W,
                           zero_rows, (float)y_offset, act_kind, beta, zinv, grad_beta, grad_grid);
        return 0;
    });
    LF_CHECK_LAUNCH("wls_bwd_grid");
    return 0;
}
