// The per-lane losses for gfx950: area, MSE, back-projection and cross-entropy losses with their gradients, and the trapezoid
// metric.  The whole-step criterion (lf_criterion.hip) runs the area and back-projection bodies of lf_loss_dev.h too.
//
// Reference behaviour (no code shared): BEV/Loss_crit.py:12-35,61-150, BP/Loss_crit.py:166-218.   Math: SURVEY.md 2.2.
#include "lf_common.h"
#include "lf_loss_dev.h"

// ---------------------------------------------------------------------------------------
// Area loss (single workgroup; N is a batch size)
// ---------------------------------------------------------------------------------------
namespace {

template <typename T>
__global__ __launch_bounds__(256) void area_loss_kernel(const T* __restrict__ beta, long bstride, const T* __restrict__ gt,
                                                       int N, int order, int wf, T* __restrict__ loss, T* __restrict__ grad) {
    const int D = order + 1;
    __shared__ double sL[4], sC[4];
    __shared__ double tot[2];
    double Lsum = 0.0, cnt = 0.0;
    for (int i = threadIdx.x; i < N; i += 256) {
        double d[3] = {0, 0, 0};
        bool keep = true;
        for (int j = 0; j < D; ++j) {
            const double gj = (double)gt[(long)i * D + j];
            d[j] = (double)beta[(long)i * bstride + j] - gj;
            keep = keep && (gj != 0.0);
        }
        if (keep) { Lsum += lf_area_value(d[0], d[1], d[2], order, wf); cnt += 1.0; }
    }
    Lsum = lf_wave_sum(Lsum);
    cnt = lf_wave_sum(cnt);
    if ((threadIdx.x & 63) == 0) { sL[threadIdx.x >> 6] = Lsum; sC[threadIdx.x >> 6] = cnt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        tot[0] = sL[0] + sL[1] + sL[2] + sL[3];
        tot[1] = sC[0] + sC[1] + sC[2] + sC[3];
        loss[0] = (T)(tot[1] > 0 ? tot[0] / tot[1] : 0.0);
    }
    __syncthreads();
    const double inv = tot[1] > 0 ? 1.0 / tot[1] : 0.0;
    for (int i = threadIdx.x; i < N; i += 256) {
        double d[3] = {0, 0, 0};
        bool keep = true;
        for (int j = 0; j < D; ++j) {
            const double gj = (double)gt[(long)i * D + j];
            d[j] = (double)beta[(long)i * bstride + j] - gj;
            keep = keep && (gj != 0.0);
        }
        double g[3];
        lf_area_grad(d[0], d[1], d[2], order, wf, g);
        for (int j = 0; j < D; ++j) grad[(long)i * D + j] = (T)(keep ? g[j] * inv : 0.0);
    }
}

// Back-projection loss: one workgroup, the lane body of lf_loss_dev.h on an (N, .) lane of its own (K = 1, weight 1)
__global__ __launch_bounds__(LF_LOSS_THREADS) void backproj_kernel(const double* __restrict__ beta, long bstride,
                                                                  const double* __restrict__ x_gt, const double* __restrict__ valid,
                                                                  const double* __restrict__ Y, const double* __restrict__ yp,
                                                                  double m00, double m01, double m02, double m20, double m21, double m22,
                                                                  int N, int S, int order, double* __restrict__ loss,
                                                                  double* __restrict__ xcv, double* __restrict__ grad) {
    __shared__ double sh[4];
    const LfBackprojConsts c = {Y, yp, m00, m01, m02, m20, m21, m22};
    const double mean = lf_backproject_lane<double>(beta, bstride, x_gt, valid, S, c, N, S, order, 1, 0, 1.0, xcv, grad, sh);
    if (threadIdx.x == 0) loss[0] = mean;
}

// Cross entropy: one thread per pixel, NCHW logits (channel planes are contiguous in w => coalesced).
__global__ __launch_bounds__(256) void ce_fwd_kernel(const float* __restrict__ z, const int64_t* __restrict__ tgt,
                                                    const float* __restrict__ wts, int C, long HW, long total,
                                                    double* __restrict__ acc) {
    double num = 0.0, den = 0.0, nbad = 0.0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long n = i / HW, p = i % HW;
        const float* zp = z + n * C * HW + p;
        float v[CE_MAXC], mx = -INFINITY;
        for (int c = 0; c < C; ++c) { v[c] = zp[(long)c * HW]; mx = fmaxf(mx, v[c]); }
        float se = 0.f;
        for (int c = 0; c < C; ++c) se += expf(v[c] - mx);
        const int64_t t64 = tgt[i];
        const bool okt = t64 >= 0 && t64 < C;               // a label outside [0, C) is counted and ignored (weight 0)
        const int t = okt ? (int)t64 : 0;
        float zt = 0.f;
        for (int c = 0; c < C; ++c) zt = (c == t) ? v[c] : zt;
        const float w = okt ? wts[t] : 0.f;
        num += (double)(w * (mx + logf(se) - zt));
        den += (double)w;
        nbad += okt ? 0.0 : 1.0;
    }
    num = lf_wave_sum(num);
    den = lf_wave_sum(den);
    nbad = lf_wave_sum(nbad);
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(acc, num); atomicAdd(acc + 1, den);
        if (nbad != 0.0) atomicAdd(acc + 2, nbad);
    }
}
__global__ void ce_finish_kernel(const double* acc, float* loss) { loss[0] = (float)(acc[0] / acc[1]); }
__global__ __launch_bounds__(256) void ce_bwd_kernel(const float* __restrict__ z, const int64_t* __restrict__ tgt,
                                                    const float* __restrict__ wts, int C, long HW, long total,
                                                    const double* __restrict__ acc, const float* __restrict__ up,
                                                    float* __restrict__ gz) {
    const float scale = up[0] / (float)acc[1];
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long n = i / HW, p = i % HW;
        const float* zp = z + n * C * HW + p;
        float* gp = gz + n * C * HW + p;
        float v[CE_MAXC], mx = -INFINITY;
        for (int c = 0; c < C; ++c) { v[c] = zp[(long)c * HW]; mx = fmaxf(mx, v[c]); }
        float se = 0.f;
        for (int c = 0; c < C; ++c) { v[c] = expf(v[c] - mx); se += v[c]; }
        const int64_t t64 = tgt[i];
        const bool okt = t64 >= 0 && t64 < C;
        const int t = okt ? (int)t64 : 0;
        const float w = okt ? wts[t] * scale : 0.f, ise = 1.f / se;
        for (int c = 0; c < C; ++c) gp[(long)c * HW] = w * (v[c] * ise - (c == t ? 1.f : 0.f));
    }
}

}  // namespace

extern "C" int lf_area_loss(const void* beta, long beta_stride, const void* gt, int N, int order, int weight_funct,
                            int dtype, void* loss, void* grad, void* stream) {
    LF_REQUIRE(beta && gt && loss && grad, "lf_area_loss: null pointer");
    LF_REQUIRE(order == 1 || order == 2, "lf_area_loss: order %d not implemented (reference: Loss_crit.py:125-128)", order);
    LF_REQUIRE(weight_funct >= 0 && weight_funct <= 2, "lf_area_loss: bad weight function %d", weight_funct);
    LF_REQUIRE(N > 0, "lf_area_loss: N must be positive");
    hipStream_t st = (hipStream_t)stream;
    if (dtype == LF_F64)
        hipLaunchKernelGGL(area_loss_kernel<double>, dim3(1), dim3(256), 0, st, (const double*)beta, beta_stride,
                           (const double*)gt, N, order, weight_funct, (double*)loss, (double*)grad);
    else
        hipLaunchKernelGGL(area_loss_kernel<float>, dim3(1), dim3(256), 0, st, (const float*)beta, beta_stride,
                           (const float*)gt, N, order, weight_funct, (float*)loss, (float*)grad);
    LF_CHECK_LAUNCH("area_loss");
    return 0;
}

namespace {
// MSE_Loss: mean over all n elements of (p - q)^2 and its gradient 2 (p - q) / n; one block, fp64 accumulation
template <typename T>
__global__ __launch_bounds__(256) void mse_loss_kernel(const T* __restrict__ p, const T* __restrict__ q, long n,
                                                      T* __restrict__ loss, T* __restrict__ grad) {
    __shared__ double sw[4];
    double acc = 0.0;
    const double inv = 1.0 / (double)n;
    for (long i = threadIdx.x; i < n; i += 256) {
        const double d = (double)p[i] - (double)q[i];
        acc += d * d;
        grad[i] = (T)(2.0 * d * inv);
    }
    acc = lf_wave_sum(acc);
    if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) *loss = (T)(((sw[0] + sw[1]) + (sw[2] + sw[3])) * inv);
}
}  // namespace

extern "C" int lf_mse_loss(const void* params, const void* gt, long n, int dtype, void* loss, void* grad, void* stream) {
    LF_REQUIRE(params && gt && loss && grad && n > 0, "lf_mse_loss: bad arguments");
    if (dtype == LF_F64)
        hipLaunchKernelGGL(mse_loss_kernel<double>, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)params, (const double*)gt, n,
                           (double*)loss, (double*)grad);
    else
        hipLaunchKernelGGL(mse_loss_kernel<float>, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)params, (const float*)gt, n,
                           (float*)loss, (float*)grad);
    LF_CHECK_LAUNCH("mse_loss");
    return 0;
}

extern "C" int lf_backproj_loss(const double* beta, long beta_stride, const double* x_gt, const double* valid,
                                const double* Y, const double* y_prime, const double* minv_host, int N, int S,
                                int order, double* loss, double* x_cal_valid, double* grad, void* stream) {
    LF_REQUIRE(beta && x_gt && valid && Y && y_prime && minv_host && loss && x_cal_valid && grad,
               "lf_backproj_loss: null pointer");
    LF_REQUIRE(order >= 0 && order <= 3 && N > 0 && S > 0, "lf_backproj_loss: bad shape");
    const double* m = minv_host;
    hipLaunchKernelGGL(backproj_kernel, dim3(1), dim3(LF_LOSS_THREADS), 0, (hipStream_t)stream, beta, beta_stride, x_gt, valid, Y,
                       y_prime, m[0], m[1], m[2], m[6], m[7], m[8], N, S, order, loss, x_cal_valid, grad);
    LF_CHECK_LAUNCH("backproj_loss");
    return 0;
}

extern "C" int lf_ce2d_fwd(const float* logits, const int64_t* target, const float* weights, int N, int C, int H, int W,
                           double* acc, float* loss, void* stream) {
    LF_REQUIRE(logits && target && weights && acc && loss, "lf_ce2d_fwd: null pointer");
    LF_REQUIRE(C >= 1 && C <= CE_MAXC, "lf_ce2d_fwd: C=%d not in 1..%d", C, CE_MAXC);
    hipStream_t st = (hipStream_t)stream;
    const long HW = (long)H * W, total = (long)N * HW;
    if (hipMemsetAsync(acc, 0, 3 * sizeof(double), st) != hipSuccess) return lf_fail("lf_ce2d_fwd: memset failed");
    int grid = lf_cdiv(total, 256);
    if (grid > 2048) grid = 2048;
    hipLaunchKernelGGL(ce_fwd_kernel, dim3(grid), dim3(256), 0, st, logits, target, weights, C, HW, total, acc);
    hipLaunchKernelGGL(ce_finish_kernel, dim3(1), dim3(1), 0, st, acc, loss);
    LF_CHECK_LAUNCH("ce2d_fwd");
    return 0;
}

extern "C" int lf_ce2d_bwd(const float* logits, const int64_t* target, const float* weights, int N, int C, int H, int W,
                           const double* acc, const float* upstream, float* grad_logits, void* stream) {
    LF_REQUIRE(logits && target && weights && acc && upstream && grad_logits, "lf_ce2d_bwd: null pointer");
    LF_REQUIRE(C >= 1 && C <= CE_MAXC, "lf_ce2d_bwd: C=%d not in 1..%d", C, CE_MAXC);
    const long HW = (long)H * W, total = (long)N * HW;
    int grid = lf_cdiv(total, 256);
    if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(ce_bwd_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, logits, target, weights, C, HW,
                       total, acc, upstream, grad_logits);
    LF_CHECK_LAUNCH("ce2d_bwd");
    return 0;
}

// ---- exact-area metric (BEV/Loss_crit.py:12-35 polynomial.trapezoidal) ------------------------------------
// One thread per curve pair; the sum runs in the reference's order and dtype so fp32 inputs round identically.
template <typename T>
__global__ __launch_bounds__(256) void trapezoid_kernel(const T* __restrict__ p, const T* __restrict__ q, int B, double a,
                                                       double b, int n, T* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= B) return;
    const T pa = p[3 * i], pb = p[3 * i + 1], pc = p[3 * i + 2];
    const T qa = q[3 * i], qb = q[3 * i + 1], qc = q[3 * i + 2];
    const double h = (b - a) / n;
    auto ev = [](T c2, T c1, T c0, double x) -> T { return c2 * (T)(x * x) + c1 * (T)x + c0; };
    T s = (T)0;
    s += fabs(ev(pa, pb, pc, a) / (T)2 - ev(qa, qb, qc, a) / (T)2);
    for (int k = 1; k < n; ++k) s += fabs(ev(pa, pb, pc, a + k * h) - ev(qa, qb, qc, a + k * h));
    s += fabs(ev(pa, pb, pc, b) / (T)2 - ev(qa, qb, qc, b) / (T)2);
    out[i] = s * (T)h;
}

// p, q: (B, 3) coefficient rows [a, b, c] of a*x^2 + b*x + c; is_double selects fp64 / fp32 storage.
extern "C" int lf_trapezoid(const void* p, const void* q, int B, double a, double b, int n, int is_double, void* out,
                            void* stream) {
    LF_REQUIRE(p && q && out && B > 0 && n > 0, "lf_trapezoid: bad arguments");
    if (is_double)
        hipLaunchKernelGGL(trapezoid_kernel<double>, dim3(lf_cdiv(B, 256)), dim3(256), 0, (hipStream_t)stream, (const double*)p,
                           (const double*)q, B, a, b, n, (double*)out);
    else
        hipLaunchKernelGGL(trapezoid_kernel<float>, dim3(lf_cdiv(B, 256)), dim3(256), 0, (hipStream_t)stream, (const float*)p,
                           (const float*)q, B, a, b, n, (float*)out);
    LF_CHECK_LAUNCH("trapezoid");
    return 0;
}
