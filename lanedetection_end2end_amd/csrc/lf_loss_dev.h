// Device bodies that the per-lane loss kernels (area_loss_kernel, backproj_kernel in lf_losses.hip) share with the whole-step
// criterion (step_loss_kernel in lf_criterion.hip): ONE text per body, so the fused launch gives the per-lane modules' bits.
#pragma once
#include "lf_common.h"

constexpr int LF_LOSS_THREADS = 256;     // workgroup of every kernel that calls block_sum: four waves

// sum over the workgroup, the four wave sums added in wave order; sh: 4 doubles of LDS.  The whole workgroup calls it.
__device__ __forceinline__ double block_sum(double v, double* sh) {
    v = lf_wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return sh[0] + sh[1] + sh[2] + sh[3];
}

// Area_Loss integrand and its gradient in the coefficient differences (BEV/Loss_crit.py:103-126)
__device__ __forceinline__ double lf_area_value(double a, double b, double c, int order, int wf) {
    const double t = 0.7;
    const double t2 = t * t, t3 = t2 * t, t4 = t3 * t, t5 = t4 * t, t6 = t5 * t;
    if (order != 2) return b * b * t + a * b * t2 + (a * a * t3) / 3;
    if (wf == LF_WF_NONE)
        return a * a * t5 / 5 + 2 * a * b * t4 / 4 + (b * b + c * 2 * a) * t3 / 3 + 2 * b * c * t2 / 2 + c * c * t;
    if (wf == LF_WF_LINEAR)
        return c * c * t - t5 * ((2 * a * b) / 5 - a * a / 5) + t2 * (b * c - c * c / 2) - (a * a * t6) / 6 -
               t4 * (b * b / 4 - (a * b) / 2 + (a * c) / 2) + t3 * (b * b / 3 - (2 * c * b) / 3 + (2 * a * c) / 3);
    const double t15 = pow(t, 1.5), t25 = pow(t, 2.5), t35 = pow(t, 3.5), t45 = pow(t, 4.5), t55 = pow(t, 5.5);
    return t3 * (b * b / 3 + 2.0 / 3 * a * c) - t35 * (2.0 / 7 * b * b + 4.0 / 7 * a * c) + c * c * t + 0.2 * a * a * t5 -
           2.0 / 11 * a * a * t55 - 2.0 / 3 * c * c * t15 + 0.5 * a * b * t4 - 4.0 / 9 * a * b * t45 + b * c * t2 - 0.8 * b * c * t25;
}

__device__ __forceinline__ void lf_area_grad(double a, double b, double c, int order, int wf, double* g) {
    const double t = 0.7;
    const double t2 = t * t, t3 = t2 * t, t4 = t3 * t, t5 = t4 * t, t6 = t5 * t;
    g[2] = 0.0;
    if (order != 2) {
        g[0] = b * t2 + 2 * a * t3 / 3;
        g[1] = 2 * b * t + a * t2;
    } else if (wf == LF_WF_NONE) {
        g[0] = 2 * a * t5 / 5 + b * t4 / 2 + 2 * c * t3 / 3;
        g[1] = a * t4 / 2 + 2 * b * t3 / 3 + c * t2;
        g[2] = 2 * a * t3 / 3 + b * t2 + 2 * c * t;
    } else if (wf == LF_WF_LINEAR) {
        g[0] = -t5 * (2 * b / 5 - 2 * a / 5) - a * t6 / 3 - t4 * (-b / 2 + c / 2) + t3 * (2 * c / 3);
        g[1] = -t5 * (2 * a / 5) + t2 * c - t4 * (b / 2 - a / 2) + t3 * (2 * b / 3 - 2 * c / 3);
        g[2] = 2 * c * t + t2 * (b - c) - t4 * (a / 2) + t3 * (-2 * b / 3 + 2 * a / 3);
    } else {
        const double t15 = pow(t, 1.5), t25 = pow(t, 2.5), t35 = pow(t, 3.5), t45 = pow(t, 4.5), t55 = pow(t, 5.5);
        g[0] = t3 * (2.0 / 3 * c) - t35 * (4.0 / 7 * c) + 0.4 * a * t5 - 4.0 / 11 * a * t55 + 0.5 * b * t4 - 4.0 / 9 * b * t45;
        g[1] = t3 * (2.0 / 3 * b) - t35 * (4.0 / 7 * b) + 0.5 * a * t4 - 4.0 / 9 * a * t45 + c * t2 - 0.8 * c * t25;
        g[2] = t3 * (2.0 / 3 * a) - t35 * (4.0 / 7 * a) + 2 * c * t - 4.0 / 3 * c * t15 + b * t2 - 0.8 * b * t25;
    }
}

struct LfBackprojConsts {
    const double* Y;              // (S, order + 1) powers of the sample heights, highest first
    const double* yp;             // (S) y'
    double m00, m01, m02, m20, m21, m22;      // rows 0 and 2 of M_inv
};

// backprojection_loss of one lane (BP/Loss_crit.py:202-218) by one workgroup of LF_LOSS_THREADS threads, in two phases.  The lane is
// slot k of K: beta (order + 1 coefficients per image, bstride elements apart), x_gt / valid (S values per image, tstride apart;
// the pointers are the lane's own), x_cal * valid -> xcv[(n, k, .)] and d mean / d beta times w -> grad[(n, k, .)].  Returns the mean
// of err^2 over the valid points, 0 without one.
template <typename T>
__device__ __forceinline__ double lf_backproject_lane(const T* __restrict__ beta, long bstride, const double* __restrict__ x_gt,
                                                      const double* __restrict__ valid, long tstride, const LfBackprojConsts& c, int N,
                                                      int S, int order, int K, int k, double w, double* __restrict__ xcv,
                                                      T* __restrict__ grad, double* sh) {
    const int D = order + 1;
    const double *Y = c.Y, *yp = c.yp;
    double e2 = 0.0, nv = 0.0;
    for (long idx = threadIdx.x; idx < (long)N * S; idx += LF_LOSS_THREADS) {
        const int n = (int)(idx / S), j = (int)(idx % S);
        double xp = 0.0;
        for (int i = 0; i < D; ++i) xp = fma(Y[(long)j * D + i], (double)beta[(long)n * bstride + i], xp);
        const double t0 = c.m00 * xp + c.m01 * yp[j] + c.m02;
        const double t2 = c.m20 * xp + c.m21 * yp[j] + c.m22;
        const double xc = t0 / t2;
        const double v = valid[(long)n * tstride + j];
        const double err = (x_gt[(long)n * tstride + j] - xc) * v;
        xcv[((long)n * K + k) * S + j] = xc * v;
        e2 = fma(err, err, e2);
        nv += v;
    }
    const double te = block_sum(e2, sh), tv = block_sum(nv, sh);
    const double inv = tv != 0.0 ? 1.0 / tv : 0.0;
    // gradient: FOUR threads per image, each taking every fourth sample height, merged in a fixed order by two butterfly steps
    // (one thread per image walked all 56 heights -- 112 dependent fp64 divisions on ONE wave, 43 us per launch)
    for (int n0 = 0; n0 < N; n0 += 64) {
        const int n = n0 + (int)(threadIdx.x >> 2), q = (int)(threadIdx.x & 3);
        const bool live = n < N;
        const int nn = live ? n : 0;
        double g[4] = {0, 0, 0, 0};
        for (int j = q; j < S && live; j += 4) {
            double xp = 0.0;
            for (int i = 0; i < D; ++i) xp = fma(Y[(long)j * D + i], (double)beta[(long)nn * bstride + i], xp);
            const double t0 = c.m00 * xp + c.m01 * yp[j] + c.m02;
            const double t2 = c.m20 * xp + c.m21 * yp[j] + c.m22;
            const double v = valid[(long)nn * tstride + j];
            const double err = (x_gt[(long)nn * tstride + j] - t0 / t2) * v;
            const double dxc = (c.m00 * t2 - c.m20 * t0) / (t2 * t2);
            const double gx = -2.0 * err * v * inv * dxc;
            for (int i = 0; i < D; ++i) g[i] = fma(gx, Y[(long)j * D + i], g[i]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            g[i] += __shfl_xor(g[i], 1, 64);
            g[i] += __shfl_xor(g[i], 2, 64);
        }
        if (live && q == 0)
            for (int i = 0; i < D; ++i) grad[((long)n * K + k) * D + i] = (T)(g[i] * w);
    }
    return tv != 0.0 ? te / tv : 0.0;
}
