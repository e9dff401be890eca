// Device bodies that the --clas tail shares between its one-purpose kernels (poolflat_*_fwd_kernel in lf_convchain.hip,
// linear_fwd_kernel in lf_linear.hip, lane_decode_kernel in lf_lanes.hip) and the fused tail of the frozen detector
// (lf_clas_tail.hip): ONE text per body, so the fused launches give the composed path's bits.
#pragma once
#include "lf_common.h"
#include "lf_types.h"

typedef float lf_f32x4 __attribute__((ext_vector_type(4)));

constexpr int LF_LINEAR_NB = 8;      // batch rows per workgroup of the nn.Linear forward

// MaxPool2d(2, 2) of an NHWC tensor at flat NCHW output index u (< N * C * (H/2) * (W/2))
template <typename T>
__device__ __forceinline__ float lf_poolflat_max_at(const T* __restrict__ y, long u, int H, int W, int C) {
    const int Ho = H / 2, Wo = W / 2;
    const int j = (int)(u % Wo);
    long r = u / Wo;
    const int i = (int)(r % Ho);
    r /= Ho;
    const int c = (int)(r % C), n = (int)(r / C);
    const T* b = y + (((long)n * H + 2 * i) * W + 2 * j) * C + c;
    return fmaxf(fmaxf(lf_ld1(b), lf_ld1(b + C)), fmaxf(lf_ld1(b + (long)W * C), lf_ld1(b + (long)W * C + C)));
}

// AvgPool2d((1, W)) of an NHWC tensor, element u (< N * H * C) in (n, i, c) order; *o = its flat NCHW output index
template <typename T>
__device__ __forceinline__ float lf_poolflat_avg_at(const T* __restrict__ y, long u, int H, int W, int C, long* o) {
    const int c = (int)(u % C);
    const long r = u / C;
    const int i = (int)(r % H), n = (int)(r / H);
    const T* b = y + ((long)n * H + i) * W * C + c;
    float s = 0.f;
    for (int j = 0; j < W; ++j) s += lf_ld1(b + (long)j * C);
    *o = ((long)n * C + c) * H + i;
    return s / (float)W;
}

__device__ __forceinline__ float lf_block_sum_256(float v, float* sm) {      // sum over 256 threads, fixed order; sm: 4 floats of LDS
    v = lf_wave_sum(v);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    const float r = (sm[0] + sm[1]) + (sm[2] + sm[3]);
    __syncthreads();
    return r;
}

// y[n][o] = act(b[o] + sum_k x[n][k] * w[o][k]) for output feature o and the batch rows n0 .. n0 + 7, by one workgroup of 256
// threads (all of them must call); the weight row is read once
__device__ __forceinline__ void lf_linear_rows(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b,
                                               float* __restrict__ y, int N, int K, int O, int relu, int o, int n0, float* sm) {
    constexpr int NB = LF_LINEAR_NB;
    float acc[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) acc[j] = 0.f;
    const float* wr = w + (long)o * K;
    if ((K & 3) == 0) {
        for (int k = threadIdx.x * 4; k < K; k += 1024) {
            const lf_f32x4 wv = *reinterpret_cast<const lf_f32x4*>(wr + k);
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                if (n0 + j < N) {
                    const lf_f32x4 xv = *reinterpret_cast<const lf_f32x4*>(x + (long)(n0 + j) * K + k);
                    acc[j] = fmaf(xv.x, wv.x, fmaf(xv.y, wv.y, fmaf(xv.z, wv.z, fmaf(xv.w, wv.w, acc[j]))));
                }
            }
        }
    } else {
        for (int k = threadIdx.x; k < K; k += 256) {
            const float wv = wr[k];
#pragma unroll
            for (int j = 0; j < NB; ++j)
                if (n0 + j < N) acc[j] = fmaf(x[(long)(n0 + j) * K + k], wv, acc[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        const float s = lf_block_sum_256(acc[j], sm);
        if (threadIdx.x == 0 && n0 + j < N) {
            float v = s + (b ? b[o] : 0.f);
            if (relu) v = fmaxf(v, 0.f);
            y[(long)(n0 + j) * O + o] = v;
        }
    }
}

struct LfDecodeConsts { double m0, m1, m2, m6, m7, m8, scale, lo, hi, fill; };

// One (image, lane, sample height) of Projections.compute_coordinates + test_model's gates, in its order: line-type flag == 0 ->
// fill; sample index below the horizon bound (python slice [:bd]) -> fill; outside [lo, hi] -> fill.  b: the lane's order + 1
// coefficients, highest power first.
__device__ __forceinline__ double lf_lane_decode_at(const double* __restrict__ b, int order, double ye, double yp, const LfDecodeConsts& c,
                                                    bool flag_off, bool has_bound, int bd, int s, int S) {
    double xp = b[0];
    for (int k = 1; k <= order; ++k) xp = xp * ye + b[k];          // highest power first, as Projections.Y
    double x = (c.m0 * xp + c.m1 * yp + c.m2) / (c.m6 * xp + c.m7 * yp + c.m8) * c.scale;
    if (flag_off) x = c.fill;
    if (has_bound) {
        if (bd < 0) bd = S + bd < 0 ? 0 : S + bd;
        if (s < bd) x = c.fill;
    }
    if (x > c.hi) x = c.fill;
    if (x < c.lo) x = c.fill;
    return x;
}
