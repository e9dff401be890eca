// The tail of both --clas heads and the lane decoding of one camera frame, fused (include/lanefit.h, "additions since 5 -- frozen
// --clas heads"): what follows the two conv trunks in Classification.forward (BP/Networks/LSQ_layer.py:197-207) and the tail of
// test_model (BP/test.py:60-88) -- pooling, the fully connected layers, the line-type flags, the horizon row, and the 56
// x-coordinates of every lane with test_model's gates -- as THREE dependent launches instead of about 25:
//
//   A  clas_tail_pool_kernel     MaxPool2d(2,2) of the line trunk and AvgPool2d((1,W)) of the horizon trunk, both flattened in NCHW order
//   B  clas_tail_gemv_kernel     fully_connected1 (+ReLU) and fully_connected_horizon in one grid: O1 + R workgroups x ceil(N / 8)
//   C  clas_tail_finish_kernel   fully_connected_line1, the flags, the horizon row and the N * L * S decode; one workgroup per 8 images
//
// Every body is the one-purpose kernel's own text (lf_clas_dev.h), so the logits and the lanes are the composed path's bit for
// bit.  The horizon row sums its sigmoids in fp64 in a fixed order; torch sums them in fp32 in its own order, and the row is then
// snapped to a 10-pixel grid, so the two agree wherever (p * 2.5 + 80) / 10 is not within ~1e-3 of a half (the tests assert the
// margin).  C is a launch of its own, not the last-arriving workgroup of B behind a ticket: the kernel boundary is what makes B's
// N * (O1 + R) outputs visible to the vector loads of the shared GEMV body.
#include "lf_clas_dev.h"

namespace {

struct TailArgs {
    const void *y_line, *y_hor;
    int N, H, W, C, O1, R, L, order, S;
    const float *w1, *b1, *wl, *bl, *wh, *bh;
    const double *beta, *y_eval, *y_prime;
    LfDecodeConsts dc;
    float *feat_line, *feat_hor, *f1;                 // workspace
    float *line, *horizon, *line_flags;
    int *horizon_row, *lanes;
    int pool_line_blocks;
};

template <typename T>
__global__ __launch_bounds__(256) void clas_tail_pool_kernel(const TailArgs a) {
    if ((int)blockIdx.x < a.pool_line_blocks) {
        const long u = (long)blockIdx.x * 256 + threadIdx.x;
        if (u < (long)a.N * a.C * (a.H / 2) * (a.W / 2)) a.feat_line[u] = lf_poolflat_max_at((const T*)a.y_line, u, a.H, a.W, a.C);
    } else {
        const long u = (long)((int)blockIdx.x - a.pool_line_blocks) * 256 + threadIdx.x;
        if (u < (long)a.N * a.H * a.C) {
            long o;
            const float v = lf_poolflat_avg_at((const T*)a.y_hor, u, a.H, a.W, a.C, &o);
            a.feat_hor[o] = v;
        }
    }
}

__global__ __launch_bounds__(256) void clas_tail_gemv_kernel(const TailArgs a) {
    __shared__ float sm[4];
    const int o = blockIdx.x, n0 = blockIdx.y * LF_LINEAR_NB;
    if (o < a.O1) lf_linear_rows(a.feat_line, a.w1, a.b1, a.f1, a.N, a.C * (a.H / 2) * (a.W / 2), a.O1, 1, o, n0, sm);
    else lf_linear_rows(a.feat_hor, a.wh, a.bh, a.horizon, a.N, a.C * a.H, a.R, 0, o - a.O1, n0, sm);
}

__device__ __forceinline__ double sigmoid64(float z) { return 1.0 / (1.0 + exp(-(double)z)); }

__global__ __launch_bounds__(256) void clas_tail_finish_kernel(const TailArgs a) {
    __shared__ float sm[4];
    __shared__ double sd[4];
    const int n0 = blockIdx.x * LF_LINEAR_NB, n1 = min(n0 + LF_LINEAR_NB, a.N), tid = threadIdx.x;
    for (int o = 0; o < 4; ++o) lf_linear_rows(a.f1, a.wl, a.bl, a.line, a.N, a.O1, 4, 0, o, n0, sm);
    __syncthreads();                                  // (thread 0's logits of this workgroup's rows, read below by the others)
    // torch.round(torch.sigmoid(line)), half to even
    if (tid < (n1 - n0) * 4) a.line_flags[n0 * 4 + tid] = (float)rint(sigmoid64(a.line[n0 * 4 + tid]));
    // horizon row: sigmoid votes summed in fp64 -- a thread's rows in ascending order, then the wave butterfly, then the four waves
    for (int n = n0; n < n1; ++n) {
        double s = 0.0;
        for (int r = tid; r < a.R; r += 256) s += sigmoid64(a.horizon[(long)n * a.R + r]);
        s = lf_wave_sum(s);
        if ((tid & 63) == 0) sd[tid >> 6] = s;
        __syncthreads();
        if (tid == 0) {
            const double p = (sd[0] + sd[1]) + (sd[2] + sd[3]);
            a.horizon_row[n] = (int)(rint((p * 2.5 + 80.0) / 10.0) * 10.0);
        }
        __syncthreads();
    }
    // (the flags and rows above were written by this workgroup: visible to it behind the barrier)
    const int perm[4] = {1, 2, 0, 3};                 // test_model's re-index of the line flags into lane order
    const int per = a.L * a.S;
    for (int u = tid; u < (n1 - n0) * per; u += 256) {
        const int n = n0 + u / per, ls = u % per, l = ls / a.S, s = ls % a.S;
        const long nl = (long)n * a.L + l;
        const int bd = (a.horizon_row[n] - 160) / 10;         // torch.div(row - 160, 10, rounding_mode='trunc')
        const double x = lf_lane_decode_at(a.beta + nl * (a.order + 1), a.order, a.y_eval[s], a.y_prime[s], a.dc,
                                           a.line_flags[n * 4 + perm[l]] == 0.f, true, bd, s, a.S);
        a.lanes[nl * a.S + s] = (int)rint(x);
    }
}

struct TailLayout { long feat_line, feat_hor, f1, total; };
TailLayout tail_layout(int N, int H, int W, int C, int O1) {
    auto al = [](long b) { return (b + 255) / 256 * 256; };
    TailLayout L;
    long cur = 0;
    L.feat_line = cur; cur += al((long)N * C * (H / 2) * (W / 2) * 4);
    L.feat_hor = cur; cur += al((long)N * C * H * 4);
    L.f1 = cur; cur += al((long)N * O1 * 4);
    L.total = cur;
    return L;
}

}  // namespace

extern "C" {

size_t lf_clas_tail_workspace_bytes(int N, int H, int W, int C, int O1) {
    if (N < 1 || H < 2 || W < 2 || C < 1 || O1 < 1) return 0;
    return (size_t)tail_layout(N, H, W, C, O1).total;
}

int lf_clas_tail(const void* y_line, const void* y_hor, int bf16, int N, int H, int W, int C, const float* w1, const float* b1, int O1,
                 const float* wl, const float* bl, const float* wh, const float* bh, int R, const double* beta, int L, int order,
                 const double* y_eval, const double* y_prime, int S, const double* minv_host, double scale, double lo, double hi,
                 double fill, float* line, float* horizon, float* line_flags, int32_t* horizon_row, int32_t* lanes, void* workspace,
                 size_t workspace_bytes, void* stream) {
    LF_REQUIRE(y_line && y_hor && w1 && b1 && wl && bl && wh && bh && beta && y_eval && y_prime && minv_host && line && horizon &&
               line_flags && horizon_row && lanes && workspace, "lf_clas_tail: null pointer");
    LF_REQUIRE(N > 0 && H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0 && C > 0 && O1 > 0 && R > 0,
               "lf_clas_tail: bad shape (N=%d H=%d W=%d C=%d O1=%d R=%d; max-pool needs even H, W)", N, H, W, C, O1, R);
    LF_REQUIRE(L >= 1 && L <= 4 && order >= 0 && order <= 3 && S > 0, "lf_clas_tail: bad lanes (L=%d not in 1..4, order=%d, S=%d)", L, order, S);
    LF_REQUIRE((long)N * C * (H / 2) * (W / 2) < (1l << 31) && (long)C * H * (long)W < (1l << 31), "lf_clas_tail: tensor too large");
    const TailLayout lay = tail_layout(N, H, W, C, O1);
    LF_REQUIRE(workspace_bytes >= (size_t)lay.total, "lf_clas_tail: workspace too small (%zu < %ld)", workspace_bytes, lay.total);
    if (lo > hi) { lo = -1e300; hi = 1e300; }
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    const double* m = minv_host;
    TailArgs a;
    a.y_line = y_line; a.y_hor = y_hor;
    a.N = N; a.H = H; a.W = W; a.C = C; a.O1 = O1; a.R = R; a.L = L; a.order = order; a.S = S;
    a.w1 = w1; a.b1 = b1; a.wl = wl; a.bl = bl; a.wh = wh; a.bh = bh;
    a.beta = beta; a.y_eval = y_eval; a.y_prime = y_prime;
    a.dc = LfDecodeConsts{m[0], m[1], m[2], m[6], m[7], m[8], scale, lo, hi, fill};
    a.feat_line = (float*)(ws + lay.feat_line); a.feat_hor = (float*)(ws + lay.feat_hor); a.f1 = (float*)(ws + lay.f1);
    a.line = line; a.horizon = horizon; a.line_flags = line_flags; a.horizon_row = horizon_row; a.lanes = lanes;
    a.pool_line_blocks = lf_cdiv((long)N * C * (H / 2) * (W / 2), 256);
    const dim3 gridA((unsigned)(a.pool_line_blocks + lf_cdiv((long)N * H * C, 256)));
    if (bf16) hipLaunchKernelGGL(clas_tail_pool_kernel<lf_bf16>, gridA, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(clas_tail_pool_kernel<float>, gridA, dim3(256), 0, st, a);
    LF_CHECK_LAUNCH("clas_tail_pool");
    const int groups = lf_cdiv(N, LF_LINEAR_NB);
    hipLaunchKernelGGL(clas_tail_gemv_kernel, dim3(O1 + R, groups), dim3(256), 0, st, a);
    LF_CHECK_LAUNCH("clas_tail_gemv");
    hipLaunchKernelGGL(clas_tail_finish_kernel, dim3(groups), dim3(256), 0, st, a);
    LF_CHECK_LAUNCH("clas_tail_finish");
    return 0;
}

}  // extern "C"
