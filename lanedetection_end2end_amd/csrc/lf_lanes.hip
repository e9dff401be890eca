// Decoded lanes for gfx950: the fitted polynomials back in image coordinates (both trees' decoders) and the TuSimple scorer.
//
// Reference behaviour (no code shared): BP/test.py:60-88,128-186, BP/eval_lane.py:15-57,
// BEV/Dataloader/Load_Data_new.py:334-420, BEV/main.py:445-488.
#include "lf_clas_dev.h"
#include "lf_common.h"

// ---- inference-side back-projection + lane post-processing (BP/test.py:60-88, Projections :128-186) -------
// One thread per (image, lane, sample height): evaluate the fitted polynomial at y_eval, map (x', y') back
// through M_inv, scale to the 1280-wide frame, then apply the three gates of test_model in its order:
// line-type flag == 0 -> fill; sample index below the horizon bound -> fill; outside [lo, hi] -> fill.
__global__ __launch_bounds__(256) void lane_decode_kernel(const double* __restrict__ beta, const double* __restrict__ y_eval,
                                                         const double* __restrict__ y_prime, double m0, double m1, double m2,
                                                         double m6, double m7, double m8, double scale,
                                                         const float* __restrict__ line_flag, const int* __restrict__ bound,
                                                         double lo, double hi, double fill, int N, int L, int S, int order,
                                                         double* __restrict__ x_out, int* __restrict__ x_int) {
    const long total = (long)N * L * S;
    const LfDecodeConsts c = {m0, m1, m2, m6, m7, m8, scale, lo, hi, fill};
    for (long u = (long)blockIdx.x * 256 + threadIdx.x; u < total; u += (long)gridDim.x * 256) {
        const int s = (int)(u % S);
        const long nl = u / S;
        const int n = (int)(nl / L);
        // (the arithmetic and the gates: lf_lane_decode_at, lf_clas_dev.h -- the fused --clas tail runs the same text)
        const double x = lf_lane_decode_at(beta + nl * (order + 1), order, y_eval[s], y_prime[s], c, line_flag && line_flag[nl] == 0.f,
                                           bound != nullptr, bound ? bound[n] : 0, s, S);
        if (x_out) x_out[u] = x;
        if (x_int) x_int[u] = (int)rint(x);                             // np.round: half to even
    }
}

// beta (N, L, order+1) fp64 contiguous; line_flag (N, L) fp32 (already in lane order) or NULL; bound (N) int32 or NULL;
// lo > hi disables the range gate.  x_out (N, L, S) fp64 and/or x_int (N, L, S) int32.
extern "C" int lf_lane_decode(const double* beta, const double* y_eval, const double* y_prime, const double* minv_host,
                              double scale, const float* line_flag, const int* bound, double lo, double hi, double fill, int N,
                              int L, int S, int order, double* x_out, int* x_int, void* stream) {
    LF_REQUIRE(beta && y_eval && y_prime && minv_host && (x_out || x_int), "lf_lane_decode: null pointer");
    LF_REQUIRE(order >= 0 && order <= 3 && N > 0 && L > 0 && S > 0, "lf_lane_decode: bad shape");
    const double* m = minv_host;
    if (lo > hi) { lo = -1e300; hi = 1e300; }
    hipLaunchKernelGGL(lane_decode_kernel, dim3(lf_cdiv((long)N * L * S, 256)), dim3(256), 0, (hipStream_t)stream, beta, y_eval,
                       y_prime, m[0], m[1], m[2], m[6], m[7], m[8], scale, line_flag, bound, lo, hi, fill, N, L, S, order, x_out,
                       x_int);
    LF_CHECK_LAUNCH("lane_decode");
    return 0;
}

// ---- TuSimple scoring of decoded lanes (BP/eval_lane.py:15-57, LaneEval.bench) ------------------------------
// One wave per image, lane = sample index (S <= 256: up to four samples per lane, kept in registers).  Every count is a
// ballot / popcount and every fp64 sum a butterfly in a fixed order, so a result does not depend on the launch; past the
// ballots all values are wave-uniform and the statements below are bench's, in its order:
//   angle      k = slope of x on y over the gt samples with x >= 0 (centred, two passes); 0 with fewer than two of them
//   threshold  pixel_thresh * sqrt(1 + k^2)      (= pixel_thresh / cos(arctan k))
//   hits       negative coordinates become -100 on both sides, then |pred - gt| < threshold
//   max_acc    max over the pred lanes of hits / S (lowest pred index on a tie); 0 without pred lanes
//   fn / fp    gt lanes below pt_thresh; pred lanes that matched nothing; with more than four gt lanes one miss is forgiven and the
//              smallest max_acc leaves the sum.  The sum runs in ascending gt order in fp64, as Python's sum() does.
constexpr int LE_MAXL = 8;       // pred / gt lanes per image
constexpr int LE_MAXS = 256;     // samples per lane
constexpr int LE_WAVES = 4;      // images per workgroup
constexpr int LE_ITER = LE_MAXS / LF_WAVE;

__device__ __forceinline__ int le_wave_count(bool pred) { return __popcll(__ballot(pred)); }

__global__ __launch_bounds__(LE_WAVES * LF_WAVE) void lane_eval_kernel(
    const int32_t* __restrict__ pred, const int32_t* __restrict__ pred_count, const int32_t* __restrict__ gt,
    const int32_t* __restrict__ gt_count, const int32_t* __restrict__ index, const double* __restrict__ y_samples, long y_stride,
    const float* __restrict__ run_time, int N, int M, int P, int G, int S, double pixel_thresh, double pt_thresh,
    double* __restrict__ per_image, double* __restrict__ best_acc, int32_t* __restrict__ best_pred, int32_t* __restrict__ bad_index) {
    const int lane = threadIdx.x & (LF_WAVE - 1);
    const int n = blockIdx.x * LE_WAVES + (threadIdx.x >> 6);
    if (n >= N) return;                                        // (whole waves leave: no barrier below)
    double acc_out = 0., fp_out = 0., fn_out = 1.;             // what a bad index and bench's early exit score
    double lane_best = 0.;                                     // this lane's entry of the (G) rows: lane g holds gt lane g
    int lane_arg = -1;
    long row = index ? (long)index[n] : (long)n;
    const bool in_range = row >= 0 && row < M;
    if (!in_range) {                                           // counted for the host (IndexError), never dereferenced
        if (lane == 0) atomicAdd(bad_index, 1);
        row = 0;
    }
    int Pn = pred_count ? pred_count[n] : P;
    Pn = Pn < 0 ? 0 : (Pn > P ? P : Pn);
    int Gn = gt_count[row];
    Gn = Gn < 0 ? 0 : (Gn > G ? G : Gn);
    const float rt = run_time ? run_time[n] : 20.f;
    if (in_range && !(rt > 200.f || Gn + 2 < Pn)) {
        const double* ys = y_samples + row * y_stride;
        const int32_t* gt_n = gt + row * (long)G * S;
        const int32_t* pr_n = pred + (long)n * P * S;
        double y[LE_ITER];
#pragma unroll
        for (int i = 0; i < LE_ITER; ++i) {
            const int s = i * LF_WAVE + lane;
            y[i] = s < S ? ys[s] : 0.;
        }
        double sum = 0., lowest = 0.;
        int fn = 0;
        for (int g = 0; g < Gn; ++g) {
            int xg[LE_ITER];
            bool ok[LE_ITER];
            int cnt = 0;
            double sx = 0., sy = 0.;
#pragma unroll
            for (int i = 0; i < LE_ITER; ++i) {
                const int s = i * LF_WAVE + lane;
                xg[i] = s < S ? gt_n[(long)g * S + s] : -1;
                ok[i] = s < S && xg[i] >= 0;
                cnt += le_wave_count(ok[i]);
                sx += ok[i] ? (double)xg[i] : 0.;
                sy += ok[i] ? y[i] : 0.;
            }
            double k = 0.;
            if (cnt > 1) {
                const double mx = lf_wave_sum(sx) / cnt, my = lf_wave_sum(sy) / cnt;
                double sxy = 0., syy = 0.;
#pragma unroll
                for (int i = 0; i < LE_ITER; ++i) {
                    const double dy = ok[i] ? y[i] - my : 0.;
                    sxy += ok[i] ? dy * ((double)xg[i] - mx) : 0.;
                    syy += dy * dy;
                }
                sxy = lf_wave_sum(sxy);
                syy = lf_wave_sum(syy);
                k = syy > 0. ? sxy / syy : 0.;
            }
            const double thresh = pixel_thresh * sqrt(1. + k * k);
            double max_acc = 0.;
            int arg = -1;
            for (int p = 0; p < Pn; ++p) {
                int hits = 0;
#pragma unroll
                for (int i = 0; i < LE_ITER; ++i) {
                    const int s = i * LF_WAVE + lane;
                    const int xp = s < S ? pr_n[(long)p * S + s] : -1;
                    const double d = fabs((double)(xp >= 0 ? xp : -100) - (double)(xg[i] >= 0 ? xg[i] : -100));
                    hits += le_wave_count(s < S && d < thresh);
                }
                const double a = (double)hits / (double)S;
                if (p == 0 || a > max_acc) { max_acc = a; arg = p; }
            }
            fn += max_acc < pt_thresh ? 1 : 0;
            sum += max_acc;
            lowest = (g == 0 || max_acc < lowest) ? max_acc : lowest;
            if (lane == g) { lane_best = max_acc; lane_arg = arg; }
        }
        const int matched = Gn - fn;
        const double fp = (double)(Pn - matched);
        if (Gn > 4 && fn > 0) fn -= 1;
        if (Gn > 4) sum -= lowest;
        const double denom = (double)(Gn < 4 ? (Gn > 1 ? Gn : 1) : 4);
        acc_out = sum / denom;
        fp_out = Pn > 0 ? fp / (double)Pn : 0.;
        fn_out = (double)fn / denom;
    }
    if (lane == 0) {
        per_image[3 * (long)n + 0] = acc_out;
        per_image[3 * (long)n + 1] = fp_out;
        per_image[3 * (long)n + 2] = fn_out;
    }
    if (best_acc && lane < G) best_acc[(long)n * G + lane] = lane_best;
    if (best_pred && lane < G) best_pred[(long)n * G + lane] = lane_arg;
}

// Sums of the (N, 3) per-image scores: one workgroup; thread t adds rows t, t + 256, ... in that order, then a fixed tree in LDS.
__global__ __launch_bounds__(256) void lane_eval_totals_kernel(const double* __restrict__ per_image, int N, double* __restrict__ totals) {
    __shared__ double part[3][256];
    double a[3] = {0., 0., 0.};
    for (int n = threadIdx.x; n < N; n += 256)
        for (int c = 0; c < 3; ++c) a[c] += per_image[3 * (long)n + c];
    for (int c = 0; c < 3; ++c) part[c][threadIdx.x] = a[c];
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w)
            for (int c = 0; c < 3; ++c) part[c][threadIdx.x] += part[c][threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x < 3) totals[threadIdx.x] = part[threadIdx.x][0];
}

// pred (N, P, S) int32, pred_count (N) or NULL (= P lanes each); gt (M, G, S) + gt_count (M): the resident label table, image n
// scored against row index[n] (or n with index NULL, which needs N <= M); y_samples (S) with y_stride 0 or (M, S) with
// y_stride S; run_time (N) fp32 or NULL (= 20).  per_image (N, 3) = accuracy, fp, fn; best_acc / best_pred (N, G) or NULL;
// totals (3) or NULL: the sums over the N images, from a second launch.  An index outside [0, M) bumps *bad_index, scores
// (0, 0, 1) and reads nothing out of range; counts outside [0, P] / [0, G] are clamped.
extern "C" int lf_lane_eval(const int32_t* pred, const int32_t* pred_count, const int32_t* gt, const int32_t* gt_count,
                            const int32_t* index, const double* y_samples, long y_stride, const float* run_time, int N, int M, int P,
                            int G, int S, double pixel_thresh, double pt_thresh, double* per_image, double* best_acc,
                            int32_t* best_pred, double* totals, int32_t* bad_index, void* stream) {
    LF_REQUIRE(pred && gt && gt_count && y_samples && per_image && bad_index, "lf_lane_eval: null pointer");
    LF_REQUIRE(N > 0 && M > 0, "lf_lane_eval: bad shape N=%d M=%d", N, M);
    LF_REQUIRE(P >= 1 && P <= LE_MAXL, "lf_lane_eval: P=%d not in 1..%d", P, LE_MAXL);
    LF_REQUIRE(G >= 1 && G <= LE_MAXL, "lf_lane_eval: G=%d not in 1..%d", G, LE_MAXL);
    LF_REQUIRE(S >= 1 && S <= LE_MAXS, "lf_lane_eval: S=%d not in 1..%d", S, LE_MAXS);
    LF_REQUIRE(y_stride == 0 || y_stride == S, "lf_lane_eval: y_stride %ld is neither 0 nor S=%d", y_stride, S);
    LF_REQUIRE(index || N <= M, "lf_lane_eval: %d images against %d labels need an index", N, M);
    hipLaunchKernelGGL(lane_eval_kernel, dim3(lf_cdiv(N, LE_WAVES)), dim3(LE_WAVES * LF_WAVE), 0, (hipStream_t)stream, pred,
                       pred_count, gt, gt_count, index, y_samples, y_stride, run_time, N, M, P, G, S, pixel_thresh, pt_thresh,
                       per_image, best_acc, best_pred, bad_index);
    if (totals)
        hipLaunchKernelGGL(lane_eval_totals_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)per_image, N, totals);
    LF_CHECK_LAUNCH("lane_eval");
    return 0;
}

// ---- BEV lane decoding (BEV/Dataloader/Load_Data_new.py:334-420 write_lsq_results, the tail of BEV/main.py:445-488) ------
// One wave per image, LE_WAVES images per workgroup, lane = sample index, as lane_eval_kernel: both read the same label table.
// Per predicted lane j the extent of gt lane j -- count, lowest and highest sample height among its x != -2 -- comes from a ballot
// and two fixed butterflies (no order of the heights assumed); past them every gate value is wave-uniform.  The statements are
// the reference's, in fp64:
//   y_d = (h - 80) / 639,  y' = (M11 y_d + M12) / (M21 y_d + M22)
//   ortho:     y = 1 - y',  x' = a y^2 + b y + c,  x = (Minv row 0 . [x', y', 1]) / (Minv row 2 . [x', y', 1])
//   no_ortho:  y = 1 - y_d, x  = a y^2 + b y + c
//   out = round-half-even(1279 x) where max(210, minimum) <= h <= maximum, -2 elsewhere
__device__ __forceinline__ double lf_wave_min(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ double lf_wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

enum { LDB_ALL_BRANCHES = 1, LDB_HORIZON = 2, LDB_NO_ORTHO = 4 };

template <typename T>
__global__ __launch_bounds__(LE_WAVES * LF_WAVE) void lane_decode_bev_kernel(
    const T* __restrict__ beta, const int32_t* __restrict__ gt, const int32_t* __restrict__ gt_count,
    const int32_t* __restrict__ index, const double* __restrict__ h_samples, long h_stride, const int32_t* __restrict__ line_id,
    const float* __restrict__ horizon, int R, double factor, double m11, double m12, double m21, double m22, double i00, double i01,
    double i02, double i20, double i21, double i22, int N, int M, int L, int G, int S, int order, int nclasses, int flags,
    int32_t* __restrict__ lanes, int32_t* __restrict__ bad_index) {
    const int lane = threadIdx.x & (LF_WAVE - 1);
    const int n = blockIdx.x * LE_WAVES + (threadIdx.x >> 6);
    if (n >= N) return;                                        // (whole waves leave: no barrier below)
    int32_t* out = lanes + (long)n * nclasses * S;
    const long row = index ? (long)index[n] : (long)n;
    if (row < 0 || row >= M) {                                 // counted for the host (IndexError), never dereferenced
        if (lane == 0) atomicAdd(bad_index, 1);
        for (int u = lane; u < nclasses * S; u += LF_WAVE) out[u] = -2;
        return;
    }
    const bool all_branches = flags & LDB_ALL_BRANCHES, horizon_on = flags & LDB_HORIZON, no_ortho = flags & LDB_NO_ORTHO;
    int Gn = gt_count[row];
    Gn = Gn < 0 ? 0 : (Gn > G ? G : Gn);
    const double* hs = h_samples + row * h_stride;
    const int32_t* gt_n = gt + row * (long)G * S;
    double h[LE_ITER], y[LE_ITER], yp[LE_ITER];
#pragma unroll
    for (int i = 0; i < LE_ITER; ++i) {
        const int s = i * LF_WAVE + lane;
        h[i] = s < S ? hs[s] : 0.;
        const double y_d = (h[i] - 80.) / 639.;
        yp[i] = (m11 * y_d + m12) / (m21 * y_d + m22);
        y[i] = no_ortho ? 1. - y_d : 1. - yp[i];
    }
    double horizon_min = 0.;
    if (all_branches && horizon_on) {                          // sum(horizon_est) * factor + 80: 0/1 values, exact in any order
        double acc = 0.;
        for (int r = lane; r < R; r += LF_WAVE) acc += (double)horizon[(long)n * R + r];
        horizon_min = lf_wave_sum(acc) * factor + 80.;
    }
    for (int j = 0; j < nclasses; ++j) {
        bool skip = j >= L;
        double lo = 250., hi = 710.;                           // the extent of a gt lane without a valid sample
        double a = 0., b = 0., c = 0.;
        if (!skip) {
            int cnt = 0;
            double mn = INFINITY, mx = -INFINITY;
#pragma unroll
            for (int i = 0; i < LE_ITER; ++i) {
                const int s = i * LF_WAVE + lane;
                const bool ok = s < S && j < Gn && gt_n[(long)j * S + s] != -2;
                cnt += le_wave_count(ok);
                mn = ok ? fmin(mn, h[i]) : mn;
                mx = ok ? fmax(mx, h[i]) : mx;
            }
            if (cnt > 0) {
                lo = lf_wave_min(mn);
                hi = lf_wave_max(mx);
            }
            if (all_branches) {
                skip = (j == 2 && line_id[4 * (long)n + 0] == 0) || (j == 3 && line_id[4 * (long)n + 3] == 0);
                if (horizon_on) lo = horizon_min;
            } else {
                skip = cnt == 0;
            }
            const T* bj = beta + ((long)n * L + j) * (order + 1);       // highest power first; missing leading coefficients are 0
            c = (double)bj[order];
            if (order >= 1) b = (double)bj[order - 1];
            if (order >= 2) a = (double)bj[0];
        }
        lo = lo > 210. ? lo : 210.;
#pragma unroll
        for (int i = 0; i < LE_ITER; ++i) {
            const int s = i * LF_WAVE + lane;
            if (s >= S) continue;
            int32_t v = -2;
            if (!skip && h[i] >= lo && h[i] <= hi) {
                double x = a * (y[i] * y[i]) + b * y[i] + c;
                if (!no_ortho) x = (i00 * x + i01 * yp[i] + i02) / (i20 * x + i21 * yp[i] + i22);
                const double r = rint(x * 1279.);              // np.round: half to even
                // int32 store: saturated, NaN -> INT32_MIN (the reference's int64 there is negative or huge; LaneEval maps every
                // negative to -100 and no label lies within a threshold of either bound)
                v = r != r ? INT32_MIN : (r <= -2147483648. ? INT32_MIN : (r >= 2147483647. ? INT32_MAX : (int32_t)r));
            }
            out[(long)j * S + s] = v;
        }
    }
}

// beta (N, L, order+1) contiguous, fp32 or fp64 by beta_dtype (LF_F32 | LF_F64), order 0..2.  gt / gt_count / index / h_samples +
// h_stride: the label table exactly as lf_lane_eval takes it.  line_id (N, 4) int32 (needed with all_branches_ready), horizon (N, R)
// fp32 0/1 values with factor = 640 / resize (needed with all_branches_ready and horizon_on).  lanes (N, nclasses, S) int32 out.
extern "C" int lf_lane_decode_bev(const void* beta, int beta_dtype, const int32_t* gt, const int32_t* gt_count, const int32_t* index,
                                  const double* h_samples, long h_stride, const int32_t* line_id, const float* horizon, int R,
                                  double factor, const double* m_host, const double* minv_host, int N, int M, int L, int G, int S,
                                  int order, int nclasses, int all_branches_ready, int horizon_on, int no_ortho, int32_t* lanes,
                                  int32_t* bad_index, void* stream) {
    LF_REQUIRE(beta && gt && gt_count && h_samples && m_host && minv_host && lanes && bad_index, "lf_lane_decode_bev: null pointer");
    LF_REQUIRE(beta_dtype == LF_F32 || beta_dtype == LF_F64, "lf_lane_decode_bev: beta_dtype %d is neither LF_F32 nor LF_F64", beta_dtype);
    LF_REQUIRE(N > 0 && M > 0, "lf_lane_decode_bev: bad shape N=%d M=%d", N, M);
    LF_REQUIRE(order >= 0 && order <= 2, "lf_lane_decode_bev: order=%d not in 0..2", order);
    LF_REQUIRE(L >= 1 && L <= LE_MAXL, "lf_lane_decode_bev: L=%d not in 1..%d", L, LE_MAXL);
    LF_REQUIRE(G >= 1 && G <= LE_MAXL, "lf_lane_decode_bev: G=%d not in 1..%d", G, LE_MAXL);
    LF_REQUIRE(S >= 1 && S <= LE_MAXS, "lf_lane_decode_bev: S=%d not in 1..%d", S, LE_MAXS);
    LF_REQUIRE(nclasses >= L && nclasses <= 1024, "lf_lane_decode_bev: nclasses=%d not in L=%d..1024", nclasses, L);
    LF_REQUIRE(h_stride == 0 || h_stride == S, "lf_lane_decode_bev: h_stride %ld is neither 0 nor S=%d", h_stride, S);
    LF_REQUIRE(index || N <= M, "lf_lane_decode_bev: %d images against %d labels need an index", N, M);
    LF_REQUIRE(!all_branches_ready || line_id, "lf_lane_decode_bev: all_branches_ready needs line_id");
    LF_REQUIRE(!(all_branches_ready && horizon_on) || (horizon && R >= 0), "lf_lane_decode_bev: horizon_on needs horizon (N, R)");
    const double *m = m_host, *w = minv_host;
    const int flags = (all_branches_ready ? LDB_ALL_BRANCHES : 0) | (horizon_on ? LDB_HORIZON : 0) | (no_ortho ? LDB_NO_ORTHO : 0);
    const dim3 grid(lf_cdiv(N, LE_WAVES)), block(LE_WAVES * LF_WAVE);
    if (beta_dtype == LF_F32)
        hipLaunchKernelGGL(lane_decode_bev_kernel<float>, grid, block, 0, (hipStream_t)stream, (const float*)beta, gt, gt_count, index,
                           h_samples, h_stride, line_id, horizon, R, factor, m[4], m[5], m[7], m[8], w[0], w[1], w[2], w[6], w[7], w[8],
                           N, M, L, G, S, order, nclasses, flags, lanes, bad_index);
    else
        hipLaunchKernelGGL(lane_decode_bev_kernel<double>, grid, block, 0, (hipStream_t)stream, (const double*)beta, gt, gt_count, index,
                           h_samples, h_stride, line_id, horizon, R, factor, m[4], m[5], m[7], m[8], w[0], w[1], w[2], w[6], w[7], w[8],
                           N, M, L, G, S, order, nclasses, flags, lanes, bad_index);
    LF_CHECK_LAUNCH("lane_decode_bev");
    return 0;
}
