// Whole-step criterion: every lane loss, the two --clas head losses, their gradients, the validation accuracies and the
// weighted total of one training / validation step in ONE launch (lf_step_loss).
//   Backprojection_Loss/main.py:296-326, :459-501 and Birds_Eye_View_Loss/main.py:223-253, :395-431 are the statements it replaces;
//   the back-projection lane body and the Area_Loss integrand with its gradient live in lf_loss_dev.h, which backproj_kernel and
//   area_loss_kernel (lf_losses.hip, the per-lane modules) call too; the area mean and the MSE sums are each kernel's own; the head
//   losses are nn.BCEWithLogitsLoss / nn.CrossEntropyLoss in fp64.
// Grid: one 256-thread workgroup per task -- K lanes, then (with the heads) line and horizon.  Each workgroup reduces its task in a
// fixed order, writes its gradient slice already multiplied by the task's static weight, publishes its scalars in a workspace slot
// and draws a ticket; whoever draws the last ticket adds the slots up in the loop's order and writes the totals.  Nobody waits on
// anybody, no value depends on which workgroup came last, and the ticket goes back to zero for the next call.
#include "lf_common.h"
#include "lf_loss_dev.h"

namespace {

constexpr int ST_MAXK = 4;
constexpr int ST_THREADS = LF_LOSS_THREADS;
// workspace: 9 fp64 slots (4 lane losses, line loss, horizon loss, line hits, horizon hits, bad labels) + the ticket
constexpr int WS_LINE = 4, WS_HOR = 5, WS_LINE_HITS = 6, WS_HOR_HITS = 7, WS_BAD = 8, WS_TICKET = 9, WS_WORDS = 16;

struct StepArgs {
    const void* beta[ST_MAXK];
    long bstride;                 // elements between the images of one lane
    const void* target;           // backproject: x_gt (N, Kt, S) fp64; area / mse: gt (N, Kt, D) in beta's type
    const double* valid;          // backproject: (N, Kt, S) fp64
    long tstride;                 // elements between the images of target / valid
    const double* Y;
    const double* yp;
    double m00, m01, m02, m20, m21, m22;
    const float* line;
    const void* line_t;
    const float* hor;
    const float* hor_t;
    int tree, kind, K, N, order, wf, S, R, heads, nclasses;
    double w_lane, w_fit, w_class;
    double* out;
    double* xcal;
    void* grad;
    double* meters;
    double* ws;
};

// backprojection_loss of one lane (BP/Loss_crit.py:202-218): lane k of the (N, K, .) tensors, its gradient times the lane's weight
template <typename T>
__device__ double lane_backproject(const StepArgs& a, int k, double* sh) {
    const LfBackprojConsts c = {a.Y, a.yp, a.m00, a.m01, a.m02, a.m20, a.m21, a.m22};
    return lf_backproject_lane<T>((const T*)a.beta[k], a.bstride, (const double*)a.target + (long)k * a.S, a.valid + (long)k * a.S,
                                  a.tstride, c, a.N, a.S, a.order, a.K, k, a.w_lane, a.xcal, (T*)a.grad, sh);
}

// Area_Loss (BEV/Loss_crit.py:98-134) or MSE_Loss of one lane.  An image whose ground truth has a zero coefficient is dropped
// from the area mean (:131-133); for lanes 2 and 3 of the BEV tree its coefficients are multiplied by 0 first (BEV/main.py:226-234),
// which is what the mse policy sees of an absent lane.
template <typename T>
__device__ double lane_coeff(const StepArgs& a, int k, double* sh) {
    const int D = a.order + 1, N = a.N, K = a.K;
    const T* beta = (const T*)a.beta[k];
    const T* gt = (const T*)a.target + (long)k * D;
    T* grad = (T*)a.grad;
    const bool masked = a.tree == LF_TREE_BEV && k >= 2;
    const bool area = a.kind == LF_LANE_AREA;
    double Lsum = 0.0, cnt = 0.0;
    for (int i = threadIdx.x; i < N; i += ST_THREADS) {
        double d[4] = {0, 0, 0, 0}, gj[4] = {0, 0, 0, 0};
        bool keep = true;
        for (int j = 0; j < D; ++j) {
            gj[j] = (double)gt[(long)i * a.tstride + j];
            keep = keep && (gj[j] != 0.0);
        }
        for (int j = 0; j < D; ++j) d[j] = ((masked && !keep) ? 0.0 : (double)beta[(long)i * a.bstride + j]) - gj[j];
        if (area) {
            if (keep) { Lsum += lf_area_value(d[0], d[1], d[2], a.order, a.wf); cnt += 1.0; }
        } else {
            for (int j = 0; j < D; ++j) Lsum = fma(d[j], d[j], Lsum);
        }
    }
    const double tl = block_sum(Lsum, sh);
    const double tc = area ? block_sum(cnt, sh) : (double)N * D;
    const double inv = tc > 0 ? 1.0 / tc : 0.0;
    for (int i = threadIdx.x; i < N; i += ST_THREADS) {
        double d[4] = {0, 0, 0, 0}, gj[4] = {0, 0, 0, 0}, g[4] = {0, 0, 0, 0};
        bool keep = true;
        for (int j = 0; j < D; ++j) {
            gj[j] = (double)gt[(long)i * a.tstride + j];
            keep = keep && (gj[j] != 0.0);
        }
        for (int j = 0; j < D; ++j) d[j] = ((masked && !keep) ? 0.0 : (double)beta[(long)i * a.bstride + j]) - gj[j];
        bool live;
        if (area) {
            lf_area_grad(d[0], d[1], d[2], a.order, a.wf, g);
            live = keep;
        } else {
            for (int j = 0; j < D; ++j) g[j] = 2.0 * d[j];
            live = keep || !masked;
        }
        for (int j = 0; j < D; ++j) grad[((long)i * K + k) * D + j] = (T)(live ? g[j] * inv * a.w_lane : 0.0);
    }
    return tl * inv;
}

// nn.BCEWithLogitsLoss (mean) of n fp32 logits in fp64, max(x,0) - x*y + log1p(exp(-|x|)); prediction x > 0
__device__ void bce_task(const float* __restrict__ x, const float* __restrict__ y, long n, double w, float* __restrict__ gx,
                         double* sh, double* loss, double* hits) {
    double s = 0.0, h = 0.0;
    const double inv = 1.0 / (double)n;
    for (long i = threadIdx.x; i < n; i += ST_THREADS) {
        const double xi = (double)x[i], yi = (double)y[i];
        const double e = exp(-fabs(xi));
        s += fmax(xi, 0.0) - xi * yi + log1p(e);
        const double sig = xi >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e);
        gx[i] = (float)((sig - yi) * inv * w);
        h += ((xi > 0.0 ? 1.0 : 0.0) == yi) ? 1.0 : 0.0;
    }
    const double ts = block_sum(s, sh), th = block_sum(h, sh);
    *loss = ts * inv;
    *hits = th;
}

// nn.CrossEntropyLoss (unweighted mean) of (N, C, J) fp32 logits against (N, J) int64 labels in fp64; a label outside [0, C) carries
// weight 0 and is counted (the lf_ce2d_fwd convention); prediction = first arg-max over the class axis
constexpr int CE_C = 3;
__device__ void ce_task(const float* __restrict__ z, const int64_t* __restrict__ tgt, int N, int J, double w, float* __restrict__ gz,
                        double* sh, double* loss, double* hits, double* bad) {
    double s = 0.0, h = 0.0, ok = 0.0, nb = 0.0;
    const long n = (long)N * J;
    for (long i = threadIdx.x; i < n; i += ST_THREADS) {
        const int64_t t = tgt[i];
        const bool okt = t >= 0 && t < CE_C;
        ok += okt ? 1.0 : 0.0;
        nb += okt ? 0.0 : 1.0;
    }
    const double tok = block_sum(ok, sh), tbad = block_sum(nb, sh);
    const double inv = tok > 0.0 ? 1.0 / tok : 0.0;
    for (long i = threadIdx.x; i < n; i += ST_THREADS) {
        const long im = i / J, j = i % J;
        const float* zp = z + im * CE_C * J + j;
        float* gp = gz + im * CE_C * J + j;
        double v[CE_C], mx = -INFINITY;
        int am = 0;
        for (int c = 0; c < CE_C; ++c) {
            v[c] = (double)zp[(long)c * J];
            if (v[c] > mx) { mx = v[c]; am = c; }
        }
        double se = 0.0;
        for (int c = 0; c < CE_C; ++c) { v[c] = exp(v[c] - mx); se += v[c]; }
        const int64_t t = tgt[i];
        const bool okt = t >= 0 && t < CE_C;
        double zt = 0.0;
        for (int c = 0; c < CE_C; ++c) zt = (c == (int)t) ? (double)zp[(long)c * J] : zt;
        if (okt) s += mx + log(se) - zt;
        h += ((int64_t)am == t) ? 1.0 : 0.0;
        const double sc = okt ? inv * w : 0.0;
        for (int c = 0; c < CE_C; ++c) gp[(long)c * J] = (float)(sc * (v[c] / se - (c == (int)t ? 1.0 : 0.0)));
    }
    const double ts = block_sum(s, sh), th = block_sum(h, sh);
    *loss = ts * inv;
    *hits = th;
    *bad = tbad;
}

__device__ __forceinline__ void publish(double* p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ double collect(const double* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

template <typename T>
__global__ __launch_bounds__(ST_THREADS) void step_loss_kernel(const StepArgs a) {
    __shared__ double sh[4];
    const int task = blockIdx.x, K = a.K, N = a.N;
    double* ws = a.ws;
    if (task < K) {
        const double l = a.kind == LF_LANE_BACKPROJECT ? lane_backproject<T>(a, task, sh) : lane_coeff<T>(a, task, sh);
        if (threadIdx.x == 0) publish(ws + task, l);
    } else {
        // the two head gradients follow the (N, K, D) coefficient gradient in the flat buffer: line, then horizon
        float* gline = (float*)((char*)a.grad + (size_t)N * K * (a.order + 1) * sizeof(T));
        const long nline = a.tree == LF_TREE_BEV ? (long)N * CE_C * 4 : (long)N * 4;
        double l, h, bad = 0.0;
        if (task == K) {
            if (a.tree == LF_TREE_BEV)
                ce_task(a.line, (const int64_t*)a.line_t, N, 4, a.w_class, gline, sh, &l, &h, &bad);
            else
                bce_task(a.line, (const float*)a.line_t, (long)N * 4, a.w_class, gline, sh, &l, &h);
            if (threadIdx.x == 0) { publish(ws + WS_LINE, l); publish(ws + WS_LINE_HITS, h); publish(ws + WS_BAD, bad); }
        } else {
            bce_task(a.hor, a.hor_t, (long)N * a.R, a.w_class, gline + nline, sh, &l, &h);
            if (threadIdx.x == 0) { publish(ws + WS_HOR, l); publish(ws + WS_HOR_HITS, h); }
        }
    }
    if (threadIdx.x != 0) return;
    // the slots above are write-through stores: once they have left this wave the ticket may be drawn; the last arriver reads every
    // slot past its L1.  No workgroup waits for another.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    unsigned* ticket = (unsigned*)(ws + WS_TICKET);
    const unsigned drawn = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (drawn != gridDim.x - 1) return;
    __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    double l[ST_MAXK] = {0, 0, 0, 0};
    for (int k = 0; k < K; ++k) l[k] = collect(ws + k);
    double fit;
    if (K == 4)          // BP/main.py:296-305: (l0 + l2) + (l1 + l3); BEV/main.py:223,237: (l0 + l1) + (l2 + l3)
        fit = a.tree == LF_TREE_BEV ? (l[0] + l[1]) + (l[2] + l[3]) : (l[0] + l[2]) + (l[1] + l[3]);
    else
        fit = ((l[0] + l[1]) + l[2]) + l[3];
    if (a.tree == LF_TREE_BP) fit = fit / (double)a.nclasses;
    double line = 0.0, hor = 0.0, acc_line = 0.0, acc_hor = 0.0, bad = 0.0, total = fit;
    if (a.heads) {
        line = collect(ws + WS_LINE);
        hor = collect(ws + WS_HOR);
        bad = collect(ws + WS_BAD);
        acc_line = collect(ws + WS_LINE_HITS) / ((double)a.nclasses * N);
        acc_hor = collect(ws + WS_HOR_HITS) / ((double)a.R * N);
        total = fit * a.w_fit + (line + hor) * a.w_class;
    }
    double* out = a.out;
    out[0] = total; out[1] = fit; out[2] = line; out[3] = hor; out[4] = acc_line; out[5] = acc_hor; out[6] = bad;
    out[7] = a.heads ? collect(ws + WS_LINE_HITS) : 0.0;
    out[8] = a.heads ? collect(ws + WS_HOR_HITS) : 0.0;
    out[9] = 0.0;
    if (a.meters) {      // AverageMeter sums: update(value, n) for the losses, update(value) for the accuracies
        double* m = a.meters;
        m[0] += total * N; m[1] += N; m[2] += fit * N; m[3] += N;
        m[4] += acc_line; m[5] += 1.0; m[6] += acc_hor; m[7] += 1.0;
    }
}

// the flat gradient buffer times the upstream scalar: n_beta elements of type T, then n_head fp32
template <typename T>
__global__ __launch_bounds__(ST_THREADS) void step_scale_kernel(const void* __restrict__ g, long n_beta, long n_head,
                                                               const double* __restrict__ up, void* __restrict__ out) {
    const double u = up[0];
    const T* gb = (const T*)g;
    T* ob = (T*)out;
    const float* gh = (const float*)(gb + n_beta);
    float* oh = (float*)(ob + n_beta);
    for (long i = (long)blockIdx.x * ST_THREADS + threadIdx.x; i < n_beta + n_head; i += (long)gridDim.x * ST_THREADS) {
        if (i < n_beta) ob[i] = (T)((double)gb[i] * u);
        else oh[i - n_beta] = (float)((double)gh[i - n_beta] * u);
    }
}

}  // namespace

extern "C" size_t lf_step_loss_workspace_bytes(void) { return WS_WORDS * sizeof(double); }

extern "C" int lf_step_loss(int tree, int kind, int K, int N, int order, int weight_funct, int nclasses,
                            const void* const* beta_lanes, long beta_stride, int beta_dtype,
                            const void* target, const double* valid, long target_stride, int S,
                            const double* Y, const double* y_prime, const double* minv_host,
                            const float* line_logits, const void* line_target, const float* horizon_logits,
                            const float* horizon_target, int R, double weight_fit, double weight_class,
                            double* out, double* x_cal_valid, void* grad, double* meters, void* workspace, void* stream) {
    LF_REQUIRE(tree == LF_TREE_BP || tree == LF_TREE_BEV, "lf_step_loss: bad tree %d", tree);
    LF_REQUIRE(kind >= LF_LANE_BACKPROJECT && kind <= LF_LANE_MSE, "lf_step_loss: bad lane kind %d", kind);
    LF_REQUIRE(K >= 1 && K <= ST_MAXK && N > 0 && nclasses > 0, "lf_step_loss: K=%d N=%d nclasses=%d", K, N, nclasses);
    LF_REQUIRE(beta_dtype == LF_F32 || beta_dtype == LF_F64, "lf_step_loss: bad dtype %d", beta_dtype);
    LF_REQUIRE(beta_lanes && target && out && grad && workspace, "lf_step_loss: null pointer");
    for (int k = 0; k < K; ++k) LF_REQUIRE(beta_lanes[k], "lf_step_loss: lane %d has no coefficients", k);
    LF_REQUIRE(beta_stride >= order + 1, "lf_step_loss: beta_stride %ld below order + 1", beta_stride);
    if (kind == LF_LANE_BACKPROJECT) {
        LF_REQUIRE(order >= 0 && order <= 3 && S > 0, "lf_step_loss: backproject wants order 0..3 and S > 0");
        LF_REQUIRE(valid && Y && y_prime && minv_host && x_cal_valid, "lf_step_loss: backproject: null pointer");
        LF_REQUIRE(target_stride >= (long)K * S, "lf_step_loss: target_stride %ld below K * S", target_stride);
    } else {
        if (kind == LF_LANE_AREA) {
            LF_REQUIRE(order == 1 || order == 2, "lf_step_loss: area order %d not implemented (reference: Loss_crit.py:125-128)", order);
            LF_REQUIRE(weight_funct >= 0 && weight_funct <= 2, "lf_step_loss: bad weight function %d", weight_funct);
        } else {
            LF_REQUIRE(order >= 0 && order <= 3, "lf_step_loss: mse order %d not in 0..3", order);
        }
        LF_REQUIRE(target_stride >= (long)K * (order + 1), "lf_step_loss: target_stride %ld below K * (order + 1)", target_stride);
    }
    const int heads = line_logits || line_target || horizon_logits || horizon_target;
    if (heads)
        LF_REQUIRE(line_logits && line_target && horizon_logits && horizon_target && R > 0,
                   "lf_step_loss: the two heads come together (logits and targets of both)");
    StepArgs a;
    memset(&a, 0, sizeof(a));
    for (int k = 0; k < K; ++k) a.beta[k] = beta_lanes[k];
    a.bstride = beta_stride;
    a.target = target; a.valid = valid; a.tstride = target_stride;
    a.Y = Y; a.yp = y_prime;
    if (minv_host) {
        const double* m = minv_host;
        a.m00 = m[0]; a.m01 = m[1]; a.m02 = m[2]; a.m20 = m[6]; a.m21 = m[7]; a.m22 = m[8];
    }
    a.line = line_logits; a.line_t = line_target; a.hor = horizon_logits; a.hor_t = horizon_target;
    a.tree = tree; a.kind = kind; a.K = K; a.N = N; a.order = order; a.wf = weight_funct; a.S = S; a.R = R; a.heads = heads;
    a.nclasses = nclasses;
    // static weights of the total: fit * weight_fit + (line + horizon) * weight_class with the heads, fit alone without
    a.w_fit = heads ? weight_fit : 1.0;
    a.w_class = weight_class;
    a.w_lane = a.w_fit / (tree == LF_TREE_BP ? (double)nclasses : 1.0);
    a.out = out; a.xcal = x_cal_valid; a.grad = grad; a.meters = meters; a.ws = (double*)workspace;
    const dim3 grid(K + (heads ? 2 : 0));
    if (beta_dtype == LF_F64)
        hipLaunchKernelGGL(step_loss_kernel<double>, grid, dim3(ST_THREADS), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(step_loss_kernel<float>, grid, dim3(ST_THREADS), 0, (hipStream_t)stream, a);
    LF_CHECK_LAUNCH("step_loss");
    return 0;
}

extern "C" int lf_step_loss_bwd(const void* grad, int beta_dtype, long n_beta, long n_head, const double* upstream,
                                void* grad_out, void* stream) {
    LF_REQUIRE(grad && upstream && grad_out && n_beta > 0 && n_head >= 0, "lf_step_loss_bwd: bad arguments");
    LF_REQUIRE(beta_dtype == LF_F32 || beta_dtype == LF_F64, "lf_step_loss_bwd: bad dtype %d", beta_dtype);
    int blocks = lf_cdiv(n_beta + n_head, ST_THREADS);
    if (blocks > 256) blocks = 256;
    if (beta_dtype == LF_F64)
        hipLaunchKernelGGL(step_scale_kernel<double>, dim3(blocks), dim3(ST_THREADS), 0, (hipStream_t)stream, grad, n_beta, n_head,
                           upstream, grad_out);
    else
        hipLaunchKernelGGL(step_scale_kernel<float>, dim3(blocks), dim3(ST_THREADS), 0, (hipStream_t)stream, grad, n_beta, n_head,
                           upstream, grad_out);
    LF_CHECK_LAUNCH("step_loss_bwd");
    return 0;
}
