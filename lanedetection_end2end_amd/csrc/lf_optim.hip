// Fused multi-tensor Adam step (the step right after the hot path; the reference builds
// torch.optim.Adam(lr=1e-4, weight_decay=wd) in BEV/Networks/utils.py:411-420 and calls optimizer.step() at
// BEV/main.py:266).  ONE launch updates all 226 parameter tensors: a device table maps each workgroup to a
// (tensor, 4096-element chunk); arithmetic follows torch.optim.Adam (L2 weight decay folded into the gradient,
// bias-corrected moments, eps added after the square root).  The step count -- hence the bias correction -- is PER TENSOR, as in
// torch.optim.Adam: the reference's pretrained schedule switches heads under one optimizer (BEV/main.py get_flags), so
// decoder.output_conv gets its first gradient when the other tensors are at step k.  The counts live in the device table,
// double-buffered: a launch reads step[parity] of its tensor and the tensor's first workgroup writes step[parity ^ 1].
//
// Gradient-norm clipping (BP/main.py:334-335, nn.utils.clip_grad_norm between loss.backward() and optimizer.step()) rides on the
// same tables: grad_sumsq_kernel reads the gradients once into one fp64 partial per workgroup, grad_norm_finish_kernel adds the
// partials in a fixed order and leaves {total_norm, coef} in device memory, and the <.., true> instances of opt_kernel pick coef up
// from there -- the gradients get no second pass and the host never waits.  grad_scale_inplace_kernel is the drop-in form's
// rewrite of the gradients.
#include "lf_common.h"

struct LfAdamTensor { float* p; const float* g; float* m; float* v; long numel; long step[2]; };

namespace {
constexpr int ADAM_CHUNK = 4096;
typedef float f32x4 __attribute__((ext_vector_type(4)));

enum { OPT_ADAM = 0, OPT_SGD = 1, OPT_RMSPROP = 2 };
struct OptScalars { float a, b, c, d, e, f; };      // per-optimizer constants (see update())

// One element.  OPT_ADAM: a = step_size (lr / bias correction 1), b = beta1, c = beta2, d = eps, e = weight decay, f = sqrt(bias
// correction 2); torch.optim.Adam's arithmetic (lerp for the first moment, eps added after the square root).  OPT_SGD: a = lr,
// b = momentum, e = weight decay (dampening 0, no Nesterov; a zero buffer reproduces torch's first step).  OPT_RMSPROP: a = lr,
// b = momentum, c = alpha, d = eps, e = weight decay (not centered).  Record fields: m = exp_avg / momentum buffer, v =
// exp_avg_sq / square average.
template <int OP>
__device__ __forceinline__ void update(float& p, float g, float& m, float& v, const OptScalars& k) {
    if (k.e != 0.f) g = fmaf(k.e, p, g);
    if constexpr (OP == OPT_ADAM) {
        m = fmaf(1.f - k.b, g - m, m);
        v = fmaf(k.c, v, (1.f - k.c) * g * g);
        p = p - k.a * (m / (sqrtf(v) / k.f + k.d));
    } else if constexpr (OP == OPT_SGD) {
        m = fmaf(k.b, m, g);
        p = p - k.a * m;
    } else {
        v = fmaf(k.c, v, (1.f - k.c) * g * g);
        m = fmaf(k.b, m, g / (sqrtf(v) + k.d));
        p = p - k.a * m;
    }
}

// One workgroup = one (tensor, 4096-element chunk).  A full chunk is 16 elements per thread as four float4 groups with ALL
// their loads issued before the first update (round 4: the first version walked the chunk in 16 dependent scalar rounds --
// 188 us per step where the 58 MB it moves take 10); the gradient is a view into the flat gradient buffer at an arbitrary
// element offset, so its vector form is taken only when the pointer happens to be 16-byte aligned.
//
// CLIP (compiled in, never a run-time branch of the unclipped instances): the effective gradient is fl32(fl32(g * grad_scale) * coef)
// with coef read once per workgroup from device memory -- two separately rounded products, the value torch leaves in p.grad after
// clip_grad_norm_ -- so the step equals grad_scale_inplace_kernel followed by the unclipped step bit for bit.
__device__ __forceinline__ float mul_rn(float a, float b) {      // a product no later add or fma may absorb (__fmul_rn's contract)
#pragma clang fp contract(off)
    return a * b;
}

template <int OP, bool CLIP>
__global__ __launch_bounds__(256) void opt_kernel(const LfAdamTensor* __restrict__ tensors, const int2* __restrict__ work,
                                                 OptScalars k, float lr, int parity, float grad_scale,
                                                 const float* __restrict__ coef_dev) {
    const int2 wk = work[blockIdx.x];
    const LfAdamTensor t = tensors[wk.x];
    const long base = (long)wk.y * ADAM_CHUNK;
    float coef = 1.f;
    if constexpr (CLIP) coef = *coef_dev;
    auto eff = [&](float g) {
        if constexpr (CLIP) return mul_rn(mul_rn(g, grad_scale), coef);
        else return g * grad_scale;
    };
    if constexpr (OP == OPT_ADAM) {
        const long step = t.step[parity] + 1;               // 1-based count of THIS tensor's updates, including this one
        if (wk.y == 0 && threadIdx.x == 0) const_cast<LfAdamTensor*>(tensors)[wk.x].step[parity ^ 1] = step;
        k.a = lr / (float)(1.0 - pow((double)k.b, (double)step));
        k.f = (float)sqrt(1.0 - pow((double)k.c, (double)step));
    }
    const bool gvec = ((reinterpret_cast<unsigned long long>(t.g) & 15ull) == 0ull);
    if (base + ADAM_CHUNK <= t.numel) {
        float P[4][4], G[4][4], M[4][4], V[4][4];
        auto ld = [](float (&d)[4], const float* s) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(s);
            d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        };
        auto st = [](float* d, const float (&s)[4]) { *reinterpret_cast<f32x4*>(d) = f32x4{s[0], s[1], s[2], s[3]}; };
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long e = base + j * 1024 + threadIdx.x * 4;
            ld(P[j], t.p + e);
            ld(M[j], t.m + e);
            if constexpr (OP != OPT_SGD) ld(V[j], t.v + e);
            else { V[j][0] = V[j][1] = V[j][2] = V[j][3] = 0.f; }
            if (gvec) ld(G[j], t.g + e);
            else { G[j][0] = t.g[e]; G[j][1] = t.g[e + 1]; G[j][2] = t.g[e + 2]; G[j][3] = t.g[e + 3]; }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long e = base + j * 1024 + threadIdx.x * 4;
#pragma unroll
            for (int q = 0; q < 4; ++q) update<OP>(P[j][q], eff(G[j][q]), M[j][q], V[j][q], k);
            st(t.p + e, P[j]);
            st(t.m + e, M[j]);
            if constexpr (OP != OPT_SGD) st(t.v + e, V[j]);
        }
        return;
    }
    for (int i = threadIdx.x; i < ADAM_CHUNK; i += 256) {     // a tensor's last (or only) chunk
        const long e = base + i;
        if (e >= t.numel) break;
        float p = t.p[e], m = t.m[e], v = OP != OPT_SGD ? t.v[e] : 0.f;
        update<OP>(p, eff(t.g[e]), m, v, k);
        t.p[e] = p;
        t.m[e] = m;
        if constexpr (OP != OPT_SGD) t.v[e] = v;
    }
}

// Workgroup sum in a fixed order: butterfly within each wave, then the four wave sums added 0, 1, 2, 3 by every thread.
__device__ __forceinline__ double block_sum(double v) {
    __shared__ double wave[4];
    v = lf_wave_sum(v);
    if ((threadIdx.x & 63) == 0) wave[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((wave[0] + wave[1]) + wave[2]) + wave[3];
}

// Sum of squares of one (tensor, chunk) per workgroup, same tables and the same two gradient load forms as opt_kernel.  Every
// element is widened to fp64 BEFORE it is squared (g * g overflows fp32 beyond 1.8e19) and the sum is fp64 from the first product
// on; one partial per workgroup into its own slot, no atomics.
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const LfAdamTensor* __restrict__ tensors, const int2* __restrict__ work,
                                                        double* __restrict__ partials) {
    const int2 wk = work[blockIdx.x];
    const LfAdamTensor t = tensors[wk.x];
    const long base = (long)wk.y * ADAM_CHUNK;
    double acc = 0.0;
    if (base + ADAM_CHUNK <= t.numel) {
        const bool gvec = ((reinterpret_cast<unsigned long long>(t.g) & 15ull) == 0ull);
        float G[4][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long e = base + j * 1024 + threadIdx.x * 4;
            if (gvec) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(t.g + e);
                G[j][0] = v.x; G[j][1] = v.y; G[j][2] = v.z; G[j][3] = v.w;
            } else { G[j][0] = t.g[e]; G[j][1] = t.g[e + 1]; G[j][2] = t.g[e + 2]; G[j][3] = t.g[e + 3]; }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) { const double g = (double)G[j][q]; acc = fma(g, g, acc); }
    } else {
        for (int i = threadIdx.x; i < ADAM_CHUNK; i += 256) {     // a tensor's last (or only) chunk
            const long e = base + i;
            if (e >= t.numel) break;
            const double g = (double)t.g[e];
            acc = fma(g, g, acc);
        }
    }
    acc = block_sum(acc);
    if (threadIdx.x == 0) partials[blockIdx.x] = acc;
}

// One workgroup: the partials of ALL param groups added in one fixed order (thread i takes i, i + 256, ... in turn, then
// block_sum), total_norm = fl32(grad_scale * sqrt(sum)) and torch's clip coefficient in fp32, clamp(max_norm / (total_norm + 1e-6),
// max = 1): written so that a NaN stays a NaN (fminf(1, NaN) would make it 1) and an Inf norm gives 0.
__global__ __launch_bounds__(256) void grad_norm_finish_kernel(const double* __restrict__ partials, int n, float grad_scale,
                                                              float max_norm, float* __restrict__ out2) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) acc += partials[i];
    acc = block_sum(acc);
    if (threadIdx.x == 0) {
        const float total = (float)((double)grad_scale * sqrt(acc));
        const float c = (float)((double)max_norm / (double)(total + 1e-6f));      // the correctly rounded fp32 quotient
        out2[0] = total;
        out2[1] = c > 1.f ? 1.f : c;
    }
}

// The drop-in form's rewrite: g = fl32(fl32(g * grad_scale) * coef) on the elements inside each tensor's numel, nothing else (the
// gaps and the reducer tail of a flat gradient buffer are not written).
__global__ __launch_bounds__(256) void grad_scale_inplace_kernel(const LfAdamTensor* __restrict__ tensors, const int2* __restrict__ work,
                                                                float grad_scale, const float* __restrict__ coef_dev) {
    const int2 wk = work[blockIdx.x];
    const LfAdamTensor t = tensors[wk.x];
    const long base = (long)wk.y * ADAM_CHUNK;
    const float coef = *coef_dev;
    float* g = const_cast<float*>(t.g);
    if (base + ADAM_CHUNK <= t.numel && (reinterpret_cast<unsigned long long>(g) & 15ull) == 0ull) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long e = base + j * 1024 + threadIdx.x * 4;
            f32x4 v = *reinterpret_cast<const f32x4*>(g + e);
            v.x = mul_rn(mul_rn(v.x, grad_scale), coef);
            v.y = mul_rn(mul_rn(v.y, grad_scale), coef);
            v.z = mul_rn(mul_rn(v.z, grad_scale), coef);
            v.w = mul_rn(mul_rn(v.w, grad_scale), coef);
            *reinterpret_cast<f32x4*>(g + e) = v;
        }
        return;
    }
    for (int i = threadIdx.x; i < ADAM_CHUNK; i += 256) {
        const long e = base + i;
        if (e >= t.numel) break;
        g[e] = mul_rn(mul_rn(g[e], grad_scale), coef);
    }
}

template <int OP, bool CLIP>
int launch_opt(const void* tensors_dev, const void* work_dev, int nblocks, const OptScalars& k, float lr, int parity, float grad_scale,
               const float* coef_dev, void* stream) {
    hipLaunchKernelGGL((opt_kernel<OP, CLIP>), dim3(nblocks), dim3(256), 0, (hipStream_t)stream, (const LfAdamTensor*)tensors_dev,
                       (const int2*)work_dev, k, lr, parity, grad_scale, coef_dev);
    return 0;
}
}  // namespace

extern "C" {

int lf_adam_chunk(void) { return ADAM_CHUNK; }

// The other two optimizers the reference's define_optim builds (BEV/Networks/utils.py:411-420): SGD(momentum 0.9) and
// RMSprop(momentum 0.9), one launch each over the same record / work tables as lf_adam_step (the step slots are unused).
int lf_sgd_step(const void* tensors_dev, const void* work_dev, int nblocks, float lr, float momentum, float weight_decay,
                float grad_scale, void* stream) {
    LF_REQUIRE(tensors_dev && work_dev && nblocks > 0, "lf_sgd_step: bad arguments");
    const OptScalars k = {lr, momentum, 0.f, 0.f, weight_decay, 0.f};
    launch_opt<OPT_SGD, false>(tensors_dev, work_dev, nblocks, k, lr, 0, grad_scale, nullptr, stream);
    LF_CHECK_LAUNCH("sgd_step");
    return 0;
}
int lf_rmsprop_step(const void* tensors_dev, const void* work_dev, int nblocks, float lr, float alpha, float eps, float momentum,
                    float weight_decay, float grad_scale, void* stream) {
    LF_REQUIRE(tensors_dev && work_dev && nblocks > 0, "lf_rmsprop_step: bad arguments");
    const OptScalars k = {lr, momentum, alpha, eps, weight_decay, 0.f};
    launch_opt<OPT_RMSPROP, false>(tensors_dev, work_dev, nblocks, k, lr, 0, grad_scale, nullptr, stream);
    LF_CHECK_LAUNCH("rmsprop_step");
    return 0;
}

// tensors_dev: n LfAdamTensor records {p, g, m, v, numel, step[2]} (7 x 8 bytes each); work_dev: nblocks int2 (tensor, chunk).
// parity (0 / 1): which of a record's two step slots holds the number of updates the tensor has received so far; the launch
// leaves that number + 1 in the other slot, so the caller alternates parity and never uploads a count.  grad_scale multiplies
// every gradient first (1/world for summed data-parallel gradients, 1 otherwise).
int lf_adam_step(const void* tensors_dev, const void* work_dev, int nblocks, float lr, float beta1, float beta2, float eps,
                 float weight_decay, int parity, float grad_scale, void* stream) {
    LF_REQUIRE(tensors_dev && work_dev && nblocks > 0 && (parity == 0 || parity == 1), "lf_adam_step: bad arguments");
    const OptScalars k = {0.f, beta1, beta2, eps, weight_decay, 1.f};      // a (step size) and f (bias correction 2) per tensor, in the kernel
    launch_opt<OPT_ADAM, false>(tensors_dev, work_dev, nblocks, k, lr, parity, grad_scale, nullptr, stream);
    LF_CHECK_LAUNCH("adam_step");
    return 0;
}

// ---- gradient-norm clipping (include/lanefit.h, "additions since 5 -- gradient-norm clipping") ----
size_t lf_grad_norm_workspace_bytes(int total_blocks) { return total_blocks > 0 ? (size_t)total_blocks * sizeof(double) : 0; }

int lf_grad_sumsq(const void* tensors_dev, const void* work_dev, int nblocks, int slot0, void* workspace, void* stream) {
    LF_REQUIRE(tensors_dev && work_dev && workspace && nblocks > 0 && slot0 >= 0 && ((uintptr_t)workspace & 7) == 0,
               "lf_grad_sumsq: bad arguments");
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3(nblocks), dim3(256), 0, (hipStream_t)stream, (const LfAdamTensor*)tensors_dev,
                       (const int2*)work_dev, (double*)workspace + slot0);
    LF_CHECK_LAUNCH("grad_sumsq");
    return 0;
}

int lf_grad_norm_finish(const void* workspace, int total_blocks, float grad_scale, float max_norm, float* out2, void* stream) {
    LF_REQUIRE(workspace && out2 && total_blocks > 0 && ((uintptr_t)workspace & 7) == 0, "lf_grad_norm_finish: bad arguments");
    hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)workspace, total_blocks,
                       grad_scale, max_norm, out2);
    LF_CHECK_LAUNCH("grad_norm_finish");
    return 0;
}

int lf_grad_scale_inplace(const void* tensors_dev, const void* work_dev, int nblocks, float grad_scale, const float* coef_dev,
                          void* stream) {
    LF_REQUIRE(tensors_dev && work_dev && coef_dev && nblocks > 0, "lf_grad_scale_inplace: bad arguments");
    hipLaunchKernelGGL(grad_scale_inplace_kernel, dim3(nblocks), dim3(256), 0, (hipStream_t)stream, (const LfAdamTensor*)tensors_dev,
                       (const int2*)work_dev, grad_scale, coef_dev);
    LF_CHECK_LAUNCH("grad_scale_inplace");
    return 0;
}

// The three steps with the effective gradient fl32(fl32(g * grad_scale) * coef_dev[0]); everything else as the unclipped entry points.
int lf_sgd_step_clipped(const void* tensors_dev, const void* work_dev, int nblocks, float lr, float momentum, float weight_decay,
                        float grad_scale, const float* coef_dev, void* stream) {
    LF_REQUIRE(tensors_dev && work_dev && coef_dev && nblocks > 0, "lf_sgd_step_clipped: bad arguments");
    const OptScalars k = {lr, momentum, 0.f, 0.f, weight_decay, 0.f};
    launch_opt<OPT_SGD, true>(tensors_dev, work_dev, nblocks, k, lr, 0, grad_scale, coef_dev, stream);
    LF_CHECK_LAUNCH("sgd_step_clipped");
    return 0;
}
int lf_rmsprop_step_clipped(const void* tensors_dev, const void* work_dev, int nblocks, float lr, float alpha, float eps,
                            float momentum, float weight_decay, float grad_scale, const float* coef_dev, void* stream) {
    LF_REQUIRE(tensors_dev && work_dev && coef_dev && nblocks > 0, "lf_rmsprop_step_clipped: bad arguments");
    const OptScalars k = {lr, momentum, alpha, eps, weight_decay, 0.f};
    launch_opt<OPT_RMSPROP, true>(tensors_dev, work_dev, nblocks, k, lr, 0, grad_scale, coef_dev, stream);
    LF_CHECK_LAUNCH("rmsprop_step_clipped");
    return 0;
}
int lf_adam_step_clipped(const void* tensors_dev, const void* work_dev, int nblocks, float lr, float beta1, float beta2, float eps,
                         float weight_decay, int parity, float grad_scale, const float* coef_dev, void* stream) {
    LF_REQUIRE(tensors_dev && work_dev && coef_dev && nblocks > 0 && (parity == 0 || parity == 1), "lf_adam_step_clipped: bad arguments");
    const OptScalars k = {0.f, beta1, beta2, eps, weight_decay, 1.f};
    launch_opt<OPT_ADAM, true>(tensors_dev, work_dev, nblocks, k, lr, parity, grad_scale, coef_dev, stream);
    LF_CHECK_LAUNCH("adam_step_clipped");
    return 0;
}

}  // extern "C"
