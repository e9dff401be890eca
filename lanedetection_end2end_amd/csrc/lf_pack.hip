// Weight-packing kernels of the tap-GEMM convolutions for gfx950 (see lf_conv.h for the contract): the parameter tensors in the
// operand orders the kernels of lf_conv.hip (fp32, 3-way bf16 split) and lf_conv_bf16.hip (bf16) read, and the inference engine's fold-and-pack, which
// scales every weight by the BatchNorm factor of its output channel on the way.
#include "lf_conv.h"

namespace {

__global__ __launch_bounds__(256) void pack_weights_kernel(const LfPackEntry* __restrict__ entries,
                                                          const float* const* __restrict__ params,
                                                          float* __restrict__ arena) {
    const LfPackEntry e = entries[blockIdx.x];
    const float* w = params[e.param];
    float* dst = arena + e.dst_off;
    // (32-bit index arithmetic: an entry has at most 9 * 128 * 128 elements, and the 64-bit divisions of the first version expanded
    // to ~100 instructions each -- 34 us for 2 M floats)
    const unsigned total = (unsigned)(e.ntaps * e.Kc * e.Nc), Nc = (unsigned)e.Nc, kbn = (unsigned)(e.Kc >> 2);
    for (unsigned i = blockIdx.y * 256u + threadIdx.x; i < total; i += gridDim.y * 256u) {
        const unsigned k4 = i & 3u, r = i >> 2, r2 = r / Nc, n = r - r2 * Nc, t = r2 / kbn, kb = r2 - t * kbn;
        const unsigned k = kb * 4u + k4;
        dst[i] = w[(long)k * e.sk + (long)n * e.sn + e.tapidx[t]];
    }
}

// bf16 operand order of tapgemm_bf16_kernel: [tap][ceil(Kc/32)*4][Nc][8], zero beyond Kc
__global__ __launch_bounds__(256) void pack_weights_bf16_kernel(const LfPackEntry* __restrict__ entries,
                                                               const float* const* __restrict__ params,
                                                               __bf16* __restrict__ arena) {
    const LfPackEntry e = entries[blockIdx.x];
    const float* w = params[e.param];
    __bf16* dst = arena + e.dst16_off;
    const int kb_per_tap = ((e.Kc + 31) >> 5) * 4;
    const unsigned total = (unsigned)(e.ntaps * kb_per_tap * e.Nc * 8), Nc = (unsigned)e.Nc, kbn = (unsigned)kb_per_tap;     // (32-bit: see pack_weights_kernel)
    for (unsigned i = blockIdx.y * 256u + threadIdx.x; i < total; i += gridDim.y * 256u) {
        const unsigned k8 = i & 7u, r = i >> 3, r2 = r / Nc, n = r - r2 * Nc, t = r2 / kbn, kb = r2 - t * kbn;
        const int k = (int)(kb * 8u + k8);
        dst[i] = (__bf16)(k < e.Kc ? w[(long)k * e.sk + (long)n * e.sn + e.tapidx[t]] : 0.f);
    }
}

// split operand order of tapgemm_split_kernel: [tap][Kc/8][Nc][3][8] bf16, pieces h, m, l of every weight (exact:
// h + m + l == w); entries whose Kc is not a multiple of 32 are never used by that kernel and skipped here
__global__ __launch_bounds__(256) void pack_weights_split_kernel(const LfPackEntry* __restrict__ entries,
                                                                const float* const* __restrict__ params,
                                                                __bf16* __restrict__ arena) {
    const LfPackEntry e = entries[blockIdx.x];
    if (e.Kc % 32 != 0) return;
    const float* w = params[e.param];
    __bf16* dst = arena + 3 * e.dst16_off;
    const int kb_per_tap = e.Kc >> 3;
    const long total = (long)e.ntaps * kb_per_tap * e.Nc * 8;
    for (long i = (long)blockIdx.y * 256 + threadIdx.x; i < total; i += (long)gridDim.y * 256) {
        const int k8 = (int)(i & 7);
        long r = i >> 3;
        const int n = (int)(r % e.Nc);
        const long row = r;                       // (t * kb_per_tap + kb) * Nc + n
        r /= e.Nc;
        const int kb = (int)(r % kb_per_tap);
        const int t = (int)(r / kb_per_tap);
        const float v = w[(kb * 8 + k8) * e.sk + n * e.sn + e.tapidx[t]];
        const __bf16 vh = (__bf16)v;
        const float r1 = v - (float)vh;
        const __bf16 vm = (__bf16)r1;
        const float r2 = r1 - (float)vm;
        dst[row * 24 + k8] = vh; dst[row * 24 + 8 + k8] = vm; dst[row * 24 + 16 + k8] = (__bf16)r2;
    }
}

// Inference fold-and-pack (lf_conv.h, LfFoldEntry): one workgroup row per entry, the three operand orders of the pack kernels
// above, every weight scaled by its output channel's BatchNorm factor in fp64 and rounded once to fp32 (the bf16 / split forms are
// taken from that fp32 value, as the training packs take theirs from the fp32 parameter).  Row y = 0 also writes the entry's
// per-channel vectors.
__device__ __forceinline__ double fold_scale(const LfFoldEntry& f, int n, float eps) {
    if (!f.gamma) return 1.0;
    const int c = f.ch_off + n;
    return (double)f.gamma[c] / sqrt((double)f.var[c] + (double)eps);
}
__device__ __forceinline__ float fold_w(const LfFoldEntry& f, const float* w, int k, int n, int t, float eps) {
    const float v = w[(long)k * f.pk.sk + (long)n * f.pk.sn + f.pk.tapidx[t]];
    return f.gamma ? (float)((double)v * fold_scale(f, n, eps)) : v;
}
__global__ __launch_bounds__(256) void fold_pack_kernel(const LfFoldEntry* __restrict__ entries, const float* const* __restrict__ params,
                                                       float eps, float* __restrict__ vec, float* __restrict__ arena, __bf16* __restrict__ arena16,
                                                       __bf16* __restrict__ arena48) {
    const LfFoldEntry f = entries[blockIdx.x];
    const LfPackEntry& e = f.pk;
    if (blockIdx.y == 0) {
        for (int n = threadIdx.x; n < f.C; n += 256) {
            const double s = fold_scale(f, n, eps);
            const int c = f.ch_off + n;
            float* out = vec + f.out_off;
            if (e.ntaps > 0) {
                out[n] = f.gamma ? (float)(((double)f.bias[n] - (double)f.mean[c]) * s + (double)f.beta[c]) : f.bias[n];
            } else {
                out[n] = (float)s;
                out[f.C + n] = (float)((double)f.beta[c] - (double)f.mean[c] * s);
            }
        }
    }
    if (e.ntaps == 0) return;
    const float* w = params[e.param];
    const unsigned Nc = (unsigned)e.Nc;
    if (arena) {            // [tap][Kc/4][Nc][4] (pack_weights_kernel)
        float* dst = arena + e.dst_off;
        const unsigned total = (unsigned)(e.ntaps * e.Kc * e.Nc), kbn = (unsigned)(e.Kc >> 2);
        for (unsigned i = blockIdx.y * 256u + threadIdx.x; i < total; i += gridDim.y * 256u) {
            const unsigned k4 = i & 3u, r = i >> 2, r2 = r / Nc, n = r - r2 * Nc, t = r2 / kbn, kb = r2 - t * kbn;
            dst[i] = fold_w(f, w, (int)(kb * 4u + k4), (int)n, (int)t, eps);
        }
    }
    if (arena16) {          // [tap][ceil(Kc/32)*4][Nc][8], zero beyond Kc (pack_weights_bf16_kernel)
        __bf16* dst = arena16 + e.dst16_off;
        const unsigned kbn = (unsigned)(((e.Kc + 31) >> 5) * 4), total = (unsigned)e.ntaps * kbn * Nc * 8u;
        for (unsigned i = blockIdx.y * 256u + threadIdx.x; i < total; i += gridDim.y * 256u) {
            const unsigned k8 = i & 7u, r = i >> 3, r2 = r / Nc, n = r - r2 * Nc, t = r2 / kbn, kb = r2 - t * kbn;
            const int k = (int)(kb * 8u + k8);
            dst[i] = (__bf16)(k < e.Kc ? fold_w(f, w, k, (int)n, (int)t, eps) : 0.f);
        }
    }
    if (arena48 && e.Kc % 32 == 0) {     // [tap][Kc/8][Nc][3][8], exact 3-way split (pack_weights_split_kernel)
        __bf16* dst = arena48 + 3 * e.dst16_off;
        const unsigned kbn = (unsigned)(e.Kc >> 3), total = (unsigned)e.ntaps * kbn * Nc * 8u;
        for (unsigned i = blockIdx.y * 256u + threadIdx.x; i < total; i += gridDim.y * 256u) {
            const unsigned k8 = i & 7u, row = i >> 3, r2 = row / Nc, n = row - r2 * Nc, t = r2 / kbn, kb = r2 - t * kbn;
            const float v = fold_w(f, w, (int)(kb * 8u + k8), (int)n, (int)t, eps);
            const __bf16 vh = (__bf16)v;
            const float r1 = v - (float)vh;
            const __bf16 vm = (__bf16)r1;
            dst[row * 24u + k8] = vh; dst[row * 24u + 8u + k8] = vm; dst[row * 24u + 16u + k8] = (__bf16)(r1 - (float)vm);
        }
    }
}

std::atomic<long> g_fold_pack_launches{0};      // (the backbone's engine and the --clas heads' chains both fold through here)

}  // namespace

int lf_fold_pack_launch(const LfFoldEntry* entries_dev, int nentries, const float* const* params_dev, float eps, float* vec, float* arena,
                        void* arena16, void* arena48, hipStream_t st) {
    if (nentries <= 0) return 0;
    LF_REQUIRE(vec, "fold_pack: null vector region");
    hipLaunchKernelGGL(fold_pack_kernel, dim3(nentries, 16), dim3(256), 0, st, entries_dev, params_dev, eps, vec, arena,
                       reinterpret_cast<__bf16*>(arena16), reinterpret_cast<__bf16*>(arena48));
    LF_CHECK_LAUNCH("fold_pack");
    ++g_fold_pack_launches;
    return 0;
}
long lf_fold_pack_launches() { return g_fold_pack_launches.load(); }

int lf_pack_weights_launch(const LfPackEntry* entries_dev, int nentries, const float* const* params_dev, float* arena,
                           hipStream_t st) {
    hipLaunchKernelGGL(pack_weights_kernel, dim3(nentries, 16), dim3(256), 0, st, entries_dev, params_dev, arena);
    LF_CHECK_LAUNCH("pack_weights");
    return 0;
}

int lf_pack_weights_bf16_launch(const LfPackEntry* entries_dev, int nentries, const float* const* params_dev, void* arena16,
                                hipStream_t st) {
    hipLaunchKernelGGL(pack_weights_bf16_kernel, dim3(nentries, 16), dim3(256), 0, st, entries_dev, params_dev,
                       reinterpret_cast<__bf16*>(arena16));
    LF_CHECK_LAUNCH("pack_weights_bf16");
    return 0;
}

int lf_pack_weights_split_launch(const LfPackEntry* entries_dev, int nentries, const float* const* params_dev, void* arena48,
                                 hipStream_t st) {
    hipLaunchKernelGGL(pack_weights_split_kernel, dim3(nentries, 16), dim3(256), 0, st, entries_dev, params_dev,
                       reinterpret_cast<__bf16*>(arena48));
    LF_CHECK_LAUNCH("pack_weights_split");
    return 0;
}

long lf_pack_bf16_elems(int Kc, int Nc, int ntaps) { return (long)ntaps * (((Kc + 31) >> 5) * 32) * Nc; }
