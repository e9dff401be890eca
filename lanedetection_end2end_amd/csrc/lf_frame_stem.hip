// The frozen detector on raw camera frames: crop + Pillow-exact BILINEAR resize + ToTensor (lf_pipeline.hip) and the inference form
// of the stem (lf_stem.hip, stem_fwd_kernel<3, T, true>) in ONE launch.  The resized fp32 image never exists in HBM: a workgroup owns
// a TH x TW tile of STEM output pixels, stages the source window of the (2 TH + 1) x (2 TW + 1) resized pixels its 3x3 stride-2
// patches read, resizes it LDS -> LDS (horizontal pass to uint8, vertical pass to fp32 of v / 255) and feeds the stem's 16-pixel MFMA
// tiles their B operands from LDS where stem_fwd_kernel takes them by buffer loads.
//
// Bit contract: the output equals lf_pipeline_image followed by lf_stem_fwd_infer on the same frames, fp32 and bf16 storage alike.
//   - the resize passes are resize_bilinear_kernel's integer arithmetic on the same tables, and ToTensor is the same (float)v / 255.0f;
//   - the MFMA sequence is stem_fwd_kernel's: 7 K-steps of v_mfma_f32_16x16x4_f32, k = 4 s + kq, the same A and B per step, zeros for
//     the padding taps and the padded K-step; the pooled channels after the same permutes, bias / affine + ReLU in the same order.
// The staging (and its guard against the end of the frames buffer) is SHARED with resize_bilinear_kernel (lf_pipeline_dev.h), and it
// is the only stage that knows the frame format: frame_stem_kernel is the packed-RGB kernel, frame_format_stem_kernel<.., FMT> the same
// body behind lf_stage_window_format<FMT> (BGR, NV12, YUYV -> the same RGB triples in the same LDS rows; the same LDS budget), and
// frame_surface_stem_kernel<.., FMT> the same body behind lf_stage_surface<FMT> for a plan with a frame layout (decoder surfaces:
// pitch, plane offsets or pointers, frame stride; all seven formats).  The
// two resize passes and the stem's per-tile arithmetic are LABELLED COPIES: the passes here walk a window
// with a one-pixel zero border and write LDS, not NCHW rows, and stem_fwd_kernel interleaves its operand addressing with the MFMA
// issue -- a common body would change the registers of both existing kernels.
//
// LDS (4 x 32 tile, 640 x 1280 -> 256 x 512: ~30 KB): [shift per staged row][source window, bytes][horizontal pass, bytes]
// [resized window, fp32, 3 planes].  The fp32 planes hold even and odd columns apart (column c at (c & 1) * CW + (c >> 1)): the 16
// pixels of an MFMA tile read columns 2 lx + kw, a stride of two floats -- kept apart, the 16 lanes of a k-slot read consecutive words
// (the four k-slots of a wave read different taps: lanes l and l + 16 may still meet on a bank, 2x at worst, 7 reads per tile).
#include "lf_pipeline_dev.h"
#include "lf_types.h"

#define FS_LDS_BUDGET (64 * 1024)

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

struct FsLayout { size_t in, h, v, total; int in_stride, h_stride, cw; };
// tw: tile width in stem pixels; the resized window is 2 th + 1 rows of 2 tw + 1 columns, stored as 2 cw = 2 tw + 2 floats per row
inline FsLayout fs_layout(int th, int tw, int max_rows, int max_cols, int ksx, int ksy) {
    FsLayout L;
    L.in_stride = lf_pipeline_in_stride(max_cols, ksx);
    L.h_stride = ((2 * tw + 1) * 3 + 3) / 4 * 4;
    L.cw = tw + 1;
    L.in = ((size_t)(max_rows + 1) * sizeof(int) + 15) / 16 * 16;
    L.h = L.in + (size_t)(max_rows + 1) * L.in_stride;
    L.v = (L.h + (size_t)(max_rows + ksy) * L.h_stride + 15) / 16 * 16;
    L.total = L.v + (size_t)3 * (2 * th + 1) * (2 * L.cw) * sizeof(float);
    return L;
}

// KSX / KSY: compile-time tap counts (table rows are zero-padded to them); 0 = generic (runtime count), as resize_bilinear_kernel
// FMT: the frame format (LF_FRAME_*), which only the staging knows; cf: its YCbCr coefficients (unused for RGB / BGR)
// SURF: the frames are decoder surfaces laid out as S says (lf_stage_surface; total_bytes is then the end of the whole batch)
template <int KSX, int KSY, typename T, int FMT, bool SURF = false>
__device__ __forceinline__ void frame_stem_body(const uint8_t* __restrict__ frames, size_t total_bytes, int Hin, int Win, int crop_top,
                                                const int* __restrict__ tables, int oh, int ow, int ksx, int ksy, int TH, int TW,
                                                int max_rows, int in_stride, const float* __restrict__ w, const float* __restrict__ b,
                                                const float* __restrict__ sc, const float* __restrict__ sh, T* __restrict__ cat,
                                                const lf_yuv_coef cf, const lf_surface& S = lf_surface{}) {
    constexpr int CIN = 3, Cc = 16 - CIN, KK = 9 * CIN, KS = (KK + 3) / 4;
    extern __shared__ uint8_t smem[];
    const int ncw = 2 * TW + 1, nrw = 2 * TH + 1;             // resized window: columns, rows
    const int h_stride = (ncw * 3 + 3) / 4 * 4, CW = TW + 1, ROWW = 2 * CW, PLANE = nrw * ROWW;
    int* s_shift = reinterpret_cast<int*>(smem);                                   // [max_rows + 1]
    uint8_t* s_in = smem + ((size_t)(max_rows + 1) * sizeof(int) + 15) / 16 * 16;    // [max_rows + 1][in_stride]
    uint8_t* s_h = s_in + (size_t)(max_rows + 1) * in_stride;                      // [max_rows + ksy][h_stride]
    float* s_v = reinterpret_cast<float*>(smem + ((size_t)(s_h - smem) + (size_t)(max_rows + ksy) * h_stride + 15) / 16 * 16);   // [3][nrw][ROWW]
    const Tables Tb = table_ptrs(tables, oh, ow, ksx, ksy);
    const int n = blockIdx.z, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int Ho = oh / 2, Wo = ow / 2;
    const int ty0 = blockIdx.y * TH, tx0 = blockIdx.x * TW;                         // stem pixels
    const int th = min(TH, Ho - ty0), tw = min(TW, Wo - tx0);
    // resized pixels the tile reads: rows [ya, yb], columns [xa, xb]; window position (wy, wx) is resized pixel (wy + 2 ty0 - 1,
    // wx + 2 tx0 - 1), and row / column -1 is the convolution's zero padding (the far edges never pad: oh, ow even)
    const int ya = max(0, 2 * ty0 - 1), yb = 2 * (ty0 + th) - 1, xa = max(0, 2 * tx0 - 1), xb = 2 * (tx0 + tw) - 1;
    const int r0 = Tb.by[2 * ya], r1 = Tb.by[2 * yb] + Tb.by[2 * yb + 1];
    const int c0 = Tb.bx[2 * xa], c1 = Tb.bx[2 * xb] + Tb.bx[2 * xb + 1];
    const int nr = r1 - r0, ncb = (c1 - c0) * 3;
    if constexpr (SURF)
        lf_stage_surface<FMT>(frames, total_bytes, S, n, crop_top + r0, c0, nr, ncb, s_in, in_stride, s_shift, lane, wave, cf);
    else if constexpr (FMT == LF_FRAME_RGB)
        lf_stage_window(frames, total_bytes, n, Hin, Win, crop_top + r0, c0, nr, ncb, s_in, in_stride, s_shift, lane, wave);
    else
        lf_stage_window_format<FMT>(frames, total_bytes, n, Hin, Win, crop_top + r0, c0, nr, ncb, s_in, in_stride, s_shift, lane, wave, cf);
    __syncthreads();
    // ---- horizontal pass (copy of resize_bilinear_kernel's): one (x, channel) column of the window per thread, rows in sequence
    const int nxc = (xb - xa + 1) * 3;
    for (int j = threadIdx.x; j < nxc; j += 256) {
        const int x = j / 3, c = j - x * 3;
        const int first = (Tb.bx[2 * (xa + x)] - c0) * 3 + c;
        const int* k = Tb.kx + (long)(xa + x) * ksx;
        if (KSX > 0) {
            int wt[KSX > 0 ? KSX : 1];
#pragma unroll
            for (int t = 0; t < KSX; ++t) wt[t] = k[t];
            for (int r = 0; r < nr; ++r) {
                const uint8_t* p = s_in + (size_t)r * in_stride + s_shift[r] + first;
                int acc = 1 << (PIL_PRECISION_BITS - 1);
#pragma unroll
                for (int t = 0; t < KSX; ++t) acc += (int)p[t * 3] * wt[t];     // taps past the count have zero weight
                s_h[r * h_stride + j] = (uint8_t)clip8(acc);
            }
        } else {
            const int cnt = Tb.bx[2 * (xa + x) + 1];
            for (int r = 0; r < nr; ++r) {
                const uint8_t* p = s_in + (size_t)r * in_stride + s_shift[r] + first;
                int acc = 1 << (PIL_PRECISION_BITS - 1);
                for (int t = 0; t < cnt; ++t) acc += (int)p[t * 3] * k[t];
                s_h[r * h_stride + j] = (uint8_t)clip8(acc);
            }
        }
    }
    __syncthreads();
    // ---- vertical pass + ToTensor (copy of resize_bilinear_kernel's) into the fp32 window; thread = (channel, window column), column
    // fastest; EVERY position of the window is written: zero where it is padding or lies beyond the tile's last row / column
    for (int j = threadIdx.x; j < 3 * ncw; j += 256) {
        const int c = j / ncw, wx = j - c * ncw;
        const int x = 2 * tx0 - 1 + wx;
        const bool xin = x >= xa && x <= xb;
        float* o = s_v + c * PLANE + (wx & 1) * CW + (wx >> 1);
        const uint8_t* col = s_h + (xin ? x - xa : 0) * 3 + c;
        for (int wy = 0; wy < nrw; ++wy) {
            const int y = 2 * ty0 - 1 + wy;                               // wave-uniform: scalar loads
            float v = 0.f;
            if (y >= ya && y <= yb) {
                const int first = Tb.by[2 * y] - r0;
                const int* k = Tb.ky + (long)y * ksy;
                const uint8_t* p = col + first * h_stride;
                int acc = 1 << (PIL_PRECISION_BITS - 1);
                if (KSY > 0) {
#pragma unroll
                    for (int t = 0; t < KSY; ++t) acc += (int)p[t * h_stride] * k[t];
                } else {
                    const int cnt = Tb.by[2 * y + 1];
                    for (int t = 0; t < cnt; ++t) acc += (int)p[t * h_stride] * k[t];
                }
                v = xin ? (float)clip8(acc) / 255.0f : 0.f;
            }
            o[wy * ROWW] = v;
        }
    }
    __syncthreads();
    // ---- the stem (copy of stem_fwd_kernel<3, T, true>'s tile arithmetic; operands from the window).  A = the weights (lane: row co =
    // l & 15, k-slot l >> 4), B = the patches of 16 consecutive pixels of one tile row (lane: pixel l & 15, k-slot l >> 4)
    const int pl = lane & 15, kq = lane >> 4;
    float wa[KS];
    int toff[KS];
    bool tap[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        const int k = 4 * s + kq, ci = k / 9, r = k - ci * 9, kh = r / 3, kw = r - kh * 3;
        tap[s] = k < KK;
        wa[s] = (tap[s] && pl < Cc) ? w[pl * KK + k] : 0.f;
        toff[s] = tap[s] ? ci * PLANE + kh * ROWW + (kw & 1) * CW + (kw >> 1) : 0;      // window column 2 lx + kw
    }
    float bv[4], av[4], cv[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        bv[e] = 4 * kq + e < Cc ? b[4 * kq + e] : 0.f;
        av[e] = sc[4 * kq + e]; cv[e] = sh[4 * kq + e];
    }
    const int tpr = TW >> 4, ntiles = TH * tpr;                            // 16-pixel tiles per tile row, per workgroup
    for (int m = wave; m < ntiles; m += 4) {
        const int ly = m / tpr, lx = (m - ly * tpr) * 16 + pl;
        const bool valid = ly < th && lx < tw;
        const float* base = s_v + 2 * ly * ROWW + lx;                      // window position (2 ly, 2 lx)
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const float x = base[toff[s]];
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[s], tap[s] ? x : 0.f, acc, 0, 0, 0);
        }
        // pooled channels: lane (pixel pl, kq < 3) takes the 2x2 maximum of input channel kq: window rows 2 ly + 1, + 2, columns 2 lx + 1, + 2
        float pm = 0.f;
        if (kq < CIN) {
            const float* q = base + kq * PLANE + ROWW;
            const float v0 = q[CW], v1 = q[1], v2 = q[ROWW + CW], v3 = q[ROWW + 1];
            pm = fmaxf(fmaxf(v0, v1), fmaxf(v2, v3));
        }
        f32x4 out;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int co = 4 * kq + e;
            float pooled = 0.f;
            if (e >= 4 - CIN) pooled = __shfl(pm, (e - (4 - CIN)) * 16 + pl, 64);      // (compile-time e: CIN permutes, every lane takes part)
            out[e] = co < Cc ? acc[e] + bv[e] : pooled;
            out[e] = fmaxf(out[e] * av[e] + cv[e], 0.f);
        }
        if (valid) lf_stv(cat + (((size_t)n * Ho + ty0 + ly) * Wo + tx0 + lx) * 16 + 4 * kq, out);
    }
}

// packed RGB frames: the kernel every plan ran before there were formats, the same code
template <int KSX, int KSY, typename T>
__global__ __launch_bounds__(256) void frame_stem_kernel(const uint8_t* __restrict__ frames, size_t total_bytes, int Hin, int Win, int crop_top,
                                                        const int* __restrict__ tables, int oh, int ow, int ksx, int ksy, int TH, int TW,
                                                        int max_rows, int in_stride, const float* __restrict__ w, const float* __restrict__ b,
                                                        const float* __restrict__ sc, const float* __restrict__ sh, T* __restrict__ cat) {
    frame_stem_body<KSX, KSY, T, LF_FRAME_RGB>(frames, total_bytes, Hin, Win, crop_top, tables, oh, ow, ksx, ksy, TH, TW, max_rows, in_stride, w,
                                               b, sc, sh, cat, lf_yuv_coef{});
}
// BGR, NV12 and YUYV frames: the staging converts (lf_stage_window_format), everything behind it is the same
template <int KSX, int KSY, typename T, int FMT>
__global__ __launch_bounds__(256) void frame_format_stem_kernel(const uint8_t* __restrict__ frames, size_t total_bytes, int Hin, int Win,
                                                               int crop_top, const int* __restrict__ tables, int oh, int ow, int ksx, int ksy,
                                                               int TH, int TW, int max_rows, int in_stride, const float* __restrict__ w,
                                                               const float* __restrict__ b, const float* __restrict__ sc,
                                                               const float* __restrict__ sh, T* __restrict__ cat, const lf_yuv_coef cf) {
    frame_stem_body<KSX, KSY, T, FMT>(frames, total_bytes, Hin, Win, crop_top, tables, oh, ow, ksx, ksy, TH, TW, max_rows, in_stride, w, b, sc, sh,
                                      cat, cf);
}
// decoder surfaces (a plan with a layout), every format: lf_stage_surface, everything behind it is the same
template <int KSX, int KSY, typename T, int FMT>
__global__ __launch_bounds__(256) void frame_surface_stem_kernel(const uint8_t* __restrict__ frames, size_t total_bytes, int Hin, int Win,
                                                                int crop_top, const int* __restrict__ tables, int oh, int ow, int ksx, int ksy,
                                                                int TH, int TW, int max_rows, int in_stride, const float* __restrict__ w,
                                                                const float* __restrict__ b, const float* __restrict__ sc,
                                                                const float* __restrict__ sh, T* __restrict__ cat, const lf_yuv_coef cf,
                                                                const lf_surface S) {
    frame_stem_body<KSX, KSY, T, FMT, true>(frames, total_bytes, Hin, Win, crop_top, tables, oh, ow, ksx, ksy, TH, TW, max_rows, in_stride, w, b,
                                            sc, sh, cat, cf, S);
}

}  // namespace

// Tile of stem pixels per workgroup: the first of the candidates whose workgroup stays inside the LDS budget.  Every candidate keeps a
// whole 16-pixel MFMA tile per wave (TH * TW / 16 >= 4); 4 x 32 is 256 workgroups per 256 x 512 frame, one per CU.
void lf_frame_stem_plan(lf_pipeline_plan* P) {
    P->fs_ok = 0; P->fs_th = P->fs_tw = P->fs_max_rows = P->fs_max_cols = P->fs_in_stride = 0; P->fs_lds_bytes = 0;
    if ((P->out_h & 1) || (P->out_w & 1)) return;
    const int Ho = P->out_h / 2, Wo = P->out_w / 2;
    static const int cand[][2] = {{4, 32}, {2, 32}, {4, 16}};
    for (const auto& c : cand) {
        const int th = c[0], tw = c[1];
        int max_rows = 0, max_cols = 0;
        for (int y0 = 0; y0 < Ho; y0 += th) {
            const int ya = 2 * y0 - 1 > 0 ? 2 * y0 - 1 : 0, yb = 2 * (y0 + th < Ho ? y0 + th : Ho) - 1;
            const int n = P->by[2 * yb] + P->by[2 * yb + 1] - P->by[2 * ya];
            if (n > max_rows) max_rows = n;
        }
        for (int x0 = 0; x0 < Wo; x0 += tw) {
            const int xa = 2 * x0 - 1 > 0 ? 2 * x0 - 1 : 0, xb = 2 * (x0 + tw < Wo ? x0 + tw : Wo) - 1;
            const int n = P->bx[2 * xb] + P->bx[2 * xb + 1] - P->bx[2 * xa];
            if (n > max_cols) max_cols = n;
        }
        const FsLayout L = fs_layout(th, tw, max_rows, max_cols, P->ksx, P->ksy);
        if (L.total > FS_LDS_BUDGET) continue;
        P->fs_ok = 1; P->fs_th = th; P->fs_tw = tw; P->fs_max_rows = max_rows; P->fs_max_cols = max_cols;
        P->fs_in_stride = L.in_stride; P->fs_lds_bytes = L.total;
        return;
    }
}

int lf_frame_stem_fwd_infer(const lf_pipeline_plan* P, const uint8_t* frames, int N, const void* tables_dev, const float* w, const float* b,
                            const float* sc, const float* sh, float* cat, int s16, hipStream_t st) {
    LF_REQUIRE(P && frames && tables_dev && w && b && sc && sh && cat, "frame_stem: null pointer");
    LF_REQUIRE(N >= 1 && N <= 65535, "frame_stem: batch %d not in 1..65535", N);
    LF_REQUIRE(!(P->out_h & 1) && !(P->out_w & 1), "frame_stem: odd image size %d x %d", P->out_h, P->out_w);
    LF_REQUIRE(P->fs_ok, "frame_stem: the source window of a tile does not fit the LDS budget (%d x %d from %d x %d)", P->out_h, P->out_w,
               P->crop_h, P->Win);
    const dim3 grid(lf_cdiv(P->out_w / 2, P->fs_tw), lf_cdiv(P->out_h / 2, P->fs_th), N);
    if (P->has_layout) {
        const size_t end = (size_t)(N - 1) * P->surf.stride + P->surf.frame_span;
#define LF_FSS_LAUNCH(KX, KY, TT, F)                                                                                                         \
    hipLaunchKernelGGL((frame_surface_stem_kernel<KX, KY, TT, F>), grid, dim3(256), P->fs_lds_bytes, st, frames, end, P->Hin, P->Win,       \
                       P->crop_top, (const int*)tables_dev, P->out_h, P->out_w, P->ksx, P->ksy, P->fs_th, P->fs_tw, P->fs_max_rows,          \
                       P->fs_in_stride, w, b, sc, sh, reinterpret_cast<TT*>(cat), P->coef, P->surf)
#define LF_FSS_FORMATS(KX, KY, TT)                                               \
    switch (P->format) {                                                         \
        case LF_FRAME_RGB: LF_FSS_LAUNCH(KX, KY, TT, LF_FRAME_RGB); break;       \
        case LF_FRAME_BGR: LF_FSS_LAUNCH(KX, KY, TT, LF_FRAME_BGR); break;       \
        case LF_FRAME_NV12: LF_FSS_LAUNCH(KX, KY, TT, LF_FRAME_NV12); break;     \
        case LF_FRAME_YUYV: LF_FSS_LAUNCH(KX, KY, TT, LF_FRAME_YUYV); break;     \
        case LF_FRAME_I420: LF_FSS_LAUNCH(KX, KY, TT, LF_FRAME_I420); break;     \
        case LF_FRAME_RGBX: LF_FSS_LAUNCH(KX, KY, TT, LF_FRAME_RGBX); break;     \
        default: LF_FSS_LAUNCH(KX, KY, TT, LF_FRAME_BGRX); break;                \
    }
        // the camera geometry's 7 / 7 taps compiled in, every other geometry on the generic taps (lf_pipeline.hip does the same)
        if (P->ksx == 7 && P->ksy == 7) {
            if (s16) LF_FSS_FORMATS(7, 7, lf_bf16)
            else LF_FSS_FORMATS(7, 7, float)
        } else {
            if (s16) LF_FSS_FORMATS(0, 0, lf_bf16)
            else LF_FSS_FORMATS(0, 0, float)
        }
#undef LF_FSS_FORMATS
#undef LF_FSS_LAUNCH
        LF_CHECK_LAUNCH("frame_stem");
        return 0;
    }
    const size_t total = (size_t)N * lf_plan_frame_bytes(P);
#define LF_FS_ARGS(TT)                                                                                                                 \
    frames, total, P->Hin, P->Win, P->crop_top, (const int*)tables_dev, P->out_h, P->out_w, P->ksx, P->ksy, P->fs_th, P->fs_tw,        \
        P->fs_max_rows, P->fs_in_stride, w, b, sc, sh, reinterpret_cast<TT*>(cat)
#define LF_FS_LAUNCH(KX, KY, TT)                                                                                                       \
    do {                                                                                                                               \
        if (P->format == LF_FRAME_RGB)                                                                                                 \
            hipLaunchKernelGGL((frame_stem_kernel<KX, KY, TT>), grid, dim3(256), P->fs_lds_bytes, st, LF_FS_ARGS(TT));                 \
        else if (P->format == LF_FRAME_BGR)                                                                                            \
            hipLaunchKernelGGL((frame_format_stem_kernel<KX, KY, TT, LF_FRAME_BGR>), grid, dim3(256), P->fs_lds_bytes, st, LF_FS_ARGS(TT), \
                               P->coef);                                                                                               \
        else if (P->format == LF_FRAME_NV12)                                                                                           \
            hipLaunchKernelGGL((frame_format_stem_kernel<KX, KY, TT, LF_FRAME_NV12>), grid, dim3(256), P->fs_lds_bytes, st, LF_FS_ARGS(TT), \
                               P->coef);                                                                                               \
        else                                                                                                                           \
            hipLaunchKernelGGL((frame_format_stem_kernel<KX, KY, TT, LF_FRAME_YUYV>), grid, dim3(256), P->fs_lds_bytes, st, LF_FS_ARGS(TT), \
                               P->coef);                                                                                               \
    } while (0)
#define LF_FS_TAPS(TT)                                                      \
    do {                                                                    \
        if (P->ksx == 7 && P->ksy == 7) LF_FS_LAUNCH(7, 7, TT);             \
        else if (P->ksx == 5 && P->ksy == 5) LF_FS_LAUNCH(5, 5, TT);        \
        else LF_FS_LAUNCH(0, 0, TT);                                        \
    } while (0)
    if (s16) LF_FS_TAPS(lf_bf16);
    else LF_FS_TAPS(float);
#undef LF_FS_TAPS
#undef LF_FS_LAUNCH
#undef LF_FS_ARGS
    LF_CHECK_LAUNCH("frame_stem");
    return 0;
}

// csrc/lf_debug.h: the kernel alone
extern "C" int lf_debug_frame_stem(const lf_pipeline_plan* P, const uint8_t* frames, int N, const void* tables_dev, const float* w, const float* b,
                                   const float* sc, const float* sh, float* cat, int s16, void* stream) {
    if (!(P && frames && tables_dev && w && b && sc && sh && cat) || ((size_t)cat & 15)) {
        lf_fail("lf_debug_frame_stem: null or misaligned pointer");
        return -1;
    }
    if (N < 1) { lf_fail("lf_debug_frame_stem: bad batch %d", N); return -1; }
    return lf_frame_stem_fwd_infer(P, frames, N, tables_dev, w, b, sc, sh, cat, s16 != 0, (hipStream_t)stream) ? -1 : 0;
}
